/*
 * tamf_winding.h - C-ABI of the generalized winding number (libtamf_winding.so): the solid angle a triangle mesh subtends at a point,
 * summed over the faces in a fixed tree and divided by 4 pi (Jacobson, Kavan, Sorkine-Hornung 2013), and the inside test |w| > 0.5
 * built on it.  It is the sign for object meshes that are open or scanned: it equals the ray-parity answer of tamf_mesh_contains on a
 * clean closed mesh, degrades smoothly where the mesh has a hole, and has no preferred direction.
 *
 * Conventions: those of tamf_meshdist.h.  Plain C types; every function returns 0 (or a byte count) or a negative tamf_status
 * (tamf_hip.h, included for that enum only); the message of the calling thread's last failure is tamf_winding_last_error().  "dev"
 * pointers are device memory owned by the caller, on the current device, "host" pointers host memory; `stream` is a hipStream_t passed
 * as void*, the work is enqueued on it and no call synchronises the device (host arrays are copied from pageable memory,
 * stream-ordered, and have been read when the call returns).  No state is kept between calls.  Invalid arguments launch nothing.
 *
 * THE DEFINITION.  Everything is float64 without fused multiply-adds (fp contract off), IEEE division and a correctly rounded sqrt.
 *   dot(u, v) = (u0 v0 + u1 v1) + u2 v2   (tamf_meshdist.h's).      cross(u, v) = (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0).
 *
 *   Valid faces.  tamf_meshdist.h's predicate: face f = (i0, i1, i2) of a mesh of V vertices is VALID when its indices lie in [0, V),
 *           are pairwise different, and its area 0.5 |(v1 - v0) x (v2 - v0)| (mesh_io.face_areas, float64) is > 0.  Only valid faces
 *           are summed: a degenerate face with the query point between its collinear vertices would otherwise add a spurious 2 pi.
 *   One face.  a, b, c = the face's vertices minus the query point p (per coordinate);  la = sqrt(dot(a, a)), lb, lc likewise.
 *               det   = dot(a, cross(b, c))
 *               den   = ((la lb) lc + dot(a, b) lc) + (dot(b, c) la + dot(c, a) lb)
 *               omega = 2 atan2(det, den)                                  (van Oosterom and Strackee 1983)
 *   Summation.  The tree depends on the mesh alone.  The valid faces, in ascending original index, are cut into chunks of
 *           TAMF_WINDING_CHUNK; a chunk's partial is the serial sum of its omega in index order, starting from +0; the total is the
 *           serial sum of the partials in chunk order, starting from +0;  w = total / (4 pi), 4 pi the float64 nearest to it
 *           (TAMF_WINDING_FOUR_PI).
 *   Inside.  inside = |w| > 0.5.  The absolute value makes a consistently inverted mesh work, as ray parity does.  A NaN w is outside.
 *   Query point of a job with rows [R | t]: tamf_meshdist.h's, ((R00 x + R01 y) + R02 z) + t0 (rows 1, 2 alike) of the float32 point
 *           widened exactly.
 *
 * DETERMINISM.  No atomics anywhere.  The same call gives the same bits, and a point's w depends on (mesh, point) alone: not on the
 * batch or the job list it is in, not on the launch geometry, not on whether the chunks were spread over work groups (the partials
 * then go through memory and a second small launch adds them in chunk order) or looped over in one thread.  Whether to spread is
 * decided on the host from the call's sizes (or forced by the flags) and changes no result.
 *
 * WHAT IS NOT BIT-DEFINED.  atan2 is the device library's and is not restated bit for bit: it is the one operation this definition
 * leaves open, and the reason the tests of this library compare with a gate where tamf_meshdist.h's compare bits.  Everything around
 * it (a, b, c, the lengths, det, den, the doubling, the summation tree, the division) is as stated.
 *
 * POINTS ON THE SURFACE.  A point in the plane of a face and inside that face has den < 0 and a det that is a rounding residue of
 * either sign (or a zero of either sign), so that face contributes omega = +2 pi or -2 pi: +0.5 or -0.5 to w, and `inside` of such a
 * point is not meaningful.  At a vertex of a face a = 0 (say), so det = +-0 and den = +0 (the first term (la lb) lc is +0 and decides
 * the sign of the sum of zeros): the face contributes +-0.  On an edge, outside the vertices, det = +-0 or a residue and den is a
 * residue of either sign: 0 or +-2 pi.  atan2 is finite for every finite or zero pair, so w is finite for every finite input whose
 * intermediate products do not overflow; a NaN coordinate of the point or of its job's transform gives w = NaN and inside = 0.
 */
#ifndef TAMF_WINDING_H
#define TAMF_WINDING_H

#include <stdint.h>

#include "tamf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TAMF_WINDING_CHUNK 1024                     /* valid faces per partial sum */
#define TAMF_WINDING_FOUR_PI 12.566370614359172     /* the float64 nearest to 4 pi */
#define TAMF_WINDING_MAX_MESHES 65535
#define TAMF_WINDING_FORCE_LOOP 1u                  /* flags bit 0: every thread loops over the chunks of its point (one launch) */
#define TAMF_WINDING_FORCE_SPREAD 2u                /* flags bit 1: one work group per (256 points, chunk), then the second launch */

/* message of the last failure of a call made by THIS thread ("" when none) */
const char* tamf_winding_last_error(void);

/* bytes of device workspace tamf_winding_prepare fills for M meshes; the three HOST offset arrays have M + 1 entries, start at 0 and
 * do not decrease: mesh m owns vertices [vert_off[m], vert_off[m+1]), faces [face_off[m], face_off[m+1]) and the entries
 * [valid_off[m], valid_off[m+1]) of the list of valid faces.  Negative tamf_status: M outside [1, 65535], a null or ill-formed offset
 * array, a mesh without a vertex, a face or a valid face, more valid faces than faces. */
int64_t tamf_winding_workspace(int32_t M, const int64_t* vert_off_host, const int64_t* face_off_host, const int64_t* valid_off_host);

/* Packs M meshes into `workspace_dev` (one host-to-device copy on `stream`, no launch).
 *   verts (V_total,3) f64, faces (F_total,3) int32 with indices local to their mesh: HOST
 *   valid (valid_off[M],) int32 HOST: per mesh the VALID faces as original (local) indices in strictly ascending order
 *   workspace: tamf_winding_workspace(...) bytes, 16-byte aligned
 * TAMF_ERR_INVALID, nothing copied: whatever tamf_winding_workspace refuses, a null pointer, a workspace too small or misaligned, a
 * list that is not strictly ascending or names a face outside its mesh, or a listed face with an index outside [0, V) or a repeated
 * index.  (That a listed face has a positive area is the caller's word.) */
int tamf_winding_prepare(const double* verts_host, const int32_t* faces_host, int32_t M, const int64_t* vert_off_host,
                         const int64_t* face_off_host, const int32_t* valid_host, const int64_t* valid_off_host, void* workspace_dev,
                         int64_t workspace_bytes, void* stream);

/* bytes of device scratch tamf_winding_points needs for these J jobs: the job records and, when the call spreads the chunks over
 * work groups, one partial per (output point, chunk).  mesh_id, pt_len (J,) and valid_off (M + 1,) are the HOST arrays the call and
 * tamf_winding_prepare get; `flags` those of the call.  Negative tamf_status: what tamf_winding_points refuses of these arguments. */
int64_t tamf_winding_points_workspace(int32_t J, int32_t M, const int32_t* mesh_id_host, const int64_t* pt_len_host,
                                      const int64_t* valid_off_host, uint32_t flags);

/* J jobs (mesh, rigid transform, slice of points); the outputs of the jobs lie end to end in job order.
 *   prepared: the workspace tamf_winding_prepare filled for M meshes with valid_off             points (P_total,3) f32 device
 *   mesh_id (J,) int32, transf (J,12) f64 = rows of [R | t], pt_off / pt_len (J,) int64, valid_off (M + 1,) int64: HOST
 *   flags: 0 (the host decides whether to spread the chunks, from J, pt_len and the chunk counts), TAMF_WINDING_FORCE_LOOP or
 *     TAMF_WINDING_FORCE_SPREAD
 *   jobs_workspace: tamf_winding_points_workspace(...) bytes for the same arguments, 16-byte aligned, device
 *   w_out (sum pt_len,) f64;  inside_out (sum pt_len,) uint8 or NULL
 * An empty slice writes nothing.  TAMF_ERR_INVALID, nothing launched: a null pointer (inside_out may be null; points may be null when
 * P_total is 0), M outside [1, 65535], J < 1, P_total < 0, mesh_id outside [0, M), a negative offset or length, a slice past P_total,
 * an ill-formed valid_off, unknown flags or both bits set, a forced spread too large for one launch, a jobs workspace too small or
 * misaligned. */
int tamf_winding_points(const void* prepared_dev, int32_t M, const float* points_dev, int64_t P_total, int32_t J, const int32_t* mesh_id_host,
                        const double* transf_host, const int64_t* pt_off_host, const int64_t* pt_len_host, const int64_t* valid_off_host,
                        uint32_t flags, void* jobs_workspace_dev, int64_t jobs_workspace_bytes, double* w_out_dev, uint8_t* inside_out_dev,
                        void* stream);

/* w_out[(i R + j) R + k] = winding number of prepared mesh `mesh` at the lattice point (ticks[i,0], ticks[j,1], ticks[k,2]).
 *   ticks (R,3) f64 device, w_out (R^3,) f64 device, inside_out (R^3,) uint8 device or NULL.  A work group owns a brick of 8 x 8 x 4
 *   lattice points; every thread loops over the chunks of its point.
 * TAMF_ERR_INVALID, nothing launched: a null pointer, M outside [1, 65535], mesh outside [0, M), R outside [2, 512]. */
int tamf_winding_lattice(const void* prepared_dev, int32_t M, int32_t mesh, const double* ticks_dev, int32_t R, double* w_out_dev,
                         uint8_t* inside_out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TAMF_WINDING_H */
