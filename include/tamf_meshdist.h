/*
 * tamf_meshdist.h - C-ABI of the point-to-mesh distance (libtamf_meshdist.so): the exact unsigned distance from points to the surface
 * of a triangle mesh, defined bit for bit, with the face it is attained on and, on request, the inside test of tamf_mesh_contains for
 * the same query point.  It is the distance half of the reference's process_sdf (dev_fn/util/sdf_util.py:59-99; tamf_eval.h has the
 * sign) and what the penetration depth score is built on (metrics/pd.py).
 *
 * Conventions: those of tamf_eval.h.  Plain C types; every function returns 0 (or a byte count) or a negative tamf_status (tamf_hip.h,
 * included for that enum only); the message of the calling thread's last failure is tamf_meshdist_last_error().  "dev" pointers are
 * device memory owned by the caller, on the current device, "host" pointers host memory; `stream` is a hipStream_t passed as void*,
 * the work is enqueued on it and no call synchronises the device (host arrays are copied from pageable memory, stream-ordered, and
 * have been read when the call returns).  No state is kept between calls: what tamf_meshdist_prepare wrote into the caller's
 * workspace is all a later call needs.  Invalid arguments launch nothing.
 *
 * THE DEFINITION.  Everything is float64 without fused multiply-adds (fp contract off), IEEE division and a correctly rounded sqrt.
 *   dot(u, v) = (u0 v0 + u1 v1) + u2 v2.            u +- v, s * u: per coordinate.
 *
 *   Valid faces.  Face f = (i0, i1, i2) of a mesh of V vertices is VALID when its indices lie in [0, V), are pairwise different, and
 *           its area 0.5 |(v1 - v0) x (v2 - v0)| (mesh_io.face_areas, float64) is > 0.  Only valid faces are considered.
 *   Point and face.  a, b, c = the face's vertices, p the point.  The closest point q of the triangle is found by the region sequence
 *           of Ericson's ClosestPtPointTriangle (Real-Time Collision Detection, 5.1.5), the first region that applies, in this order:
 *               ab = b - a, ac = c - a, ap = p - a         d1 = dot(ab, ap), d2 = dot(ac, ap)
 *               bp = p - b                                 d3 = dot(ab, bp), d4 = dot(ac, bp)
 *               cp = p - c                                 d5 = dot(ab, cp), d6 = dot(ac, cp)
 *               vc = d1 d4 - d3 d2,  vb = d5 d2 - d1 d6,  va = d3 d6 - d5 d4
 *             1 vertex A   d1 <= 0 and d2 <= 0                                q = a
 *             2 vertex B   d3 >= 0 and d4 <= d3                               q = b
 *             3 edge AB    vc <= 0 and d1 >= 0 and d3 <= 0                    v = d1 / (d1 - d3),  q = a + ab v
 *             4 vertex C   d6 >= 0 and d5 <= d6                               q = c
 *             5 edge AC    vb <= 0 and d2 >= 0 and d6 <= 0                    w = d2 / (d2 - d6),  q = a + ac w
 *             6 edge BC    va <= 0 and (d4 - d3) >= 0 and (d5 - d6) >= 0      w = (d4 - d3) / ((d4 - d3) + (d5 - d6)),  q = b + (c - b) w
 *             7 interior   otherwise        denom = 1 / ((va + vb) + vc),  v = vb denom,  w = vc denom,  q = (a + ab v) + ac w
 *           d2(p, f) = dot(p - q, p - q).  (A comparison with a NaN is false: such a point falls through to region 7.)
 *   Point and mesh.  (d2, f) = the lexicographic minimum of (d2(p, f), f) over the valid faces f: a candidate replaces the best only
 *           when its d2 is smaller, or equal with a smaller face index.  A NaN d2 never wins; the lowest ORIGINAL face index wins a
 *           tie (a closest point on a shared edge or vertex ties every time).  dist = sqrt(d2).  When no candidate ever wins (every d2 a
 *           NaN: a NaN point) dist = +inf and face = -1.
 *   Query point of a job with rows [R | t]: ((R00 x + R01 y) + R02 z) + t0 (rows 1, 2 alike) of the float32 point widened exactly.
 *   Inside.  The boolean of tamf_mesh_contains (tamf_hip.h) for the query point and the mesh made of the faces whose indices lie in
 *           [0, V) (the faces that can be read at all), with the mesh's scale3 / translate3 and hash_resolution given at prepare.
 *
 * The result is a minimum over a set, so it depends on (mesh, point) alone: not on the face permutation, the tiles, the launch
 * geometry, the batch a point is in, or the culling.  No atomics anywhere.
 *
 * CULLING.  The valid faces are packed TAMF_MESHDIST_TILE at a time in the order of the caller's permutation (Morton order of the
 * centroids makes a tile compact); every tile has an axis-aligned box over its vertices, inflated on every side by
 * TAMF_MESHDIST_BOX_MARGIN * (the largest |coordinate| of the box).  A work group of 256 points takes the box B of its points, starts
 * with the tile whose box is nearest to B, and before any other tile compares
 *     lb = ((gx^2 + gy^2) + gz^2) * (1 - 2^-40),   g_k = max(0, tile_lo_k - B_hi_k, B_lo_k - tile_hi_k)
 * with the largest current best d2 of its points: the tile is skipped when lb is strictly larger.  Why that is conservative: q is a
 * combination a + ab v + ac w with computed weights v, w, v + w in [0, 1] up to rounding, so every coordinate of q lies in the
 * tile's box to within a few 2^-53 of the box's largest |coordinate| - the inflation is 2^33 times that - hence |p_k - q_k| >= g_k
 * exactly for every point of B; the subtractions, squares and sums of d2 and of lb each err by 2^-53 relative, which the factor
 * (1 - 2^-40) covers.  (The weights of region 7 are quotients of positive numbers once va, vb, vc > 0.  A sliver so thin that rounding
 * lets a point reach region 7 with a weight outside [-2^-21, 1 + 2^-21] is beyond this argument; flag bit 0 is the yardstick.)
 */
#ifndef TAMF_MESHDIST_H
#define TAMF_MESHDIST_H

#include <stdint.h>

#include "tamf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TAMF_MESHDIST_TILE 64                      /* triangle records per tile */
#define TAMF_MESHDIST_BOX_MARGIN 9.5367431640625e-07 /* 2^-20: relative inflation of a tile's box */
#define TAMF_MESHDIST_MAX_MESHES 65535
#define TAMF_MESHDIST_NO_CULL 1u                   /* flags bit 0: visit every tile (the yardstick of the culled path) */

/* message of the last failure of a call made by THIS thread ("" when none) */
const char* tamf_meshdist_last_error(void);

/* bytes of device workspace tamf_meshdist_prepare fills for M meshes; the three HOST offset arrays have M + 1 entries, start at 0 and
 * do not decrease: mesh m owns vertices [vert_off[m], vert_off[m+1]), faces [face_off[m], face_off[m+1]) and the entries
 * [perm_off[m], perm_off[m+1]) of the permutation.  Negative tamf_status: M outside [1, 65535], a null or ill-formed offset array, a
 * mesh without a vertex, a face or a valid face (an empty permutation slice), more valid faces than faces. */
int64_t tamf_meshdist_workspace(int32_t M, const int64_t* vert_off_host, const int64_t* face_off_host, const int64_t* perm_off_host);

/* Packs M meshes into `workspace_dev` (one host-to-device copy and one small launch per mesh on `stream`).
 *   verts (V_total,3) f64, faces (F_total,3) int32 with indices local to their mesh: HOST
 *   perm (perm_off[M],) int32 HOST: per mesh the VALID faces (local indices, each at most once) in the order they are packed
 *   scale3 / translate3 (M,3) f64 HOST and hash_resolution: the rescaling of tamf_mesh_contains per mesh, as geometry.mesh_contains
 *     computes it over the faces with indices in [0, V)
 *   workspace: tamf_meshdist_workspace(...) bytes, 16-byte aligned
 * TAMF_ERR_INVALID, nothing copied or launched: whatever tamf_meshdist_workspace refuses, a null pointer, hash_resolution < 2, a
 * workspace too small or misaligned, a permutation entry outside its mesh's faces or listed twice, or one whose face has an index
 * outside [0, V) or a repeated index.  (That a listed face has a positive area is the caller's word: a zero-area face that is listed
 * only costs time, its d2 is that of a segment or point and is still a distance to the surface.) */
int tamf_meshdist_prepare(const double* verts_host, const int32_t* faces_host, int32_t M, const int64_t* vert_off_host,
                          const int64_t* face_off_host, const int32_t* perm_host, const int64_t* perm_off_host, const double* scale3_host,
                          const double* translate3_host, int32_t hash_resolution, void* workspace_dev, int64_t workspace_bytes, void* stream);

/* bytes of device scratch tamf_meshdist_points needs for J jobs (negative tamf_status for J < 1) */
int64_t tamf_meshdist_points_workspace(int32_t J);

/* J jobs (mesh, rigid transform, slice of points) in one launch; the outputs of the jobs lie end to end in job order.
 *   prepared: the workspace tamf_meshdist_prepare filled for M meshes            points (P_total,3) f32 device
 *   mesh_id (J,) int32, transf (J,12) f64 = rows of [R | t], pt_off / pt_len (J,) int64: HOST
 *   jobs_workspace: tamf_meshdist_points_workspace(J) bytes, 16-byte aligned, device
 *   dist_out (sum pt_len,) f64, face_out (sum pt_len,) int32: the original face index, local to the mesh
 *   inside_out (sum pt_len,) uint8 or NULL (distance only)
 * An empty slice writes nothing.  TAMF_ERR_INVALID, nothing launched: a null pointer (inside_out may be null; points may be null when
 * P_total is 0), M outside [1, 65535], J < 1, P_total < 0, mesh_id outside [0, M), a negative offset or length, a slice past
 * P_total, flags with unknown bits, a jobs workspace too small or misaligned. */
int tamf_meshdist_points(const void* prepared_dev, int32_t M, const float* points_dev, int64_t P_total, int32_t J,
                         const int32_t* mesh_id_host, const double* transf_host, const int64_t* pt_off_host, const int64_t* pt_len_host,
                         uint32_t flags, void* jobs_workspace_dev, int64_t jobs_workspace_bytes, double* dist_out_dev, int32_t* face_out_dev,
                         uint8_t* inside_out_dev, void* stream);

/* dist_out[(i R + j) R + k] = distance of the lattice point (ticks[i,0], ticks[j,1], ticks[k,2]) to prepared mesh `mesh`.
 *   ticks (R,3) f64 device, dist_out (R^3,) f64 device.  A work group owns a brick of 8 x 8 x 4 lattice points.
 * TAMF_ERR_INVALID, nothing launched: a null pointer, M outside [1, 65535], mesh outside [0, M), R outside [2, 512], unknown flags. */
int tamf_meshdist_lattice(const void* prepared_dev, int32_t M, int32_t mesh, const double* ticks_dev, int32_t R, uint32_t flags,
                          double* dist_out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TAMF_MESHDIST_H */
