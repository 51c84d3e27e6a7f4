/*
 * tamf_surface.h - C-ABI of the surface sampler (libtamf_surface.so): points drawn uniformly by area from a triangle mesh, defined bit
 * for bit, so that the same mesh, seed and key give the same point cloud on every machine.  It is the first stage of the object
 * chain: <obj_pointcloud_prefix>/<obj_id>.npz["point"] is made from these samples (launch/sample_object_points.py).
 *
 * Conventions: those of tamf_hip.h (included for the tamf_status enum only).  Plain C types; every function returns 0 or a negative
 * tamf_status; the message of the calling thread's last failure is tamf_surface_last_error().  "dev" pointers are device memory owned
 * by the caller, on the current device; `stream` is a hipStream_t passed as void*, the work is enqueued on it.  No state is kept
 * between calls.  tamf_surface_sample synchronises `stream` ONCE (see there); nothing else waits.
 *
 * THE DEFINITION.  Everything is computed in float64 without fused multiply-adds (fp contract off); float32 vertices are widened
 * exactly; every sum below is evaluated left to right as written.
 *
 *   Area.   c = (v1 - v0) x (v2 - v0), c.x = e1.y e2.z - e1.z e2.y (and cyclic), area[f] = 0.5 * sqrt((c.x^2 + c.y^2) + c.z^2).
 *           A face with an index outside [0, V), or with a non-finite area, has area 0.
 *   CDF.    cdf[f] is the inclusive prefix sum of area, total = cdf[F-1].  The summation order is fixed and depends on F alone:
 *           faces are taken in blocks of TAMF_SURFACE_SCAN_BLOCK = 1024 consecutive faces; in a block, thread t of 256 owns the
 *           TAMF_SURFACE_SCAN_ITEMS = 4 consecutive faces 4t .. 4t+3 and sums them one after the other (l_0 .. l_3, l_3 its total);
 *           the 64 lanes of a wave chain their totals one after the other from 0 (base_{t+1} = base_t + total_t); the 4 waves of a
 *           block chain their totals the same way; the blocks chain theirs the same way, in one fixed carry pass (block 0 first):
 *               cdf[f] = carry_block + (base_wave + (base_lane + l_k))
 *           Every base is the LAST value of the group before it, bit for bit, and every area is >= 0, so the CDF is non-decreasing.
 *           An element's value has passed through at most f roundings, each of a partial sum: |cdf[f] - exact| <= F * 2^-53 * total
 *           (to first order).  The same input gives the same bits whatever M, first_sample and the launch geometry of the sampling.
 *   Draw.   Sample i = first_sample + m draws the Philox4x32-10 block with counter (i_lo, i_hi, key_lo, key_hi) under key
 *           (seed_lo, seed_hi) -> r0 .. r3 (uint32):
 *               u_f = (((r0 << 21) | (r1 >> 11)) + 0.5) * 2^-53     (the sum in float64: above 2^52 it rounds to even)
 *               u_1 = (r2 + 0.5) * 2^-32          u_2 = (r3 + 0.5) * 2^-32
 *   Face.   x = u_f * total; the smallest j with cdf[j] > x, by binary search.  A zero-area face can therefore never be picked.
 *           When no such j exists (x rounded up to total: probability about 2^-53) the smallest j with cdf[j] >= total is taken,
 *           the last face of positive area.
 *   Point.  s = sqrt(u_1); w = (1 - s, s (1 - u_2), s u_2); p = (w0 v0 + w1 v1) + w2 v2 per coordinate, rounded once to float32.
 *   Normal. c / sqrt((c.x^2 + c.y^2) + c.z^2) of the picked face, rounded once to float32.
 *
 * What follows: sample i depends on (mesh, seed, key, i) alone - not on M, not on how a range of samples is split over calls with
 * first_sample; the same call gives the same bits.  No atomics anywhere.
 */
#ifndef TAMF_SURFACE_H
#define TAMF_SURFACE_H

#include <stdint.h>

#include "tamf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TAMF_SURFACE_SCAN_BLOCK 1024 /* faces one workgroup scans: 256 threads x TAMF_SURFACE_SCAN_ITEMS */
#define TAMF_SURFACE_SCAN_ITEMS 4    /* consecutive faces one thread sums */
#define TAMF_SURFACE_MAX_FACES (1 << 26)
#define TAMF_SURFACE_MAX_SAMPLES 2147483647

/* message of the last failure of a call made by THIS thread ("" when none) */
const char* tamf_surface_last_error(void);

/* bytes of device workspace tamf_surface_sample needs for a mesh of F faces (the CDF, the block carries, the total); a negative
 * tamf_status for F outside [1, TAMF_SURFACE_MAX_FACES] */
int64_t tamf_surface_workspace_bytes(int32_t F);

/* M samples i = first_sample .. first_sample + M - 1 of the mesh, as defined above.
 *   verts (V,3) f32, faces (F,3) int32: device.  Face indices are NOT trusted: a face with one outside [0, V) has area 0.
 *   points_out (M,3) f32; normals_out (M,3) f32 or NULL; face_out (M,) int32 or NULL: device
 *   workspace: tamf_surface_workspace_bytes(F) bytes, 16-byte aligned, device; overwritten
 * The CDF is built on `stream` (three launches that write the workspace only); `total` has to be known on the host before anything
 * is drawn, so the call then copies it back and SYNCHRONISES `stream` once (it cannot be captured into a hipGraph), and launches the
 * sampling kernel, which is not waited for.
 * TAMF_ERR_INVALID: a null pointer (normals_out and face_out may be null), V < 1, F outside [1, 2^26], M outside [1, 2^31 - 1],
 * first_sample < 0 or first_sample + M past 2^63 - 1, a workspace too small or misaligned - nothing is launched; total == 0 (every
 * face degenerate) or non-finite - the sampling kernel is not launched.  In every such case the outputs are untouched. */
int tamf_surface_sample(const float* verts_dev, const int32_t* faces_dev, int32_t V, int32_t F, int64_t M, uint64_t seed, uint64_t key,
                        int64_t first_sample, float* points_out_dev, float* normals_out_dev, int32_t* face_out_dev, void* workspace_dev,
                        int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TAMF_SURFACE_H */
