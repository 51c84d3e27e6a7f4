/*
 * tamf_eval.h - C-ABI of the evaluation kernels that have no context (libtamf_eval.so): the Solid Intersection Volume score.
 *
 * The sampler library (tamf_hip.h) is the reference's two call contracts and stays that; score kernels need no weights, no
 * workspaces owned by the library and no hipGraph, so they live here.  Reference interfaces (paths relative to src/ and script/):
 *
 *   process_sdf: sign of the SDF on the lattice    dev_fn/util/sdf_util.py:59-99           -> tamf_voxelize_lattice
 *   solid_intersection_volume, per frame / object  compute_score/compute_score_siv.py:128-155 -> tamf_mesh_contains_count
 *
 * Conventions: those of tamf_hip.h.  Plain C types; every function returns 0 or a negative tamf_status (tamf_hip.h, included for
 * that enum only); the message of the calling thread's last failure is tamf_eval_last_error().  "dev" pointers are device memory
 * owned by the caller, "host" pointers host memory; `stream` is a hipStream_t passed as void*; the work is enqueued on it and no
 * call synchronises the device (tamf_mesh_contains_count copies its job arrays from pageable host memory: see there).  No state is
 * kept between calls.
 *
 * Containment is the test of tamf_mesh_contains (dev_fn/external/libmesh/inside_mesh.py:8-149): float64, the reference's operation
 * order, no fused multiply-adds.  Both entry points give the booleans / counts that tamf_mesh_contains gives on the same points.
 */
#ifndef TAMF_EVAL_H
#define TAMF_EVAL_H

#include <stdint.h>

#include "tamf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* message of the last failure of a call made by THIS thread ("" when none) */
const char* tamf_eval_last_error(void);

/* Inside test of a closed mesh on an R x R x R lattice, one work item per lattice COLUMN (i, j): the 2D triangle test and the
 * intersection depth do not depend on k, so they are evaluated F * R^2 times, not F * R^3.
 *   verts (V,3) f64, faces (F,3) int32, device            ticks (R,3) f64 device: the tick values of the three axes
 *   scale3 / translate3: HOST, as for tamf_mesh_contains  tri_workspace: 16 * F doubles (device scratch)
 *   mask_out (R*R*R,) uint8: lattice point (ticks[i,0], ticks[j,1], ticks[k,2]) at index (i*R + j)*R + k, 1 = inside
 * mask_out equals tamf_mesh_contains on the same R^3 points byte for byte.  2 <= R <= 512, F >= 1, hash_resolution >= 2;
 * anything else, or a null pointer, is TAMF_ERR_INVALID and launches nothing. */
int tamf_voxelize_lattice(const double* verts_dev, const int32_t* faces_dev, int32_t n_faces, const double* ticks_dev, int32_t R,
                          const double* scale3, const double* translate3, int32_t hash_resolution, double* tri_workspace_dev,
                          uint8_t* mask_out_dev, void* stream);

/* bytes of device workspace tamf_mesh_contains_count needs for M meshes of F faces and J jobs (negative tamf_status on bad sizes) */
int64_t tamf_mesh_contains_count_workspace(int32_t M, int32_t F, int32_t J);

/* count[j] = number of points p of the slice [pt_off[j], pt_off[j] + pt_len[j]) of points_dev that lie inside mesh mesh_id[j]
 * after the rigid transform q = R p + t of the job.
 *   verts (M,V,3) f32 device, faces (F,3) int32 device (shared by the M meshes; indices < V)
 *   points (P_total,3) f64 device, object frame
 *   mesh_id (J,) int32, transf (J,12) f64 = rows of [R | t], pt_off / pt_len (J,) int64: HOST arrays, read before the call returns
 *     (one stream-ordered host-to-device copy from pageable memory: the runtime may hold the caller until the work queued earlier
 *     on `stream` has drained; nothing else waits, and the counts are not read back)
 *   workspace: tamf_mesh_contains_count_workspace(M, F, J) bytes, 16-byte aligned          count_out (J,) int64 device
 * Per mesh the rescaling box is taken on the device over the vertices the faces reference (f32 -> f64 is exact),
 * scale = (hash_resolution - 1) / (max - min), translate = 0.5 - scale * min in float64 (IEEE division); the query point is
 * ((R00 x + R01 y) + R02 z) + t0 (rows 1, 2 alike) in float64 without contraction.  Partial counts are combined with integer adds
 * only: count[j] depends neither on J, nor on the order of the jobs, nor on the launch geometry.  An empty slice counts 0.
 * M, V, F, J >= 1; mesh_id outside [0, M), a negative offset / length, a slice past P_total, or a null pointer: TAMF_ERR_INVALID,
 * nothing is launched. */
int tamf_mesh_contains_count(const float* verts_dev, int32_t M, int32_t V, const int32_t* faces_dev, int32_t F,
                             const double* points_dev, int64_t P_total, int32_t J, const int32_t* mesh_id_host,
                             const double* transf_host, const int64_t* pt_off_host, const int64_t* pt_len_host,
                             int32_t hash_resolution, void* workspace_dev, int64_t workspace_bytes, int64_t* count_out_dev,
                             void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TAMF_EVAL_H */
