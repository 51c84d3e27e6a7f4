/*
 * tamf_mano.h - C-ABI of the native MANO hand layer (libtamf_mano.so): forward kinematics + linear blend skinning of the MANO hand
 * model on the GPU, and their backward, from model arrays the CALLER supplies.  The MANO assets are licence-gated and are not part of this package;
 * nothing here reads a file.
 *
 * What is implemented is the published definition, not a port of a particular code base:
 *
 *   SMPL: Loper, Mahmood, Romero, Pons-Moll, Black, "SMPL: A Skinned Multi-Person Linear Model", SIGGRAPH Asia 2015 - eq. 2-4
 *         (blend skinning with the rest pose removed), eq. 8-10 (shape / pose blend shapes, joint regression from the shaped mesh)
 *   MANO: Romero, Tzionas, Black, "Embodied Hands", SIGGRAPH Asia 2017, section 3 - the same model with 16 joints, 778 vertices,
 *         10 shape and 135 pose blend-shape coefficients
 *
 * in the configuration the reference pipeline uses its hand layer in (its call sites: model/segment_refine_model.py:107-140,
 * launch/sample_refine.py:175-194, compute_score/compute_score_cr.py:189-208, 259-261 and the same lines of _psklj / _siv): quaternion pose (w, x, y, z), no PCA, flat hand
 * mean, joints = 16 chain joints + 5 fingertip vertices in a 21-joint order, optionally centred on one joint.  The fingertip vertex
 * ids, the joint order and the centre are DATA of the model (defaults: the published manopth convention), not constants of the
 * kernel.  Parity with the manotorch package itself has not been verified (its source was not available to this project).
 *
 * Conventions: those of tamf_hip.h (included for the tamf_status enum only).  Plain C types; every function returns 0 or a negative
 * tamf_status; the message of the calling thread's last failure is tamf_mano_last_error().  "dev" pointers are device memory owned by
 * the caller, "host" pointers host memory; `stream` is a hipStream_t passed as void*.  A model belongs to the device that was current
 * when it was created.
 */
#ifndef TAMF_MANO_H
#define TAMF_MANO_H

#include <stdint.h>

#include "tamf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tamf_mano_model tamf_mano_model;

/* message of the last failure of a call made by THIS thread ("" when none) */
const char* tamf_mano_last_error(void);

/* Upload one hand model (SMPL eq. 8-10 / MANO section 3: template, blend shapes, joint regressor, skinning weights, kinematic tree).
 * All arrays are HOST memory, C-contiguous, float64 as in the published model files, and are read before the call returns:
 *   v_template (V,3)   shapedirs (V,3,10)   posedirs (V,3,135)   J_regressor (16,V)   weights (V,16)
 *   parents (16,) int32: parents[0] < 0 (the root), 0 <= parents[j] < j otherwise
 *   tip_ids (5,) int32 vertex ids of the fingertips, or NULL: 745, 317, 444, 556, 673
 *   joint_order (21,) int32, a permutation of 0..20 over (16 chain joints | 5 tips), or NULL:
 *                0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20
 *   center_idx: index into the 21 OUTPUT joints that is subtracted from vertices and joints, or -1 for none
 * J_template = J_regressor . v_template and J_dirs = J_regressor . shapedirs are composed here in float64 (so that
 * J = J_template + J_dirs . betas, SMPL eq. 10 on the shaped mesh); everything is then rounded to float32, the two blend-shape bases
 * stacked into one (K = 145) per coordinate.  1 <= V <= 1024; a non-finite value, a bad tree / id / permutation or a null pointer
 * is TAMF_ERR_INVALID.  Synchronises the device once (blocking copies). */
int tamf_mano_model_create(int32_t V, const double* v_template, const double* shapedirs, const double* posedirs,
                           const double* J_regressor, const double* weights, const int32_t* parents, const int32_t* tip_ids,
                           const int32_t* joint_order, int32_t center_idx, tamf_mano_model** model_out);

/* frees the device arrays (NULL is accepted); work enqueued by tamf_mano_forward / tamf_mano_backward must have finished */
int tamf_mano_model_destroy(tamf_mano_model* model);

/* Tuning only: 16-frame tiles a workgroup keeps per basis fragment (1, 2 or 4; 0 = the built-in choice).  No output bit depends on it. */
int tamf_mano_model_set_tiles(tamf_mano_model* model, int32_t m_tiles);

/* The layer's forward (SMPL eq. 2-4 with the blend shapes of eq. 8-9; joints as described above), enqueued on `stream`:
 *   quat (N,16,4) f32 device, (w,x,y,z), normalised here as q / max(|q|, 1e-12); 16-byte aligned      betas (N,10) f32 device
 *   verts_out (N,V,3) f32 device          joints_out (N,21,3) f32 device, or NULL
 * The quaternions may have any length whose square float32 holds: |q| up to 1.8e19 (sqrt of FLT_MAX) is in the contract and a zero
 * quaternion is the identity rotation; above that the float32 norm overflows, the joint gets the identity rotation -
 * outside the contract, as are non-finite inputs (which spoil the outputs of their own frame only).
 * fp32 throughout; the blend-shape contraction runs on v_mfma_f32_16x16x4_f32 in a fixed K order.  A frame's output bits depend
 * on its own inputs and the model only - not on N, on its position in the batch or on the launch.  N = 0 launches nothing; N < 0 or
 * a null pointer is TAMF_ERR_INVALID.  Does not synchronise. */
int tamf_mano_forward(const tamf_mano_model* model, const float* quat_dev, const float* betas_dev, int64_t N, float* verts_out_dev,
                      float* joints_out_dev, void* stream);

/* The layer's backward: the vector-Jacobian product of exactly the function tamf_mano_forward computes, enqueued on `stream`.
 *   quat, betas: the forward's inputs (quat 16-byte aligned); nothing is kept from a forward call, what is needed is recomputed
 *   dverts (N,V,3) f32 device or NULL, djoints (N,21,3) f32 device or NULL: the upstream gradients of verts_out / joints_out;
 *                NULL means zeros, both NULL is TAMF_ERR_INVALID
 *   dquat_out (N,16,4) f32 device, 16-byte aligned: with respect to the input as given (the normalisation is differentiated too)
 *   dbetas_out (N,10) f32 device, or NULL
 * Covers the joint permutation, the fingertip rows (their gradient lands on the fingertip vertices) and the centre (minus the sum of
 * all upstream rows, on the centre joint or fingertip).  No gradients with respect to the model arrays.  Outputs are overwritten.
 * fp32 throughout; the contractions over the vertices run on v_mfma_f32_16x16x4_f32 in partial sums of a fixed order; no atomics.
 * A frame's gradient bits depend on its own inputs and the model only - not on N, on its position in the batch, on the launch or
 * on tamf_mano_model_set_tiles.  N = 0 launches nothing; N < 0 or a null mandatory pointer is TAMF_ERR_INVALID.  Does not synchronise. */
int tamf_mano_backward(const tamf_mano_model* model, const float* quat_dev, const float* betas_dev, int64_t N, const float* dverts_dev,
                       const float* djoints_dev, float* dquat_out_dev, float* dbetas_out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TAMF_MANO_H */
