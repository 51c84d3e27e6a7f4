/*
 * tamf_refinetrain.h - C-ABI of the SegmentRefineModel training step (libtamf_refinetrain.so): the training-mode forward of the
 * refiner's trunk (reference model/segment_refine_model.py:175-217 under train(), the hand->object distance feature supplied) and
 * the gradient of every parameter with respect to a loss the caller evaluates on the forward's output, computed by HIP kernels for
 * gfx950 in float32.  The call is split in two because the refiner's loss (MANO, nearest neighbours, float64 reductions) sits between
 * the trunk's forward and its backward, in the caller's code.  The optimiser, gradient clipping and the learning-rate schedule are
 * the caller's.
 *
 * The model is evaluated on the UNCOMPOSED maps: input_process, obj_input_process, h2o_dist_input_process and input_merge.0 each get
 * their own gradient.  The mean over a clip's objects is taken before obj_input_process / obj_embed_process, which are affine.  The
 * three nan_to_num (prefix rows, frame rows, output) pass gradient where their input is finite.
 *
 * Parameters are read where the caller keeps them (state-dict layout, device memory) and gradients are written where the caller's
 * gradient tensors live.  Gradients are OVERWRITTEN, never accumulated.
 *
 * Dropout (p in [0, 1)): the scheme of tamf_enctrain.h (Philox4x32-10, counter (e >> 2, step, clip id low, high), key (seed low ^
 * site * 0x9E3779B1, seed high), keep when >= floor(p * 2^32), scale 1 / (1 - p); p = 0 draws nothing and multiplies by exactly 1).
 * Sites, with S = T + 3 token rows (3 prefix rows, T frames) and d = latent_dim: site 0 the sum x + PE (S, d); per layer l, site
 * 1 + 4l the attention probabilities (num_heads * S head-major, S), site 2 + 4l the out-projection output (S, d), site 3 + 4l the
 * GELU output (S, ff_size), site 4 + 4l the linear2 output (S, d).  A clip's masks depend on its clip id, not on its place in the
 * batch.  The backward regenerates the masks.
 *
 * Reproducible: no floating-point atomics; the same call gives the same bits.  With obj_num_host given, a clip's forward output
 * depends on that clip alone: the same bits alone, in any batch and at any position.
 *
 * Limits: head dimension 64, i.e. latent_dim = 64 * num_heads with 1 <= num_heads <= 8; ff_size a multiple of 16 in [16, 4096];
 * 1 <= num_layers <= 64; input_dim, obj_input_dim, hand_shape_dim, obj_embed_dim and h2o_dim each in [1, 4096]; 1 <= max_frames <=
 * 1021 (S <= 1024: no kernel keeps a sequence in LDS, the bound is the range the element counters are sized for); 1 <= max_batch <=
 * 65535 (a grid dimension); per call 1 <= B <= max_batch, 1 <= T <= max_frames, 1 <= nobj <= 4096, obj_num[b] in [1, nobj],
 * dropout_p in [0, 1).  Anything else is TAMF_ERR_INVALID, with the limit in the message, and launches nothing.
 *
 * Conventions: those of tamf_hip.h (included for tamf_status and tamf_arch).  Every function returns 0 or a negative tamf_status; the
 * message of the calling thread's last failure is tamf_refinetrain_last_error().  "dev" pointers are device memory owned by the
 * caller, "host" pointers host memory; `stream` is a hipStream_t passed as void*.  Calls on one context must not overlap.
 */
#ifndef TAMF_REFINETRAIN_H
#define TAMF_REFINETRAIN_H

#include <stdint.h>

#include "tamf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tamf_refinetrain_ctx tamf_refinetrain_ctx;

const char* tamf_refinetrain_last_error(void);

/* A context on `device` for steps of up to max_batch clips of up to max_frames frames; allocates the workspace (the activations the
 * backward reads, the backward's own buffers and the weight-gradient partial sums).  arch->kind and clip_dim are ignored. */
int tamf_refinetrain_create(const tamf_arch* arch, int32_t max_batch, int32_t max_frames, int32_t device, tamf_refinetrain_ctx** out);
void tamf_refinetrain_destroy(tamf_refinetrain_ctx* ctx);

/* One state-dict tensor of SegmentRefineModel, float32 device memory that stays valid and in place until the context is destroyed or
 * the name is bound again.  Trainable tensors take grad_dev of the same shape; the buffers "hand_side_process.rh_embed",
 * "hand_side_process.lh_embed" and "sequence_pos_encoder.pe" take grad_dev = NULL.  An unknown name or a wrong shape is
 * TAMF_ERR_INVALID. */
int tamf_refinetrain_bind(tamf_refinetrain_ctx* ctx, const char* name, const float* param_dev, float* grad_dev, const int64_t* shape, int32_t ndim);

/* The training forward of one batch; does not synchronise.  Keeps the activations in the context for ONE tamf_refinetrain_backward.
 *   obj_num_host  [B] object counts, or NULL: the mean over all nobj (padded) rows - the reference's forward
 *   sample_pose (B, T, input_dim), h2o_dist (B, T, h2o_dim), shape (B, T, hand_shape_dim), hand_side [B] uint8 (0 rh, 1 lh),
 *   obj_emb (B, nobj, obj_embed_dim), obj_traj (B, nobj, T, obj_input_dim): device; sample_pose and h2o_dist are read again by the
 *   backward and must stay valid and unchanged until then
 *   clip_id_host  [B] int64 keys of the dropout masks, or NULL: b
 *   refine_pose_out_dev (B, T, input_dim)
 * A tensor that was never bound is TAMF_ERR_MISSING, naming it. */
int tamf_refinetrain_forward(tamf_refinetrain_ctx* ctx, int32_t B, int32_t T, int32_t nobj, const int32_t* obj_num_host,
                             const float* sample_pose_dev, const float* h2o_dist_dev, const float* shape_dev, const uint8_t* hand_side_dev,
                             const float* obj_emb_dev, const float* obj_traj_dev, const int64_t* clip_id_host, float dropout_p, uint64_t seed,
                             uint32_t step, float* refine_pose_out_dev, void* stream);

/* The gradient of every bound parameter from grad_refine_pose (B, T, input_dim) of the preceding forward; does not synchronise.
 * TAMF_ERR_STATE without a preceding forward on the context (a forward serves one backward). */
int tamf_refinetrain_backward(tamf_refinetrain_ctx* ctx, const float* grad_refine_pose_dev, void* stream);

/* Measurement (tools/refinetrain_bench.py): with `on`, every kernel launch of forward and backward is bracketed by a pair of events,
 * which serialises nothing but costs host time - leave it off otherwise.  tamf_refinetrain_get_profile waits for the recorded work,
 * writes one line "name<TAB>launches<TAB>milliseconds" per kind of kernel since the last read into out (size bytes, NUL-terminated)
 * and forgets the events. */
int tamf_refinetrain_set_profile(tamf_refinetrain_ctx* ctx, int32_t on);
int tamf_refinetrain_get_profile(tamf_refinetrain_ctx* ctx, char* out, int64_t size);

/* The keep-mask (1 keep, 0 drop) the step uses at `site` for the clip with this id: rows x cols uint8, row-major. */
int tamf_refinetrain_dropout_mask(uint64_t seed, uint32_t step, int64_t clip_id, int32_t site, int32_t rows, int32_t cols, float p,
                                  uint8_t* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
