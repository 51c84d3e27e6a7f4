/*
 * tamf_mdmtrain.h - C-ABI of the InterationSegmentMDM training step (libtamf_mdmtrain.so): the training-mode forward of the denoiser G
 * (reference model/interaction_segment_mdm.py:134-174 under train(), the CLIP text features supplied) and the gradient of every
 * parameter with respect to a loss the caller evaluates on the forward's output, computed by HIP kernels for gfx950 in float32.  The
 * call is split in two because the loss (the masked MSE of the diffusion objective, and the hand-interaction terms through MANO and
 * nearest neighbours) sits between the forward and the backward, in the caller's code.  q_sample, the optimiser, gradient clipping
 * and the learning-rate schedule are the caller's.
 *
 * The model, S = T + 5 token rows per clip.  The prefix rows, in order: time_embed.2(SiLU(time_embed.0(pe[t]))), embed_text(text),
 * the hand-side row (rh_embed / lh_embed), shape_embed(mean over the frames of shape), embedding(mean over the objects of obj_emb).
 * The frame rows: input_merge.2(SiLU(input_merge.0(cat(input_process(x_t), obj_input_process(mean over the objects of obj_traj))))).
 * nan_to_num on the prefix rows and on the frame rows, + pe[:S], dropout site 0, the encoder layers, poseFinal on the rows 5 ..,
 * nan_to_num.  The mean over a clip's objects is taken before obj_input_process / obj_embed_process, which are affine.  Every map is
 * evaluated UNCOMPOSED and gets its own gradient; the three nan_to_num pass gradient where their input is finite.  x_t is data and
 * gets no gradient.  cond_mask_prob is not built: the reference's launcher never sets it, so mask_cond is the identity.
 *
 * Parameters are read where the caller keeps them (state-dict layout, device memory) and gradients are written where the caller's
 * gradient tensors live.  Gradients are OVERWRITTEN, never accumulated.
 *
 * Dropout (p in [0, 1)): the scheme and the sites of tamf_refinetrain.h with S = T + 5: site 0 the sum x + PE (S, d); per layer l,
 * site 1 + 4l the attention probabilities (num_heads * S head-major, S), site 2 + 4l the out-projection output (S, d), site 3 + 4l the
 * GELU output (S, ff_size), site 4 + 4l the linear2 output (S, d).  A clip's masks depend on its clip id, not on its place in the
 * batch; p = 0 draws nothing.  The backward regenerates the masks.
 *
 * Reproducible: no floating-point atomics; the same call gives the same bits.  With obj_num_host given, a clip's forward output
 * depends on that clip alone: the same bits alone, in any batch and at any position.
 *
 * Limits: head dimension 64 or 128, i.e. latent_dim = HD * num_heads with latent_dim in [64, 512]; ff_size a multiple of 16 in
 * [16, 4096]; 1 <= num_layers <= 64; input_dim, obj_input_dim, hand_shape_dim, obj_embed_dim and clip_dim each in [1, 4096];
 * 1 <= max_frames <= 1019 (S <= 1024); 1 <= max_batch <= 65535 (a grid dimension); per call 1 <= B <= max_batch, 1 <= T <= max_frames,
 * 1 <= nobj <= 4096, obj_num[b] in [1, nobj], t[b] in [0, 4999] (the rows of sequence_pos_encoder.pe), dropout_p in [0, 1).  Anything
 * else is TAMF_ERR_INVALID, with the limit in the message, and launches nothing; tamf_mdmtrain_create checks before it touches the
 * device.
 *
 * Conventions: those of tamf_hip.h (included for tamf_status and tamf_arch).  Every function returns 0 or a negative tamf_status; the
 * message of the calling thread's last failure is tamf_mdmtrain_last_error().  "dev" pointers are device memory owned by the caller,
 * "host" pointers host memory; `stream` is a hipStream_t passed as void*.  Calls on one context must not overlap.
 */
#ifndef TAMF_MDMTRAIN_H
#define TAMF_MDMTRAIN_H

#include <stdint.h>

#include "tamf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tamf_mdmtrain_ctx tamf_mdmtrain_ctx;

const char* tamf_mdmtrain_last_error(void);

/* A context on `device` for steps of up to max_batch clips of up to max_frames frames; allocates the workspace (the activations the
 * backward reads, the backward's own buffers and the weight-gradient partial sums).  arch->kind and h2o_dim are ignored. */
int tamf_mdmtrain_create(const tamf_arch* arch, int32_t max_batch, int32_t max_frames, int32_t device, tamf_mdmtrain_ctx** out);
void tamf_mdmtrain_destroy(tamf_mdmtrain_ctx* ctx);

/* One state-dict tensor of InterationSegmentMDM, float32 device memory that stays valid and in place until the context is destroyed
 * or the name is bound again.  Trainable tensors take grad_dev of the same shape; the buffers "hand_side_process.rh_embed",
 * "hand_side_process.lh_embed" and "sequence_pos_encoder.pe" take grad_dev = NULL (the timestep embedder reads the same table).  An
 * unknown name or a wrong shape is TAMF_ERR_INVALID. */
int tamf_mdmtrain_bind(tamf_mdmtrain_ctx* ctx, const char* name, const float* param_dev, float* grad_dev, const int64_t* shape, int32_t ndim);

/* The training forward of one batch; does not synchronise.  Keeps the activations in the context for ONE tamf_mdmtrain_backward.
 *   obj_num_host  [B] object counts, or NULL: the mean over all nobj (padded) rows - the reference's forward
 *   t_host        [B] int32 timesteps, each in [0, 5000)
 *   x_t (B, T, input_dim), text_emb (B, clip_dim), shape (B, T, hand_shape_dim), hand_side [B] uint8 (0 rh, 1 lh), obj_emb (B, nobj,
 *   obj_embed_dim), obj_traj (B, nobj, T, obj_input_dim): device; x_t and text_emb are read again by the backward and must stay valid
 *   and unchanged until then
 *   clip_id_host  [B] int64 keys of the dropout masks, or NULL: b
 *   model_out_dev (B, T, input_dim)
 * A tensor that was never bound is TAMF_ERR_MISSING, naming it. */
int tamf_mdmtrain_forward(tamf_mdmtrain_ctx* ctx, int32_t B, int32_t T, int32_t nobj, const int32_t* obj_num_host, const int32_t* t_host,
                          const float* x_t_dev, const float* text_emb_dev, const float* shape_dev, const uint8_t* hand_side_dev,
                          const float* obj_emb_dev, const float* obj_traj_dev, const int64_t* clip_id_host, float dropout_p, uint64_t seed,
                          uint32_t step, float* model_out_dev, void* stream);

/* The gradient of every bound parameter from grad_model_out (B, T, input_dim) of the preceding forward; does not synchronise.
 * TAMF_ERR_STATE without a preceding forward on the context (a forward serves one backward). */
int tamf_mdmtrain_backward(tamf_mdmtrain_ctx* ctx, const float* grad_model_out_dev, void* stream);

/* Measurement: with `on`, every kernel launch of forward and backward is bracketed by a pair of events, which serialises nothing but
 * costs host time - leave it off otherwise.  tamf_mdmtrain_get_profile waits for the recorded work, writes one line
 * "name<TAB>launches<TAB>milliseconds" per kind of kernel since the last read into out (size bytes, NUL-terminated) and forgets the
 * events. */
int tamf_mdmtrain_set_profile(tamf_mdmtrain_ctx* ctx, int32_t on);
int tamf_mdmtrain_get_profile(tamf_mdmtrain_ctx* ctx, char* out, int64_t size);

/* The keep-mask (1 keep, 0 drop) the step uses at `site` for the clip with this id: rows x cols uint8, row-major. */
int tamf_mdmtrain_dropout_mask(uint64_t seed, uint32_t step, int64_t clip_id, int32_t site, int32_t rows, int32_t cols, float p,
                               uint8_t* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
