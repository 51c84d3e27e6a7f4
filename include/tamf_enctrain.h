/*
 * tamf_enctrain.h - C-ABI of the SegmentEncoder training step (libtamf_enctrain.so): the training-mode forward of the FID score's
 * encoder (reference model/segment_encoder.py:77-111 under train()), the cross-entropy of its `activation` against action labels
 * (SegmentEncoderLoss's `ce`) and the gradient of that loss with respect to every parameter, computed by HIP kernels for gfx950 in
 * float32.  The optimiser, gradient clipping and the learning-rate schedule are the caller's (any torch.optim optimiser steps on the
 * gradients this writes).
 *
 * The model is evaluated on the UNCOMPOSED maps: input_process, obj_input_process and input_merge.0 each get their own gradient.
 * The mean over a clip's objects is taken before obj_input_process / obj_embed_process, which are affine (the same function and the
 * same gradients as the mean of the per-object embeddings).  nan_to_num passes gradient where its input is finite.  The last layer
 * computes the query path, out-projection, LayerNorms and feed-forward block of the classification row alone.
 *
 * Parameters are read where the caller keeps them (state-dict layout, device memory) and gradients are written where the caller's
 * gradient tensors live: a step needs no repack and no host copy.  Gradients are OVERWRITTEN, never accumulated.
 *
 * Dropout (p in [0, 1)) at five kinds of site, placed by the published definitions of PositionalEncoding and
 * nn.TransformerEncoderLayer: site 0 the sum x + PE (rows S, cols 64); per layer l, site 1 + 4l the attention probabilities (rows
 * 4 * S: head-major, cols S), site 2 + 4l the out-projection output (S, 64), site 3 + 4l the GELU output (S, ff_size), site 4 + 4l the
 * linear2 output (S, 64).  S = T + 4 token rows (3 prefix rows, T frames, the classification token).  The keep-mask of element
 * e = row * cols + col is word (e & 3) of Philox4x32-10 at counter (e >> 2, step, clip_id low, clip_id high) under key
 * (seed low ^ site * 0x9E3779B1, seed high), kept when >= floor(p * 2^32); kept values are scaled by 1 / (1 - p).  A clip's masks
 * depend on its clip id, not on its place in the batch.  The backward regenerates the masks.  p = 0 keeps everything without drawing and
 * scales by exactly 1: the same kernels, the bits of a call whose draws all keep, and the bits of no dropout.
 *
 * Reproducible: no floating-point atomics; the same call gives the same bits.  A clip's forward depends on that clip alone.
 *
 * Limits: latent_dim 64 with 4 heads, ff_size a multiple of 16 in [16, 512], 1 <= num_layers <= 64, input_dim, obj_input_dim,
 * hand_shape_dim and obj_embed_dim each in [1, 4096], 1 <= max_frames <= 508 (one head's keys and values of the T + 4 token rows in
 * 64 KiB of LDS), 1 <= max_batch <= 65535 (a grid dimension); per step 1 <= B <= max_batch, 1 <= T <= max_frames, 1 <= nobj <= 4096,
 * obj_num[b] in [1, nobj], dropout_p in [0, 1).  Anything else is TAMF_ERR_INVALID and launches nothing.
 *
 * Conventions: those of tamf_hip.h (included for tamf_status and tamf_arch).  Every function returns 0 or a negative tamf_status; the
 * message of the calling thread's last failure is tamf_enctrain_last_error().  "dev" pointers are device memory owned by the caller,
 * "host" pointers host memory; `stream` is a hipStream_t passed as void*.  Calls on one context must not overlap.
 */
#ifndef TAMF_ENCTRAIN_H
#define TAMF_ENCTRAIN_H

#include <stdint.h>

#include "tamf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tamf_enctrain_ctx tamf_enctrain_ctx;

const char* tamf_enctrain_last_error(void);

/* A context on `device` for steps of up to max_batch clips of up to max_frames frames; allocates the per-clip workspace (the
 * activations the backward reads) and the weight-gradient partial sums.  arch->kind, clip_dim and h2o_dim are ignored. */
int tamf_enctrain_create(const tamf_arch* arch, int32_t max_batch, int32_t max_frames, int32_t device, tamf_enctrain_ctx** out);
void tamf_enctrain_destroy(tamf_enctrain_ctx* ctx);

/* One state-dict tensor, float32 device memory that stays valid and in place until the context is destroyed or the name is bound
 * again.  Trainable tensors (every parameter of the reference's key set) take grad_dev of the same shape; the buffers
 * "classification_token", "hand_side_process.rh_embed", "hand_side_process.lh_embed" and "sequence_pos_encoder.pe" take
 * grad_dev = NULL.  An unknown name or a wrong shape is TAMF_ERR_INVALID. */
int tamf_enctrain_bind(tamf_enctrain_ctx* ctx, const char* name, const float* param_dev, float* grad_dev, const int64_t* shape, int32_t ndim);

/* The training forward, loss and gradients of one batch; does not synchronise.
 *   obj_num_host  [B] object counts, or NULL: the mean over all nobj (padded) rows - as tamf_encode
 *   pose (B, T, input_dim), shape (B, T, hand_shape_dim), hand_side [B] uint8 (0 rh, 1 lh), obj_emb (B, nobj, obj_embed_dim),
 *   obj_traj (B, nobj, T, obj_input_dim): device;  labels_dev [B] int64 in [0, input_dim) (the caller checks the range)
 *   clip_id_host  [B] int64 keys of the dropout masks, or NULL: b
 *   loss_out_dev  1 float: mean_b CE(activation[b], labels[b]);  activation_out_dev (B, input_dim)
 * A tensor that was never bound is TAMF_ERR_MISSING, naming it; B > max_batch or T > max_frames is TAMF_ERR_INVALID. */
int tamf_enctrain_step(tamf_enctrain_ctx* ctx, int32_t B, int32_t T, int32_t nobj, const int32_t* obj_num_host, const float* pose_dev,
                       const float* shape_dev, const uint8_t* hand_side_dev, const float* obj_emb_dev, const float* obj_traj_dev,
                       const int64_t* labels_dev, const int64_t* clip_id_host, float dropout_p, uint64_t seed, uint32_t step,
                       float* loss_out_dev, float* activation_out_dev, void* stream);

/* The keep-mask (1 keep, 0 drop) the step uses at `site` for the clip with this id: rows x cols uint8, row-major. */
int tamf_enctrain_dropout_mask(uint64_t seed, uint32_t step, int64_t clip_id, int32_t site, int32_t rows, int32_t cols, float p,
                               uint8_t* out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif
