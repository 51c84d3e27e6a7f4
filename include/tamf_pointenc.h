/*
 * tamf_pointenc.h - C-ABI of the native object-embedding encoder (libtamf_pointenc.so): the PointBERT point encoder that turns a
 * point cloud into the 768-vector `obj_embedding` every model of this package conditions on.  Eval mode, float32 throughout.  The
 * weights are the CALLER's: none are part of this package, and nothing here reads a file.
 *
 * What is restated (reference, src/oakink2_tamf/model/pointbert/):
 *   misc.py:40-60            fps - farthest-point sampling (running minimum from 1e10, argmax); its torch.randint start is an ARGUMENT here
 *   dvae.py:107-140          knn_point / square_distance - the group_size nearest points of every centre
 *   dvae.py:150-187          Group.forward - gather, centre subtracted from xyz only, other channels kept
 *   dvae.py:189-221          Encoder - the mini-PointNet (Conv1d, BatchNorm1d, ReLU, Conv1d, max, concat, the same again)
 *   point_encoder.py:32-57   Attention (qkv without bias, scale head_dim^-0.5), :13-29 Mlp (exact GELU), :60-78 Block (pre-LN)
 *   point_encoder.py:97-100  TransformerEncoder.forward - x = block(x + pos): pos is added before EVERY block
 *   point_encoder.py:163-183 PointTransformer.forward - reduce_dim, cls_token / cls_pos, pos_embed(centre), blocks, norm,
 *                            cat(x[:, 0], max over x[:, 1:])  (use_max_pool, cfg.py:12-15)
 *   PointTransformer_8192point_2layer.yaml with cfg.py: trans_dim 384, depth 12, 6 heads, 512 groups of 32, encoder_dims 256,
 *                            point_dims 6, 8192 points
 *
 * Two deliberate differences in the grouping, both without effect on the output where the data is not degenerate:
 *   - the reference ranks neighbours by the expanded form |a|^2 + |b|^2 - 2ab; here it is the direct ((dx*dx + dy*dy) + dz*dz).  The
 *     two can disagree only on near-ties at the group_size-th place.
 *   - the reference's topk is unsorted; here neighbours come in ascending (distance, index) order.  The encoder takes a max over
 *     the group, so its result does not depend on the order of the neighbours.
 *
 * Conventions: those of tamf_hip.h (included for the tamf_status enum only).  Plain C types; every function returns 0 or a negative
 * tamf_status; the message of the calling thread's last failure is tamf_pointenc_last_error().  "dev" pointers are device memory
 * owned by the caller, "host" pointers host memory; `stream` is a hipStream_t passed as void*.  A model belongs to the device that
 * was current at tamf_pointenc_finalize.  Clouds are (B, N, C) float32, C-contiguous, channels [x y z | anything]; indices int32.
 */
#ifndef TAMF_POINTENC_H
#define TAMF_POINTENC_H

#include <stdint.h>

#include "tamf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tamf_pointenc_model tamf_pointenc_model;

typedef struct tamf_pointenc_config {
  int32_t point_dims;   /* 3 or 6 */
  int32_t trans_dim;    /* a multiple of 64, = 64 * num_heads, <= 1024 */
  int32_t depth;        /* >= 1 */
  int32_t num_heads;    /* trans_dim / 64 */
  int32_t num_group;    /* 1 .. 1024 */
  int32_t group_size;   /* 8 .. 64 */
  int32_t encoder_dims; /* a multiple of 16, 16 .. 1024 */
} tamf_pointenc_config;

/* message of the last failure of a call made by THIS thread ("" when none) */
const char* tamf_pointenc_last_error(void);

/* An empty model of this configuration (host only; anything outside the ranges above is TAMF_ERR_INVALID). */
int tamf_pointenc_model_create(const tamf_pointenc_config* cfg, tamf_pointenc_model** model_out);

/* One tensor of the state dict, float32 host memory, read before the call returns.  `key` is the reference's name without the
 * `module.point_encoder.` prefix ("encoder.first_conv.0.weight", "blocks.blocks.3.attn.qkv.weight", "cls_token", ...), `shape` the
 * tensor's own (ndim entries; Conv1d weights are (out, in, 1)).  An unknown key or a wrong shape is TAMF_ERR_INVALID; loading after
 * finalize is TAMF_ERR_STATE.  BatchNorm's num_batches_tracked is not a weight and is not accepted. */
int tamf_pointenc_load_weight(tamf_pointenc_model* model, const char* key, const float* host, int32_t ndim, const int64_t* shape);

/* Checks that every tensor is there (TAMF_ERR_MISSING names the first absent one) and finite (TAMF_ERR_RANGE), folds the two
 * BatchNorm1d of Encoder into the convolutions before them (tamf_pointenc_fold_bn), pads the 3- and 6-wide inputs to a multiple of 4
 * with zeros and uploads everything to the current device.  Synchronises the device once (blocking copies). */
int tamf_pointenc_finalize(tamf_pointenc_model* model);

/* frees the model (NULL is accepted); work enqueued by tamf_pointenc_encode must have finished */
int tamf_pointenc_destroy(tamf_pointenc_model* model);

/* Eval-mode BatchNorm1d folded into the convolution (or linear map) before it, host only:
 *   s = gamma / sqrt(running_var + 1e-5);  w_out[o][i] = s[o] w[o][i];  b_out[o] = (b[o] - running_mean[o]) s[o] + beta[o]
 * composed in float64 from the float32 inputs and rounded once.  w is (out_ch, in_ch), w_out (out_ch, ld_out) with ld_out >= in_ch
 * (columns past in_ch are set to 0).  A non-finite input or running_var + 1e-5 <= 0 is TAMF_ERR_RANGE. */
int tamf_pointenc_fold_bn(const float* w, const float* b, const float* gamma, const float* beta, const float* running_mean,
                          const float* running_var, int32_t out_ch, int32_t in_ch, int32_t ld_out, float* w_out, float* b_out);

/* Farthest-point sampling of G of the N points of each cloud, starting at start_idx[b] (misc.py:40-60): idx_out (B, G), idx_out[b][0] =
 * start_idx[b].  The distance is ((dx*dx + dy*dy) + dz*dz) in float32 with every product and sum rounded on its own (no fused
 * multiply-add: the selection is chaotic in the last bit); the running minimum starts at 1e10; the argmax takes the lowest index
 * among equals.  1 <= G <= N <= 32768, C >= 3, B >= 1.  One workgroup per cloud.  Does not synchronise. */
int tamf_pointenc_fps(const float* points_dev, const int32_t* start_idx_dev, int32_t B, int32_t N, int32_t C, int32_t G,
                      int32_t* idx_out_dev, void* stream);

/* The M nearest points of each centre by the same direct squared distance, the centre itself included: nbr_idx_out (B, G, M) in
 * ascending (distance, index) order.  1 <= M <= N <= 32768.  Does not synchronise. */
int tamf_pointenc_group(const float* points_dev, const int32_t* centre_idx_dev, int32_t B, int32_t N, int32_t C, int32_t G, int32_t M,
                        int32_t* nbr_idx_out_dev, void* stream);

/* bytes of workspace tamf_pointenc_encode needs for B clouds (0 for a bad argument) */
int64_t tamf_pointenc_workspace_bytes(const tamf_pointenc_model* model, int32_t B);

/* The encoder on given groups: points (B, N, point_dims), centre_idx (B, num_group), nbr_idx (B, num_group, group_size), all indices
 * in [0, N) (the caller checks; an index outside is read as 0) -> out (B, 2 * trans_dim) = cat(cls, max over group tokens).  In order:
 * gather with the centre subtracted from xyz only; the mini-PointNet C -> 128 (BN folded, ReLU) -> 256, max over the group, concat,
 * 512 -> 512 (BN folded, ReLU; its global-feature half applied once per group) -> encoder_dims, max over the group; reduce_dim;
 * pos_embed(centre) 3 -> 128, exact GELU, -> trans_dim; cls_token / cls_pos in front; `depth` pre-LN blocks as x = block(x + pos);
 * the final LayerNorm; the pooling.  Every contraction runs on v_mfma_f32_16x16x4_f32 in a fixed K order.  A cloud's output bits
 * depend on that cloud and the model only - not on B or on the cloud's position in the batch.  workspace_dev: 16-byte aligned, at
 * least tamf_pointenc_workspace_bytes(model, B), free to reuse once the enqueued work has finished.  Does not synchronise. */
int tamf_pointenc_encode(const tamf_pointenc_model* model, const float* points_dev, const int32_t* centre_idx_dev,
                         const int32_t* nbr_idx_dev, int32_t B, int32_t N, float* out_dev, void* workspace_dev, int64_t workspace_bytes,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TAMF_POINTENC_H */
