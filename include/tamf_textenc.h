/*
 * tamf_textenc.h - C-ABI of the native text encoder (libtamf_textenc.so): the text tower of CLIP (Radford et al. 2021; ViT-B/32's
 * text side by default) that turns a tokenised prompt into the 512-vector `text_embedding` every model of this package conditions
 * on.  Inference only, float32 activations throughout.  The weights are the CALLER's: none are part of this package, and nothing here
 * reads a file.
 *
 * What is restated (the published model definition; the reference calls it through the `clip` package,
 * src/oakink2_tamf/model/interaction_segment_mdm.py:84-132):
 *   x = token_embedding[ids] + positional_embedding[:ctx]
 *   num_layers pre-LN residual blocks:
 *     x += out_proj(MHA(ln_1(x)))              additive causal mask (upper triangle -inf), packed in_proj_weight (3W, W) + bias,
 *                                              heads of 64, scale 64^-0.5
 *     x += c_proj(QuickGELU(c_fc(ln_2(x))))    QuickGELU(v) = v * sigmoid(1.702 v), hidden width 4W
 *   out[b] = ln_final(x)[b, argmax(ids[b])] @ text_projection      (the first index among equals; (W, E), no bias)
 *   LayerNorm eps 1e-5.
 * The causal mask makes the row at the EOT position a function of the positions at or before it: a prompt costs eot + 1 rows, and
 * whatever follows the EOT id (the reference pads with zeros) cannot change a bit of the result.
 *
 * Arithmetic.  The reference's convert_weights turns the Linear and attention parameters (weights and biases) and text_projection
 * into fp16, leaves the embeddings and the LayerNorm parameters in fp32, and then runs fp16 activations.  Here activations are
 * float32; `round_fp16` rounds those same tensors to fp16 at finalize (a no-op for a checkpoint that stores them as fp16).  The
 * fp16-activation noise of the reference is not reproduced.
 *
 * Conventions: those of tamf_hip.h (included for the tamf_status enum only).  Plain C types; every function returns 0 or a negative
 * tamf_status; the message of the calling thread's last failure is tamf_textenc_last_error().  "dev" pointers are device memory
 * owned by the caller, "host" pointers host memory; `stream` is a hipStream_t passed as void*.  A model belongs to the device that
 * was current at tamf_textenc_finalize.  Calls on one model must not overlap (one thread at a time).
 */
#ifndef TAMF_TEXTENC_H
#define TAMF_TEXTENC_H

#include <stdint.h>

#include "tamf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct tamf_textenc_model tamf_textenc_model;

typedef struct tamf_textenc_config {
  int32_t vocab_size;     /* >= 2 */
  int32_t context_length; /* 2 .. 128 */
  int32_t width;          /* a multiple of 64, = 64 * num_heads, <= 1024 */
  int32_t num_heads;      /* width / 64 */
  int32_t num_layers;     /* >= 1 */
  int32_t embed_dim;      /* a multiple of 16, 16 .. 1024 */
} tamf_textenc_config;

/* message of the last failure of a call made by THIS thread ("" when none) */
const char* tamf_textenc_last_error(void);

/* An empty model of this configuration (host only; anything outside the ranges above is TAMF_ERR_INVALID). */
int tamf_textenc_model_create(const tamf_textenc_config* cfg, tamf_textenc_model** model_out);

/* One tensor of the state dict, float32 host memory, read before the call returns.  `key` is the name in OpenAI's archive:
 * "token_embedding.weight", "positional_embedding", "text_projection", "ln_final.{weight,bias}",
 * "transformer.resblocks.N.{ln_1,ln_2}.{weight,bias}", "transformer.resblocks.N.attn.{in_proj_weight,in_proj_bias}",
 * "transformer.resblocks.N.attn.out_proj.{weight,bias}", "transformer.resblocks.N.mlp.{c_fc,c_proj}.{weight,bias}"; `shape` the
 * tensor's own (ndim entries).  An unknown key or a wrong shape is TAMF_ERR_INVALID; loading after finalize was called with a
 * complete set of tensors is TAMF_ERR_STATE. */
int tamf_textenc_load_weight(tamf_textenc_model* model, const char* key, const float* host, int32_t ndim, const int64_t* shape);

/* Checks that every tensor is there (TAMF_ERR_MISSING names the first absent one) and finite (TAMF_ERR_RANGE); with round_fp16 != 0
 * rounds the tensors named under "Arithmetic" to fp16 (nearest even; a value beyond the fp16 range is TAMF_ERR_RANGE); uploads
 * everything to the current device.  Once the checks have passed the model takes no more tensors, whether or not the upload
 * succeeds (a model whose upload failed can only be destroyed).  Synchronises the device once (blocking copy). */
int tamf_textenc_finalize(tamf_textenc_model* model, int32_t round_fp16);

/* frees the model (NULL is accepted); work enqueued by tamf_textenc_encode must have finished */
int tamf_textenc_destroy(tamf_textenc_model* model);

/* bytes of workspace tamf_textenc_encode needs for B prompts that pack into total_rows = sum over prompts of (EOT position + 1) rows;
 * B * context_length is always enough.  0 for a bad argument. */
int64_t tamf_textenc_workspace_bytes(const tamf_textenc_model* model, int32_t B, int64_t total_rows);

/* tokens_host (B, context_length) int32, HOST memory (the tokenizer runs there), read before the call returns -> out_dev
 * (B, embed_dim) float32.  The library finds every row's EOT position e_b (the first index of the row's largest id), rejects ids
 * outside [0, vocab_size) (TAMF_ERR_INVALID, naming the entry), packs the M = sum(e_b + 1) rows that the outputs depend on, uploads
 * the row map through pinned memory and enqueues: token gather + positional add, the blocks (LayerNorm, QKV, causal attention per
 * (prompt, head), output projection + residual, LayerNorm, c_fc + QuickGELU, c_proj + residual), ln_final on the B EOT rows and the
 * projection.  Every contraction runs on v_mfma_f32_16x16x4_f32 in a fixed K order, nothing is reduced with atomics.  A prompt's
 * output bits depend on its ids up to e_b and on the model only - not on B, on the prompt's position in the batch or on the other
 * prompts.  workspace_dev: 16-byte aligned, at least tamf_textenc_workspace_bytes(model, B, M) bytes, free to reuse once the enqueued
 * work has finished.  Does not synchronise the device; waits on the host only for the previous call's row-map upload to have left
 * the staging buffer. */
int tamf_textenc_encode(tamf_textenc_model* model, const int32_t* tokens_host, int32_t B, float* out_dev, void* workspace_dev,
                        int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TAMF_TEXTENC_H */
