// Weight preparation of the sampler library, the part that is plain arithmetic on the host: the checkpoint key set of an architecture,
// operand packing (bf16 rounding, the hi | lo 128-byte groups of the split modes, the per-tensor power-of-two scale of f16x3), the
// deferred-LayerNorm fold, the composed input map and its bias.  Host only and HIP-free: every function maps host arrays to host
// arrays, tamf_hip.hip uploads what they return, and a stand-alone program can #include this header (tests/test_weight_prep_cpu.py).
// Needs a compiler with _Float16 (clang).
#pragma once
#include "../../include/tamf_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <string>
#include <vector>

// ------------------------------------------------------------------------------------------------
// the state-dict key set of a kind (SegmentEncoder: segment_encoder.py:16-75) with the shape of every tensor
// ------------------------------------------------------------------------------------------------
static inline std::map<std::string, std::vector<int64_t>> expected_shapes(const tamf_arch& a) {
  std::map<std::string, std::vector<int64_t>> m;
  const int64_t d = a.latent_dim, ff = a.ff_size;
  const int kind = a.kind;
  auto lin = [&](const std::string& n, int64_t o, int64_t i) {
    m[n + ".weight"] = {o, i};
    m[n + ".bias"] = {o};
  };
  m["hand_side_process.rh_embed"] = {d};
  m["hand_side_process.lh_embed"] = {d};
  lin("hand_shape_process.shape_embed", d, a.hand_shape_dim);
  lin("obj_embed_process.embedding", d, a.obj_embed_dim);
  lin("input_process.poseEmbedding", d, a.input_dim);
  lin("obj_input_process.poseEmbedding", d, a.obj_input_dim);
  lin("input_merge.0", d, (kind == TAMF_KIND_R ? 3 : 2) * d);
  lin("input_merge.2", d, d);
  m["sequence_pos_encoder.pe"] = {5000, 1, d};
  for (int l = 0; l < a.num_layers; ++l) {
    const std::string p = "seqTransEncoder.layers." + std::to_string(l);
    m[p + ".self_attn.in_proj_weight"] = {3 * d, d};
    m[p + ".self_attn.in_proj_bias"] = {3 * d};
    lin(p + ".self_attn.out_proj", d, d);
    lin(p + ".linear1", ff, d);
    lin(p + ".linear2", d, ff);
    m[p + ".norm1.weight"] = {d};
    m[p + ".norm1.bias"] = {d};
    m[p + ".norm2.weight"] = {d};
    m[p + ".norm2.bias"] = {d};
  }
  if (kind == TAMF_KIND_E) {
    m["classification_token"] = {1, 1, d};
    lin("output_process.poseFinal.0", d, d);
    lin("output_process.poseFinal.2", d, d);
    lin("output_process.poseFinal.4", a.input_dim, d);
    return m;
  }
  if (kind == TAMF_KIND_R) {
    lin("h2o_dist_input_process.poseEmbedding", d, a.h2o_dim);
  } else {
    lin("embed_timestep.time_embed.0", d, d);
    lin("embed_timestep.time_embed.2", d, d);
    lin("embed_text", d, a.clip_dim);
  }
  lin("output_process.poseFinal", a.input_dim, d);
  return m;
}

// ------------------------------------------------------------------------------------------------
// operand packing
// ------------------------------------------------------------------------------------------------
// host float -> bf16 (round to nearest even; NaN kept quiet)
static inline uint16_t h_f2bf(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  if ((u & 0x7F800000u) == 0x7F800000u && (u & 0x007FFFFFu)) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7FFFu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
static inline float h_bf2f(uint16_t h) {
  uint32_t u = (uint32_t)h << 16;
  float f;
  memcpy(&f, &u, 4);
  return f;
}

// The host image of an operand matrix, and what the caller reports about it.  `refused` is checked first: a refused operand has no
// image (nothing is stored before the checks).
struct PackedOperand {
  enum Refused { NONE = 0, BAD_LD, NON_FINITE } refused = NONE;  // ldk % 32 != 0; f16x3: a non-finite weight
  std::vector<unsigned char> image;  // the bytes to upload: N * ldk elements of 4 (f32, bf16x3, f16x3: hi + lo) or 2 (bf16) bytes
  float inv_scale = 1.0f;            // f16x3: the tensor is stored as w * 2^wexp, this is 2^-wexp; every other mode: 1
  // f16x3, the weight-range note: non-zero weights, and those of them below 2^-17.5 of the tensor's maximum (stored < 0.125)
  size_t nonzero = 0, small = 0;
  bool small_share_noted() const { return nonzero && small * 100 > nonzero; }  // more than 1 %
  // the refusal as the C-ABI reports it (tamf_status, tamf_last_error), and the note; `what` names the tensor
  int error_code() const { return refused == NON_FINITE ? TAMF_ERR_RANGE : refused == BAD_LD ? TAMF_ERR_INVALID : TAMF_OK; }
  std::string error_message(const char* what) const {
    if (refused == BAD_LD) return "operand leading dimension must be a multiple of 32";
    return std::string("f16x3: weight ") + what + " holds a non-finite value and cannot be stored as split-fp16 operands; use bf16x3 or f32";
  }
  std::string range_note(const char* what) const {
    return std::string("f16x3: ") + std::to_string(small * 100 / nonzero) + " % of the non-zero weights of " + what +
           " are below 2^-17.5 of the tensor's largest magnitude: stored with fewer than 22 significand bits (an outlier dominates the per-tensor scale)";
  }
};

// host fp32 [N][K] -> operand matrix [N][ldk] in precision `prec` (cols >= K zero; ldk % 32 == 0).
// bf16x3 / f16x3 rows are 128-byte groups of 32 elements: [hi: 32 x 16 bit | lo: 32 x 16 bit] (tamf_device.h "Operand traits").
static inline PackedOperand pack_operand(int prec, const float* w, int N, int K, int ldk) {
  PackedOperand po;
  const size_t n = (size_t)N * ldk;
  if (ldk % 32) {
    po.refused = PackedOperand::BAD_LD;
    return po;
  }
  int wexp = 0;  // f16x3: the tensor is stored as w * 2^wexp
  if (prec == TAMF_PREC_F16X3) {
    // Power-of-two pre-scaling of the split-fp16 weights: max |w| lands in [2^14, 2^15), so that the lo planes of everything down to
    // 2^-17 of the tensor's maximum are NORMAL fp16 numbers (22 significand bits; unscaled, PyTorch-default weights of ~0.04 had
    // subnormal lo parts: an absolute 3e-8, i.e. ~19 bits) and a weight beyond the fp16 range is no reason to refuse a checkpoint.
    // The product is scaled back exactly in the epilogue's bias add (EpiCtl::wscale).  Only a non-finite weight is refused.
    // (activations are checked on the device: tamf_device.h, status word)
    float mx = 0.f;
    for (size_t i = 0; i < (size_t)N * K; ++i) {
      if (!std::isfinite(w[i])) {
        po.refused = PackedOperand::NON_FINITE;
        return po;
      }
      mx = std::fmax(mx, std::fabs(w[i]));
    }
    if (mx > 0.f) {
      int e = 0;
      (void)std::frexp(mx, &e);  // mx = m 2^e, m in [0.5, 1)
      wexp = std::min(120, std::max(-120, 15 - e));
    }
    po.inv_scale = std::ldexp(1.0f, -wexp);
    // One power of two per tensor: a weight smaller than 2^-17.5 of the tensor's maximum has an fp16-SUBNORMAL lo part again (fewer than
    // 22 significand bits).  Ordinary tensors are nowhere near (max / typical ~ 2^3 .. 2^7); one huge outlier over ordinary weights is
    // (a single 7e4 among 0.04s leaves the others ~18 bits).  Reported, not refused: a status bit + the tensor's name.
    for (size_t i = 0; i < (size_t)N * K; ++i)
      if (w[i] != 0.f) {
        ++po.nonzero;
        if (std::fabs(std::ldexp(w[i], wexp)) < 0.125f) ++po.small;
      }
  }
  if (prec == TAMF_PREC_F32) {
    po.image.assign(n * 4, 0);
    for (int r = 0; r < N; ++r) memcpy(&po.image[(size_t)r * ldk * 4], &w[(size_t)r * K], (size_t)K * 4);
    return po;
  }
  auto put16 = [&](size_t at, const void* v) { memcpy(&po.image[at * 2], v, 2); };  // `at` in 16-bit units
  if (prec == TAMF_PREC_BF16) {
    po.image.assign(n * 2, 0);
    for (int r = 0; r < N; ++r)
      for (int k = 0; k < K; ++k) {
        const uint16_t h = h_f2bf(w[(size_t)r * K + k]);
        put16((size_t)r * ldk + k, &h);
      }
    return po;
  }
  po.image.assign(n * 4, 0);
  for (int r = 0; r < N; ++r)
    for (int k = 0; k < K; ++k) {
      const float v = w[(size_t)r * K + k];
      const size_t idx = (size_t)r * ldk + k;
      const size_t o = (idx >> 5) * 64 + (idx & 31);  // in uint16 units: 64 per 128-byte group
      if (prec == TAMF_PREC_F16X3) {
        const float vs = std::ldexp(v, wexp);  // exact
        const _Float16 hi = (_Float16)vs, lo = (_Float16)(vs - (float)hi);
        put16(o, &hi);
        put16(o + 32, &lo);
      } else {
        const uint16_t hi = h_f2bf(v), lo = h_f2bf(v - h_bf2f(hi));
        put16(o, &hi);
        put16(o + 32, &lo);
      }
    }
  return po;
}

// W [N][K] -> W^T [K][N] (the tables of prefix_rows_kernel)
static inline std::vector<float> transposed(const float* W, int N, int K) {
  std::vector<float> t((size_t)N * K);
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < K; ++k) t[(size_t)k * N + n] = W[(size_t)n * K + k];
  return t;
}

// ------------------------------------------------------------------------------------------------
// deferred LayerNorm (tamf_device.h)
// ------------------------------------------------------------------------------------------------
// Fold the gain AND the centring of the LayerNorm in front of a GEMM into its weight, W'' = W diag(gamma) (I - 1 1^T / d) (fp64: every
// row of W diag(gamma) minus its own mean), c2 = W beta + bias.  W is [N][d]; w and c2 have Npad >= N rows, zero beyond N (the output
// head).  gamma = beta = null (layer 0's attention block reads the encoder input itself): the plain weight and bias.
struct FoldedLinear {
  std::vector<float> w, c2;  // [Npad][d], [Npad]
};
static inline FoldedLinear fold_layernorm(const float* W, const float* bias, int N, int Npad, int d, const float* g, const float* be) {
  FoldedLinear f{std::vector<float>((size_t)Npad * d, 0.f), std::vector<float>(Npad, 0.f)};
  for (int n = 0; n < N; ++n) {
    double acc = bias[n], rowsum = 0.0;
    for (int k = 0; k < d; ++k) {
      if (g) rowsum += (double)W[(size_t)n * d + k] * g[k];
      if (be) acc += (double)W[(size_t)n * d + k] * be[k];
    }
    const double shift = g ? rowsum / d : 0.0;  // W'' = W diag(gamma) (I - 1 1^T / d): every row minus its own mean
    for (int k = 0; k < d; ++k) f.w[(size_t)n * d + k] = g ? (float)((double)W[(size_t)n * d + k] * g[k] - shift) : W[(size_t)n * d + k];
    f.c2[n] = (float)acc;
  }
  return f;
}
// ... and what the residual add behind that GEMM's block takes: gamma and beta + bias of the LayerNorm its residual input passes
// through (null: none, i.e. gain 1 and shift 0), `bias` the bias of the block's last linear map
struct ResidualLn {
  std::vector<float> g, bb;  // [d]
};
static inline ResidualLn residual_ln(const float* g, const float* be, const float* bias, int d) {
  ResidualLn r{std::vector<float>(d), std::vector<float>(d)};
  for (int n = 0; n < d; ++n) {
    r.g[n] = g ? g[n] : 1.0f;
    r.bb[n] = (be ? be[n] : 0.0f) + bias[n];
  }
  return r;
}

// ------------------------------------------------------------------------------------------------
// the composed input map: input_merge.0 applied to the concatenated embeddings, as one linear map of the raw inputs
// ------------------------------------------------------------------------------------------------
// One block, in float64: out[n * ld_n + k * ld_k] = sum_j W_m1[n][col0 + j] W_x[j][k] (n, j < d; k < K), where
// W_m1 = input_merge.0.weight [d][mk] and W_x [d][K] is the embedding that feeds its columns col0 .. col0 + d.  ld_k = 1: row-major
// rows of the fused weight; ld_n = 1: transposed (WcT of cobj_kernel).
static inline void compose_block(const float* Wm1, int mk, int col0, int d, const float* Wx, int K, float* out, long ld_n, long ld_k) {
  for (int n = 0; n < d; ++n)
    for (int k = 0; k < K; ++k) {
      double a = 0;
      for (int j = 0; j < d; ++j) a += (double)Wm1[(size_t)n * mk + col0 + j] * Wx[(size_t)j * K + k];
      out[n * ld_n + k * ld_k] = (float)a;
    }
}
// Its bias, b_m1 + sum over the embeddings of W_m1[:, block] b_x, in float64 - in TWO summation orders, which round differently and
// are both kept: the uploaded bytes of either kind stay what they were.
//   G / R (tamf_finalize_weights): one term after the other, `nb` embedding biases bx[0 .. nb) for the column blocks 0, d, 2 d, ...
static inline std::vector<float> input_bias_term_by_term(const float* Wm1, int mk, int d, const float* bm1, const float* const* bx, int nb) {
  std::vector<float> cb(d);
  for (int n = 0; n < d; ++n) {
    double acc_b = bm1[n];
    for (int b = 0; b < nb; ++b)
      for (int j = 0; j < d; ++j) acc_b += (double)Wm1[(size_t)n * mk + (size_t)b * d + j] * bx[b][j];
    cb[n] = (float)acc_b;
  }
  return cb;
}
//   SegmentEncoder (enc_finalize): its two terms inside one loop over j, written to out[0 .. d)
static inline void input_bias_two_terms_per_column(const float* Wm1, int d, const float* bm1, const float* bp, const float* bq, float* out) {
  for (int n = 0; n < d; ++n) {
    double acc_b = bm1[n];
    for (int j = 0; j < d; ++j) acc_b += (double)Wm1[(size_t)n * 2 * d + j] * bp[j] + (double)Wm1[(size_t)n * 2 * d + d + j] * bq[j];
    out[n] = (float)acc_b;
  }
}

// The fused input weight of a G / R context: w [d][XK] = [ W_m1[:, :d] W_p | (R: W_m1[:, 2d:] W_h) | 0 ], the object half hoisted out of
// the loop (cobj_kernel): W_m1[:, d:2d] (W_q m + b_q) = Wc m + ..., wct = Wc^T [qd][d], and the bias of all of it.  Wh / bh null: G.
struct FusedInput {
  std::vector<float> w, wct, bias;
};
static inline FusedInput fuse_input(int d, int F, int qd, int h2o_dim, int XK, const float* Wm1, const float* bm1, const float* Wp,
                                    const float* bp, const float* Wq, const float* bq, const float* Wh, const float* bh) {
  const int mk = Wh ? 3 * d : 2 * d;
  FusedInput f{std::vector<float>((size_t)d * XK, 0.f), std::vector<float>((size_t)qd * d), {}};
  const float* bx[3] = {bp, bq, bh};
  f.bias = input_bias_term_by_term(Wm1, mk, d, bm1, bx, Wh ? 3 : 2);
  compose_block(Wm1, mk, 0, d, Wp, F, f.w.data(), XK, 1);
  compose_block(Wm1, mk, d, d, Wq, qd, f.wct.data(), 1, d);
  if (Wh) compose_block(Wm1, mk, 2 * d, d, Wh, h2o_dim, f.w.data() + F, XK, 1);
  return f;
}
