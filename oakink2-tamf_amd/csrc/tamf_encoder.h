// SegmentEncoder forward (TAMF_KIND_E: the encoder of the FID score, reference model/segment_encoder.py:16-111) - one workgroup per
// clip, fp32 throughout, every linear map on v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulate).  There is one arithmetic
// mode only: the score has to be reproducible, so nothing here depends on the batch, the launch or a tuning word - clip b's bits are
// the same alone or in any batch, and the same on every call.
//
// Per clip (S = T + 4 token rows: 3 prefix rows, T frame rows, the classification token last):
//   prefix   rows 0..2 = nan_to_num(side | shape | object embedding) + PE, computed by prefix_rows_kernel (tamf_misc.h) beforehand
//   frames   x_t = nan_to_num(W_m2 silu(W_in [pose_t | mean_o traj_{o,t}] + b_in) + b_m2) + PE[3 + t]; W_in is input_merge.0 composed
//            with input_process.poseEmbedding and obj_input_process.poseEmbedding (float64 at tamf_finalize_weights), K = 99 + 9
//   cls      classification_token + PE[S - 1]
//   layers   nn.TransformerEncoderLayer, post-LN: x = LN1(x + MHA(x)); x = LN2(x + W2 gelu(W1 x + b1) + b2) - exact-erf GELU,
//            eps 1e-5, softmax scale 1/sqrt(hd), NO attention mask (padded frames attend and are attended to, as in the reference)
//   output   encoding = the CLS row after the last layer; activation = poseFinal (Linear, SiLU, Linear, SiLU, Linear) of it
//
// The LAST layer computes only what the CLS row needs: K and V of every row (the CLS query attends to all of them), then the query,
// attention, out-projection, LayerNorms and feed-forward block of the CLS row alone - the other rows' outputs are never read.
//
// LDS (dynamic, floats):
//   X    [S][64]          the residual stream of the clip
//   scratch, a union by phase:
//     attention   A [S][64] (head h's query in columns h*16.., overwritten by its output row by row) | K_h [S][16] | V_h [S][16]
//     frames      Ain [64][KIN] (pose | object mean, zero-padded) | Z [64][64]
//     feed-fwd    Hc [32][ff]  (32 rows of the hidden layer at a time)
// At d = 64, hd = 16 that is 160 floats per token row: S <= 256 (T <= 252) in the 160 KiB of a CU.
#pragma once
#include "tamf_device.h"

constexpr int ENC_D = 64, ENC_HD = 16, ENC_NT = 256;  // latent width, head width, threads (4 waves)
constexpr int ENC_RC = 64;                             // frame rows per input-stage chunk
constexpr int ENC_FR = 32;                             // token rows per feed-forward chunk
constexpr int ENC_P = 3;                               // prefix rows
constexpr long ENC_LDS_BYTES = 160 * 1024;

// packed weights of one encoder layer (floats, in this order; Wqkv / bqkv rows grouped per head: [q_h | k_h | v_h], 48 rows per head)
struct EncLayerOff {
  long wqkv, bqkv, wo, bo, w1, b1, w2, b2, g1, be1, g2, be2, stride;
};
__host__ __device__ inline EncLayerOff enc_layer_off(int ff) {
  const int d = ENC_D;
  EncLayerOff o;
  o.wqkv = 0;
  o.bqkv = o.wqkv + 3L * d * d;
  o.wo = o.bqkv + 3L * d;
  o.bo = o.wo + (long)d * d;
  o.w1 = o.bo + d;
  o.b1 = o.w1 + (long)ff * d;
  o.w2 = o.b1 + ff;
  o.b2 = o.w2 + (long)d * ff;
  o.g1 = o.b2 + d;
  o.be1 = o.g1 + d;
  o.g2 = o.be1 + d;
  o.be2 = o.g2 + d;
  o.stride = o.be2 + d;
  return o;
}
// packed input / output weights (floats, in this order), then the layers
struct EncHeadOff {
  long cls, win, bin, wm2, bm2, p0, pb0, p2, pb2, p4, pb4, layers;
};
__host__ __device__ inline EncHeadOff enc_head_off(int kin, int F) {
  const int d = ENC_D;
  EncHeadOff o;
  o.cls = 0;
  o.win = o.cls + d;
  o.bin = o.win + (long)d * kin;
  o.wm2 = o.bin + d;
  o.bm2 = o.wm2 + (long)d * d;
  o.p0 = o.bm2 + d;
  o.pb0 = o.p0 + (long)d * d;
  o.p2 = o.pb0 + d;
  o.pb2 = o.p2 + (long)d * d;
  o.p4 = o.pb2 + d;
  o.pb4 = o.p4 + (long)F * d;
  o.layers = (o.pb4 + F + 3) / 4 * 4;
  return o;
}
// scratch floats behind X (the union above) and the whole dynamic LDS of a launch with S rows
__host__ __device__ inline long enc_scratch_floats(int S, int ff, int kin) {
  const long att = (long)S * ENC_D + 2L * S * ENC_HD, frames = (long)ENC_RC * (kin + ENC_D), ffn = (long)ENC_FR * ff;
  const long m = att > frames ? att : frames;
  return m > ffn ? m : ffn;
}
__host__ __device__ inline long enc_lds_bytes(int S, int ff, int kin) { return ((long)S * ENC_D + enc_scratch_floats(S, ff, kin)) * 4; }

struct EncArgs {
  const float* w;        // packed weights (EncHeadOff, then L x EncLayerOff)
  const float* pe;       // [5000][64]
  const float* pstatic;  // [B][3][64] prefix rows incl. nan_to_num and PE
  const float* pose;     // [B][T][F]
  const float* traj;     // [B][nobj][T][qd]
  const int* cnt;        // [B] object counts or null (all nobj)
  float* enc;            // [B][64]
  float* act;            // [B][F] or null
  int T, nobj, F, qd, kin, ff, L;
};

// C = A . W^T over the whole workgroup: A [M][K] in LDS (row stride lda), W [N][K] row-major in global memory (row stride ldw, read
// through L2: every workgroup reads the same weights), N a multiple of 16, K a multiple of 4.  16 x 16 tiles go round the waves; a
// lane (r = lane & 15, g = lane >> 4) feeds A row r / W row r at k = g, and receives rows 4g..4g+3 of column r.  epi(row, col, v) is
// called once per element with row < M; nothing is synchronised here.
template <class Epi>
TAMF_DEV void enc_gemm(const float* A, int lda, int M, const float* __restrict__ W, int ldw, int N, int K, Epi epi) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = ENC_NT / 64;
  const int r = lane & 15, g = lane >> 4;
  const int mt = (M + 15) >> 4, nt = N >> 4;
  for (int t = wave; t < mt * nt; t += nw) {
    const int m0 = (t / nt) << 4, n0 = (t % nt) << 4;
    const bool arow = m0 + r < M;
    const float* ap = A + (long)(m0 + r) * lda + g;
    const float* wp = W + (long)(n0 + r) * ldw + g;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int k = 0; k < K; k += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(arow ? ap[k] : 0.f, wp[k], acc, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = m0 + 4 * g + i;
      if (row < M) epi(row, n0 + r, acc[i]);
    }
  }
}

// LayerNorm of one 64-wide row by one wave (lane = column); biased variance, two passes, as torch.nn.LayerNorm
TAMF_DEV void enc_ln_row(float* x, const float* __restrict__ g, const float* __restrict__ b) {
  const int lane = threadIdx.x & 63;
  const float v = x[lane];
  const float mean = wave_sum(v) * (1.0f / ENC_D);
  const float dv = v - mean;
  const float var = wave_sum(dv * dv) * (1.0f / ENC_D);
  x[lane] = dv * (1.0f / sqrtf(var + 1e-5f)) * g[lane] + b[lane];
}

__global__ __launch_bounds__(ENC_NT) void encoder_kernel(const EncArgs a) {
  extern __shared__ float4 enc_lds4[];
  float* X = reinterpret_cast<float*>(enc_lds4);
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int D = ENC_D, HD = ENC_HD, T = a.T, S = T + ENC_P + 1, F = a.F, qd = a.qd, kin = a.kin, ff = a.ff;
  float* scr = X + (long)S * D;
  const EncHeadOff ho = enc_head_off(kin, F);
  const EncLayerOff lo = enc_layer_off(ff);
  const float* __restrict__ w = a.w;
  const float* __restrict__ pe = a.pe;

  // ---- input stage: prefix rows, frame rows, classification token ----
  for (int e = tid; e < ENC_P * D; e += ENC_NT) X[e] = a.pstatic[(long)b * ENC_P * D + e];
  for (int c = tid; c < D; c += ENC_NT) X[(long)(S - 1) * D + c] = w[ho.cls + c] + pe[(long)(S - 1) * D + c];
  {
    const int n = a.cnt ? max(1, min(a.cnt[b], a.nobj)) : a.nobj;
    float* Ain = scr;                     // [ENC_RC][kin]
    float* Z = scr + (long)ENC_RC * kin;  // [ENC_RC][D]
    for (int c0 = 0; c0 < T; c0 += ENC_RC) {
      const int m = min(ENC_RC, T - c0);
      for (int e = tid; e < ENC_RC * kin; e += ENC_NT) {
        const int r = e / kin, k = e % kin;
        float v = 0.f;
        if (r < m) {
          const int t = c0 + r;
          if (k < F) {
            v = a.pose[((long)b * T + t) * F + k];
          } else if (k < F + qd) {
            float s = 0.f;
            for (int o = 0; o < n; ++o) s += a.traj[(((long)b * a.nobj + o) * T + t) * qd + (k - F)];
            v = s / (float)n;
          }
        }
        Ain[e] = v;
      }
      __syncthreads();
      enc_gemm(Ain, kin, m, w + ho.win, kin, D, kin, [&](int r, int c, float v) { Z[r * D + c] = silu_exact(v + w[ho.bin + c]); });
      __syncthreads();
      enc_gemm(Z, D, m, w + ho.wm2, D, D, D, [&](int r, int c, float v) {
        const long row = ENC_P + c0 + r;
        X[row * D + c] = nan_to_num(v + w[ho.bm2 + c]) + pe[row * D + c];
      });
      __syncthreads();
    }
  }

  // ---- encoder layers ----
  float* Abuf = scr;                   // [S][D]
  float* Kh = scr + (long)S * D;       // [S][HD]
  float* Vh = Kh + (long)S * HD;       // [S][HD]
  float* Hc = scr;                     // [ENC_FR][ff]
  const float scale = 1.0f / sqrtf((float)HD);
  for (int l = 0; l < a.L; ++l) {
    const float* lw = w + ho.layers + (long)l * lo.stride;
    const bool last = l == a.L - 1;
    const int q0 = last ? S - 1 : 0, nq = last ? 1 : S;  // query rows q0.. of this layer (the last one: the CLS row alone); query i lives in Abuf row i
    for (int h = 0; h < ENC_D / ENC_HD; ++h) {
      const float* wh = lw + lo.wqkv + (long)h * 3 * HD * D;
      const float* bh = lw + lo.bqkv + h * 3 * HD;
      // K_h, V_h of every row
      enc_gemm(X, D, S, wh + HD * D, D, 2 * HD, D, [&](int r, int c, float v) {
        v += bh[HD + c];
        if (c < HD) Kh[r * HD + c] = v;
        else Vh[r * HD + c - HD] = v;
      });
      // Q_h of the query rows, into columns h*HD.. of their Abuf rows
      enc_gemm(X + (long)q0 * D, D, nq, wh, D, HD, D, [&](int r, int c, float v) { Abuf[r * D + h * HD + c] = v + bh[c]; });
      __syncthreads();
      if (!last) {
        // one thread per query row: two passes over the keys (max, then exp / sum / weighted V), fp32
        for (int q = tid; q < S; q += ENC_NT) {
          float qv[ENC_HD], o[ENC_HD];
          float* ar = Abuf + (long)q * D + h * HD;
#pragma unroll
          for (int j = 0; j < HD; ++j) { qv[j] = ar[j]; o[j] = 0.f; }
          float mx = -__builtin_inff();
          for (int k = 0; k < S; ++k) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < HD; ++j) s = fmaf(qv[j], Kh[k * HD + j], s);
            mx = fmaxf(mx, s * scale);
          }
          float sum = 0.f;
          for (int k = 0; k < S; ++k) {
            float s = 0.f;
#pragma unroll
            for (int j = 0; j < HD; ++j) s = fmaf(qv[j], Kh[k * HD + j], s);
            const float p = expf(s * scale - mx);
            sum += p;
#pragma unroll
            for (int j = 0; j < HD; ++j) o[j] = fmaf(p, Vh[k * HD + j], o[j]);
          }
          const float inv = 1.0f / sum;
#pragma unroll
          for (int j = 0; j < HD; ++j) ar[j] = o[j] * inv;
        }
      } else if (wave == 0) {
        // the CLS query alone: the keys go round the 64 lanes of wave 0, then wave reductions
        float qv[ENC_HD], o[ENC_HD];
#pragma unroll
        for (int j = 0; j < HD; ++j) { qv[j] = Abuf[h * HD + j]; o[j] = 0.f; }
        float mx = -__builtin_inff();
        for (int k = lane; k < S; k += 64) {
          float s = 0.f;
#pragma unroll
          for (int j = 0; j < HD; ++j) s = fmaf(qv[j], Kh[k * HD + j], s);
          mx = fmaxf(mx, s * scale);
        }
        mx = wave_reduce<RedMax>(mx);
        float sum = 0.f;
        for (int k = lane; k < S; k += 64) {
          float s = 0.f;
#pragma unroll
          for (int j = 0; j < HD; ++j) s = fmaf(qv[j], Kh[k * HD + j], s);
          const float p = expf(s * scale - mx);
          sum += p;
#pragma unroll
          for (int j = 0; j < HD; ++j) o[j] = fmaf(p, Vh[k * HD + j], o[j]);
        }
        sum = wave_sum(sum);
#pragma unroll
        for (int j = 0; j < HD; ++j) o[j] = wave_sum(o[j]);
        if (lane < HD) {
          float v = o[0];
#pragma unroll
          for (int j = 1; j < HD; ++j) v = lane == j ? o[j] : v;
          Abuf[h * HD + lane] = v / sum;
        }
      }
      __syncthreads();
    }
    // out-projection + residual, LayerNorm 1
    enc_gemm(Abuf, D, nq, lw + lo.wo, D, D, D, [&](int r, int c, float v) { X[(long)(q0 + r) * D + c] += v + lw[lo.bo + c]; });
    __syncthreads();
    for (int r = q0 + wave; r < S; r += ENC_NT / 64) enc_ln_row(X + (long)r * D, lw + lo.g1, lw + lo.be1);
    __syncthreads();
    // feed-forward block in chunks of ENC_FR rows (the hidden layer of a chunk in LDS) + residual, LayerNorm 2
    for (int c0 = q0; c0 < S; c0 += ENC_FR) {
      const int m = min(ENC_FR, S - c0);
      enc_gemm(X + (long)c0 * D, D, m, lw + lo.w1, D, ff, D, [&](int r, int c, float v) { Hc[r * ff + c] = gelu_erf(v + lw[lo.b1 + c]); });
      __syncthreads();
      enc_gemm(Hc, ff, m, lw + lo.w2, ff, D, ff, [&](int r, int c, float v) { X[(long)(c0 + r) * D + c] += v + lw[lo.b2 + c]; });
      __syncthreads();
    }
    for (int r = q0 + wave; r < S; r += ENC_NT / 64) enc_ln_row(X + (long)r * D, lw + lo.g2, lw + lo.be2);
    __syncthreads();
  }

  // ---- outputs: encoding = CLS row; activation = poseFinal(CLS row) ----
  const float* xc = X + (long)(S - 1) * D;
  if (tid < D) a.enc[(long)b * D + tid] = xc[tid];
  if (a.act) {
    float* h1 = scr;
    float* h2 = scr + D;
    if (tid < D) {
      float s = w[ho.pb0 + tid];
      for (int k = 0; k < D; ++k) s = fmaf(w[ho.p0 + (long)tid * D + k], xc[k], s);
      h1[tid] = silu_exact(s);
    }
    __syncthreads();
    if (tid < D) {
      float s = w[ho.pb2 + tid];
      for (int k = 0; k < D; ++k) s = fmaf(w[ho.p2 + (long)tid * D + k], h1[k], s);
      h2[tid] = silu_exact(s);
    }
    __syncthreads();
    for (int c = tid; c < F; c += ENC_NT) {
      float s = w[ho.pb4 + c];
      for (int k = 0; k < D; ++k) s = fmaf(w[ho.p4 + (long)c * D + k], h2[k], s);
      a.act[(long)b * F + c] = s;
    }
  }
}
