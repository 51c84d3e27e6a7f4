// Training kernels of a post-LN transformer trunk at head dimension 64 or 128 (libtamf_refinetrain.so, libtamf_mdmtrain.so), fp32
// throughout.  Every contraction runs on v_mfma_f32_16x16x4_f32.  Nothing here knows the model around the layer stack: the input
// stage and the head are launch sequences of the host file over the same kernels.
//
//   tg_lin_kernel<WT>  C = epi(A . W^T + bias) over a 64 x 64 tile per workgroup, the contraction in steps of 32 through LDS.  WT = false
//                      reads W[n][k] (forward); WT = true reads the same W by its other stride, W[k][n] (data gradient).  An output
//                      element is one accumulator chain over k ascending: its bits do not depend on where its row sits in the batch.
//   tg_wgrad_kernel    part[s][n][k] = sum over the token rows of split s of dY[r][n] X[r][k], the same tile with the rows as the
//                      contraction; column k = K is the sum of dY itself (the bias gradient).  reduce_kernel adds the splits in order.
//   tg_attn_*<HD>      one wave per 16 query rows (forward, dQ) or 16 key rows (dK, dV) of a (clip, head).  Scores and dP are
//                      tg_score_tile products; a 16 x 16 tile of P (or dS) goes through LDS once, from the MFMA's output layout to its
//                      A-operand layout, and is contracted against V (K, Q, dO) rows read from global memory.  The probabilities are
//                      recomputed from the stored row maximum and sum; their dropout is regenerated.
//   tg_ln_*            LayerNorm of a row by one wave, its backward with the statistics recomputed from the stored input.
//
// LDS: 2 x 64 x 36 floats = 18 KiB per GEMM workgroup; 16 x 17 floats (forward, dQ) or twice that (dK, dV) per attention wave.  No
// kernel keeps a whole head's keys in LDS, so LDS sets no bound on the sequence length.
//
// Determinism.  No floating-point atomics.  Every output element is one lane's sum in a fixed order; dK and dV visit the query tiles
// in ascending order.
//
// Dropout sites (tamf_dropout.h for the scheme), S token rows per clip, d = latent_dim:
//   site 0               x + PE                   element = row * d + col
//   site 1 + 4 l         attention probabilities  element = (head * S + query) * S + key
//   site 2 + 4 l         out-projection output    element = row * d + col
//   site 3 + 4 l         GELU output              element = row * ff + col
//   site 4 + 4 l         linear2 output           element = row * d + col
#pragma once
#include "tamf_dropout.h"
#include "tamf_f32_tower.h"

constexpr int TG_HD = F32_HD;                            // the head dimension of the refiner's configurations (the kernels: 64 or 128)
constexpr int TG_T = 64, TG_K = 32, TG_LD = TG_K + 4;    // GEMM tile, contraction step, LDS row stride (floats)
constexpr int TG_PLD = 17;                               // row stride of an attention wave's 16 x 16 LDS tile

enum TgMode {
  TG_LIN = 0,        // C = v
  TG_SILU,           // C2 = v, C = silu(v)
  TG_GELU_DROP,      // C2 = v, C = drop(gelu(v))
  TG_DROP_RES,       // C = R + drop(v)
  TG_HEAD_RES,       // C2 = R + v, C = nan_to_num(R + v)
  TG_BWD_SILU,       // C = v * silu'(R)
  TG_BWD_GELU_DROP,  // C = v * drop factor * gelu'(R)
  TG_BWD_RES,        // C = v + R
  TG_HEAD,           // C2 = v, C = nan_to_num(v)
};

// the 32-deep step of a workgroup's 64 x 64 tile: wave (wm, wn) owns the 32 x 32 block at (32 wm, 32 wn) as 2 x 2 MFMA tiles
TAMF_DEV void tg_mma(const float* As, const float* Bs, int wm, int wn, int r, int g, f32x4 (&acc)[2][2]) {
  const float* ap = As + (wm * 32 + r) * TG_LD + g;
  const float* bp = Bs + (wn * 32 + r) * TG_LD + g;
#pragma unroll
  for (int kk = 0; kk < TG_K; kk += 4) {
    const float a0 = ap[kk], a1 = ap[16 * TG_LD + kk], b0 = bp[kk], b1 = bp[16 * TG_LD + kk];
    acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
    acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
    acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
    acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
  }
}

// C[cm(m) + n] = epilogue(sum_k A[am(m) + k] * W[n * swn + k * swk] + bias[n]), v = the sum with the bias.  Every load is guarded by
// (m < M, n < N, k < K): K and N need no padding and no alignment.
struct TgLin {
  const float* A;
  RowMap am;
  const float* W;
  long swn, swk;
  const float* bias;  // [N] or null
  float* C;
  RowMap cm;  // also the (clip, row) split of m for the dropout element: b = m / cm.G, row = m % cm.G
  float* C2;  // at cm as well
  const float* R;
  RowMap rm;
  int M, N, K, mode, site;
  Drop d;
};
template <bool WT>
__global__ __launch_bounds__(256) void tg_lin_kernel(const TgLin a) {
  __shared__ float As[TG_T * TG_LD], Ws[TG_T * TG_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.x * TG_T, n0 = blockIdx.y * TG_T;
  // the A tile: this thread loads column lc of the rows lr + 8 j; the W tile the same (WT: row n = tid & 63 at the columns wk + 4 j)
  const int lc = tid & 31, lr = tid >> 5, wl = tid & 63, wk = tid >> 6;
  long ab[8], wb[8];
  bool aok[8], wok[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int m = m0 + lr + 8 * j, n = n0 + lr + 8 * j;
    aok[j] = m < a.M;
    ab[j] = aok[j] ? a.am.at(m) : 0;
    wok[j] = WT ? n0 + wl < a.N : n < a.N;
    wb[j] = WT ? (long)(n0 + wl) * a.swn : (long)n * a.swn;
  }
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < a.K; k0 += TG_K) {
    float ra[8], rw[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int ka = k0 + lc, kw = WT ? k0 + wk + 4 * j : ka;
      ra[j] = aok[j] && ka < a.K ? a.A[ab[j] + ka] : 0.f;
      rw[j] = wok[j] && kw < a.K ? a.W[wb[j] + (long)kw * a.swk] : 0.f;
    }
    __syncthreads();  // the previous step's reads are done
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      As[(lr + 8 * j) * TG_LD + lc] = ra[j];
      if (WT) Ws[wl * TG_LD + wk + 4 * j] = rw[j];
      else Ws[(lr + 8 * j) * TG_LD + lc] = rw[j];
    }
    __syncthreads();
    tg_mma(As, Ws, wm, wn, r, g, acc);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn * 32 + j * 16 + r;
      if (n >= a.N) continue;
      const float bias = a.bias ? a.bias[n] : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int m = m0 + wm * 32 + i * 16 + 4 * g + e;
        if (m >= a.M) continue;
        const float v = acc[i][j][e] + bias;
        const int b = m / a.cm.G, row = m % a.cm.G;
        const long co = a.cm.at(m) + n;
        float o = v;
        switch (a.mode) {
          case TG_LIN: break;
          case TG_SILU:
            a.C2[co] = v;
            o = silu_exact(v);
            break;
          case TG_GELU_DROP:
            a.C2[co] = v;
            o = gelu_erf(v) * drop_factor(a.d, a.site, b, (uint32_t)row * a.N + n);
            break;
          case TG_DROP_RES: o = a.R[a.rm.at(m) + n] + v * drop_factor(a.d, a.site, b, (uint32_t)row * a.N + n); break;
          case TG_HEAD_RES:
            o = a.R[a.rm.at(m) + n] + v;
            a.C2[co] = o;
            o = nan_to_num(o);
            break;
          case TG_BWD_SILU: o = v * silu_grad(a.R[a.rm.at(m) + n]); break;
          case TG_BWD_GELU_DROP: o = v * drop_factor(a.d, a.site, b, (uint32_t)row * a.N + n) * gelu_grad(a.R[a.rm.at(m) + n]); break;
          case TG_BWD_RES: o = v + a.R[a.rm.at(m) + n]; break;
          case TG_HEAD:
            a.C2[co] = v;
            o = nan_to_num(v);
            break;
        }
        a.C[co] = o;
      }
    }
}

// part[s][n][k] = sum over the rows q of split s (rows s * chunk .. min(R, (s + 1) * chunk) - 1, ascending) of Y[ym(q) + n] * X[xm(q) + k],
// k < K; column k = K is the sum of Y itself.  chunk is a multiple of 32.
struct TgWgrad {
  const float* Y;
  RowMap ym;
  const float* X;
  RowMap xm;
  float* part;  // [nsplit][N][K + 1]
  int R, N, K, chunk;
};
__global__ __launch_bounds__(256) void tg_wgrad_kernel(const TgWgrad a) {
  __shared__ float Ys[TG_T * TG_LD], Xs[TG_T * TG_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  const int n0 = blockIdx.x * TG_T, k0 = blockIdx.y * TG_T, s = blockIdx.z, K1 = a.K + 1;
  const int r0 = s * a.chunk, r1 = min(a.R, r0 + a.chunk);
  const int cl = tid & 63, q4 = tid >> 6;  // this thread loads column cl (of Y: n, of X: k) of the rows q4 + 4 j of a step
  const int n = n0 + cl, k = k0 + cl;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int rb = r0; rb < r1; rb += TG_K) {
    float ry[8], rx[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int q = rb + q4 + 4 * j;
      const bool in = q < r1;
      ry[j] = in && n < a.N ? a.Y[a.ym.at(q) + n] : 0.f;
      rx[j] = !in ? 0.f : k < a.K ? a.X[a.xm.at(q) + k] : k == a.K ? 1.0f : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      Ys[cl * TG_LD + q4 + 4 * j] = ry[j];
      Xs[cl * TG_LD + q4 + 4 * j] = rx[j];
    }
    __syncthreads();
    tg_mma(Ys, Xs, wm, wn, r, g, acc);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int kk = k0 + wn * 32 + j * 16 + r;
      if (kk >= K1) continue;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int nn = n0 + wm * 32 + i * 16 + 4 * g + e;
        if (nn < a.N) a.part[((long)s * a.N + nn) * K1 + kk] = acc[i][j][e];
      }
    }
}
// pa[s][c], pb[s][c] = sum over the rows of split s of A[r * D + c], B[r * D + c] (LayerNorm gain / bias gradients).  Grid (nsplit,
// D / 64), block 256: wave w adds the rows r0 + w, r0 + w + 4, ... in ascending order, wave 0 adds the four sums in wave order.
__global__ __launch_bounds__(256) void tg_colsum2_kernel(const float* A, const float* B, int D, int R, int chunk, float* pa, float* pb) {
  __shared__ float sa[4][64], sb[4][64];
  const int s = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, c = blockIdx.y * 64 + lane;
  float va = 0.f, vb = 0.f;
  for (int r = s * chunk + wave; r < min(R, (s + 1) * chunk); r += 4) {
    va += A[(long)r * D + c];
    vb += B[(long)r * D + c];
  }
  sa[wave][lane] = va;
  sb[wave][lane] = vb;
  __syncthreads();
  if (wave == 0) {
    pa[(long)s * D + c] = ((sa[0][lane] + sa[1][lane]) + sa[2][lane]) + sa[3][lane];
    pb[(long)s * D + c] = ((sb[0][lane] + sb[1][lane]) + sb[2][lane]) + sb[3][lane];
  }
}

// ---- LayerNorm of D-wide rows (D = 64 NC, NC <= 8), one wave per row; biased variance, two passes, eps 1e-5 ----
constexpr int TG_MAXC = 8;
struct TgLnRow {
  float v[TG_MAXC], mean, rstd;
};
TAMF_DEV TgLnRow tg_ln_stats(const float* x, int D, int lane) {
  TgLnRow t;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < TG_MAXC; ++i) {
    t.v[i] = lane + 64 * i < D ? x[lane + 64 * i] : 0.f;
    s += t.v[i];
  }
  t.mean = wave_sum(s) / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < TG_MAXC; ++i) {
    const float dv = lane + 64 * i < D ? t.v[i] - t.mean : 0.f;
    q += dv * dv;
  }
  t.rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + 1e-5f);
  return t;
}
__global__ __launch_bounds__(256) void tg_ln_fwd_kernel(const float* X, float* Y, const float* gam, const float* bet, int M, int D) {
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (m >= M) return;
  const TgLnRow t = tg_ln_stats(X + (long)m * D, D, lane);
#pragma unroll
  for (int i = 0; i < TG_MAXC; ++i) {
    const int c = lane + 64 * i;
    if (c < D) Y[(long)m * D + c] = (t.v[i] - t.mean) * t.rstd * gam[c] + bet[c];
  }
}
// its backward from the pre-LayerNorm row: dz = d(pre), dym = dz * the dropout factor of `site` (the gradient of the linear output that
// was dropped out and added to the residual), tt = dy * xhat (summed over rows: the gain gradient).  S: token rows per clip.
__global__ __launch_bounds__(256) void tg_ln_bwd_kernel(const float* DY, const float* PRE, const float* gam, float* DZ, float* DYM, float* TT,
                                                        int M, int D, int S, int site, Drop d) {
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (m >= M) return;
  const long o = (long)m * D;
  const TgLnRow t = tg_ln_stats(PRE + o, D, lane);
  float dy[TG_MAXC], xh[TG_MAXC], s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < TG_MAXC; ++i) {
    const int c = lane + 64 * i;
    const bool in = c < D;
    dy[i] = in ? DY[o + c] : 0.f;
    xh[i] = in ? (t.v[i] - t.mean) * t.rstd : 0.f;
    const float gy = in ? dy[i] * gam[c] : 0.f;
    s1 += gy;
    s2 += gy * xh[i];
  }
  const float m1 = wave_sum(s1) / (float)D, m2 = wave_sum(s2) / (float)D;
  const int b = m / S, row = m % S;
#pragma unroll
  for (int i = 0; i < TG_MAXC; ++i) {
    const int c = lane + 64 * i;
    if (c >= D) continue;
    const float dz = t.rstd * (dy[i] * gam[c] - m1 - xh[i] * m2);
    DZ[o + c] = dz;
    DYM[o + c] = dz * drop_factor(d, site, b, (uint32_t)row * D + c);
    TT[o + c] = dy[i] * xh[i];
  }
}

// ---- attention at head dimension HD = 64 or 128.  QKV rows are [q(d) | k(d) | v(d)], head h at HD h; one wave per workgroup.  Lane
// (r, g) holds the HD / 4 contiguous floats of its row at column (HD / 4) g, as HD / 16 float4 ----
struct TgAttn {
  const float* qkv;   // [B][S][3 d]
  float* att;         // [B][S][d]    the attention output (forward: written; backward: read for delta)
  float* stat;        // [B][H][S][2] (max, sum) of the scaled scores
  const float* datt;  // [B][S][d]
  float* dqkv;        // [B][S][3 d]
  float* delta;       // [B][H][S]    sum_k P dP of every query = sum_j dO O of its head
  int S, H, site;
  Drop d;
};
template <class R>
TAMF_DEV float tg_row_reduce(float v) {  // over the 16 lanes r of a lane group; every lane gets the result
  v = R::op(v, dpp_mov<DPP_XOR1>(v));
  v = R::op(v, dpp_mov<DPP_XOR2>(v));
  v = R::op(v, dpp_mov<DPP_ROW_HALF_MIRROR>(v));
  return R::op(v, dpp_mov<DPP_ROW_MIRROR>(v));
}
// this lane's HD / 4 floats of a row; zeros for a row that is not there
template <int HD>
TAMF_DEV void tg_load_row(float4 (&q4)[HD / 16], bool in, const float* q) {
  const float4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const float4* qp = reinterpret_cast<const float4*>(q);
#pragma unroll
  for (int j = 0; j < HD / 16; ++j) q4[j] = in ? qp[j] : zero4;
}
// a 16 x 16 tile of q . k^T over the HD floats of a head, HD / 4 MFMAs -> element e: row 4g + e of q4's tile against row r of k's
// (unscaled)
template <int HD>
TAMF_DEV f32x4 tg_score_tile(const float4 (&q4)[HD / 16], const float* k, bool in) {
  float4 k4[HD / 16];
  tg_load_row<HD>(k4, in, k);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < HD / 16; ++j) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(q4[j].x, k4[j].x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(q4[j].y, k4[j].y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(q4[j].z, k4[j].z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(q4[j].w, k4[j].w, acc, 0, 0, 0);
  }
  return acc;
}
// acc[jt] += T . X over one 16-row tile: T the wave's 16 x 16 LDS tile (row r of this lane as the A operand), X the rows x0 .. x0 + 15
// of a [S][ld] buffer at column c0 (HD columns = HD / 16 output tiles), rows >= S contributing nothing
template <int HD>
TAMF_DEV void tg_tile_mma(const float* tile, const float* X, long ld, int x0, int S, int r, int g, f32x4 (&acc)[HD / 16]) {
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const int x = x0 + 4 * kk + g;
    const float av = tile[r * TG_PLD + 4 * kk + g];
    const float* xp = X + (long)x * ld + r;
#pragma unroll
    for (int jt = 0; jt < HD / 16; ++jt) acc[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, x < S ? xp[16 * jt] : 0.f, acc[jt], 0, 0, 0);
  }
}
template <int HD>
__global__ __launch_bounds__(64) void tg_attn_fwd_kernel(const TgAttn a) {
  constexpr int NQ = HD / 16, LC = HD / 4;  // float4 per lane, floats per lane
  __shared__ float tile[16 * TG_PLD];
  const int S = a.S, h = blockIdx.y, b = blockIdx.z, d = a.H * HD, lane = threadIdx.x, r = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * 16;
  const long ld = 3L * d;
  const float* base = a.qkv + (long)b * S * ld + h * HD;
  const float scale = 1.0f / sqrtf((float)HD);
  float4 q4[NQ];
  tg_load_row<HD>(q4, q0 + r < S, base + (long)min(q0 + r, S - 1) * ld + LC * g);
  float mx[4], sum[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) mx[e] = -__builtin_inff(), sum[e] = 0.f;
  for (int k0 = 0; k0 < S; k0 += 16) {
    const bool in = k0 + r < S;
    const f32x4 sc = tg_score_tile<HD>(q4, base + d + (long)min(k0 + r, S - 1) * ld + LC * g, in);
#pragma unroll
    for (int e = 0; e < 4; ++e) mx[e] = in ? fmaxf(mx[e], sc[e] * scale) : mx[e];
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) mx[e] = tg_row_reduce<RedMax>(mx[e]);
  f32x4 o[NQ];
#pragma unroll
  for (int jt = 0; jt < NQ; ++jt) o[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < S; k0 += 16) {
    const bool in = k0 + r < S;
    const f32x4 sc = tg_score_tile<HD>(q4, base + d + (long)min(k0 + r, S - 1) * ld + LC * g, in);
    __syncthreads();  // the previous tile's reads are done
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int q = q0 + 4 * g + e;
      const float p = in && q < S ? expf(sc[e] * scale - mx[e]) : 0.f;
      sum[e] += p;
      tile[(4 * g + e) * TG_PLD + r] = p == 0.f ? 0.f : p * drop_factor(a.d, a.site, b, (uint32_t)(h * S + q) * S + k0 + r);
    }
    __syncthreads();
    tg_tile_mma<HD>(tile, base + 2 * d, ld, k0, S, r, g, o);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int q = q0 + 4 * g + e;
    sum[e] = tg_row_reduce<RedSum>(sum[e]);
    if (q >= S) continue;
    const float inv = 1.0f / sum[e];
#pragma unroll
    for (int jt = 0; jt < NQ; ++jt) a.att[((long)b * S + q) * d + h * HD + 16 * jt + r] = o[jt][e] * inv;
    if (r == 0) {
      float* st = a.stat + (((long)b * a.H + h) * S + q) * 2;
      st[0] = mx[e];
      st[1] = sum[e];
    }
  }
}
// dQ of 16 query rows and their delta
template <int HD>
__global__ __launch_bounds__(64) void tg_attn_bwd_q_kernel(const TgAttn a) {
  constexpr int NQ = HD / 16, LC = HD / 4;
  __shared__ float tile[16 * TG_PLD], dl[16];
  const int S = a.S, h = blockIdx.y, b = blockIdx.z, d = a.H * HD, lane = threadIdx.x, r = lane & 15, g = lane >> 4;
  const int q0 = blockIdx.x * 16;
  const long ld = 3L * d;
  const float* base = a.qkv + (long)b * S * ld + h * HD;
  const float scale = 1.0f / sqrtf((float)HD);
  const bool qin = q0 + r < S;
  const long qr = (long)b * S + min(q0 + r, S - 1);
  float4 q4[NQ], do4[NQ];
  float dp = 0.f;
  {
    float4 o4[NQ];  // (only for delta)
    tg_load_row<HD>(q4, qin, base + (qr - (long)b * S) * ld + LC * g);
    tg_load_row<HD>(do4, qin, a.datt + qr * d + h * HD + LC * g);
    tg_load_row<HD>(o4, qin, a.att + qr * d + h * HD + LC * g);
#pragma unroll
    for (int j = 0; j < NQ; ++j) dp += do4[j].x * o4[j].x + do4[j].y * o4[j].y + do4[j].z * o4[j].z + do4[j].w * o4[j].w;
  }
  dp = groups_reduce<RedSum>(dp);  // query q0 + r
  if (g == 0) {
    dl[r] = dp;
    if (qin) a.delta[((long)b * a.H + h) * S + q0 + r] = dp;
  }
  __syncthreads();
  float mx[4], inv[4], del[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int q = min(q0 + 4 * g + e, S - 1);
    const float* st = a.stat + (((long)b * a.H + h) * S + q) * 2;
    mx[e] = st[0];
    inv[e] = 1.0f / st[1];
    del[e] = dl[4 * g + e];
  }
  f32x4 acc[NQ];
#pragma unroll
  for (int jt = 0; jt < NQ; ++jt) acc[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < S; k0 += 16) {
    const bool in = k0 + r < S;
    const long kr = (long)min(k0 + r, S - 1) * ld + LC * g;
    const f32x4 sc = tg_score_tile<HD>(q4, base + d + kr, in);
    const f32x4 dpv = tg_score_tile<HD>(do4, base + 2 * d + kr, in);
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int q = q0 + 4 * g + e;
      float ds = 0.f;
      if (in && q < S) {
        const float p = expf(sc[e] * scale - mx[e]) * inv[e];
        ds = p * (dpv[e] * drop_factor(a.d, a.site, b, (uint32_t)(h * S + q) * S + k0 + r) - del[e]);
      }
      tile[(4 * g + e) * TG_PLD + r] = ds;
    }
    __syncthreads();
    tg_tile_mma<HD>(tile, base + d, ld, k0, S, r, g, acc);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int q = q0 + 4 * g + e;
    if (q >= S) continue;
#pragma unroll
    for (int jt = 0; jt < NQ; ++jt) a.dqkv[((long)b * S + q) * ld + h * HD + 16 * jt + r] = acc[jt][e] * scale;
  }
}
// dK and dV of 16 key rows: the query tiles in ascending order
template <int HD>
__global__ __launch_bounds__(64) void tg_attn_bwd_kv_kernel(const TgAttn a) {
  constexpr int NQ = HD / 16, LC = HD / 4;
  __shared__ float tp[16 * TG_PLD], td[16 * TG_PLD];
  const int S = a.S, h = blockIdx.y, b = blockIdx.z, d = a.H * HD, lane = threadIdx.x, r = lane & 15, g = lane >> 4;
  const int k0 = blockIdx.x * 16;
  const long ld = 3L * d;
  const float* base = a.qkv + (long)b * S * ld + h * HD;
  const float* dob = a.datt + (long)b * S * d + h * HD;
  const float scale = 1.0f / sqrtf((float)HD);
  float4 k4[NQ], v4[NQ];
  const long kr = (long)min(k0 + r, S - 1) * ld + LC * g;
  tg_load_row<HD>(k4, k0 + r < S, base + d + kr);
  tg_load_row<HD>(v4, k0 + r < S, base + 2 * d + kr);
  f32x4 dk[NQ], dv[NQ];
#pragma unroll
  for (int jt = 0; jt < NQ; ++jt) dk[jt] = dv[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* st = a.stat + ((long)b * a.H + h) * S * 2;
  const float* dl = a.delta + ((long)b * a.H + h) * S;
  for (int q0 = 0; q0 < S; q0 += 16) {
    const int q = q0 + r, qc = min(q, S - 1);
    const bool in = q < S;
    const f32x4 sc = tg_score_tile<HD>(k4, base + (long)qc * ld + LC * g, in);    // element e: key 4g + e against query r
    const f32x4 dpv = tg_score_tile<HD>(v4, dob + (long)qc * d + LC * g, in);
    const float mx = st[2 * qc], inv = 1.0f / st[2 * qc + 1], del = dl[qc];
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int k = k0 + 4 * g + e;
      float pd = 0.f, ds = 0.f;
      if (in && k < S) {
        const float p = expf(sc[e] * scale - mx) * inv;
        const float f = drop_factor(a.d, a.site, b, (uint32_t)(h * S + q) * S + k);
        pd = p * f;
        ds = p * (dpv[e] * f - del) * scale;
      }
      tp[(4 * g + e) * TG_PLD + r] = pd;
      td[(4 * g + e) * TG_PLD + r] = ds;
    }
    __syncthreads();
    tg_tile_mma<HD>(tp, dob, d, q0, S, r, g, dv);
    tg_tile_mma<HD>(td, base, ld, q0, S, r, g, dk);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int k = k0 + 4 * g + e;
    if (k >= S) continue;
    float* o = a.dqkv + ((long)b * S + k) * ld + h * HD;
#pragma unroll
    for (int jt = 0; jt < NQ; ++jt) {
      o[d + 16 * jt + r] = dk[jt][e];
      o[2 * d + 16 * jt + r] = dv[jt][e];
    }
  }
}
