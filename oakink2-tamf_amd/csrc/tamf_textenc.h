// CLIP text tower (libtamf_textenc.so, include/tamf_textenc.h) - the kernels.  Float32 activations throughout: one-time preprocessing
// whose output (one embed_dim-vector per prompt) conditions every later stage, so every choice here prefers a fixed, simple
// arithmetic order over speed.
//
// The causal mask makes row t of a prompt a function of rows 0 .. t only, and the output is read at the EOT row: a prompt whose EOT
// sits at position e costs e + 1 rows.  The host packs those rows of all prompts behind one another (M = sum(e_b + 1) rows) and
// uploads the row map; every kernel below works on the packed rows.
//
//   embed_kernel     x[m] = token_embedding[id[m]] + positional_embedding[pos[m]]
//   ln_kernel        LayerNorm of a row (two passes, biased variance, eps 1e-5), one wave per row; with a row map it reads the B EOT
//                    rows only and writes them compactly (the tail)
//   gemm_kernel      C = epi(A . W^T): 64 x 64 tile per workgroup, K in steps of 32 through LDS, v_mfma_f32_16x16x4_f32, k ascending.
//                    An output element is ONE accumulator chain over its own A row and W row, so its bits do not depend on which
//                    tile its packed row landed in.  Epilogues: + bias, + bias then QuickGELU, + bias then residual add.  The grid's
//                    x axis walks the row tiles, so the workgroups that are in flight together share one 64-row weight panel: it
//                    comes from HBM once per call and serves all M rows (never once per prompt).
//   attn_kernel      causal softmax(scale q k^T) v, one workgroup per (prompt, head): the prompt's K and V rows of that head resident
//                    in LDS, a 16-query block per wave, the 16 x L score panel in LDS (exact two-pass softmax over columns <= query),
//                    both contractions on the MFMA; masked columns enter the second one as exact zeros (p = 0 against finite or
//                    zero-filled v).  Rows of different prompts never meet.
//
// Nothing is reduced with atomics and no launch parameter enters an operand: a prompt's output bits depend on its ids up to the EOT
// position and on the model.
#pragma once
#include "tamf_device.h"

constexpr int TE_NT = 256;
constexpr int TE_GT = 64, TE_GK = 32, TE_GLD = TE_GK + 4;  // gemm tile, k step, LDS row stride (floats)
constexpr int TE_HD = 64;                                    // head dimension
constexpr int TE_KLD = TE_HD + 4;                            // LDS row stride of the resident K and V rows (floats)
constexpr int TE_CTX_MAX = 128;
// row stride of a wave's score panel (floats) for prompts of up to Lp rows (Lp a multiple of 16): 4 mod 16
__host__ __device__ inline int te_att_ss(int Lp) { return Lp + 4; }
// dynamic LDS of attn_kernel (floats): K and V of Lp rows, four score panels of 16 rows, 16 reciprocal sums per wave
__host__ __device__ inline int te_att_lds_floats(int Lp) { return 2 * Lp * TE_KLD + (TE_NT / 64) * (16 * te_att_ss(Lp) + 16); }

TAMF_DEV float quick_gelu(float v) { return v / (1.0f + expf(-1.702f * v)); }

// x (M, W) = tok[id[m]] + pos[p[m]]
__global__ __launch_bounds__(TE_NT) void embed_kernel(const float* __restrict__ tok, const float* __restrict__ pos, const int* __restrict__ ids,
                                                      const int* __restrict__ posidx, float* __restrict__ x, long M, int W) {
  const long e = (long)blockIdx.x * TE_NT + threadIdx.x;
  if (e >= M * W) return;
  const long m = e / W;
  const int c = (int)(e % W);
  x[e] = tok[(long)ids[m] * W + c] + pos[(long)posidx[m] * W + c];
}

// y[i] = LayerNorm(x[rowmap ? rowmap[i] : i]) * g + b for i < rows; biased variance, two passes, eps 1e-5.  One wave per row.
__global__ __launch_bounds__(TE_NT) void ln_kernel(const float* __restrict__ x, const int* __restrict__ rowmap, const float* __restrict__ gam,
                                                   const float* __restrict__ bet, float* __restrict__ y, long rows, int D) {
  const long row = (long)blockIdx.x * (TE_NT / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const float* xr = x + (rowmap ? (long)rowmap[row] : row) * D;
  float s = 0.f;
  for (int c = lane; c < D; c += 64) s += xr[c];
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
  for (int c = lane; c < D; c += 64) {
    const float dv = xr[c] - mean;
    q += dv * dv;
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + 1e-5f);
  for (int c = lane; c < D; c += 64) y[row * D + c] = (xr[c] - mean) * rstd * gam[c] + bet[c];
}

struct TeGemm {
  const float* A;     // [M][lda]
  const float* W;     // [N][ldw]
  const float* bias;  // [N] or null
  float* C;           // [M][ldc]
  int lda, ldw, ldc, M, N, K;  // K a multiple of 32, lda and ldw multiples of 4
  int act;    // 0 none, 1 QuickGELU
  int resid;  // C += result
};

__global__ __launch_bounds__(TE_NT) void gemm_kernel(const TeGemm a) {
  __shared__ float4 As4[TE_GT * TE_GLD / 4], Ws4[TE_GT * TE_GLD / 4];
  float* As = reinterpret_cast<float*>(As4);
  float* Ws = reinterpret_cast<float*>(Ws4);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  const long m0 = (long)blockIdx.x * TE_GT;
  const int n0 = blockIdx.y * TE_GT;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < a.K; k0 += TE_GK) {
    float4 ra[2], rw[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int idx = tid + j * TE_NT, row = idx >> 3, c4 = (idx & 7) * 4;
      const bool kin = k0 + c4 < a.K;
      ra[j] = (kin && m0 + row < a.M) ? *reinterpret_cast<const float4*>(a.A + (m0 + row) * a.lda + k0 + c4) : float4{0.f, 0.f, 0.f, 0.f};
      rw[j] = (kin && n0 + row < a.N) ? *reinterpret_cast<const float4*>(a.W + (long)(n0 + row) * a.ldw + k0 + c4) : float4{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();  // the previous step's reads are done
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int idx = tid + j * TE_NT, row = idx >> 3, c4 = (idx & 7) * 4;
      *reinterpret_cast<float4*>(As + row * TE_GLD + c4) = ra[j];
      *reinterpret_cast<float4*>(Ws + row * TE_GLD + c4) = rw[j];
    }
    __syncthreads();
    const float* ap = As + (wm * 32 + r) * TE_GLD + g;
    const float* wp = Ws + (wn * 32 + r) * TE_GLD + g;
#pragma unroll
    for (int kk = 0; kk < TE_GK; kk += 4) {
      const float a0 = ap[kk], a1 = ap[16 * TE_GLD + kk], b0 = wp[kk], b1 = wp[16 * TE_GLD + kk];
      acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + wn * 32 + j * 16 + r;
      if (col >= a.N) continue;
      const float bias = a.bias ? a.bias[col] : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const long row = m0 + wm * 32 + i * 16 + 4 * g + e;
        if (row >= a.M) continue;
        float v = acc[i][j][e] + bias;
        if (a.act == 1) v = quick_gelu(v);
        float* dst = a.C + row * a.ldc + col;
        *dst = a.resid ? *dst + v : v;
      }
    }
}

// qkv (M, 3D) with columns [q | k | v], each D = H * 64 wide, head h at h * 64  ->  o (M, D).  Prompt b owns the packed rows
// [start[b], start[b] + len[b]), 1 <= len[b] <= Lp <= 128, Lp a multiple of 16.  grid (H, B).  Dynamic LDS: te_att_lds_floats(Lp).
// Query i attends to keys 0 .. i.  The contraction index of q . k is permuted (lane group g covers k = 16g .. 16g + 15, so that a lane
// reads 64 contiguous bytes); the order is the same for every score.  Everything a query row's result is made of - its score columns,
// the softmax trees over them, the P.V chain over the 16 (i / 16 + 1) keys of its block - is fixed by i alone, not by len[b].
__global__ __launch_bounds__(TE_NT) void attn_kernel(const float* __restrict__ qkv, const int* __restrict__ start, const int* __restrict__ len,
                                                     float* __restrict__ o, int D, int Lp, float scale) {
  extern __shared__ float4 te_att_lds4[];
  float* Ks = reinterpret_cast<float*>(te_att_lds4);
  float* Vs = Ks + Lp * TE_KLD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int Ss = te_att_ss(Lp);
  float* S = Vs + Lp * TE_KLD + wave * (16 * Ss + 16);
  float* inv = S + 16 * Ss;
  const int h = blockIdx.x;
  const long base = start[blockIdx.y];
  int L = len[blockIdx.y];
  L = L < 1 ? 1 : (L > Lp ? Lp : L);
  const long ld = 3L * D;
  const float4 zero4 = {0.f, 0.f, 0.f, 0.f};
  // ---- K and V of the head into LDS; rows L .. Lp - 1 are zeros ----
  for (int idx = tid; idx < Lp * (TE_HD / 4); idx += TE_NT) {
    const int row = idx >> 4, c4 = (idx & 15) * 4;
    const float* src = qkv + (base + row) * ld + D + h * TE_HD + c4;
    const bool in = row < L;
    *reinterpret_cast<float4*>(Ks + row * TE_KLD + c4) = in ? *reinterpret_cast<const float4*>(src) : zero4;
    *reinterpret_cast<float4*>(Vs + row * TE_KLD + c4) = in ? *reinterpret_cast<const float4*>(src + D) : zero4;
  }
  __syncthreads();
  // ---- 16-query blocks, one per wave and round; every wave runs every round (the barriers are uniform) ----
  for (int qb0 = 0; qb0 * 16 < L; qb0 += TE_NT / 64) {
    const int q0 = (qb0 + wave) * 16;
    const bool active = q0 < L;
    const int kend = q0 + 16;  // keys this block can see, a multiple of 16, <= Lp
    if (active) {
      float4 q4[4];
      {
        const bool in = q0 + r < L;
        const float4* qp = reinterpret_cast<const float4*>(qkv + (base + q0 + r) * ld + h * TE_HD + g * 16);
#pragma unroll
        for (int j = 0; j < 4; ++j) q4[j] = in ? qp[j] : zero4;
      }
      for (int nt = 0; nt * 16 < kend; ++nt) {
        const int key = nt * 16 + r;
        const float4* kp = reinterpret_cast<const float4*>(Ks + key * TE_KLD + g * 16);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float4 k4 = kp[j];
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(q4[j].x, k4.x, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(q4[j].y, k4.y, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(q4[j].z, k4.z, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_16x16x4f32(q4[j].w, k4.w, acc, 0, 0, 0);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) S[(4 * g + e) * Ss + key] = acc[e] * scale;
      }
    }
    __syncthreads();
    if (active) {
      // softmax of each row over columns <= its query: 4 lanes per row, columns sub, sub + 4, ... in ascending order, then the quad
      const int row = lane >> 2, sub = lane & 3, qi = q0 + row;
      float* sr = S + row * Ss;
      float mx = -__builtin_inff();
      for (int c = sub; c <= qi; c += 4) mx = fmaxf(mx, sr[c]);
      mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
      mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
      float sum = 0.f;
      for (int c = sub; c < kend; c += 4) {
        float p = 0.f;  // a masked column: an exact zero in the P.V product
        if (c <= qi) {
          p = expf(sr[c] - mx);
          sum += p;
        }
        sr[c] = p;
      }
      sum += __shfl_xor(sum, 1, 64);
      sum += __shfl_xor(sum, 2, 64);
      if (sub == 0) inv[row] = 1.0f / sum;
    }
    __syncthreads();
    if (active) {
      // out (16 x 64) = P (16 x kend) . V (kend x 64): four column tiles, one accumulator chain each, k ascending
      const float* sp = S + r * Ss + g;
#pragma unroll
      for (int n = 0; n < TE_HD / 16; ++n) {
        const float* vp = Vs + g * TE_KLD + n * 16 + r;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < kend; k0 += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(sp[k0], vp[k0 * TE_KLD], acc, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int q = q0 + 4 * g + e;
          if (q < L) o[(base + q) * D + h * TE_HD + n * 16 + r] = acc[e] * inv[4 * g + e];
        }
      }
    }
    __syncthreads();  // the panel is free for the next round
  }
}
