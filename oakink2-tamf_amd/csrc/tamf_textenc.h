// CLIP text tower (libtamf_textenc.so, include/tamf_textenc.h) - the kernels.  Float32 activations throughout: one-time preprocessing
// whose output (one embed_dim-vector per prompt) conditions every later stage, so every choice here prefers a fixed, simple
// arithmetic order over speed.
//
// The causal mask makes row t of a prompt a function of rows 0 .. t only, and the output is read at the EOT row: a prompt whose EOT
// sits at position e costs e + 1 rows.  The host packs those rows of all prompts behind one another (M = sum(e_b + 1) rows) and
// uploads the row map; every kernel below works on the packed rows.
//
//   embed_kernel     x[m] = token_embedding[id[m]] + positional_embedding[pos[m]]
//   ln_kernel        LayerNorm of a row (f32_ln_row), one wave per row; with a row map it reads the B EOT rows only and writes them
//                    compactly (the tail)
//   TeEpi            the epilogue of csrc/tamf_f32_tower.h's f32_gemm_kernel (the shared fp32 GEMM; why an output element's bits do
//                    not depend on which tile its packed row landed in is explained there): nothing, QuickGELU, or a residual add
//                    behind + bias.  The grid's x axis walks the row tiles, so the workgroups that are in flight together share one
//                    64-row weight panel: it comes from HBM once per call and serves all M rows (never once per prompt).
//   attn_kernel      causal softmax(scale q k^T) v, one workgroup per (prompt, head): the prompt's K and V rows of that head resident
//                    in LDS, a 16-query block per wave, the 16 x L score panel in LDS (exact two-pass softmax over columns <= query),
//                    both contractions on the MFMA; masked columns enter the second one as exact zeros (p = 0 against finite or
//                    zero-filled v).  Rows of different prompts never meet.
//
// Nothing is reduced with atomics and no launch parameter enters an operand: a prompt's output bits depend on its ids up to the EOT
// position and on the model.
#pragma once
#include "tamf_f32_tower.h"

constexpr int TE_KLD = F32_HD + 4;  // LDS row stride of the resident K and V rows (floats)
constexpr int TE_CTX_MAX = 128;
// row stride of a wave's score panel (floats) for prompts of up to Lp rows (Lp a multiple of 16): 4 mod 16
__host__ __device__ inline int te_att_ss(int Lp) { return Lp + 4; }
// dynamic LDS of attn_kernel (floats): K and V of Lp rows, four score panels of 16 rows, 16 reciprocal sums per wave
__host__ __device__ inline int te_att_lds_floats(int Lp) { return 2 * Lp * TE_KLD + (F32_NT / 64) * (16 * te_att_ss(Lp) + 16); }

TAMF_DEV float quick_gelu(float v) { return v / (1.0f + expf(-1.702f * v)); }

// x (M, W) = tok[id[m]] + pos[p[m]]
__global__ __launch_bounds__(F32_NT) void embed_kernel(const float* __restrict__ tok, const float* __restrict__ pos, const int* __restrict__ ids,
                                                       const int* __restrict__ posidx, float* __restrict__ x, long M, int W) {
  const long e = (long)blockIdx.x * F32_NT + threadIdx.x;
  if (e >= M * W) return;
  const long m = e / W;
  const int c = (int)(e % W);
  x[e] = tok[(long)ids[m] * W + c] + pos[(long)posidx[m] * W + c];
}

// y[i] = LayerNorm(x[rowmap ? rowmap[i] : i]) * g + b for i < rows (f32_ln_row).  One wave per row.
__global__ __launch_bounds__(F32_NT) void ln_kernel(const float* __restrict__ x, const int* __restrict__ rowmap, const float* __restrict__ gam,
                                                    const float* __restrict__ bet, float* __restrict__ y, long rows, int D) {
  const long row = (long)blockIdx.x * (F32_NT / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  const float* xr = x + (rowmap ? (long)rowmap[row] : row) * D;
  float s = 0.f;
  for (int c = lane; c < D; c += 64) s += xr[c];
  f32_ln_row(xr, s, gam, bet, y + row * D, D, lane);
}

// what follows acc + bias in the text tower's products (f32_gemm_kernel<TeEpi>), in this order
struct TeEpi {
  int act;    // 0 none, 1 QuickGELU
  int resid;  // C += result
  __device__ void operator()(const F32Gemm& a, long row, int col, float v) const {
    if (act == 1) v = quick_gelu(v);
    float* dst = a.C + row * a.ldc + col;
    *dst = resid ? *dst + v : v;
  }
};

// qkv (M, 3D) with columns [q | k | v], each D = H * 64 wide, head h at h * 64  ->  o (M, D).  Prompt b owns the packed rows
// [start[b], start[b] + len[b]), 1 <= len[b] <= Lp <= 128, Lp a multiple of 16.  grid (H, B).  Dynamic LDS: te_att_lds_floats(Lp).
// Query i attends to keys 0 .. i.  Scores by f32_score_tile (the permuted contraction order is explained there), K from LDS.
// Everything a query row's result is made of - its score columns,
// the softmax trees over them, the P.V chain over the 16 (i / 16 + 1) keys of its block - is fixed by i alone, not by len[b].
__global__ __launch_bounds__(F32_NT) void attn_kernel(const float* __restrict__ qkv, const int* __restrict__ start, const int* __restrict__ len,
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
  for (int idx = tid; idx < Lp * (F32_HD / 4); idx += F32_NT) {
    const int row = idx >> 4, c4 = (idx & 15) * 4;
    const float* src = qkv + (base + row) * ld + D + h * F32_HD + c4;
    const bool in = row < L;
    *reinterpret_cast<float4*>(Ks + row * TE_KLD + c4) = in ? *reinterpret_cast<const float4*>(src) : zero4;
    *reinterpret_cast<float4*>(Vs + row * TE_KLD + c4) = in ? *reinterpret_cast<const float4*>(src + D) : zero4;
  }
  __syncthreads();
  // ---- 16-query blocks, one per wave and round; every wave runs every round (the barriers are uniform) ----
  for (int qb0 = 0; qb0 * 16 < L; qb0 += F32_NT / 64) {
    const int q0 = (qb0 + wave) * 16;
    const bool active = q0 < L;
    const int kend = q0 + 16;  // keys this block can see, a multiple of 16, <= Lp
    if (active) {
      float4 q4[4];
      f32_load_q(q4, q0 + r < L, qkv + (base + q0 + r) * ld + h * F32_HD + g * 16);
      for (int nt = 0; nt * 16 < kend; ++nt) {
        const int key = nt * 16 + r;
        const f32x4 acc = f32_score_tile(q4, Ks + key * TE_KLD + g * 16, true);
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
      for (int n = 0; n < F32_HD / 16; ++n) {
        const float* vp = Vs + g * TE_KLD + n * 16 + r;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        for (int k0 = 0; k0 < kend; k0 += 4) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(sp[k0], vp[k0 * TE_KLD], acc, 0, 0, 0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int q = q0 + 4 * g + e;
          if (q < L) o[(base + q) * D + h * F32_HD + n * 16 + r] = acc[e] * inv[4 * g + e];
        }
      }
    }
    __syncthreads();  // the panel is free for the next round
  }
}
