// PointBERT point encoder (libtamf_pointenc.so, include/tamf_pointenc.h) - the kernels.  Eval mode, fp32 throughout: this is one-time
// preprocessing whose output (one 768-vector per object) conditions every later stage, so every choice here prefers a fixed, simple
// arithmetic order over speed.
//
//   fps_kernel       farthest-point sampling, one workgroup of 1024 threads per cloud.  A thread owns points tid, tid + 1024, ... in
//                    registers for all G iterations (N <= 16384; above that the registers do not hold 32 points per thread without
//                    spilling, and the coordinates are re-read through L2 - the cloud is 384 KiB); the running minima live in LDS
//                    (each thread touches only its own).  The squared
//                    distance is ((dx*dx + dy*dy) + dz*dz) with every product and sum rounded on its own (no FMA contraction: the
//                    selection is chaotic in the last bit).  Argmax: largest running minimum, ties to the lowest index - one 64-bit
//                    key (distance bits | ~index) reduced by max over the wave and then over the 16 waves.
//   group_kernel     the M nearest points of one centre per workgroup: N direct squared distances (the same expression) into LDS,
//                    then M rounds of a 64-bit (distance bits | index) minimum - ascending (distance, index) order by construction.
//   PeEpi            the epilogue of csrc/tamf_f32_tower.h's f32_gemm_kernel (the shared fp32 GEMM; why an output element's bits do
//                    not depend on where its row sits in the batch is explained there): + a per-group row (the global half of the
//                    512 -> 512 layer, applied once per group), ReLU / exact-erf GELU, optional row remap (group g of cloud b -> token
//                    row 1 + g), residual add.
//   attn_kernel      softmax(scale q k^T) v for 16 queries of one (cloud, head) per workgroup, head dimension 64, up to 1025 tokens:
//                    the 16 x T score panel in LDS (exact two-pass softmax, no running rescale), both contractions on the MFMA.
//   row kernels      gather (centre subtracted from xyz only), max over a group, LayerNorm (optionally x += pos first), cls rows,
//                    cat(cls, max over group tokens).
//
// Nothing is reduced with atomics and no launch parameter enters an operand: a cloud's output bits depend on the cloud and the model.
#pragma once
#include "tamf_f32_tower.h"

constexpr int PE_FPS_NT = 1024;
constexpr int PE_AQ = 16;  // queries per attention workgroup
// row stride of the attention score panel (floats): >= round_up(T, 4), and 4 mod 32 so that the 16 rows of an MFMA A fragment
// fall into 16 different 4-bank groups
__host__ __device__ inline int pe_att_ts(int T) { return (((T + 3) & ~3) + 31) / 32 * 32 + 4; }

TAMF_DEV float pe_sqdist(float ax, float ay, float az, float bx, float by, float bz) {
#pragma clang fp contract(off)
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  const float xx = dx * dx, yy = dy * dy, zz = dz * dz;
  const float s = xx + yy;
  return s + zz;
}

TAMF_DEV unsigned long long pe_wave_max_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o, 64);
    v = w > v ? w : v;
  }
  return v;
}
TAMF_DEV unsigned long long pe_wave_min_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const unsigned long long w = __shfl_xor(v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}

// points (B, N, C) f32, start (B) i32 in [0, N) -> idx_out (B, G).  Dynamic LDS: N floats.  PPT * 1024 >= N.  REG: the thread's
// points are kept in registers.
template <int PPT, bool REG>
__global__ __launch_bounds__(PE_FPS_NT) void fps_kernel(const float* __restrict__ pts, const int* __restrict__ start, int* __restrict__ out,
                                                        int N, int C, int G) {
  extern __shared__ float pe_fps_lds[];
  __shared__ unsigned long long red[2][PE_FPS_NT / 64];
  float* mind = pe_fps_lds;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* P = pts + (long)blockIdx.x * N * C;
  constexpr int NR = REG ? PPT : 1, UNR = REG ? PPT : 4;
  float px[NR], py[NR], pz[NR];
#pragma unroll
  for (int k = 0; k < PPT; ++k) {
    const int i = tid + k * PE_FPS_NT;
    const bool in = i < N;
    if (REG) {
      px[k] = in ? P[(long)i * C] : 0.f;
      py[k] = in ? P[(long)i * C + 1] : 0.f;
      pz[k] = in ? P[(long)i * C + 2] : 0.f;
    }
    if (in) mind[i] = 1e10f;
  }
  int far = start[blockIdx.x];
  far = (unsigned)far < (unsigned)N ? far : 0;
  for (int it = 0; it < G; ++it) {
    if (tid == 0) out[(long)blockIdx.x * G + it] = far;
    if (it == G - 1) break;
    const float cx = P[(long)far * C], cy = P[(long)far * C + 1], cz = P[(long)far * C + 2];
    unsigned long long best = 0;
#pragma unroll UNR
    for (int k = 0; k < PPT; ++k) {
      const int i = tid + k * PE_FPS_NT;
      if (i < N) {
        const float x = REG ? px[k] : P[(long)i * C], y = REG ? py[k] : P[(long)i * C + 1], z = REG ? pz[k] : P[(long)i * C + 2];
        const float m = fminf(mind[i], pe_sqdist(x, y, z, cx, cy, cz));
        mind[i] = m;
        const unsigned long long key = ((unsigned long long)__builtin_bit_cast(unsigned, m) << 32) | (0xFFFFFFFFu - (unsigned)i);
        best = key > best ? key : best;
      }
    }
    best = pe_wave_max_u64(best);
    if (lane == 0) red[it & 1][wave] = best;
    __syncthreads();
    unsigned long long b = red[it & 1][0];
#pragma unroll
    for (int w = 1; w < PE_FPS_NT / 64; ++w) {
      const unsigned long long v = red[it & 1][w];
      b = v > b ? v : b;
    }
    far = (int)(0xFFFFFFFFu - (unsigned)(b & 0xFFFFFFFFu));
  }
}

// points (B, N, C), centre_idx (B, G) -> nbr_out (B, G, M): one workgroup per centre.  Dynamic LDS: N floats.  M <= N.
__global__ __launch_bounds__(F32_NT) void group_kernel(const float* __restrict__ pts, const int* __restrict__ cidx, int* __restrict__ out,
                                                       int N, int C, int G, int M) {
  extern __shared__ float pe_grp_lds[];
  __shared__ unsigned long long red[2][F32_NT / 64];
  float* d = pe_grp_lds;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x / G;
  const float* P = pts + (long)b * N * C;
  int ci = cidx[blockIdx.x];
  ci = (unsigned)ci < (unsigned)N ? ci : 0;
  const float cx = P[(long)ci * C], cy = P[(long)ci * C + 1], cz = P[(long)ci * C + 2];
  for (int i = tid; i < N; i += F32_NT) d[i] = pe_sqdist(P[(long)i * C], P[(long)i * C + 1], P[(long)i * C + 2], cx, cy, cz);
  // (a thread reads and marks only its own elements until the reduction: no barrier needed before the first round)
  for (int m = 0; m < M; ++m) {
    unsigned long long best = ~0ull;
    for (int i = tid; i < N; i += F32_NT) {
      const unsigned long long key = ((unsigned long long)__builtin_bit_cast(unsigned, d[i]) << 32) | (unsigned)i;
      best = key < best ? key : best;
    }
    best = pe_wave_min_u64(best);
    if (lane == 0) red[m & 1][wave] = best;
    __syncthreads();
    unsigned long long r = red[m & 1][0];
#pragma unroll
    for (int w = 1; w < F32_NT / 64; ++w) {
      const unsigned long long v = red[m & 1][w];
      r = v < r ? v : r;
    }
    const int sel = (int)(unsigned)(r & 0xFFFFFFFFu);
    if (tid == 0) out[(long)blockIdx.x * M + m] = sel;
    if (sel % F32_NT == tid) d[sel] = __builtin_bit_cast(float, 0xFFFFFFFFu);  // above every distance key; its owner marks it
  }
}

// x0 (B*G*M, Cp) = [xyz(nbr) - xyz(centre) | other channels of nbr | 0];  c0 (B*G, 4) = [xyz(centre) | 0]
__global__ __launch_bounds__(F32_NT) void gather_kernel(const float* __restrict__ pts, const int* __restrict__ cidx, const int* __restrict__ nidx,
                                                        float* __restrict__ x0, float* __restrict__ c0, long rows, int N, int C, int Cp, int G, int M) {
  const long e = (long)blockIdx.x * F32_NT + threadIdx.x;
  if (e >= rows * Cp) return;
  const long row = e / Cp;
  const int c = (int)(e % Cp);
  const long grp = row / M, b = grp / G;
  const float* P = pts + b * N * C;
  int ci = cidx[grp], ni = nidx[row];
  ci = (unsigned)ci < (unsigned)N ? ci : 0;
  ni = (unsigned)ni < (unsigned)N ? ni : 0;
  float v = 0.f;
  if (c < 3) v = P[(long)ni * C + c] - P[(long)ci * C + c];
  else if (c < C) v = P[(long)ni * C + c];
  x0[e] = v;
  if (row % M == 0 && c < 4) c0[grp * 4 + c] = c < 3 ? P[(long)ci * C + c] : 0.f;
}

// out (groups, W) = max over the M rows of each group of in (groups * M, W), rows in ascending order
__global__ __launch_bounds__(F32_NT) void groupmax_kernel(const float* __restrict__ in, float* __restrict__ out, long groups, int M, int W) {
  const long e = (long)blockIdx.x * F32_NT + threadIdx.x;
  if (e >= groups * W) return;
  const long grp = e / W;
  const int c = (int)(e % W);
  const float* p = in + grp * M * W + c;
  float m = p[0];
  for (int i = 1; i < M; ++i) m = fmaxf(m, p[(long)i * W]);
  out[e] = m;
}

// what follows acc + bias in the point encoder's products (f32_gemm_kernel<PeEpi>), in this order
struct PeEpi {
  const float* radd;  // [M / rgrp][N] or null: added to every row of its group
  int act;            // 0 none, 1 ReLU, 2 exact GELU
  int rgrp;           // rows per radd row
  int resid;          // C += result
  int tokmap;         // > 0: output row = row + row / tokmap + 1 (group rows -> token rows behind each cloud's cls row)
  __device__ void operator()(const F32Gemm& a, long row, int col, float v) const {
    if (radd) v += radd[(row / rgrp) * a.N + col];
    if (act == 1) v = fmaxf(v, 0.f);
    else if (act == 2) v = gelu_erf(v);
    const long orow = tokmap > 0 ? row + row / tokmap + 1 : row;
    float* dst = a.C + orow * a.ldc + col;
    *dst = resid ? *dst + v : v;
  }
};

// x (rows, D): if pos: x += pos (stored, fused into the pass that sums the row); y = LayerNorm(x) * g + b (f32_ln_row).  One wave per row.
__global__ __launch_bounds__(F32_NT) void ln_kernel(float* __restrict__ x, const float* __restrict__ pos, const float* __restrict__ gam,
                                                    const float* __restrict__ bet, float* __restrict__ y, long rows, int D) {
  const long row = (long)blockIdx.x * (F32_NT / 64) + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int lane = threadIdx.x & 63;
  float* xr = x + row * D;
  float s = 0.f;
  for (int c = lane; c < D; c += 64) {
    float v = xr[c];
    if (pos) {
      v += pos[row * D + c];
      xr[c] = v;
    }
    s += v;
  }
  f32_ln_row(xr, s, gam, bet, y + row * D, D, lane);
}

// the cls rows: x[b][0] = cls_token, pos[b][0] = cls_pos
__global__ __launch_bounds__(F32_NT) void cls_kernel(float* __restrict__ x, float* __restrict__ pos, const float* __restrict__ cls,
                                                     const float* __restrict__ cpos, int B, int T, int D) {
  const int e = blockIdx.x * F32_NT + threadIdx.x;
  if (e >= B * D) return;
  const int b = e / D, c = e % D;
  x[(long)b * T * D + c] = cls[c];
  pos[(long)b * T * D + c] = cpos[c];
}

// out (B, 2D) = cat(y[b][0], max over y[b][1:]), rows in ascending order
__global__ __launch_bounds__(F32_NT) void pool_kernel(const float* __restrict__ y, float* __restrict__ out, int B, int T, int D) {
  const int e = blockIdx.x * F32_NT + threadIdx.x;
  if (e >= B * D) return;
  const int b = e / D, c = e % D;
  const float* p = y + (long)b * T * D + c;
  float m = p[D];
  for (int t = 2; t < T; ++t) m = fmaxf(m, p[(long)t * D]);
  out[(long)b * 2 * D + c] = p[0];
  out[(long)b * 2 * D + D + c] = m;
}

// qkv (B*T, 3D) with columns [q | k | v], each D = H * 64 wide, head h at h * 64  ->  o (B*T, D).
// grid (ceil(T / 16), H, B).  Dynamic LDS: 16 * Ts + 16 floats, Ts = pe_att_ts(T).
// Scores by f32_score_tile (the permuted contraction order is explained there), K and V read through L2.
__global__ __launch_bounds__(F32_NT) void attn_kernel(const float* __restrict__ qkv, float* __restrict__ o, int T, int D, float scale) {
  extern __shared__ float4 pe_att_lds4[];
  float* S = reinterpret_cast<float*>(pe_att_lds4);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int Tp = (T + 3) & ~3, Ts = pe_att_ts(T);
  float* inv = S + PE_AQ * Ts;
  const int q0 = blockIdx.x * PE_AQ, h = blockIdx.y;
  const long base = (long)blockIdx.z * T;
  const long ld = 3L * D;
  // ---- scores ----
  float4 q4[4];
  f32_load_q(q4, q0 + r < T, qkv + (base + q0 + r) * ld + h * F32_HD + g * 16);
  for (int nt = wave; nt * 16 < T; nt += F32_NT / 64) {
    const int key = nt * 16 + r;
    const bool in = key < T;
    const f32x4 acc = f32_score_tile(q4, qkv + (base + key) * ld + D + h * F32_HD + g * 16, in);
    if (in) {
#pragma unroll
      for (int e = 0; e < 4; ++e) S[(4 * g + e) * Ts + key] = acc[e] * scale;
    }
  }
  __syncthreads();
  // ---- softmax of each row: 16 threads per row ----
  {
    const int row = tid >> 4, sub = tid & 15;
    float* sr = S + row * Ts;
    float mx = -__builtin_inff();
    for (int c = sub; c < T; c += 16) mx = fmaxf(mx, sr[c]);
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    float sum = 0.f;
    for (int c = sub; c < T; c += 16) {
      const float p = expf(sr[c] - mx);
      sr[c] = p;
      sum += p;
    }
#pragma unroll
    for (int off = 8; off >= 1; off >>= 1) sum += __shfl_xor(sum, off, 64);
    if (sub == 0) inv[row] = 1.0f / sum;
    if (sub < Tp - T) sr[T + sub] = 0.f;
  }
  __syncthreads();
  // ---- output: wave w owns columns 16w .. 16w + 15 of the head; two accumulator chains (even / odd k steps), summed at the end ----
  {
    const float* vp = qkv + base * ld + 2L * D + h * F32_HD + wave * 16 + r;
    const float* sp = S + r * Ts + g;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    int k0 = 0;
    for (; k0 + 8 <= Tp; k0 += 8) {
      const int ka = k0 + g, kb = k0 + 4 + g;
      const float va = ka < T ? vp[ka * ld] : 0.f, vb = kb < T ? vp[kb * ld] : 0.f;
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(sp[k0], va, acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(sp[k0 + 4], vb, acc1, 0, 0, 0);
    }
    if (k0 < Tp) {
      const int ka = k0 + g;
      const float va = ka < T ? vp[ka * ld] : 0.f;
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(sp[k0], va, acc0, 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int q = q0 + 4 * g + e;
      if (q < T) o[(base + q) * D + h * F32_HD + wave * 16 + r] = (acc0[e] + acc1[e]) * inv[4 * g + e];
    }
  }
}
