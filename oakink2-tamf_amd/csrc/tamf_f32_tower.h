// What the two fp32 encoder towers share on the device: the PointBERT point encoder (csrc/tamf_pointenc.h) and the CLIP text tower
// (csrc/tamf_textenc.h).  Both are one-time preprocessing whose output conditions every later stage, so every choice here prefers a
// fixed, simple arithmetic order over speed.
//
//   f32_gemm_kernel  C = epi(A . W^T + bias): 64 x 64 tile per workgroup, K in steps of 32 through LDS, v_mfma_f32_16x16x4_f32, k
//                    ascending.  An output element is ONE accumulator chain over its own A row and W row, so its bits do not depend
//                    on where its row sits - in the batch, or in which tile a packed row landed.  What follows acc + bias (an
//                    activation, a residual add, a row remap) is the library's own Epi, instantiated into a kernel of its own.
//   f32_ln_row       LayerNorm of a row (two passes, biased variance, eps 1e-5) by one wave.
//   f32_score_tile   a 16 x 16 tile of q . k^T over the 64 floats of a head, on the MFMA.
#pragma once
#include "tamf_device.h"

constexpr int F32_NT = 256;                                    // threads per workgroup
constexpr int F32_GT = 64, F32_GK = 32, F32_GLD = F32_GK + 4;  // gemm tile, k step, LDS row stride (floats)
constexpr int F32_HD = 64;                                     // head dimension

struct F32Gemm {
  const float* A;     // [M][lda]
  const float* W;     // [N][ldw]
  const float* bias;  // [N] or null
  float* C;           // [rows][ldc]; which row an element goes to is the epilogue's business
  int lda, ldw, ldc, M, N, K;  // lda and ldw multiples of 4
};

// Epi: passed by value, `__device__ void operator()(const F32Gemm&, long row, int col, float v) const` with v = acc + bias of the
// element (row, col), row < M and col < N; it stores.
template <class Epi>
__global__ __launch_bounds__(F32_NT) void f32_gemm_kernel(const F32Gemm a, const Epi epi) {
  __shared__ float4 As4[F32_GT * F32_GLD / 4], Ws4[F32_GT * F32_GLD / 4];
  float* As = reinterpret_cast<float*>(As4);
  float* Ws = reinterpret_cast<float*>(Ws4);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  const long m0 = (long)blockIdx.x * F32_GT;
  const int n0 = blockIdx.y * F32_GT;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < a.K; k0 += F32_GK) {
    float4 ra[2], rw[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int idx = tid + j * F32_NT, row = idx >> 3, c4 = (idx & 7) * 4;
      const bool kin = k0 + c4 < a.K;
      ra[j] = (kin && m0 + row < a.M) ? *reinterpret_cast<const float4*>(a.A + (m0 + row) * a.lda + k0 + c4) : float4{0.f, 0.f, 0.f, 0.f};
      rw[j] = (kin && n0 + row < a.N) ? *reinterpret_cast<const float4*>(a.W + (long)(n0 + row) * a.ldw + k0 + c4) : float4{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();  // the previous step's reads are done
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int idx = tid + j * F32_NT, row = idx >> 3, c4 = (idx & 7) * 4;
      *reinterpret_cast<float4*>(As + row * F32_GLD + c4) = ra[j];
      *reinterpret_cast<float4*>(Ws + row * F32_GLD + c4) = rw[j];
    }
    __syncthreads();
    const float* ap = As + (wm * 32 + r) * F32_GLD + g;
    const float* wp = Ws + (wn * 32 + r) * F32_GLD + g;
#pragma unroll
    for (int kk = 0; kk < F32_GK; kk += 4) {
      const float a0 = ap[kk], a1 = ap[16 * F32_GLD + kk], b0 = wp[kk], b1 = wp[16 * F32_GLD + kk];
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
        epi(a, row, col, acc[i][j][e] + bias);
      }
    }
}

template <class Epi>
inline void f32_gemm(hipStream_t st, const F32Gemm& a, const Epi& epi) {
  hipLaunchKernelGGL(f32_gemm_kernel<Epi>, dim3((unsigned)((a.M + F32_GT - 1) / F32_GT), (unsigned)((a.N + F32_GT - 1) / F32_GT)), dim3(F32_NT), 0, st, a, epi);
}

// yr[c] = (xr[c] - mean) * rstd * gam[c] + bet[c] over the D columns of one row, by one wave: biased variance, two passes, eps 1e-5.
// s: this lane's sum of its columns lane, lane + 64, ... in ascending order (the caller's pass: it may have more to do on the way).
TAMF_DEV void f32_ln_row(const float* xr, float s, const float* gam, const float* bet, float* yr, int D, int lane) {
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
  for (int c = lane; c < D; c += 64) {
    const float dv = xr[c] - mean;
    q += dv * dv;
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + 1e-5f);
  for (int c = lane; c < D; c += 64) yr[c] = (xr[c] - mean) * rstd * gam[c] + bet[c];
}

// The 16 x 16 score tile of an attention kernel.  Lane (r, g) = (lane & 15, lane >> 4) holds sixteen floats of query row r and of key
// row r: columns 16g .. 16g + 15 of the head.  So the contraction index of q . k is permuted (lane group g covers k = 16g .. 16g + 15
// and a lane reads 64 contiguous bytes); the order is the same for every score.
TAMF_DEV void f32_load_q(float4 (&q4)[4], bool in, const float* q) {  // zeros for a row that is not there
  const float4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const float4* qp = reinterpret_cast<const float4*>(q);
#pragma unroll
  for (int j = 0; j < 4; ++j) q4[j] = in ? qp[j] : zero4;
}
// -> element e: query row 4g + e against key row r (unscaled)
TAMF_DEV f32x4 f32_score_tile(const float4 (&q4)[4], const float* k, bool in) {
  const float4 zero4 = {0.f, 0.f, 0.f, 0.f};
  const float4* kp = reinterpret_cast<const float4*>(k);
  float4 k4[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) k4[j] = in ? kp[j] : zero4;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(q4[j].x, k4[j].x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(q4[j].y, k4[j].y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(q4[j].z, k4[j].z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(q4[j].w, k4[j].w, acc, 0, 0, 0);
  }
  return acc;
}
