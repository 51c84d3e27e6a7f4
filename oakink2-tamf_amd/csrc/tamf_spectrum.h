// Power spectrum of joint accelerations, summed over clips: the device half of the PSKL-J score (reference
// script/compute_score/compute_score_psklj.py:270-271 tail hold, :280-285 np.diff(n=2) -> np.fft.fft -> |.|^2, :305 sum over clips).
//
// One pass, no workspace, no floating-point atomics.  A workgroup owns a tile of PS_FT features x PS_KT frequency bins and walks the
// clips in order, PS_C at a time: thread (c, kk, ff) transforms clip n0 + c at bin k of feature f - a direct DFT of length L = T - 2 in
// float64 over the float32 accelerations held in LDS, twiddles from an L-entry float64 table indexed by (k * n) mod L kept as an integer
// recurrence - and leaves |X_k|^2 in LDS; the threads of c == 0 then add the PS_C values onto their running sums in clip order.
// Every (k, f) sum is therefore psd_sum[k, f] (+)= p(0), p(1), ..., p(N - 1), one addition after the other, whatever the grid, the
// call's N or the chunking of consecutive calls with accumulate = 1.  Only bins k <= L / 2 are computed; the input is real, so bin
// L - k receives the same |X|^2 (its own running sum, fed the same addends).
#pragma once
#include "tamf_device.h"

constexpr int PS_FT = 8;     // features per workgroup (consecutive in memory: 32-byte runs of the (N, T, F) input)
constexpr int PS_KT = 16;    // frequency bins per workgroup
constexpr int PS_C = 8;      // clips in flight per workgroup
constexpr int PS_NT = PS_FT * PS_KT * PS_C;  // 1024 threads
constexpr int PS_MAX_T = 512;                // LDS: 16 L (twiddles) + 4 PS_C PS_FT L (accelerations) + 8 PS_NT (stage) = 272 L + 8 KiB <= 160 KiB
constexpr int PS_LENS = 1024;                // clip lengths per launch, passed by value in the kernel arguments (2 KiB of the 4 KiB)

struct PsLens {
  uint16_t v[PS_LENS];
};

static inline size_t ps_lds_bytes(int L) { return (size_t)L * 16 + (size_t)PS_NT * 8 + (size_t)PS_C * PS_FT * L * 4; }

// x (N, T, F) float32; lens.v[n] in [1, T] (has_len) or every clip T frames; psd_sum (L, F) float64; psd_clip (N, L, F) float64 or null.
// grid (ceil(F / PS_FT), ceil((L / 2 + 1) / PS_KT)), PS_NT threads, ps_lds_bytes(L) dynamic LDS.
__global__ __launch_bounds__(PS_NT) void power_spectrum_kernel(const float* __restrict__ x, const PsLens lens, int has_len, int N, int T,
                                                               int F, int accumulate, double* __restrict__ psd_sum,
                                                               double* __restrict__ psd_clip) {
  extern __shared__ double2 ps_smem[];
  const int L = T - 2, K = L / 2 + 1;
  double2* tw = ps_smem;                                   // [L] (cos, sin)(2 pi j / L)
  double* stage = reinterpret_cast<double*>(tw + L);       // [PS_C][PS_KT][PS_FT] |X|^2 of the clips in flight
  float* acc = reinterpret_cast<float*>(stage + PS_NT);    // [PS_C][L][PS_FT] accelerations
  const int tid = threadIdx.x;
  const int ff = tid % PS_FT, kk = (tid / PS_FT) % PS_KT, c = tid / (PS_FT * PS_KT);
  const int f0 = blockIdx.x * PS_FT, f = f0 + ff, k = blockIdx.y * PS_KT + kk;
  const bool active = f < F && k < K;
  const bool mirror = active && k != 0 && 2 * k != L;       // bin L - k is a different bin with the same power
  const int kstep = active ? k : 0;

  for (int j = tid; j < L; j += PS_NT) {
    double s, co;
    sincospi(2.0 * (double)j / (double)L, &s, &co);
    tw[j] = make_double2(co, s);
  }
  double sum_k = 0.0, sum_m = 0.0;
  if (c == 0 && active && accumulate) {
    sum_k = psd_sum[(size_t)k * F + f];
    if (mirror) sum_m = psd_sum[(size_t)(L - k) * F + f];
  }

  for (int n0 = 0; n0 < N; n0 += PS_C) {
    // accelerations of PS_C clips x PS_FT features: two float32 subtractions in numpy's order, frames past the clip's length held
    for (int i = tid; i < PS_C * L * PS_FT; i += PS_NT) {
      const int lf = i % PS_FT, t = (i / PS_FT) % L, cc = i / (PS_FT * L);
      const int n = n0 + cc;
      float a = 0.f;
      if (n < N && f0 + lf < F) {
        const int last = (has_len ? (int)lens.v[n] : T) - 1;
        const float* xc = x + (size_t)n * T * F + (f0 + lf);
        const float x0 = xc[(size_t)min(t, last) * F], x1 = xc[(size_t)min(t + 1, last) * F], x2 = xc[(size_t)min(t + 2, last) * F];
        a = __fsub_rn(__fsub_rn(x2, x1), __fsub_rn(x1, x0));
      }
      acc[i] = a;
    }
    __syncthreads();
    {
      const float* ap = acc + (size_t)c * L * PS_FT + ff;
      double re = 0.0, im = 0.0;
      int idx = 0;
      for (int n = 0; n < L; ++n) {
        const double a = (double)ap[n * PS_FT];
        const double2 w = tw[idx];
        re = fma(a, w.x, re);
        im = fma(a, w.y, im);
        idx += kstep;
        if (idx >= L) idx -= L;
      }
      const double p = fma(re, re, im * im);
      stage[tid] = p;
      if (psd_clip && active && n0 + c < N) {
        double* o = psd_clip + (size_t)(n0 + c) * L * F + f;
        o[(size_t)k * F] = p;
        if (mirror) o[(size_t)(L - k) * F] = p;
      }
    }
    __syncthreads();
    if (c == 0 && active) {
      const int nc = min(PS_C, N - n0);
      for (int cc = 0; cc < nc; ++cc) {
        const double p = stage[cc * (PS_FT * PS_KT) + tid];
        sum_k += p;
        sum_m += p;
      }
    }
    __syncthreads();
  }
  if (c == 0 && active) {
    psd_sum[(size_t)k * F + f] = sum_k;
    if (mirror) psd_sum[(size_t)(L - k) * F + f] = sum_m;
  }
}
