// Kernels of libtamf_surface.so (include/tamf_surface.h holds the definition they implement, word for word): face areas scanned per
// block of 1024 faces, the fixed carry pass over the block totals, the carries added, and the sampling kernel - one thread per sample,
// Philox draw, binary search on the CDF, barycentric point.  float64, no fused multiply-adds, no atomics; wave64.
#pragma once
#include "tamf_device.h"

#pragma clang fp contract(off)

constexpr int SURF_NT = 256;                            // threads of a scan workgroup: 4 waves
constexpr int SURF_ITEMS = 4;                           // consecutive faces one thread sums
constexpr int SURF_SCAN_BLOCK = SURF_NT * SURF_ITEMS;   // faces one workgroup scans
constexpr int SURF_WAVES = SURF_NT / 64;

// c = (v1 - v0) x (v2 - v0) of face f in float64; false when an index lies outside [0, V)
TAMF_DEV bool surf_face_cross(const float* __restrict__ verts, int V, const int* __restrict__ faces, long f, double (&p)[3][3], double (&c)[3]) {
  const int i0 = faces[3 * f], i1 = faces[3 * f + 1], i2 = faces[3 * f + 2];
  if ((unsigned)i0 >= (unsigned)V || (unsigned)i1 >= (unsigned)V || (unsigned)i2 >= (unsigned)V) return false;
  const int idx[3] = {i0, i1, i2};
#pragma unroll
  for (int k = 0; k < 3; ++k)
#pragma unroll
    for (int a = 0; a < 3; ++a) p[k][a] = (double)verts[3 * (size_t)idx[k] + a];
  const double e1x = p[1][0] - p[0][0], e1y = p[1][1] - p[0][1], e1z = p[1][2] - p[0][2];
  const double e2x = p[2][0] - p[0][0], e2y = p[2][1] - p[0][1], e2z = p[2][2] - p[0][2];
  c[0] = e1y * e2z - e1z * e2y;
  c[1] = e1z * e2x - e1x * e2z;
  c[2] = e1x * e2y - e1y * e2x;
  return true;
}

TAMF_DEV double surf_cross_len(const double (&c)[3]) { return sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]); }

TAMF_DEV double surf_face_area(const float* __restrict__ verts, int V, const int* __restrict__ faces, long f) {
  double p[3][3], c[3];
  if (!surf_face_cross(verts, V, faces, f, p, c)) return 0.0;
  const double a = 0.5 * surf_cross_len(c);
  return isfinite(a) ? a : 0.0;
}

// Block b scans faces [1024 b, 1024 b + 1024): local[f] = base_wave + (base_lane + l_k), every base the chained totals of the groups
// before it inside the block; block_sum[b] = the block's last local value.  Faces past F count as area 0 and are not written.
__global__ __launch_bounds__(SURF_NT) void surface_area_scan_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                                    double* __restrict__ cdf, double* __restrict__ block_sum) {
  __shared__ double wave_total[SURF_WAVES];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long f0 = (long)blockIdx.x * SURF_SCAN_BLOCK + (long)t * SURF_ITEMS;
  double l[SURF_ITEMS];
  double run = 0.0;
#pragma unroll
  for (int k = 0; k < SURF_ITEMS; ++k) {
    run = run + (f0 + k < F ? surf_face_area(verts, V, faces, f0 + k) : 0.0);
    l[k] = run;
  }
  // the lanes' totals chained one after the other: every lane walks the same 64 additions and keeps the sum that stood before its own
  double base = 0.0, acc = 0.0;
#pragma unroll
  for (int i = 0; i < 64; ++i) {
    if (i == lane) base = acc;
    acc = acc + __shfl(run, i, 64);
  }
  if (lane == 0) wave_total[wave] = acc;
  __syncthreads();
  double wbase = 0.0;
  for (int w = 0; w < wave; ++w) wbase = wbase + wave_total[w];
#pragma unroll
  for (int k = 0; k < SURF_ITEMS; ++k)
    if (f0 + k < F) cdf[f0 + k] = wbase + (base + l[k]);
  if (t == 0) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < SURF_WAVES; ++w) s = s + wave_total[w];
    block_sum[blockIdx.x] = s;
  }
}

// The fixed carry pass, one thread: block_sum[b] <- the chained totals of blocks 0 .. b-1, block_sum[n_blocks] <- total.
__global__ __launch_bounds__(64) void surface_carry_kernel(double* __restrict__ block_sum, int n_blocks) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double c = 0.0;
  for (int b = 0; b < n_blocks; ++b) {
    const double s = block_sum[b];
    block_sum[b] = c;
    c = c + s;
  }
  block_sum[n_blocks] = c;
}

__global__ __launch_bounds__(SURF_NT) void surface_add_carry_kernel(double* __restrict__ cdf, const double* __restrict__ block_sum, int F) {
  const long f = (long)blockIdx.x * SURF_NT + threadIdx.x;
  if (f < F) cdf[f] = block_sum[f / SURF_SCAN_BLOCK] + cdf[f];
}

// One thread per sample m of [0, M): sample i = first + m.
__global__ __launch_bounds__(SURF_NT) void surface_sample_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                                 const double* __restrict__ cdf, double total, long M, uint64_t seed,
                                                                 uint64_t key, uint64_t first, float* __restrict__ points,
                                                                 float* __restrict__ normals, int* __restrict__ face_out) {
  const long m = (long)blockIdx.x * SURF_NT + threadIdx.x;
  if (m >= M) return;
  const uint64_t i = first + (uint64_t)m;
  uint32_t r[4];
  philox4x32_10((uint32_t)i, (uint32_t)(i >> 32), (uint32_t)key, (uint32_t)(key >> 32), (uint32_t)seed, (uint32_t)(seed >> 32), r);
  const double uf = ((double)(((uint64_t)r[0] << 21) | (uint64_t)(r[1] >> 11)) + 0.5) * 0x1p-53;
  const double u1 = ((double)r[2] + 0.5) * 0x1p-32;
  const double u2 = ((double)r[3] + 0.5) * 0x1p-32;
  const double x = uf * total;
  int lo = 0, hi = F;  // the smallest j with cdf[j] > x
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (cdf[mid] > x) hi = mid; else lo = mid + 1;
  }
  if (lo >= F) {  // x == total: the smallest j with cdf[j] >= total
    lo = 0, hi = F - 1;
    while (lo < hi) {
      const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
      if (cdf[mid] >= total) hi = mid; else lo = mid + 1;
    }
  }
  const int j = lo;
  double p[3][3], c[3];
  float out[3] = {0.f, 0.f, 0.f}, nrm[3] = {0.f, 0.f, 0.f};
  if (surf_face_cross(verts, V, faces, j, p, c)) {  // (a picked face has a positive area, hence indices inside the vertices)
    const double s = sqrt(u1);
    const double w0 = 1.0 - s, w1 = s * (1.0 - u2), w2 = s * u2;
    const double len = surf_cross_len(c);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      out[a] = (float)((w0 * p[0][a] + w1 * p[1][a]) + w2 * p[2][a]);
      nrm[a] = (float)(c[a] / len);
    }
  }
#pragma unroll
  for (int a = 0; a < 3; ++a) points[3 * (size_t)m + a] = out[a];
  if (normals) {
#pragma unroll
    for (int a = 0; a < 3; ++a) normals[3 * (size_t)m + a] = nrm[a];
  }
  if (face_out) face_out[m] = j;
}
