// What the training libraries share (libtamf_enctrain.so, libtamf_refinetrain.so): the row selection of a batched buffer, the Philox
// dropout of include/tamf_enctrain.h and the derivatives of the two activations.
//
// Dropout.  keep(seed, step, clip, site, element) is word (element & 3) of Philox4x32-10 block (element >> 2, step, clip_lo, clip_hi)
// under key (seed_lo ^ site * 0x9E3779B1, seed_hi), compared against p * 2^32; kept values are scaled by 1 / (1 - p).  At p = 0 the
// threshold is 0 (everything kept, the draw skipped) and the scale is exactly 1.
#pragma once
#include <algorithm>
#include <cmath>

#include "tamf_device.h"

// rows of a (clips x rows-per-clip) selection inside a [B][S][ld] buffer: row m lives at (m / G) * gs + (m % G) * ld floats
constexpr int ROWMAP_FLAT = 1 << 30;  // G of a plain [M][ld] buffer
struct RowMap {
  int G;
  long gs, ld;
  TAMF_DEV long at(int m) const { return G == ROWMAP_FLAT ? (long)m * ld : (long)(m / G) * gs + (long)(m % G) * ld; }
};

struct Drop {
  uint32_t k0, k1, step, thr;  // key, step, keep threshold (keep when the draw >= thr)
  float scale;                 // 1 / (1 - p)
  const long long* clip;       // [B] clip ids or null (b)
};
inline Drop make_drop(uint64_t seed, uint32_t step, float p, const long long* clip) {
  Drop d;
  d.k0 = (uint32_t)(seed & 0xFFFFFFFFu);
  d.k1 = (uint32_t)(seed >> 32);
  d.step = step;
  d.thr = (uint32_t)std::min(4294967295.0, std::floor((double)p * 4294967296.0));
  d.scale = 1.0f / (1.0f - p);
  d.clip = clip;
  return d;
}
TAMF_DEV uint32_t drop_key0(const Drop& d, int site) { return d.k0 ^ ((uint32_t)site * 0x9E3779B1u); }
TAMF_DEV bool drop_keep_id(const Drop& d, int site, unsigned long long c, uint32_t e) {
  if (d.thr == 0) return true;
  uint32_t r[4];
  philox4x32_10(e >> 2, d.step, (uint32_t)(c & 0xFFFFFFFFu), (uint32_t)(c >> 32), drop_key0(d, site), d.k1, r);
  const uint32_t v = (e & 3) == 0 ? r[0] : (e & 3) == 1 ? r[1] : (e & 3) == 2 ? r[2] : r[3];
  return v >= d.thr;
}
TAMF_DEV bool drop_keep(const Drop& d, int site, int b, uint32_t e) {
  if (d.thr == 0) return true;
  return drop_keep_id(d, site, d.clip ? (unsigned long long)d.clip[b] : (unsigned long long)b, e);
}
// the factor of a dropped-out value: 0 or 1 / (1 - p)
TAMF_DEV float drop_factor(const Drop& d, int site, int b, uint32_t e) { return drop_keep(d, site, b, e) ? d.scale : 0.f; }

__global__ void dropout_mask_kernel(Drop d, int site, unsigned long long clip, long n, unsigned char* out) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) out[e] = drop_keep_id(d, site, clip, (uint32_t)e) ? 1 : 0;
}

TAMF_DEV float silu_grad(float x) {
  const float s = 1.0f / (1.0f + expf(-x));
  return s * (1.0f + x * (1.0f - s));
}
TAMF_DEV float gelu_grad(float x) {
  return 0.5f * (1.0f + erff(x * 0.70710678118654752440f)) + x * 0.3989422804014327f * expf(-0.5f * x * x);
}

// dW[n][k] (k < K) and db[n] (k = K, K1 = K + 1) = the partial sums of a weight gradient added in split order; K1 = K: no bias column
__global__ void reduce_kernel(const float* part, int nsplit, int N, int K1, int K, float* dW, float* db) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x, tot = (long)N * K1;
  if (e >= tot) return;
  float s = 0.f;
  for (int i = 0; i < nsplit; ++i) s += part[(long)i * tot + e];
  const int n = (int)(e / K1), k = (int)(e % K1);
  if (k < K) dW[(long)n * K + k] = s;
  else db[n] = s;
}
