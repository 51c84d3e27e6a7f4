// Device code of libtamf_optim.so (include/tamf_optim.h): per-tensor gradient norms and the clip + AdamW update over a chunk table.
//
// One workgroup of OPT_NT threads owns one chunk of OPT_CHUNK consecutive elements of ONE tensor: small tensors (the biases and
// LayerNorm vectors that make up most of a model's table) cost one workgroup that loops over their few elements only, large ones
// stream as OPT_CHUNK / (4 OPT_NT) 16-byte accesses per lane and stream.  Lane `l` of a chunk always owns the elements
// 4 (i OPT_NT + l) .. + 3, i ascending, whether they arrive as one 16-byte access or as four 4-byte ones, and the arithmetic after
// the load is the same code: the aligned and the unaligned path give the same bits.  Contraction is off in this file, so every
// rounding is the one written.
#ifndef TAMF_OPTIM_DEVICE_H
#define TAMF_OPTIM_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)

constexpr int OPT_NT = 256;      // threads of a workgroup: 4 waves
constexpr int OPT_CHUNK = 4096;  // elements of a chunk (TAMF_OPTIM_CHUNK): 4 passes of one float4 per lane
constexpr int OPT_WAVES = OPT_NT / 64;

struct OptTensor {  // one row of the tensor table
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t numel;
  int32_t first_chunk;  // of this tensor in the chunk table and in the chunk sums
  int32_t n_chunks;
  int32_t aligned;  // all four bases are 16-byte aligned
  int32_t pad_;
};

struct OptChunk {  // one row of the chunk table = one workgroup
  int32_t tensor;
  int32_t index;  // chunk of the tensor: elements index * OPT_CHUNK ...
};

struct OptScalars {  // the step's host-formed constants, rounded once from double
  float decay;      // 1 - lr * weight_decay
  float w1;         // 1 - beta1
  float beta2;
  float w2;         // 1 - beta2
  float step_size;  // lr / (1 - beta1^t)
  float bc2_sqrt;   // sqrt(1 - beta2^t)
  float eps;
  float max_norm;  // < 0: no clipping
};

// The sum of `x` over the workgroup, the same bits in every thread: a wave64 xor butterfly (both partners add the same two numbers,
// so all lanes agree), then the waves' sums in wave order through LDS.  Ends with a barrier: `red` may be reused at once.
__device__ __forceinline__ float opt_block_sum(float x, float* red) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) red[wave] = x;
  __syncthreads();
  float s = red[0];
#pragma unroll
  for (int w = 1; w < OPT_WAVES; ++w) s += red[w];
  __syncthreads();
  return s;
}

// elements i .. i + 3 of a chunk of n elements at `base`; those at or past n read as 0
__device__ __forceinline__ float4 opt_load4(const float* base, int i, int n, bool vec) {
  if (vec && i + 4 <= n) return *reinterpret_cast<const float4*>(base + i);
  float4 r;
  r.x = i < n ? base[i] : 0.f;
  r.y = i + 1 < n ? base[i + 1] : 0.f;
  r.z = i + 2 < n ? base[i + 2] : 0.f;
  r.w = i + 3 < n ? base[i + 3] : 0.f;
  return r;
}

__device__ __forceinline__ void opt_store4(float* base, int i, int n, bool vec, float4 x) {
  if (vec && i + 4 <= n) {
    *reinterpret_cast<float4*>(base + i) = x;
    return;
  }
  if (i < n) base[i] = x.x;
  if (i + 1 < n) base[i + 1] = x.y;
  if (i + 2 < n) base[i + 2] = x.z;
  if (i + 3 < n) base[i + 3] = x.w;
}

// Launch 1: sums[chunk] = sum of g^2 over the chunk (one workgroup per chunk)
__global__ __launch_bounds__(OPT_NT) void optim_sumsq_kernel(const OptTensor* __restrict__ tensors, const OptChunk* __restrict__ chunks,
                                                             float* __restrict__ sums) {
  __shared__ float red[OPT_WAVES];
  const OptChunk ck = chunks[blockIdx.x];
  const OptTensor t = tensors[ck.tensor];
  const int64_t off = (int64_t)ck.index * OPT_CHUNK;
  const int64_t left = t.numel - off;
  const int n = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
  const float* g = t.g + off;
  const bool vec = t.aligned != 0;
  float acc = 0.f;
  for (int i = 4 * threadIdx.x; i < n; i += 4 * OPT_NT) {
    const float4 x = opt_load4(g, i, n, vec);
    acc += x.x * x.x;
    acc += x.y * x.y;
    acc += x.z * x.z;
    acc += x.w * x.w;
  }
  const float s = opt_block_sum(acc, red);
  if (threadIdx.x == 0) sums[blockIdx.x] = s;
}

// a tensor's sum of g^2 from its chunk sums: lane l takes chunks l, l + OPT_NT, ... in order, then the workgroup sum
__device__ __forceinline__ float opt_tensor_sumsq(const OptTensor& t, const float* __restrict__ sums, float* red) {
  float acc = 0.f;
  for (int j = threadIdx.x; j < t.n_chunks; j += OPT_NT) acc += sums[t.first_chunk + j];
  return opt_block_sum(acc, red);
}

// grad_norms: out[tensor] = sqrt(sum g^2) (one workgroup per tensor, after optim_sumsq_kernel)
__global__ __launch_bounds__(OPT_NT) void optim_norm_kernel(const OptTensor* __restrict__ tensors, const float* __restrict__ sums,
                                                            float* __restrict__ out) {
  __shared__ float red[OPT_WAVES];
  const OptTensor t = tensors[blockIdx.x];
  const float s = opt_tensor_sumsq(t, sums, red);
  if (threadIdx.x == 0) out[blockIdx.x] = sqrtf(s);
}

__device__ __forceinline__ void opt_update1(float& p, float g, float& m, float& v, float c, bool clip, const OptScalars& k) {
  if (clip) g = g * c;
  p = p * k.decay;
  m = m + (g - m) * k.w1;
  v = v * k.beta2 + (k.w2 * g) * g;
  const float denom = sqrtf(v) / k.bc2_sqrt + k.eps;
  p = p - k.step_size * (m / denom);
}

// Launch 2: the clip coefficient of the chunk's tensor from the chunk sums, then p, m, v of the chunk (one workgroup per chunk)
__global__ __launch_bounds__(OPT_NT) void optim_update_kernel(const OptTensor* __restrict__ tensors, const OptChunk* __restrict__ chunks,
                                                              const float* __restrict__ sums, OptScalars k) {
  __shared__ float red[OPT_WAVES];
  const OptChunk ck = chunks[blockIdx.x];
  const OptTensor t = tensors[ck.tensor];
  const bool clip = k.max_norm >= 0.f;
  float c = 1.f;
  if (clip) {
    const float coef = k.max_norm / (sqrtf(opt_tensor_sumsq(t, sums, red)) + 1e-6f);
    c = coef < 1.f || coef != coef ? coef : 1.f;  // (torch.clamp(max = 1) keeps a NaN)
  }
  const int64_t off = (int64_t)ck.index * OPT_CHUNK;
  const int64_t left = t.numel - off;
  const int n = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
  float* p = t.p + off;
  const float* g = t.g + off;
  float* m = t.m + off;
  float* v = t.v + off;
  const bool vec = t.aligned != 0;
  for (int i = 4 * threadIdx.x; i < n; i += 4 * OPT_NT) {
    float4 P = opt_load4(p, i, n, vec);
    const float4 G = opt_load4(g, i, n, vec);
    float4 M = opt_load4(m, i, n, vec);
    float4 V = opt_load4(v, i, n, vec);
    opt_update1(P.x, G.x, M.x, V.x, c, clip, k);
    opt_update1(P.y, G.y, M.y, V.y, c, clip, k);
    opt_update1(P.z, G.z, M.z, V.z, c, clip, k);
    opt_update1(P.w, G.w, M.w, V.w, c, clip, k);
    opt_store4(p, i, n, vec, P);
    opt_store4(m, i, n, vec, M);
    opt_store4(v, i, n, vec, V);
  }
}

#endif  // TAMF_OPTIM_DEVICE_H
