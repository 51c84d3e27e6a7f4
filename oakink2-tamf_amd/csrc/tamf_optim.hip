// libtamf_optim.so: the C-ABI of include/tamf_optim.h - per-parameter gradient clipping + AdamW over a tensor table.  One translation unit.
#include "../../include/tamf_optim.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "tamf_optim.h"

static_assert(OPT_CHUNK == TAMF_OPTIM_CHUNK, "the header's chunk size is the kernels'");
static_assert(OPT_CHUNK % (4 * OPT_NT) == 0, "a chunk is a whole number of float4 passes");

static thread_local std::string g_optim_error;

static int fail(int code, const std::string& msg) {
  g_optim_error = msg;
  return code;
}

static int hip_fail(const char* what, hipError_t e) { return fail(TAMF_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }

extern "C" const char* tamf_optim_last_error(void) { return g_optim_error.c_str(); }

namespace {

struct OptimCtx {
  int device = 0;
  // the host copy of the tables: kept for the context's lifetime, so it outlives every upload made from it
  std::vector<OptTensor> tensors;
  std::vector<OptChunk> chunks;
  OptTensor* tensors_dev = nullptr;
  OptChunk* chunks_dev = nullptr;
  float* sums_dev = nullptr;
  size_t tensors_cap = 0, chunks_cap = 0, sums_cap = 0;  // rows allocated
  bool bound = false;
  bool has_state = false;  // every tensor with elements was bound with exp_avg and exp_avg_sq: step() may run
};

struct DeviceGuard {  // the context's device for the span of a call
  int prev = -1;
  bool switched = false;
  explicit DeviceGuard(int device) {
    if (hipGetDevice(&prev) == hipSuccess && prev != device) switched = hipSetDevice(device) == hipSuccess;
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
};

template <class T>
int grow(T** dev, size_t* cap, size_t rows) {
  if (rows <= *cap) return 0;
  if (*dev) (void)hipFree(*dev);
  *dev = nullptr;
  *cap = 0;
  const hipError_t e = hipMalloc((void**)dev, rows * sizeof(T));
  if (e != hipSuccess) return fail(TAMF_ERR_NOMEM, std::string("hipMalloc of the optimiser table: ") + hipGetErrorString(e));
  *cap = rows;
  return 0;
}

bool aligned16(const void* q) { return ((uintptr_t)q & 15u) == 0; }

}  // namespace

extern "C" int tamf_optim_create(int32_t device, void** out) {
  if (!out) return fail(TAMF_ERR_INVALID, "null argument: out_handle");
  *out = nullptr;
  int count = 0;
  const hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess) return hip_fail("hipGetDeviceCount", e);
  if (device < 0 || device >= count) return fail(TAMF_ERR_INVALID, "device " + std::to_string(device) + " outside [0, " + std::to_string(count) + ")");
  OptimCtx* c = new OptimCtx();
  c->device = device;
  *out = c;
  return 0;
}

extern "C" void tamf_optim_destroy(void* handle) {
  OptimCtx* c = (OptimCtx*)handle;
  if (!c) return;
  DeviceGuard guard(c->device);
  if (c->tensors_dev) (void)hipFree(c->tensors_dev);
  if (c->chunks_dev) (void)hipFree(c->chunks_dev);
  if (c->sums_dev) (void)hipFree(c->sums_dev);
  delete c;
}

extern "C" int tamf_optim_bind(void* handle, int32_t n, const void* const* p, const void* const* g, const void* const* m, const void* const* v,
                               const int64_t* numel) {
  OptimCtx* c = (OptimCtx*)handle;
  if (!c) return fail(TAMF_ERR_INVALID, "null handle");
  if (n < 0 || (n > 0 && (!p || !g || !m || !v || !numel))) return fail(TAMF_ERR_INVALID, "null argument: bind needs n >= 0 and five arrays of n entries");
  std::vector<OptTensor> tensors((size_t)n);
  std::vector<OptChunk> chunks;
  int64_t total = 0;
  bool has_state = true;
  for (int32_t i = 0; i < n; ++i) {
    if (numel[i] < 0) return fail(TAMF_ERR_INVALID, "tensor " + std::to_string(i) + ": numel " + std::to_string(numel[i]) + " is negative");
    if (numel[i] > 0 && (!p[i] || !g[i]))
      return fail(TAMF_ERR_INVALID, "tensor " + std::to_string(i) + ": null pointer (p and grad are required)");
    if (numel[i] > 0 && !m[i] != !v[i])
      return fail(TAMF_ERR_INVALID, "tensor " + std::to_string(i) + ": exp_avg and exp_avg_sq must both be given, or both be null (norms only)");
    if (numel[i] > 0 && !m[i]) has_state = false;
    const int64_t nc = (numel[i] + OPT_CHUNK - 1) / OPT_CHUNK;
    if (total + nc > 0x7fffffff) return fail(TAMF_ERR_INVALID, "more than 2^31 - 1 chunks: split the table");
    OptTensor& t = tensors[(size_t)i];
    t.p = (float*)p[i];
    t.g = (const float*)g[i];
    t.m = (float*)m[i];
    t.v = (float*)v[i];
    t.numel = numel[i];
    t.first_chunk = (int32_t)total;
    t.n_chunks = (int32_t)nc;
    t.aligned = aligned16(p[i]) && aligned16(g[i]) && aligned16(m[i]) && aligned16(v[i]);
    t.pad_ = 0;
    for (int64_t j = 0; j < nc; ++j) chunks.push_back(OptChunk{i, (int32_t)j});
    total += nc;
  }
  DeviceGuard guard(c->device);
  // the tables being replaced may still be read by a step in flight on any stream
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) return hip_fail("hipDeviceSynchronize", e);
  c->bound = false;
  int rc = grow(&c->tensors_dev, &c->tensors_cap, tensors.size());
  if (!rc) rc = grow(&c->sums_dev, &c->sums_cap, chunks.size());
  if (!rc) rc = grow(&c->chunks_dev, &c->chunks_cap, chunks.size());
  if (rc) return rc;
  c->tensors.swap(tensors);
  c->chunks.swap(chunks);
  if (!c->tensors.empty()) {
    e = hipMemcpy(c->tensors_dev, c->tensors.data(), c->tensors.size() * sizeof(OptTensor), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail("hipMemcpy of the tensor table", e);
  }
  if (!c->chunks.empty()) {
    e = hipMemcpy(c->chunks_dev, c->chunks.data(), c->chunks.size() * sizeof(OptChunk), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail("hipMemcpy of the chunk table", e);
  }
  c->has_state = has_state;
  c->bound = true;
  return 0;
}

static int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : hip_fail(what, e);
}

extern "C" int tamf_optim_grad_norms(void* handle, float* out, void* stream) {
  OptimCtx* c = (OptimCtx*)handle;
  if (!c) return fail(TAMF_ERR_INVALID, "null handle");
  if (!c->bound) return fail(TAMF_ERR_STATE, "grad_norms before bind");
  if (c->tensors.empty()) return 0;
  if (!out) return fail(TAMF_ERR_INVALID, "null argument: out");
  DeviceGuard guard(c->device);
  hipStream_t st = (hipStream_t)stream;
  if (!c->chunks.empty())
    hipLaunchKernelGGL(optim_sumsq_kernel, dim3((unsigned)c->chunks.size()), dim3(OPT_NT), 0, st, c->tensors_dev, c->chunks_dev, c->sums_dev);
  hipLaunchKernelGGL(optim_norm_kernel, dim3((unsigned)c->tensors.size()), dim3(OPT_NT), 0, st, c->tensors_dev, c->sums_dev, out);
  return launched("grad_norms");
}

extern "C" int tamf_optim_step(void* handle, double lr, double beta1, double beta2, double eps, double weight_decay, double max_norm,
                               int64_t step_index, void* stream) {
  OptimCtx* c = (OptimCtx*)handle;
  if (!c) return fail(TAMF_ERR_INVALID, "null handle");
  if (!c->bound) return fail(TAMF_ERR_STATE, "step before bind");
  if (!c->has_state) return fail(TAMF_ERR_STATE, "step on a table bound without exp_avg / exp_avg_sq (norms only): bind the state first");
  if (step_index < 1) return fail(TAMF_ERR_INVALID, "step_index " + std::to_string(step_index) + " must be at least 1");
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return fail(TAMF_ERR_INVALID, "beta1 and beta2 must lie in [0, 1)");
  if (!(eps >= 0.0) || !std::isfinite(lr) || !std::isfinite(weight_decay) || std::isnan(max_norm))
    return fail(TAMF_ERR_INVALID, "eps must be >= 0, lr and weight_decay finite, max_norm a number");
  if (c->chunks.empty()) return 0;
  OptScalars k;
  k.decay = (float)(1.0 - lr * weight_decay);
  k.w1 = (float)(1.0 - beta1);
  k.beta2 = (float)beta2;
  k.w2 = (float)(1.0 - beta2);
  k.step_size = (float)(lr / (1.0 - std::pow(beta1, (double)step_index)));
  k.bc2_sqrt = (float)std::sqrt(1.0 - std::pow(beta2, (double)step_index));
  k.eps = (float)eps;
  k.max_norm = max_norm < 0.0 ? -1.f : (float)max_norm;
  DeviceGuard guard(c->device);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)c->chunks.size());
  if (max_norm >= 0.0) hipLaunchKernelGGL(optim_sumsq_kernel, grid, dim3(OPT_NT), 0, st, c->tensors_dev, c->chunks_dev, c->sums_dev);
  hipLaunchKernelGGL(optim_update_kernel, grid, dim3(OPT_NT), 0, st, c->tensors_dev, c->chunks_dev, c->sums_dev, k);
  return launched("step");
}
