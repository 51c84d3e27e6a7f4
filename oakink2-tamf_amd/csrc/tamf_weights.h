// Host side of the native model libraries that take a state dict tensor by tensor (libtamf_pointenc.so, libtamf_textenc.so, and
// libtamf_enctrain.so, which binds the tensors where they live): the last-error string, the table of declared tensors with its checks,
// the packer and the upload of the device weight buffer, and the small helpers of an encode call.  Host only; each library compiles its own copy (its own error string) and calls the steps in its
// own order.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <map>
#include <string>
#include <vector>

#include "../../include/tamf_hip.h"

static thread_local std::string g_error;  // what the library's *_last_error returns

static int fail(int code, const std::string& msg) {
  g_error = msg;
  return code;
}

namespace {

struct Tensor {
  std::vector<int64_t> shape;
  std::vector<float> data;
  bool loaded = false;
  bool fp16 = false;  // for the owner: a tensor it rounds to fp16 on request
  long numel() const {
    long n = 1;
    for (int64_t s : shape) n *= s;
    return n;
  }
};

std::string shape_str(const int64_t* s, int n) {
  std::string r = "(";
  for (int i = 0; i < n; ++i) r += (i ? ", " : "") + std::to_string(s[i]);
  return r + ")";
}

// the entry declared under `key` in a table of tensors (anything with a `shape`), or null with the error set: an unknown key, or a
// shape other than the declared one
template <class T>
T* find_declared(std::map<std::string, T>& t, const char* key, const int64_t* shape, int32_t ndim) {
  auto it = t.find(key);
  if (it == t.end()) return fail(TAMF_ERR_INVALID, std::string("unknown key '") + key + "'"), nullptr;
  T& x = it->second;
  if ((size_t)ndim != x.shape.size() || !std::equal(x.shape.begin(), x.shape.end(), shape))
    return fail(TAMF_ERR_INVALID, std::string(key) + ": expected shape " + shape_str(x.shape.data(), (int)x.shape.size()) + ", got " + shape_str(shape, ndim)), nullptr;
  return &x;
}

struct WeightTable {
  std::vector<std::string> order;  // the keys in state-dict order
  std::map<std::string, Tensor> t;
  bool closed = false;  // set by the owner: nothing can be loaded any more

  void declare(const std::string& key, std::vector<int64_t> shape, bool fp16 = false) {
    order.push_back(key);
    Tensor& x = t[key];
    x.shape = std::move(shape);
    x.fp16 = fp16;
  }
  Tensor& operator[](const std::string& key) { return t[key]; }

  int load(const char* key, const float* host, int32_t ndim, const int64_t* shape) {
    if (!key || !host || (ndim > 0 && !shape) || ndim < 0) return fail(TAMF_ERR_INVALID, "null argument");
    if (closed) return fail(TAMF_ERR_STATE, "the model is finalised");
    Tensor* x = find_declared(t, key, shape, ndim);
    if (!x) return TAMF_ERR_INVALID;
    x->data.assign(host, host + x->numel());
    x->loaded = true;
    return 0;
  }

  int require_loaded_and_finite() {
    for (const std::string& k : order) {
      const Tensor& x = t[k];
      if (!x.loaded) return fail(TAMF_ERR_MISSING, "missing key '" + k + "'");
      for (float v : x.data)
        if (!std::isfinite(v)) return fail(TAMF_ERR_RANGE, k + ": holds a non-finite value");
    }
    return 0;
  }

  void release() {  // the host copies, once they are not needed any more
    for (auto& kv : t) std::vector<float>().swap(kv.second.data);
  }
};

// the host image of the device weight buffer (offsets in floats): every tensor on a multiple of 4 floats, zero padded
struct Packer {
  WeightTable& w;
  bool release_packed;  // free a tensor's host copy as soon as it is packed
  std::vector<float> h;

  long reserve(long n) {
    const long off = (long)h.size();
    h.resize((size_t)(off + (n + 3) / 4 * 4), 0.f);
    return off;
  }
  long put(const std::string& key) {
    Tensor& x = w[key];
    const long off = reserve(x.numel());
    std::copy(x.data.begin(), x.data.end(), h.begin() + off);
    if (release_packed) std::vector<float>().swap(x.data);
    return off;
  }
};

// h -> a device buffer of its own in *dev.  `after` runs behind a successful copy (what else the model needs from the device) and
// fails like the copy: the buffer freed, *dev null, "<what>: ..." as the error.
template <class After>
int upload(const std::vector<float>& h, float** dev, const char* what, After after) {
  hipError_t e = hipMalloc((void**)dev, h.size() * sizeof(float));
  if (e != hipSuccess) {
    *dev = nullptr;
    return fail(e == hipErrorOutOfMemory ? TAMF_ERR_NOMEM : TAMF_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
  }
  e = hipMemcpy(*dev, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = after();
  if (e != hipSuccess) {
    (void)hipFree(*dev);
    *dev = nullptr;
    return fail(TAMF_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
  }
  return 0;
}

// dynamic LDS above 64 KiB has to be allowed per kernel (an attribute of the kernel on the current device; setting it again costs
// a host call, no device work)
template <class K>
hipError_t allow_lds(K kernel, size_t bytes) {
  if (bytes <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// carves a workspace: offsets in 4-byte words, every buffer on a multiple of 4
struct Carver {
  long total = 0;
  long take(long n) {
    const long at = total;
    total += (n + 3) / 4 * 4;
    return at;
  }
};

int check_workspace(const void* ws, int64_t bytes, long need_words) {
  if ((uintptr_t)ws & 15) return fail(TAMF_ERR_INVALID, "the workspace must be 16-byte aligned");
  if (bytes < need_words * (int64_t)sizeof(float))
    return fail(TAMF_ERR_INVALID, "workspace of " + std::to_string(bytes) + " bytes, need " + std::to_string(need_words * sizeof(float)));
  return 0;
}

unsigned blocks(long n, int threads) { return (unsigned)((n + threads - 1) / threads); }

}  // namespace
