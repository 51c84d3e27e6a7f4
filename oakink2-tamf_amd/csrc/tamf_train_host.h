// Host side of the two training libraries (libtamf_enctrain.so, libtamf_refinetrain.so), which bind a module's tensors where torch
// keeps them: the table of bound tensors, the base of a context with its device buffers, the checks and the staging of a call, the
// launcher, and the row addressing of a step with the workspace of one transformer layer.  Host conventions of tamf_weights.h; like it,
// compiled into each library.  What differs between the two (the model around the layers, the kernels and their argument structs, the
// wording of the architecture checks) is in tamf_enctrain.hip and tamf_refinetrain.hip.
#pragma once
#include "tamf_weights.h"

#include "tamf_dropout.h"

namespace {

// ---- the parameter table ----
struct Bound {
  std::vector<int64_t> shape;
  bool trainable = true;
  const float* p = nullptr;
  float* g = nullptr;
};
// one declared (weight, bias) pair, N x K and N, where it is bound - a linear map, or the gain and bias of a LayerNorm (K = 0)
struct Lin {
  const Bound *w = nullptr, *b = nullptr;
  int N = 0, K = 0;
};
struct LayerP {
  Lin inproj, out, l1, l2, n1, n2;
};

struct ParamTable {
  std::map<std::string, Bound> t;                                 // (nodes are address-stable: Lin points into them)
  std::vector<const std::pair<const std::string, Bound>*> order;  // in declaration order
  long slab_nk = 0;                                               // the largest N (K + 1) of a declared linear map

  const Bound* declare(const std::string& k, std::vector<int64_t> shape, bool trainable = true) {
    auto it = t.emplace(k, Bound{std::move(shape), trainable}).first;
    order.push_back(&*it);
    return &it->second;
  }
  Lin declare_pair(const std::string& wk, const std::string& bk, int o, int i) {
    slab_nk = std::max(slab_nk, (long)o * (i + 1));
    const Bound* w = declare(wk, {o, i});
    return Lin{w, declare(bk, {o}), o, i};
  }
  Lin declare_linear(const std::string& k, int o, int i) { return declare_pair(k + ".weight", k + ".bias", o, i); }
  Lin declare_norm(const std::string& k, int D) {
    const Bound* w = declare(k + ".weight", {D});
    return Lin{w, declare(k + ".bias", {D}), D, 0};
  }
  // the six tensors of encoder layer l, in the state dict's order
  LayerP declare_layer(int l, int D, int ff) {
    const std::string p = "seqTransEncoder.layers." + std::to_string(l) + ".";
    LayerP x;
    x.inproj = declare_pair(p + "self_attn.in_proj_weight", p + "self_attn.in_proj_bias", 3 * D, D);
    x.out = declare_linear(p + "self_attn.out_proj", D, D);
    x.l1 = declare_linear(p + "linear1", ff, D);
    x.l2 = declare_linear(p + "linear2", D, ff);
    x.n1 = declare_norm(p + "norm1", D);
    x.n2 = declare_norm(p + "norm2", D);
    return x;
  }
  // 0, or TAMF_ERR_MISSING with the first declared tensor that is not bound
  int require_bound() const {
    for (const auto* kv : order)
      if (!kv->second.p) return fail(TAMF_ERR_MISSING, "missing binding '" + kv->first + "'");
    return 0;
  }
};

// *_bind: `tab` is null for a null context
int bind_declared(ParamTable* tab, const char* name, const float* param_dev, float* grad_dev, const int64_t* shape, int32_t ndim) {
  if (!tab || !name || !param_dev || ndim < 0 || (ndim > 0 && !shape)) return fail(TAMF_ERR_INVALID, "null argument");
  Bound* b = find_declared(tab->t, name, shape, ndim);
  if (!b) return TAMF_ERR_INVALID;
  if (b->trainable && !grad_dev) return fail(TAMF_ERR_INVALID, std::string(name) + ": a trainable tensor needs a gradient buffer");
  if (!b->trainable && grad_dev) return fail(TAMF_ERR_INVALID, std::string(name) + ": a buffer takes no gradient");
  b->p = param_dev;
  b->g = grad_dev;
  return 0;
}

// ---- the base of a context: what *_create was given, the table, the device buffers ----
struct TrainCtx {
  tamf_arch arch;
  int maxB, maxT, device;
  ParamTable tab;
  float* ws = nullptr;
  int* cnt = nullptr;         // [maxB]
  long long* clip = nullptr;  // [maxB]
  TrainCtx(const tamf_arch& a, int max_batch, int max_frames, int dev) : arch(a), maxB(max_batch), maxT(max_frames), device(dev) {}
};

// the workspace a Carver laid out, and the staging buffers of obj_num and the clip ids; after a failure the caller destroys the context
int alloc_buffers(TrainCtx* c, const Carver& cv) {
  hipError_t e = hipMalloc((void**)&c->ws, cv.total * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&c->cnt, c->maxB * sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void**)&c->clip, c->maxB * sizeof(long long));
  if (e == hipSuccess) return 0;
  return fail(e == hipErrorOutOfMemory ? TAMF_ERR_NOMEM : TAMF_ERR_HIP,
              std::string("hipMalloc of the workspace (") + std::to_string(cv.total * sizeof(float)) + " bytes): " + hipGetErrorString(e));
}
void free_buffers(TrainCtx* c) {
  if (c->ws) (void)hipFree(c->ws);
  if (c->cnt) (void)hipFree(c->cnt);
  if (c->clip) (void)hipFree(c->clip);
}

// ---- a call on a batch ----
std::string range(const char* what, long v, long lo, long hi) {
  return std::string(what) + " = " + std::to_string(v) + " outside [" + std::to_string(lo) + ", " + std::to_string(hi) + "]";
}

// the checks that need no device, in this order
int check_call(const TrainCtx* c, int B, int T, int nobj, float dropout_p, const int32_t* obj_num_host) {
  if (B < 1 || B > c->maxB) return fail(TAMF_ERR_INVALID, "B = " + std::to_string(B) + " outside [1, max_batch = " + std::to_string(c->maxB) + "]");
  if (T < 1 || T > c->maxT) return fail(TAMF_ERR_INVALID, "T = " + std::to_string(T) + " outside [1, max_frames = " + std::to_string(c->maxT) + "]");
  if (nobj < 1 || nobj > 4096) return fail(TAMF_ERR_INVALID, range("nobj", nobj, 1, 4096));
  if (!(dropout_p >= 0.f && dropout_p < 1.f)) return fail(TAMF_ERR_INVALID, "dropout_p must be in [0, 1)");
  if (obj_num_host)
    for (int b = 0; b < B; ++b)
      if (obj_num_host[b] < 1 || obj_num_host[b] > nobj)
        return fail(TAMF_ERR_INVALID, "obj_num[" + std::to_string(b) + "] = " + std::to_string(obj_num_host[b]) + " outside [1, nobj = " + std::to_string(nobj) + "]");
  return c->tab.require_bound();  // every tensor has to be there before anything is launched
}
int use_device(const TrainCtx* c) {
  const hipError_t e = hipSetDevice(c->device);
  return e == hipSuccess ? 0 : fail(TAMF_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
}
// the context's device, and obj_num and the clip ids (each may be null) into the context's copies
int stage_call(TrainCtx* c, int B, const int32_t* obj_num_host, const int64_t* clip_id_host, hipStream_t st) {
  if (int rc = use_device(c)) return rc;
  hipError_t e = hipSuccess;
  if (obj_num_host) e = hipMemcpyAsync(c->cnt, obj_num_host, B * sizeof(int), hipMemcpyHostToDevice, st);
  if (e == hipSuccess && clip_id_host) e = hipMemcpyAsync(c->clip, clip_id_host, B * sizeof(long long), hipMemcpyHostToDevice, st);
  return e == hipSuccess ? 0 : fail(TAMF_ERR_HIP, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
}

// ---- the launcher: every launch of a library goes through it, the first launch error is kept ----
struct Launcher {
  hipStream_t st = nullptr;
  hipError_t err = hipSuccess;

  template <class K, class... A>
  void launch(K kernel, dim3 grid, int block, size_t lds, A... args) {
    kernel<<<grid, block, lds, st>>>(args...);
    if (err == hipSuccess) err = hipGetLastError();
  }
  int status() const { return err == hipSuccess ? 0 : fail(TAMF_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(err)); }
};

// *_dropout_mask
int dropout_mask(uint64_t seed, uint32_t step, int64_t clip_id, int32_t site, int32_t rows, int32_t cols, float p, uint8_t* out_dev, void* stream) {
  if (!out_dev) return fail(TAMF_ERR_INVALID, "null argument");
  if (rows < 1 || cols < 1 || (long)rows * cols > 0xFFFFFFFFL) return fail(TAMF_ERR_INVALID, "rows * cols must be in [1, 2^32)");
  if (site < 0) return fail(TAMF_ERR_INVALID, "site must be >= 0");
  if (!(p >= 0.f && p < 1.f)) return fail(TAMF_ERR_INVALID, "p must be in [0, 1)");
  Launcher s;
  s.st = (hipStream_t)stream;
  const long n = (long)rows * cols;
  s.launch(dropout_mask_kernel, blocks(n, 256), 256, 0, make_drop(seed, step, p, nullptr), site, (unsigned long long)clip_id, n, out_dev);
  return s.status();
}

// ---- what the forward of one layer keeps for its backward (offsets in floats; R token rows of D floats, H heads) ----
struct LayerWs {
  long x, qkv, stat, att, x1pre, x1, x2pre, hpre, gel;
};
LayerWs carve_layer(Carver& cv, long R, int D, int H, int ff) {
  LayerWs x;
  x.x = cv.take(R * D);                   // [R][d]        the layer's input
  x.qkv = cv.take(R * 3 * D);             // [R][3 d]
  x.stat = cv.take(R * H * 2);            // [B][H][S][2]  softmax (max, sum)
  x.att = cv.take(R * D);                 // [R][d]        attention output
  x.x1pre = cv.take(R * D);               // [R][d]        LayerNorm 1: input,
  x.x1 = cv.take(R * D);                  //               output
  x.x2pre = cv.take(R * D);               // [R][d]        LayerNorm 2: input (its output is the next layer's x)
  x.hpre = cv.take(R * ff);               // [R][ff]       the feed-forward hidden rows before GELU,
  x.gel = cv.take(R * ff);                //               after GELU and dropout
  return x;
}

// ---- the rows of a step: B clips of S token rows, T of them frames, D floats wide ----
RowMap flat(long ld) { return RowMap{ROWMAP_FLAT, 0, ld}; }

struct StepRows : Launcher {
  float* ws = nullptr;                        // the context's workspace,
  const std::vector<LayerWs>* lw = nullptr;   // its layers
  long xlast = 0;                             // and the last layer's output
  int B = 0, T = 0, S = 0, D = 0;

  float* w(long off) const { return ws + off; }
  float* xof(int l) const { return w(l < (int)lw->size() ? (*lw)[l].x : xlast); }  // layer l's input; xof(L): the output
  RowMap rows(int nq, long ld) const { return RowMap{nq, (long)S * ld, ld}; }      // nq rows of every clip inside [B][S][ld]
  RowMap one() const { return rows(1, D); }
  RowMap frames() const { return rows(T, D); }
};

}  // namespace
