// libtamf_textenc.so: the C-ABI of include/tamf_textenc.h - the native CLIP text tower.  One translation unit.
#include "../../include/tamf_textenc.h"

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "tamf_textenc.h"
#include "tamf_weights.h"

extern "C" const char* tamf_textenc_last_error(void) { return g_error.c_str(); }

namespace {

// offsets (floats) into the device weight buffer; every tensor starts on a multiple of 4 floats
struct LayerOff {
  long g1, b1, wqkv, bqkv, wout, bout, g2, b2, wfc, bfc, wproj, bproj;
};

// the workspace of one call (offsets in 4-byte words, every buffer on a multiple of 4): the row map first, then the activations
struct Workspace {
  long ids, pos, start, len, eot, x, y, qkv, ao, hh, t, total;
  long map_words;  // what the host uploads: [ids | pos | start | len | eot]
};

}  // namespace

struct tamf_textenc_model {
  tamf_textenc_config cfg{};
  WeightTable w;  // closed once finalize has checked (and possibly rounded) the tensors, whether or not the upload succeeds; fp16: one of
                  // the tensors the reference's convert_weights turns into fp16
  long tok = 0, pos = 0, proj = 0, gf = 0, bf = 0;
  std::vector<LayerOff> lo;
  float* dev = nullptr;
  bool finalized = false;  // the weights are on the device
  // the row map of a call goes through pinned host memory; the event says when the previous call's upload has left it
  int32_t* stage = nullptr;
  long stage_words = 0;
  hipEvent_t stage_ev = nullptr;
};

extern "C" int tamf_textenc_model_create(const tamf_textenc_config* c, tamf_textenc_model** model_out) {
  if (!c || !model_out) return fail(TAMF_ERR_INVALID, "null argument");
  *model_out = nullptr;
  if (c->vocab_size < 2) return fail(TAMF_ERR_INVALID, "vocab_size = " + std::to_string(c->vocab_size) + ": at least 2");
  if (c->context_length < 2 || c->context_length > TE_CTX_MAX)
    return fail(TAMF_ERR_INVALID, "context_length = " + std::to_string(c->context_length) + " outside [2, 128]");
  if (c->width < 64 || c->width > 1024 || c->width % 64) return fail(TAMF_ERR_INVALID, "width = " + std::to_string(c->width) + ": a multiple of 64 up to 1024");
  if (c->num_heads * F32_HD != c->width) return fail(TAMF_ERR_INVALID, "num_heads = " + std::to_string(c->num_heads) + ": the head dimension must be 64 (width / 64 heads)");
  if (c->num_layers < 1) return fail(TAMF_ERR_INVALID, "num_layers = " + std::to_string(c->num_layers) + ": at least 1");
  if (c->embed_dim < 16 || c->embed_dim > 1024 || c->embed_dim % 16) return fail(TAMF_ERR_INVALID, "embed_dim = " + std::to_string(c->embed_dim) + ": a multiple of 16 up to 1024");
  tamf_textenc_model* m = new tamf_textenc_model;
  m->cfg = *c;
  const int64_t W = c->width, E = c->embed_dim;
  m->w.declare("token_embedding.weight", {c->vocab_size, W}, false);
  m->w.declare("positional_embedding", {c->context_length, W}, false);
  for (int l = 0; l < c->num_layers; ++l) {
    const std::string p = "transformer.resblocks." + std::to_string(l) + ".";
    m->w.declare(p + "ln_1.weight", {W}, false);
    m->w.declare(p + "ln_1.bias", {W}, false);
    m->w.declare(p + "attn.in_proj_weight", {3 * W, W}, true);
    m->w.declare(p + "attn.in_proj_bias", {3 * W}, true);
    m->w.declare(p + "attn.out_proj.weight", {W, W}, true);
    m->w.declare(p + "attn.out_proj.bias", {W}, true);
    m->w.declare(p + "ln_2.weight", {W}, false);
    m->w.declare(p + "ln_2.bias", {W}, false);
    m->w.declare(p + "mlp.c_fc.weight", {4 * W, W}, true);
    m->w.declare(p + "mlp.c_fc.bias", {4 * W}, true);
    m->w.declare(p + "mlp.c_proj.weight", {W, 4 * W}, true);
    m->w.declare(p + "mlp.c_proj.bias", {W}, true);
  }
  m->w.declare("ln_final.weight", {W}, false);
  m->w.declare("ln_final.bias", {W}, false);
  m->w.declare("text_projection", {W, E}, true);
  *model_out = m;
  return 0;
}

extern "C" int tamf_textenc_load_weight(tamf_textenc_model* m, const char* key, const float* host, int32_t ndim, const int64_t* shape) {
  return m ? m->w.load(key, host, ndim, shape) : fail(TAMF_ERR_INVALID, "null argument");
}

extern "C" int tamf_textenc_finalize(tamf_textenc_model* m, int32_t round_fp16) {
  if (!m) return fail(TAMF_ERR_INVALID, "null argument");
  if (m->w.closed) return fail(TAMF_ERR_STATE, "the model is finalised already");
  if (int rc = m->w.require_loaded_and_finite()) return rc;
  if (round_fp16)
    for (const std::string& k : m->w.order) {
      Tensor& t = m->w[k];
      if (!t.fp16) continue;
      for (float& v : t.data) {
        v = (float)(_Float16)v;  // round to nearest even, as torch's .half()
        if (!std::isfinite(v)) return fail(TAMF_ERR_RANGE, k + ": holds a value beyond the fp16 range");
      }
    }
  m->w.closed = true;
  const int W = m->cfg.width, E = m->cfg.embed_dim, L = m->cfg.num_layers;
  Packer pk{m->w, true};
  std::vector<float>& h = pk.h;
  m->tok = pk.put("token_embedding.weight"), m->pos = pk.put("positional_embedding");
  m->lo.resize(L);
  for (int l = 0; l < L; ++l) {
    const std::string p = "transformer.resblocks." + std::to_string(l) + ".";
    LayerOff& o = m->lo[l];
    o.g1 = pk.put(p + "ln_1.weight"), o.b1 = pk.put(p + "ln_1.bias");
    o.wqkv = pk.put(p + "attn.in_proj_weight"), o.bqkv = pk.put(p + "attn.in_proj_bias");
    o.wout = pk.put(p + "attn.out_proj.weight"), o.bout = pk.put(p + "attn.out_proj.bias");
    o.g2 = pk.put(p + "ln_2.weight"), o.b2 = pk.put(p + "ln_2.bias");
    o.wfc = pk.put(p + "mlp.c_fc.weight"), o.bfc = pk.put(p + "mlp.c_fc.bias");
    o.wproj = pk.put(p + "mlp.c_proj.weight"), o.bproj = pk.put(p + "mlp.c_proj.bias");
  }
  m->gf = pk.put("ln_final.weight"), m->bf = pk.put("ln_final.bias");
  {  // text_projection (W, E) is stored transposed, (E, W): the tail is the same C = A . W^T as every other product
    Tensor& t = m->w["text_projection"];
    m->proj = pk.reserve((long)E * W);
    for (int k = 0; k < W; ++k)
      for (int n = 0; n < E; ++n) h[m->proj + (long)n * W + k] = t.data[(long)k * E + n];
    std::vector<float>().swap(t.data);
  }
  if (int rc = upload(h, &m->dev, "upload", [m] { return hipEventCreateWithFlags(&m->stage_ev, hipEventDisableTiming); })) {
    m->stage_ev = nullptr;
    return rc;
  }
  m->finalized = true;
  return 0;
}

extern "C" int tamf_textenc_destroy(tamf_textenc_model* m) {
  if (!m) return 0;
  hipError_t e = hipSuccess, e2;
  if (m->stage_ev && (e2 = hipEventDestroy(m->stage_ev)) != hipSuccess) e = e2;
  if (m->stage && (e2 = hipHostFree(m->stage)) != hipSuccess) e = e2;
  if (m->dev && (e2 = hipFree(m->dev)) != hipSuccess) e = e2;
  delete m;
  if (e != hipSuccess) return fail(TAMF_ERR_HIP, std::string("destroy: ") + hipGetErrorString(e));
  return 0;
}

namespace {

Workspace workspace(const tamf_textenc_model* m, long B, long M) {
  const long W = m->cfg.width;
  Workspace w;
  Carver cv;
  // (the five parts of the row map are contiguous: one upload)
  w.ids = 0, w.pos = M, w.start = 2 * M, w.len = 2 * M + B, w.eot = 2 * M + 2 * B;
  w.map_words = 2 * M + 3 * B;
  cv.take(w.map_words);
  w.x = cv.take(M * W), w.y = cv.take(M * W), w.qkv = cv.take(M * 3 * W), w.ao = cv.take(M * W), w.hh = cv.take(M * 4 * W), w.t = cv.take(B * W);
  w.total = cv.total;
  return w;
}

void gemm(hipStream_t st, const float* A, int lda, long M, const float* W, int ldw, int N, int K, const float* bias, float* C, int ldc, int act, int resid) {
  f32_gemm(st, F32Gemm{A, W, bias, C, lda, ldw, ldc, (int)M, N, K}, TeEpi{act, resid});
}

bool rows_ok(const tamf_textenc_model* m, long B, long M) {
  return B >= 1 && B <= 65535 && M >= B && M <= B * m->cfg.context_length && M * 4 * m->cfg.width < (1L << 31);
}

}  // namespace

extern "C" int64_t tamf_textenc_workspace_bytes(const tamf_textenc_model* m, int32_t B, int64_t total_rows) {
  if (!m || !rows_ok(m, B, total_rows)) return 0;
  return workspace(m, B, total_rows).total * (int64_t)sizeof(float);
}

extern "C" int tamf_textenc_encode(tamf_textenc_model* m, const int32_t* tokens_host, int32_t B, float* out_dev, void* workspace_dev,
                                   int64_t workspace_bytes, void* stream) {
  if (!m) return fail(TAMF_ERR_INVALID, "null argument");
  if (!m->finalized) return fail(TAMF_ERR_STATE, "the weights are not finalised");
  if (!tokens_host || !out_dev || !workspace_dev) return fail(TAMF_ERR_INVALID, "null argument");
  if (B < 1 || B > 65535) return fail(TAMF_ERR_INVALID, "B = " + std::to_string(B) + " outside [1, 65535]");
  const int ctx = m->cfg.context_length, V = m->cfg.vocab_size, W = m->cfg.width, E = m->cfg.embed_dim, H = m->cfg.num_heads;
  // every row's EOT position: the first index of its largest id
  std::vector<int> eot(B);
  long M = 0;
  int Lmax = 0;
  for (int b = 0; b < B; ++b) {
    const int32_t* row = tokens_host + (long)b * ctx;
    int e = 0;
    for (int i = 0; i < ctx; ++i) {
      if (row[i] < 0 || row[i] >= V)
        return fail(TAMF_ERR_INVALID, "tokens[" + std::to_string(b) + "][" + std::to_string(i) + "] = " + std::to_string(row[i]) + " outside [0, " + std::to_string(V) + ")");
      if (row[i] > row[e]) e = i;
    }
    eot[b] = e;
    M += e + 1;
    Lmax = e + 1 > Lmax ? e + 1 : Lmax;
  }
  if (!rows_ok(m, B, M)) return fail(TAMF_ERR_INVALID, "B = " + std::to_string(B) + " is too large for one call: split the batch");
  const Workspace ws = workspace(m, B, M);
  if (int rc = check_workspace(workspace_dev, workspace_bytes, ws.total)) return rc;
  const int Lp = (Lmax + 15) / 16 * 16;
  const size_t att_lds = (size_t)te_att_lds_floats(Lp) * sizeof(float);
  hipError_t e = allow_lds(attn_kernel, att_lds);
  if (e != hipSuccess) return fail(TAMF_ERR_HIP, hipGetErrorString(e));
  hipStream_t st = (hipStream_t)stream;
  // the row map, through the pinned staging buffer (waits on the host only until the previous call's upload has been executed)
  e = hipEventSynchronize(m->stage_ev);
  if (e != hipSuccess) return fail(TAMF_ERR_HIP, std::string("hipEventSynchronize: ") + hipGetErrorString(e));
  if (m->stage_words < ws.map_words) {
    if (m->stage) (void)hipHostFree(m->stage);
    m->stage = nullptr, m->stage_words = 0;
    e = hipHostMalloc((void**)&m->stage, (size_t)ws.map_words * sizeof(int32_t), hipHostMallocDefault);
    if (e != hipSuccess) {
      m->stage = nullptr;
      return fail(TAMF_ERR_NOMEM, std::string("hipHostMalloc: ") + hipGetErrorString(e));
    }
    m->stage_words = ws.map_words;
  }
  {
    int32_t* s = m->stage;
    long at = 0;
    for (int b = 0; b < B; ++b) {
      const int32_t* row = tokens_host + (long)b * ctx;
      s[ws.start + b] = (int32_t)at;
      s[ws.len + b] = eot[b] + 1;
      s[ws.eot + b] = (int32_t)(at + eot[b]);
      for (int i = 0; i <= eot[b]; ++i, ++at) s[ws.ids + at] = row[i], s[ws.pos + at] = i;
    }
  }
  float* w = static_cast<float*>(workspace_dev);
  const int32_t* wi = static_cast<const int32_t*>(workspace_dev);
  e = hipMemcpyAsync(workspace_dev, m->stage, (size_t)ws.map_words * sizeof(int32_t), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipEventRecord(m->stage_ev, st);
  if (e != hipSuccess) return fail(TAMF_ERR_HIP, std::string("row map upload: ") + hipGetErrorString(e));
  const float* p = m->dev;
  hipLaunchKernelGGL(embed_kernel, dim3(blocks(M * W, F32_NT)), dim3(F32_NT), 0, st, p + m->tok, p + m->pos, wi + ws.ids, wi + ws.pos, w + ws.x, M, W);
  const unsigned ln_blocks = blocks(M, F32_NT / 64);
  const float scale = 0.125f;  // 64^-0.5
  for (int l = 0; l < m->cfg.num_layers; ++l) {
    const LayerOff& lo = m->lo[l];
    hipLaunchKernelGGL(ln_kernel, dim3(ln_blocks), dim3(F32_NT), 0, st, w + ws.x, (const int*)nullptr, p + lo.g1, p + lo.b1, w + ws.y, M, W);
    gemm(st, w + ws.y, W, M, p + lo.wqkv, W, 3 * W, W, p + lo.bqkv, w + ws.qkv, 3 * W, 0, 0);
    hipLaunchKernelGGL(attn_kernel, dim3((unsigned)H, (unsigned)B), dim3(F32_NT), att_lds, st, w + ws.qkv, wi + ws.start, wi + ws.len, w + ws.ao, W, Lp, scale);
    gemm(st, w + ws.ao, W, M, p + lo.wout, W, W, W, p + lo.bout, w + ws.x, W, 0, 1);
    hipLaunchKernelGGL(ln_kernel, dim3(ln_blocks), dim3(F32_NT), 0, st, w + ws.x, (const int*)nullptr, p + lo.g2, p + lo.b2, w + ws.y, M, W);
    gemm(st, w + ws.y, W, M, p + lo.wfc, W, 4 * W, W, p + lo.bfc, w + ws.hh, 4 * W, 1, 0);
    gemm(st, w + ws.hh, 4 * W, M, p + lo.wproj, 4 * W, W, 4 * W, p + lo.bproj, w + ws.x, W, 0, 1);
  }
  // the tail: ln_final on the B EOT rows, then the projection
  hipLaunchKernelGGL(ln_kernel, dim3(blocks(B, F32_NT / 64)), dim3(F32_NT), 0, st, w + ws.x, wi + ws.eot, p + m->gf, p + m->bf, w + ws.t, (long)B, W);
  gemm(st, w + ws.t, W, B, p + m->proj, W, E, W, nullptr, out_dev, E, 0, 0);
  e = hipGetLastError();
  if (e != hipSuccess) return fail(TAMF_ERR_HIP, hipGetErrorString(e));
  return 0;
}
