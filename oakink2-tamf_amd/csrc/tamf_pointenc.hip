// libtamf_pointenc.so: the C-ABI of include/tamf_pointenc.h - the native PointBERT point encoder.  One translation unit.
#include "../../include/tamf_pointenc.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "tamf_pointenc.h"
#include "tamf_weights.h"

extern "C" const char* tamf_pointenc_last_error(void) { return g_error.c_str(); }

namespace {

constexpr int PE_NMAX = 32768;

// offsets (floats) into the device weight buffer; every matrix starts on a multiple of 4 floats
struct LayerOff {
  long g1, b1, wqkv, wproj, bproj, g2, b2, wfc1, bfc1, wfc2, bfc2;
};
struct HeadOff {
  long w1, b1, w2, b2, w3, b3, w4, b4, wr, br, cls, cpos, wp0, bp0, wp2, bp2, ng, nb;
};

}  // namespace

struct tamf_pointenc_model {
  tamf_pointenc_config cfg{};
  int Cp = 0;
  WeightTable w;  // closed by a successful finalize: the weights are on the device
  HeadOff ho{};
  std::vector<LayerOff> lo;
  float* dev = nullptr;
};

extern "C" int tamf_pointenc_model_create(const tamf_pointenc_config* c, tamf_pointenc_model** model_out) {
  if (!c || !model_out) return fail(TAMF_ERR_INVALID, "null argument");
  *model_out = nullptr;
  if (c->point_dims != 3 && c->point_dims != 6) return fail(TAMF_ERR_INVALID, "point_dims = " + std::to_string(c->point_dims) + ": 3 or 6");
  if (c->trans_dim < 64 || c->trans_dim > 1024 || c->trans_dim % 64) return fail(TAMF_ERR_INVALID, "trans_dim = " + std::to_string(c->trans_dim) + ": a multiple of 64 up to 1024");
  if (c->num_heads * F32_HD != c->trans_dim) return fail(TAMF_ERR_INVALID, "num_heads = " + std::to_string(c->num_heads) + ": the head dimension must be 64 (trans_dim / 64 heads)");
  if (c->depth < 1) return fail(TAMF_ERR_INVALID, "depth = " + std::to_string(c->depth) + ": at least 1");
  if (c->num_group < 1 || c->num_group > 1024) return fail(TAMF_ERR_INVALID, "num_group = " + std::to_string(c->num_group) + " outside [1, 1024]");
  if (c->group_size < 8 || c->group_size > 64) return fail(TAMF_ERR_INVALID, "group_size = " + std::to_string(c->group_size) + " outside [8, 64]");
  if (c->encoder_dims < 16 || c->encoder_dims > 1024 || c->encoder_dims % 16) return fail(TAMF_ERR_INVALID, "encoder_dims = " + std::to_string(c->encoder_dims) + ": a multiple of 16 up to 1024");
  tamf_pointenc_model* m = new tamf_pointenc_model;
  m->cfg = *c;
  m->Cp = (c->point_dims + 3) / 4 * 4;
  const int64_t C = c->point_dims, D = c->trans_dim, E = c->encoder_dims;
  for (int s = 0; s < 2; ++s) {
    const std::string p = s == 0 ? "encoder.first_conv." : "encoder.second_conv.";
    const int64_t in0 = s == 0 ? C : 512, mid = s == 0 ? 128 : 512, out = s == 0 ? 256 : E;
    m->w.declare(p + "0.weight", {mid, in0, 1});
    m->w.declare(p + "0.bias", {mid});
    for (const char* n : {"weight", "bias", "running_mean", "running_var"}) m->w.declare(p + "1." + n, {mid});
    m->w.declare(p + "3.weight", {out, mid, 1});
    m->w.declare(p + "3.bias", {out});
  }
  m->w.declare("reduce_dim.weight", {D, E});
  m->w.declare("reduce_dim.bias", {D});
  m->w.declare("cls_token", {1, 1, D});
  m->w.declare("cls_pos", {1, 1, D});
  m->w.declare("pos_embed.0.weight", {128, 3});
  m->w.declare("pos_embed.0.bias", {128});
  m->w.declare("pos_embed.2.weight", {D, 128});
  m->w.declare("pos_embed.2.bias", {D});
  for (int l = 0; l < c->depth; ++l) {
    const std::string p = "blocks.blocks." + std::to_string(l) + ".";
    m->w.declare(p + "norm1.weight", {D});
    m->w.declare(p + "norm1.bias", {D});
    m->w.declare(p + "norm2.weight", {D});
    m->w.declare(p + "norm2.bias", {D});
    m->w.declare(p + "mlp.fc1.weight", {4 * D, D});
    m->w.declare(p + "mlp.fc1.bias", {4 * D});
    m->w.declare(p + "mlp.fc2.weight", {D, 4 * D});
    m->w.declare(p + "mlp.fc2.bias", {D});
    m->w.declare(p + "attn.qkv.weight", {3 * D, D});
    m->w.declare(p + "attn.proj.weight", {D, D});
    m->w.declare(p + "attn.proj.bias", {D});
  }
  m->w.declare("norm.weight", {D});
  m->w.declare("norm.bias", {D});
  *model_out = m;
  return 0;
}

extern "C" int tamf_pointenc_load_weight(tamf_pointenc_model* m, const char* key, const float* host, int32_t ndim, const int64_t* shape) {
  return m ? m->w.load(key, host, ndim, shape) : fail(TAMF_ERR_INVALID, "null argument");
}

extern "C" int tamf_pointenc_fold_bn(const float* w, const float* b, const float* gamma, const float* beta, const float* mean,
                                     const float* var, int32_t out_ch, int32_t in_ch, int32_t ld_out, float* w_out, float* b_out) {
  if (!w || !b || !gamma || !beta || !mean || !var || !w_out || !b_out) return fail(TAMF_ERR_INVALID, "null argument");
  if (out_ch < 1 || in_ch < 1 || ld_out < in_ch) return fail(TAMF_ERR_INVALID, "bad dimensions");
  for (int o = 0; o < out_ch; ++o) {
    const double v = (double)var[o] + 1e-5;
    if (!std::isfinite(v) || v <= 0.0 || !std::isfinite(gamma[o]) || !std::isfinite(beta[o]) || !std::isfinite(mean[o]) || !std::isfinite(b[o]))
      return fail(TAMF_ERR_RANGE, "BatchNorm channel " + std::to_string(o) + ": non-finite parameter or running_var + eps <= 0");
    const double s = (double)gamma[o] / std::sqrt(v);
    for (int i = 0; i < ld_out; ++i) {
      if (i < in_ch && !std::isfinite(w[(long)o * in_ch + i])) return fail(TAMF_ERR_RANGE, "non-finite weight in channel " + std::to_string(o));
      w_out[(long)o * ld_out + i] = i < in_ch ? (float)(s * (double)w[(long)o * in_ch + i]) : 0.f;
    }
    b_out[o] = (float)(((double)b[o] - (double)mean[o]) * s + (double)beta[o]);
  }
  return 0;
}

extern "C" int tamf_pointenc_finalize(tamf_pointenc_model* m) {
  if (!m) return fail(TAMF_ERR_INVALID, "null argument");
  if (m->w.closed) return fail(TAMF_ERR_STATE, "the model is finalised already");
  if (int rc = m->w.require_loaded_and_finite()) return rc;
  const int C = m->cfg.point_dims, Cp = m->Cp, L = m->cfg.depth;
  Packer pk{m->w, false};  // (put_folded reads tensors that are not packed themselves: the host copies go after the upload)
  std::vector<float>& h = pk.h;
  auto put_folded = [&](const std::string& p, int out_ch, int in_ch, int ld, long& w_off, long& b_off) {
    w_off = pk.reserve((long)out_ch * ld);
    b_off = pk.reserve(out_ch);
    return tamf_pointenc_fold_bn(m->w[p + "0.weight"].data.data(), m->w[p + "0.bias"].data.data(), m->w[p + "1.weight"].data.data(),
                                 m->w[p + "1.bias"].data.data(), m->w[p + "1.running_mean"].data.data(), m->w[p + "1.running_var"].data.data(),
                                 out_ch, in_ch, ld, h.data() + w_off, h.data() + b_off);
  };
  HeadOff& ho = m->ho;
  int rc = put_folded("encoder.first_conv.", 128, C, Cp, ho.w1, ho.b1);
  if (rc) return rc;
  ho.w2 = pk.put("encoder.first_conv.3.weight"), ho.b2 = pk.put("encoder.first_conv.3.bias");
  rc = put_folded("encoder.second_conv.", 512, 512, 512, ho.w3, ho.b3);
  if (rc) return rc;
  ho.w4 = pk.put("encoder.second_conv.3.weight"), ho.b4 = pk.put("encoder.second_conv.3.bias");
  ho.wr = pk.put("reduce_dim.weight"), ho.br = pk.put("reduce_dim.bias");
  ho.cls = pk.put("cls_token"), ho.cpos = pk.put("cls_pos");
  ho.wp0 = pk.reserve(128 * 4);
  for (int o = 0; o < 128; ++o)
    for (int i = 0; i < 3; ++i) h[ho.wp0 + o * 4 + i] = m->w["pos_embed.0.weight"].data[o * 3 + i];
  ho.bp0 = pk.put("pos_embed.0.bias");
  ho.wp2 = pk.put("pos_embed.2.weight"), ho.bp2 = pk.put("pos_embed.2.bias");
  ho.ng = pk.put("norm.weight"), ho.nb = pk.put("norm.bias");
  m->lo.resize(L);
  for (int l = 0; l < L; ++l) {
    const std::string p = "blocks.blocks." + std::to_string(l) + ".";
    LayerOff& o = m->lo[l];
    o.g1 = pk.put(p + "norm1.weight"), o.b1 = pk.put(p + "norm1.bias");
    o.wqkv = pk.put(p + "attn.qkv.weight");
    o.wproj = pk.put(p + "attn.proj.weight"), o.bproj = pk.put(p + "attn.proj.bias");
    o.g2 = pk.put(p + "norm2.weight"), o.b2 = pk.put(p + "norm2.bias");
    o.wfc1 = pk.put(p + "mlp.fc1.weight"), o.bfc1 = pk.put(p + "mlp.fc1.bias");
    o.wfc2 = pk.put(p + "mlp.fc2.weight"), o.bfc2 = pk.put(p + "mlp.fc2.bias");
  }
  rc = upload(h, &m->dev, "hipMemcpy", [] { return hipSuccess; });
  if (rc) return rc;
  m->w.release();
  m->w.closed = true;
  return 0;
}

extern "C" int tamf_pointenc_destroy(tamf_pointenc_model* m) {
  if (!m) return 0;
  hipError_t e = m->dev ? hipFree(m->dev) : hipSuccess;
  delete m;
  if (e != hipSuccess) return fail(TAMF_ERR_HIP, std::string("hipFree: ") + hipGetErrorString(e));
  return 0;
}

static int check_cloud(const void* points, int32_t B, int32_t N, int32_t C) {
  if (!points) return fail(TAMF_ERR_INVALID, "null argument");
  if (B < 1) return fail(TAMF_ERR_INVALID, "B = " + std::to_string(B) + ": at least one cloud");
  if (N < 1 || N > PE_NMAX) return fail(TAMF_ERR_INVALID, "N = " + std::to_string(N) + " outside [1, 32768]");
  if (C < 3) return fail(TAMF_ERR_INVALID, "C = " + std::to_string(C) + ": at least the three coordinates");
  return 0;
}

extern "C" int tamf_pointenc_fps(const float* points_dev, const int32_t* start_idx_dev, int32_t B, int32_t N, int32_t C, int32_t G,
                                 int32_t* idx_out_dev, void* stream) {
  if (int rc = check_cloud(points_dev, B, N, C)) return rc;
  if (!start_idx_dev || !idx_out_dev) return fail(TAMF_ERR_INVALID, "null argument");
  if (G < 1 || G > N) return fail(TAMF_ERR_INVALID, "G = " + std::to_string(G) + " outside [1, N]");
  const size_t lds = (size_t)N * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e;
  auto run = [&](auto kernel) {
    hipError_t err = allow_lds(kernel, lds);
    if (err != hipSuccess) return err;
    hipLaunchKernelGGL(kernel, dim3(B), dim3(PE_FPS_NT), lds, st, points_dev, start_idx_dev, idx_out_dev, N, C, G);
    return hipGetLastError();
  };
  e = N <= 8 * PE_FPS_NT ? run(fps_kernel<8, true>) : N <= 16 * PE_FPS_NT ? run(fps_kernel<16, true>) : run(fps_kernel<32, false>);
  if (e != hipSuccess) return fail(TAMF_ERR_HIP, hipGetErrorString(e));
  return 0;
}

extern "C" int tamf_pointenc_group(const float* points_dev, const int32_t* centre_idx_dev, int32_t B, int32_t N, int32_t C, int32_t G,
                                   int32_t M, int32_t* nbr_idx_out_dev, void* stream) {
  if (int rc = check_cloud(points_dev, B, N, C)) return rc;
  if (!centre_idx_dev || !nbr_idx_out_dev) return fail(TAMF_ERR_INVALID, "null argument");
  if (G < 1 || (long)B * G > (1L << 30)) return fail(TAMF_ERR_INVALID, "G = " + std::to_string(G) + ": at least 1 (and B * G below 2^30)");
  if (M < 1 || M > N) return fail(TAMF_ERR_INVALID, "M = " + std::to_string(M) + " outside [1, N]");
  const size_t lds = (size_t)N * sizeof(float);
  hipError_t e = allow_lds(group_kernel, lds);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(group_kernel, dim3((unsigned)(B * G)), dim3(F32_NT), lds, (hipStream_t)stream, points_dev, centre_idx_dev, nbr_idx_out_dev, N, C, G, M);
    e = hipGetLastError();
  }
  if (e != hipSuccess) return fail(TAMF_ERR_HIP, hipGetErrorString(e));
  return 0;
}

namespace {

// the workspace of B clouds (offsets in floats, every buffer on a multiple of 4)
struct Workspace {
  long x0, c0, h1, f, fg, gg, h3, f4, tok, ph, x, pos, y, qkv, ao, hh, total;
};

Workspace workspace(const tamf_pointenc_model* m, long B) {
  const long G = m->cfg.num_group, M = m->cfg.group_size, D = m->cfg.trans_dim, E = m->cfg.encoder_dims;
  const long R = B * G * M, Q = B * G, BT = B * (G + 1);
  Workspace w;
  Carver cv;
  w.x0 = cv.take(R * m->Cp), w.c0 = cv.take(Q * 4), w.h1 = cv.take(R * 128), w.f = cv.take(R * 256), w.fg = cv.take(Q * 256), w.gg = cv.take(Q * 512);
  w.h3 = cv.take(R * 512), w.f4 = cv.take(R * E), w.tok = cv.take(Q * E), w.ph = cv.take(Q * 128);
  w.x = cv.take(BT * D), w.pos = cv.take(BT * D), w.y = cv.take(BT * D), w.qkv = cv.take(BT * 3 * D), w.ao = cv.take(BT * D), w.hh = cv.take(BT * 4 * D);
  w.total = cv.total;
  return w;
}

void gemm(hipStream_t st, const float* A, int lda, long M, const float* W, int ldw, int N, int K, const float* bias, float* C, int ldc, int act = 0,
          const float* radd = nullptr, int rgrp = 1, int resid = 0, int tokmap = 0) {
  f32_gemm(st, F32Gemm{A, W, bias, C, lda, ldw, ldc, (int)M, N, K}, PeEpi{radd, act, rgrp, resid, tokmap});
}

}  // namespace

extern "C" int64_t tamf_pointenc_workspace_bytes(const tamf_pointenc_model* m, int32_t B) {
  if (!m || B < 1) return 0;
  return workspace(m, B).total * (int64_t)sizeof(float);
}

extern "C" int tamf_pointenc_encode(const tamf_pointenc_model* m, const float* points_dev, const int32_t* centre_idx_dev,
                                    const int32_t* nbr_idx_dev, int32_t B, int32_t N, float* out_dev, void* workspace_dev,
                                    int64_t workspace_bytes, void* stream) {
  if (!m) return fail(TAMF_ERR_INVALID, "null argument");
  if (!m->w.closed) return fail(TAMF_ERR_STATE, "the weights are not finalised");
  if (int rc = check_cloud(points_dev, B, N, m->cfg.point_dims)) return rc;
  if (!centre_idx_dev || !nbr_idx_dev || !out_dev || !workspace_dev) return fail(TAMF_ERR_INVALID, "null argument");
  const int C = m->cfg.point_dims, Cp = m->Cp, G = m->cfg.num_group, M = m->cfg.group_size, D = m->cfg.trans_dim, E = m->cfg.encoder_dims;
  const int H = m->cfg.num_heads, T = G + 1;
  if (M > N) return fail(TAMF_ERR_INVALID, "N = " + std::to_string(N) + " is below group_size");
  const long R = (long)B * G * M, Q = (long)B * G, BT = (long)B * T;
  if (R * 512 >= (1L << 31) || B > 65535) return fail(TAMF_ERR_INVALID, "B = " + std::to_string(B) + " is too large for one call: split the batch");
  const Workspace ws = workspace(m, B);
  if (int rc = check_workspace(workspace_dev, workspace_bytes, ws.total)) return rc;
  const size_t att_lds = ((size_t)PE_AQ * pe_att_ts(T) + PE_AQ) * sizeof(float);
  hipError_t e = allow_lds(attn_kernel, att_lds);
  if (e != hipSuccess) return fail(TAMF_ERR_HIP, hipGetErrorString(e));
  hipStream_t st = (hipStream_t)stream;
  float* w = static_cast<float*>(workspace_dev);
  const float* p = m->dev;
  const HeadOff& ho = m->ho;

  // groups -> tokens (dvae.py:150-221)
  hipLaunchKernelGGL(gather_kernel, dim3(blocks(R * Cp, F32_NT)), dim3(F32_NT), 0, st, points_dev, centre_idx_dev, nbr_idx_dev, w + ws.x0, w + ws.c0, R, N, C, Cp, G, M);
  gemm(st, w + ws.x0, Cp, R, p + ho.w1, Cp, 128, Cp, p + ho.b1, w + ws.h1, 128, 1);
  gemm(st, w + ws.h1, 128, R, p + ho.w2, 128, 256, 128, p + ho.b2, w + ws.f, 256);
  hipLaunchKernelGGL(groupmax_kernel, dim3(blocks(Q * 256, F32_NT)), dim3(F32_NT), 0, st, w + ws.f, w + ws.fg, Q, M, 256);
  // second_conv.0 on cat(global, local): the global half (input channels 0..255) once per group, with the folded bias
  gemm(st, w + ws.fg, 256, Q, p + ho.w3, 512, 512, 256, p + ho.b3, w + ws.gg, 512);
  gemm(st, w + ws.f, 256, R, p + ho.w3 + 256, 512, 512, 256, nullptr, w + ws.h3, 512, 1, w + ws.gg, M);
  gemm(st, w + ws.h3, 512, R, p + ho.w4, 512, E, 512, p + ho.b4, w + ws.f4, E);
  hipLaunchKernelGGL(groupmax_kernel, dim3(blocks(Q * E, F32_NT)), dim3(F32_NT), 0, st, w + ws.f4, w + ws.tok, Q, M, E);
  // reduce_dim and pos_embed into the token rows behind each cloud's cls row (point_encoder.py:167-176)
  gemm(st, w + ws.tok, E, Q, p + ho.wr, E, D, E, p + ho.br, w + ws.x, D, 0, nullptr, 1, 0, G);
  gemm(st, w + ws.c0, 4, Q, p + ho.wp0, 4, 128, 4, p + ho.bp0, w + ws.ph, 128, 2);
  gemm(st, w + ws.ph, 128, Q, p + ho.wp2, 128, D, 128, p + ho.bp2, w + ws.pos, D, 0, nullptr, 1, 0, G);
  hipLaunchKernelGGL(cls_kernel, dim3(blocks((long)B * D, F32_NT)), dim3(F32_NT), 0, st, w + ws.x, w + ws.pos, p + ho.cls, p + ho.cpos, B, T, D);
  // blocks (point_encoder.py:60-100)
  const unsigned ln_blocks = blocks(BT, F32_NT / 64);
  const float scale = 1.0f / sqrtf((float)F32_HD);
  for (int l = 0; l < m->cfg.depth; ++l) {
    const LayerOff& lo = m->lo[l];
    hipLaunchKernelGGL(ln_kernel, dim3(ln_blocks), dim3(F32_NT), 0, st, w + ws.x, w + ws.pos, p + lo.g1, p + lo.b1, w + ws.y, BT, D);
    gemm(st, w + ws.y, D, BT, p + lo.wqkv, D, 3 * D, D, nullptr, w + ws.qkv, 3 * D);
    hipLaunchKernelGGL(attn_kernel, dim3((unsigned)((T + PE_AQ - 1) / PE_AQ), (unsigned)H, (unsigned)B), dim3(F32_NT), att_lds, st, w + ws.qkv, w + ws.ao, T, D, scale);
    gemm(st, w + ws.ao, D, BT, p + lo.wproj, D, D, D, p + lo.bproj, w + ws.x, D, 0, nullptr, 1, 1);
    hipLaunchKernelGGL(ln_kernel, dim3(ln_blocks), dim3(F32_NT), 0, st, w + ws.x, (const float*)nullptr, p + lo.g2, p + lo.b2, w + ws.y, BT, D);
    gemm(st, w + ws.y, D, BT, p + lo.wfc1, D, 4 * D, D, p + lo.bfc1, w + ws.hh, 4 * D, 2);
    gemm(st, w + ws.hh, 4 * D, BT, p + lo.wfc2, 4 * D, D, 4 * D, p + lo.bfc2, w + ws.x, D, 0, nullptr, 1, 1);
  }
  hipLaunchKernelGGL(ln_kernel, dim3(ln_blocks), dim3(F32_NT), 0, st, w + ws.x, (const float*)nullptr, p + ho.ng, p + ho.nb, w + ws.y, BT, D);
  hipLaunchKernelGGL(pool_kernel, dim3(blocks((long)B * D, F32_NT)), dim3(F32_NT), 0, st, w + ws.y, out_dev, B, T, D);
  e = hipGetLastError();
  if (e != hipSuccess) return fail(TAMF_ERR_HIP, hipGetErrorString(e));
  return 0;
}
