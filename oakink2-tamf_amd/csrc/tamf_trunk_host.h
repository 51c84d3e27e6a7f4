// The layer stack of the two trunk training libraries (libtamf_refinetrain.so, libtamf_mdmtrain.so) on the host: the launch sequences
// of the kernels of tamf_trunk_grad.h for the forward and the backward of one post-LN encoder layer, the helpers a model's input stage
// and head are written with (fwd / dgrad / wgrad of a linear map, the epilogues), the backward's workspace, and the profile of a
// context.  It sees token rows [B][S][d] and nothing of the model around them, and declares no tensor: a model's table is its own
// file's.  On tamf_train_host.h; like it, compiled into each library.
//
// TrunkStep<Self> is a CRTP base: every launch goes through Self::launch, so a library decides what surrounds a launch (both bracket
// it with the context's profile events).  The attention kernels are chosen by the head dimension D / H (64 or 128).
#pragma once
#include "tamf_train_host.h"

#include <tuple>

#include "tamf_trunk_grad.h"

namespace {

constexpr int MAX_SPLIT = 64, SPLIT_ROWS = 256, MAX_S = 1024;

// ---- the backward's buffers of the layer stack (offsets in floats; R token rows of D floats, H heads) ----
struct TrunkGrads {
  long dx, dz, dym, tt, dx1, datt, dqkv, dh, delta, slab;
};
TrunkGrads carve_trunk_grads(Carver& cv, long R, int D, int H, int ff) {
  TrunkGrads x{};
  x.dx = cv.take(R * D);                  // [R][d] each: the gradient of a layer's output / input,
  x.dz = cv.take(R * D);                  //   of a LayerNorm's input,
  x.dym = cv.take(R * D);                 //   of the linear output under that LayerNorm's residual dropout,
  x.tt = cv.take(R * D);                  //   dy * xhat (the gain gradient before the column sum),
  x.dx1 = cv.take(R * D);                 //   of LayerNorm 1's output,
  x.datt = cv.take(R * D);                //   of the attention output
  x.dqkv = cv.take(R * 3 * D);            // [R][3 d]
  x.dh = cv.take(R * ff);                 // [R][ff]
  x.delta = cv.take(R * H);               // [B][H][S]  sum_k P dP of every query
  return x;
}
// [<= 64 splits][N][K + 1] weight-gradient partial sums of the largest linear map; carved after a model's own gradient buffers
long carve_slab(Carver& cv, long slab_nk) { return cv.take(slab_nk * MAX_SPLIT); }

// ---- *_set_profile / *_get_profile: a pair of events around every launch, read and freed by report() ----
struct Profile {
  bool on = false;
  std::vector<std::tuple<const char*, hipEvent_t, hipEvent_t>> marks;

  template <class F>
  void around(const char* tag, hipStream_t st, F&& launch) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    const bool timed = on && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
    if (timed) (void)hipEventRecord(e0, st);
    launch();
    if (timed) {
      (void)hipEventRecord(e1, st);
      marks.emplace_back(tag, e0, e1);
    }
  }
  void clear() {
    for (auto& m : marks) (void)hipEventDestroy(std::get<1>(m)), (void)hipEventDestroy(std::get<2>(m));
    marks.clear();
  }
  // one line "name<TAB>launches<TAB>milliseconds" per kind of kernel since the last read; waits for the recorded work
  int report(char* out, int64_t size) {
    std::map<std::string, std::pair<long, double>> sum;  // name -> (launches, ms)
    hipError_t e = hipSuccess;
    for (auto& m : marks) {
      float ms = 0.f;
      if (e == hipSuccess) e = hipEventSynchronize(std::get<2>(m));
      if (e == hipSuccess) e = hipEventElapsedTime(&ms, std::get<1>(m), std::get<2>(m));
      auto& s = sum[std::get<0>(m)];
      s.first += 1;
      s.second += ms;
    }
    clear();
    if (e != hipSuccess) return fail(TAMF_ERR_HIP, std::string("profile events: ") + hipGetErrorString(e));
    std::string text;
    for (const auto& kv : sum) text += kv.first + "\t" + std::to_string(kv.second.first) + "\t" + std::to_string(kv.second.second) + "\n";
    if ((int64_t)text.size() + 1 > size) return fail(TAMF_ERR_INVALID, "the profile needs " + std::to_string(text.size() + 1) + " bytes");
    std::copy(text.begin(), text.end(), out);
    out[text.size()] = 0;
    return 0;
  }
};

// the epilogue of a tg_lin_kernel launch: a TgMode with the operands that mode reads
struct Epi {
  int mode = TG_LIN;
  float* C2 = nullptr;
  const float* R = nullptr;
  int site = 0;
};
Epi silu(float* pre) { return {TG_SILU, pre}; }
Epi gelu_drop(float* pre, int site) { return {TG_GELU_DROP, pre, nullptr, site}; }
Epi drop_res(const float* res, int site) { return {TG_DROP_RES, nullptr, res, site}; }
Epi bwd_silu(const float* pre) { return {TG_BWD_SILU, nullptr, pre}; }
Epi bwd_gelu_drop(const float* pre, int site) { return {TG_BWD_GELU_DROP, nullptr, pre, site}; }
Epi bwd_res(const float* res) { return {TG_BWD_RES, nullptr, res}; }

// X0 = drop(nan_to_num(pre) + PE) over [B][S][d]; its backward: dpre = dX0 * drop factor * isfinite(pre)
__global__ void assemble_kernel(const float* pre, const float* pe, float* x0, const float* dx0, float* dpre, int B, int S, int D, Drop d) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long)B * S * D) return;
  const int b = (int)(e / ((long)S * D));
  const uint32_t el = (uint32_t)(e % ((long)S * D));
  const float f = drop_factor(d, 0, b, el), v = pre[e];
  if (x0) x0[e] = (nan_to_num(v) + pe[el]) * f;
  else dpre[e] = (v - v == 0.f) ? dx0[e] * f : 0.f;  // (v - v: 0 for a finite v, NaN otherwise)
}
// dpre = isfinite(pre) ? dout : 0 (the output's nan_to_num)
__global__ void finite_mask_kernel(const float* pre, const float* dout, float* dpre, long n) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const float v = pre[e];
  dpre[e] = (v - v == 0.f) ? dout[e] : 0.f;
}

// whether the attention kernels are instantiated for D / H
bool trunk_head_dim_ok(int D, int H) { return H >= 1 && (D == 64 * H || D == 128 * H); }

template <class Self>
struct TrunkStep : StepRows {
  const std::vector<LayerP>* lp = nullptr;  // the layers' tensors,
  TrunkGrads tg{};                          // the backward's buffers
  long R = 0;                               // B S token rows
  int H = 0, ff = 0;
  Drop drop{};
  const char* tag = "other";  // what the next launches are called in the profile

  RowMap tok(long ld) const { return rows(S, ld); }  // every token row, split into (clip, row)

  template <class K, class... A>
  void go(K kernel, dim3 grid, int block, size_t lds, A... args) {
    static_cast<Self*>(this)->launch(kernel, grid, block, lds, args...);
  }

  void lin(TgLin a, const Epi& e, bool wt) {
    a.rm = a.cm;
    a.mode = e.mode;
    a.C2 = e.C2;
    a.R = e.R;
    a.site = e.site;
    a.d = drop;
    const dim3 grid((a.M + TG_T - 1) / TG_T, (a.N + TG_T - 1) / TG_T);
    tag = wt ? "tg_lin_kernel<dgrad>" : "tg_lin_kernel<fwd>";
    if (wt) go(tg_lin_kernel<true>, grid, 256, 0, a);
    else go(tg_lin_kernel<false>, grid, 256, 0, a);
  }
  // C (M, N) = epilogue(A (M, K) . W^T + b) of a linear map
  void fwd(const Lin& l, const float* A, RowMap am, float* C, RowMap cm, int M, const Epi& e = {}) {
    TgLin a{};
    a.A = A, a.am = am, a.W = l.w->p, a.swn = l.K, a.swk = 1, a.bias = l.b->p, a.C = C, a.cm = cm, a.M = M, a.N = l.N, a.K = l.K;
    lin(a, e, false);
  }
  // the data gradient of the same map: dA (M, K) = epilogue(dY (M, N) . W)
  void dgrad(const Lin& l, const float* dY, RowMap ym, float* dA, RowMap cm, int M, const Epi& e = {}) {
    TgLin a{};
    a.A = dY, a.am = ym, a.W = l.w->p, a.swn = 1, a.swk = l.K, a.C = dA, a.cm = cm, a.M = M, a.N = l.K, a.K = l.N;
    lin(a, e, true);
  }
  // the split of R rows: a function of the row count alone
  static int splits(int R) { return std::max(1, std::min(MAX_SPLIT, (R + SPLIT_ROWS - 1) / SPLIT_ROWS)); }
  // its weight and bias gradients from its output gradient Y and its input A over R rows
  void wgrad(const Lin& l, const float* Y, RowMap ym, const float* A, RowMap am, int R) {
    const int N = l.N, K = l.K, nsplit = splits(R), chunk = ((R + nsplit - 1) / nsplit + TG_K - 1) / TG_K * TG_K;
    tag = "tg_wgrad_kernel";
    go(tg_wgrad_kernel, dim3((N + TG_T - 1) / TG_T, (K + 1 + TG_T - 1) / TG_T, nsplit), 256, 0, TgWgrad{Y, ym, A, am, w(tg.slab), R, N, K, chunk});
    tag = "reduce_kernel";
    go(reduce_kernel, blocks((long)N * (K + 1), 256), 256, 0, w(tg.slab), nsplit, N, K + 1, K, l.w->g, l.b->g);
  }
  // the column sums of two [R][d] buffers at once (a LayerNorm's gain and bias gradients), through the two halves of the slab
  void colsum2(const float* A, const float* Bm, int R, float* outa, float* outb) {
    const int nsplit = splits(R);
    float *pa = w(tg.slab), *pb = pa + (long)MAX_SPLIT * D;
    tag = "tg_colsum2_kernel + reduce";
    go(tg_colsum2_kernel, dim3(nsplit, D / 64), 256, 0, A, Bm, D, R, (R + nsplit - 1) / nsplit, pa, pb);
    go(reduce_kernel, blocks(D, 256), 256, 0, pa, nsplit, 1, D, D, outa, nullptr);
    go(reduce_kernel, blocks(D, 256), 256, 0, pb, nsplit, 1, D, D, outb, nullptr);
  }
  void ln_fwd(const float* X, float* Y, const Lin& norm) {
    tag = "tg_ln_fwd_kernel";
    go(tg_ln_fwd_kernel, blocks(R, 4), 256, 0, X, Y, norm.w->p, norm.b->p, (int)R, D);
  }
  // LayerNorm backward of dy (offsets): dz, dym = dz under the dropout of `site`, the gain and bias gradients
  void ln_bwd(long dy, long pre, const Lin& norm, int site) {
    tag = "tg_ln_bwd_kernel";
    go(tg_ln_bwd_kernel, blocks(R, 4), 256, 0, w(dy), w(pre), norm.w->p, w(tg.dz), w(tg.dym), w(tg.tt), (int)R, D, S, site, drop);
    colsum2(w(tg.tt), w(dy), (int)R, norm.w->g, norm.b->g);
  }
  dim3 attn_grid() const { return dim3((S + 15) / 16, H, B); }
  // the three attention launches at this stack's head dimension
  template <int HD>
  void attn_launch(int which, const TgAttn& a) {
    if (which == 0) tag = "tg_attn_fwd_kernel", go(tg_attn_fwd_kernel<HD>, attn_grid(), 64, 0, a);
    else if (which == 1) tag = "tg_attn_bwd_q_kernel", go(tg_attn_bwd_q_kernel<HD>, attn_grid(), 64, 0, a);
    else tag = "tg_attn_bwd_kv_kernel", go(tg_attn_bwd_kv_kernel<HD>, attn_grid(), 64, 0, a);
  }
  void attn(int which, const TgAttn& a) {  // (Self::MAX_HD: a library whose create refuses 128 carries no kernels for it)
    if constexpr (Self::MAX_HD >= 128) {
      if (D == 128 * H) return attn_launch<128>(which, a);
    }
    attn_launch<64>(which, a);
  }

  // ---- the layer stack: token rows in, token rows out ----
  void forward_layer(int l) {
    const LayerWs& x = (*lw)[l];
    const LayerP& p = (*lp)[l];
    const int site = 1 + 4 * l, R = (int)this->R;
    fwd(p.inproj, xof(l), flat(D), w(x.qkv), flat(3 * D), R);
    attn(0, TgAttn{w(x.qkv), w(x.att), w(x.stat), nullptr, nullptr, nullptr, S, H, site, drop});
    fwd(p.out, w(x.att), flat(D), w(x.x1pre), tok(D), R, drop_res(xof(l), site + 1));
    ln_fwd(w(x.x1pre), w(x.x1), p.n1);
    fwd(p.l1, w(x.x1), flat(D), w(x.gel), tok(ff), R, gelu_drop(w(x.hpre), site + 2));
    fwd(p.l2, w(x.gel), flat(ff), w(x.x2pre), tok(D), R, drop_res(w(x.x1), site + 3));
    ln_fwd(w(x.x2pre), xof(l + 1), p.n2);
  }
  // tg.dx: the gradient of the layer's output on entry, of its input on return
  void backward_layer(int l) {
    const LayerWs& x = (*lw)[l];
    const LayerP& p = (*lp)[l];
    const TrunkGrads& g = tg;
    const int site = 1 + 4 * l, R = (int)this->R;
    // LayerNorm 2, the feed-forward block
    ln_bwd(g.dx, x.x2pre, p.n2, site + 3);
    wgrad(p.l2, w(g.dym), flat(D), w(x.gel), flat(ff), R);
    dgrad(p.l2, w(g.dym), flat(D), w(g.dh), tok(ff), R, bwd_gelu_drop(w(x.hpre), site + 2));
    wgrad(p.l1, w(g.dh), flat(ff), w(x.x1), flat(D), R);
    dgrad(p.l1, w(g.dh), flat(ff), w(g.dx1), flat(D), R, bwd_res(w(g.dz)));
    // LayerNorm 1, out-projection, attention, in-projection
    ln_bwd(g.dx1, x.x1pre, p.n1, site + 1);
    wgrad(p.out, w(g.dym), flat(D), w(x.att), flat(D), R);
    dgrad(p.out, w(g.dym), flat(D), w(g.datt), flat(D), R);
    const TgAttn a{w(x.qkv), w(x.att), w(x.stat), w(g.datt), w(g.dqkv), w(g.delta), S, H, site, drop};
    attn(1, a);
    attn(2, a);
    wgrad(p.inproj, w(g.dqkv), flat(3 * D), xof(l), flat(D), R);
    dgrad(p.inproj, w(g.dqkv), flat(3 * D), w(g.dx), flat(D), R, bwd_res(w(g.dz)));
  }
};

}  // namespace
