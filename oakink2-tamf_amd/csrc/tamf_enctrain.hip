// libtamf_enctrain.so (include/tamf_enctrain.h): the host side of the SegmentEncoder training step - the declared tensors, the
// workspace and the launch sequence of the kernels of tamf_encoder_grad.h, on the host code of tamf_train_host.h (the table, the
// context base, the call checks, the launcher).  Host conventions of tamf_weights.h: an int status, a thread-local last-error string,
// nothing thrown across the ABI.
//
// Row counts of the workspace structs below: R = B (T + 4) token rows (3 prefix rows, T frames, the classification row of every clip),
// BT = B T frame rows; the context carves them for (max_batch, max_frames), a step addresses them with its own B and T.
#include "tamf_train_host.h"

#include "../../include/tamf_enctrain.h"
#include "tamf_encoder_grad.h"

namespace {

constexpr int MAX_SPLIT = 64, SPLIT_ROWS = 128, D = ENC_D;

struct Dims {
  long B, BT, R;
  int F, ff, sd, od, qd;
};
Dims dims(const tamf_arch& a, long B, long T) {
  return {B, B * T, B * (T + ENC_P + 1), a.input_dim, a.ff_size, a.hand_shape_dim, a.obj_embed_dim, a.obj_input_dim};
}

// ---- the workspace (offsets in floats): what the forward keeps for the backward, then the backward's own buffers ----
struct InputWs {
  long shm, oem, trm, cat, zpre, z, pre;
};
InputWs carve_input(Carver& cv, const Dims& n) {
  InputWs x;
  x.shm = cv.take(n.B * n.sd);            // [B][sd]    the hand shape, mean over the frames
  x.oem = cv.take(n.B * n.od);            // [B][od]    the object embedding, mean over the objects
  x.trm = cv.take(n.BT * n.qd);           // [BT][qd]   the object trajectory, mean over the objects
  x.cat = cv.take(n.BT * 2 * D);          // [BT][128]  pose embedding | trajectory embedding
  x.zpre = cv.take(n.BT * D);             // [BT][64]   the first merge map before ...
  x.z = cv.take(n.BT * D);                //            ... and after SiLU
  x.pre = cv.take(n.R * D);               // [R][64]    token rows before nan_to_num and PE
  return x;
}
struct HeadWs {
  long xlast, h1pre, h1, h2pre, h2;
};
HeadWs carve_head(Carver& cv, const Dims& n) {
  HeadWs x;
  x.xlast = cv.take(n.R * D);             // [R][64]  the last layer's output
  x.h1pre = cv.take(n.B * D);             // [B][64]  the output head's two hidden rows, each before ...
  x.h1 = cv.take(n.B * D);                //          ... and after SiLU
  x.h2pre = cv.take(n.B * D);
  x.h2 = cv.take(n.B * D);
  return x;
}
struct GradWs {
  long dx, dz, dym, tt, dx1, datt, dqkv, dh, delta, dpre, dzin, dcat, dact, dh1, dh2, lb, slab;
};
GradWs carve_grads(Carver& cv, const Dims& n, long slab_nk) {
  GradWs x;
  x.dx = cv.take(n.R * D);                // [R][64] each: the gradient of a layer's output / input,
  x.dz = cv.take(n.R * D);                //   of a LayerNorm's input,
  x.dym = cv.take(n.R * D);               //   of the linear output under that LayerNorm's residual dropout,
  x.tt = cv.take(n.R * D);                //   dy * xhat (the gain gradient before the column sum),
  x.dx1 = cv.take(n.R * D);               //   of LayerNorm 1's output,
  x.datt = cv.take(n.R * D);              //   of the attention output
  x.dqkv = cv.take(n.R * 3 * D);          // [R][192]
  x.dh = cv.take(n.R * n.ff);             // [R][ff]
  x.delta = cv.take(n.R * EG_H);          // [B][4][S]  sum_k P dP of every query
  x.dpre = cv.take(n.R * D);              // [R][64]    of InputWs::pre,
  x.dzin = cv.take(n.BT * D);             // [BT][64]   zpre,
  x.dcat = cv.take(n.BT * 2 * D);         // [BT][128]  cat
  x.dact = cv.take(n.B * n.F);            // [B][F]     of the activation,
  x.dh1 = cv.take(n.B * D);               // [B][64]    HeadWs::h1pre,
  x.dh2 = cv.take(n.B * D);               //            h2pre
  x.lb = cv.take(n.B);                    // [B]        the per-clip losses
  x.slab = cv.take(slab_nk * MAX_SPLIT);  // [<= 64 splits][N][K + 1] weight-gradient partial sums of the largest linear map
  return x;
}

}  // namespace

struct tamf_enctrain_ctx : TrainCtx {
  using TrainCtx::TrainCtx;
  const Bound *rh, *lh, *cls, *pe;
  Lin shape, obj, pose, traj, m0, m2, p0, p2, p4;
  std::vector<LayerP> lp;
  InputWs in;
  std::vector<LayerWs> lw;
  HeadWs head;
  GradWs g;
};

namespace {

// every tensor of the state dict, in its order
void declare_model(tamf_enctrain_ctx* c) {
  const tamf_arch& a = c->arch;
  ParamTable& t = c->tab;
  c->rh = t.declare("hand_side_process.rh_embed", {D}, false);
  c->lh = t.declare("hand_side_process.lh_embed", {D}, false);
  c->shape = t.declare_linear("hand_shape_process.shape_embed", D, a.hand_shape_dim);
  c->obj = t.declare_linear("obj_embed_process.embedding", D, a.obj_embed_dim);
  c->cls = t.declare("classification_token", {1, 1, D}, false);
  c->pose = t.declare_linear("input_process.poseEmbedding", D, a.input_dim);
  c->traj = t.declare_linear("obj_input_process.poseEmbedding", D, a.obj_input_dim);
  c->m0 = t.declare_linear("input_merge.0", D, 2 * D);
  c->m2 = t.declare_linear("input_merge.2", D, D);
  c->pe = t.declare("sequence_pos_encoder.pe", {5000, 1, D}, false);
  for (int l = 0; l < a.num_layers; ++l) c->lp.push_back(t.declare_layer(l, D, a.ff_size));
  c->p0 = t.declare_linear("output_process.poseFinal.0", D, D);
  c->p2 = t.declare_linear("output_process.poseFinal.2", D, D);
  c->p4 = t.declare_linear("output_process.poseFinal.4", a.input_dim, D);
}

// the epilogue of a lin_kernel launch: an EgMode with the operands that mode reads
struct Epi {
  int mode = EG_LIN;
  float* C2 = nullptr;
  const float* R = nullptr;
  int site = 0, q0 = 0, rq0 = 0;
};
Epi silu(float* pre) { return {EG_SILU, pre}; }
Epi gelu_drop(float* pre, int site, int q0) { return {EG_GELU_DROP, pre, nullptr, site, q0}; }
Epi drop_res(const float* res, int site, int q0) { return {EG_DROP_RES, nullptr, res, site, q0}; }
Epi bwd_silu(const float* pre) { return {EG_BWD_SILU, nullptr, pre}; }
Epi bwd_gelu_drop(const float* pre, int site, int q0) { return {EG_BWD_GELU_DROP, nullptr, pre, site, q0}; }
Epi bwd_res(const float* res) { return {EG_BWD_RES, nullptr, res}; }
Epi bwd_res_q0(const float* res, int rq0) { return {EG_BWD_RES_Q0, nullptr, res, 0, 0, rq0}; }

// the caller's tensors of one step (device memory; cnt is the context's copy of obj_num or null)
struct Batch {
  const float *pose, *shape, *oemb, *traj;
  const uint8_t* side;
  const int* cnt;
  const long long* labels;
  float *loss, *act;
  int nobj;
};

// the rows a layer computes: all S of every clip, or - the last layer - the classification row alone (K and V of every row)
struct LayerView {
  int q0, nq, M, site;  // first row and rows per clip, rows in all, the layer's first dropout site
  RowMap r64, rff;      // those rows inside [B][S][64] and [B][S][ff],
  long o64, off;        // from these offsets
};

struct Step : StepRows {
  tamf_enctrain_ctx* c = nullptr;
  Dims n{};
  Batch io{};
  Drop drop{};

  float* cls_rows() const { return xof((int)c->lw.size()) + (long)(S - 1) * D; }  // the encoder's classification rows, at one()
  size_t att_lds() const { return (size_t)S * ENC_HD * 2 * sizeof(float); }
  LayerView layer_view(int l) const {
    const int q0 = l == (int)c->lw.size() - 1 ? S - 1 : 0, nq = S - q0;
    return {q0, nq, B * nq, 1 + 4 * l, rows(nq, D), rows(nq, n.ff), (long)q0 * D, (long)q0 * n.ff};
  }

  void lin(LinArgs a, const Epi& e) {
    a.rm = a.cm;
    a.mode = e.mode;
    a.C2 = e.C2;
    a.R = e.R;
    a.site = e.site;
    a.q0 = e.q0;
    a.rq0 = e.rq0;
    a.d = drop;
    launch(lin_kernel, blocks((long)((a.M + 15) / 16) * ((a.N + 15) / 16), 4), 256, 0, a);
  }
  // C (M, N) = epilogue(A (M, K) . W^T + b) of a linear map
  void fwd(const Lin& l, const float* A, RowMap am, float* C, RowMap cm, int M, const Epi& e = {}) {
    LinArgs a{};
    a.A = A, a.am = am, a.W = l.w->p, a.swn = l.K, a.swk = 1, a.bias = l.b->p, a.C = C, a.cm = cm, a.M = M, a.N = l.N, a.K = l.K;
    lin(a, e);
  }
  // the data gradient of the same map: dA (M, K) = epilogue(dY (M, N) . W)
  void dgrad(const Lin& l, const float* dY, RowMap ym, float* dA, RowMap cm, int M, const Epi& e = {}) {
    LinArgs a{};
    a.A = dY, a.am = ym, a.W = l.w->p, a.swn = 1, a.swk = l.K, a.C = dA, a.cm = cm, a.M = M, a.N = l.K, a.K = l.N;
    lin(a, e);
  }
  // its weight and bias gradients from its output gradient Y and its input A over R rows
  void wgrad(const Lin& l, const float* Y, RowMap ym, const float* A, RowMap am, int R) {
    const int N = l.N, K = l.K, nsplit = std::max(1, std::min(MAX_SPLIT, (R + SPLIT_ROWS - 1) / SPLIT_ROWS));
    const int chunk = ((R + nsplit - 1) / nsplit + 3) / 4 * 4;
    const long tiles = (long)((N + 15) / 16) * ((K + 1 + 15) / 16) * nsplit;
    launch(wgrad_kernel, blocks(tiles, 4), 256, 0, WgradArgs{Y, ym, A, am, w(c->g.slab), R, N, K, nsplit, chunk});
    launch(reduce_kernel, blocks((long)N * (K + 1), 256), 256, 0, w(c->g.slab), nsplit, N, K + 1, K, l.w->g, l.b->g);
  }
  void colsum(const float* X, RowMap xm, int R, float* out) {
    const int nsplit = std::max(1, std::min(MAX_SPLIT, (R + SPLIT_ROWS - 1) / SPLIT_ROWS));
    launch(colsum_kernel, nsplit, D, 0, X, xm, R, (R + nsplit - 1) / nsplit, w(c->g.slab));
    launch(reduce_kernel, 1, D, 0, w(c->g.slab), nsplit, 1, D, D, out, nullptr);
  }
  void ln_fwd(const LayerView& v, const float* X, float* Y, const Lin& norm) {
    launch(ln_fwd_kernel, blocks(v.M, 4), 256, 0, X, v.r64, Y, v.r64, norm.w->p, norm.b->p, v.M);
  }
  // LayerNorm backward over the view's rows of dy (offsets): dz, dym = dz under the dropout of `site`, the gain and bias gradients
  void ln_bwd(const LayerView& v, long dy, long pre, const Lin& norm, int site) {
    const GradWs& g = c->g;
    const long o = v.o64;
    launch(ln_bwd_kernel, blocks(v.M, 4), 256, 0, w(dy) + o, w(pre) + o, v.r64, norm.w->p, w(g.dz) + o, w(g.dym) + o, w(g.tt) + o, v.M, v.q0, site, drop);
    colsum(w(g.tt) + o, v.r64, v.M, norm.w->g);
    colsum(w(dy) + o, v.r64, v.M, norm.b->g);
  }

  void forward_input() {
    const InputWs& x = c->in;
    const PrepArgs a{io.shape, io.oemb, io.traj, io.side, io.cnt, c->rh->p, c->lh->p, c->cls->p, w(x.shm), w(x.oem), w(x.trm), w(x.pre),
                     B, T, io.nobj, n.sd, n.od, n.qd};
    launch(prep_kernel, blocks(n.B * n.sd + n.B * n.od + n.BT * n.qd + n.B * 2 * D, 256), 256, 0, a);
    fwd(c->shape, w(x.shm), flat(n.sd), w(x.pre) + 1 * D, one(), B);
    fwd(c->obj, w(x.oem), flat(n.od), w(x.pre) + 2 * D, one(), B);
    fwd(c->pose, io.pose, flat(n.F), w(x.cat), flat(2 * D), n.BT);
    fwd(c->traj, w(x.trm), flat(n.qd), w(x.cat) + D, flat(2 * D), n.BT);
    fwd(c->m0, w(x.cat), flat(2 * D), w(x.z), flat(D), n.BT, silu(w(x.zpre)));
    fwd(c->m2, w(x.z), flat(D), w(x.pre) + ENC_P * D, frames(), n.BT);
    launch(assemble_kernel, blocks(n.R * D, 256), 256, 0, w(x.pre), c->pe->p, xof(0), nullptr, nullptr, B, S, drop);
  }
  void forward_layer(int l) {
    const LayerWs& x = c->lw[l];
    const LayerP& p = c->lp[l];
    const LayerView v = layer_view(l);
    const long o = v.o64, of = v.off;
    fwd(p.inproj, xof(l), flat(D), w(x.qkv), flat(3 * D), n.R);
    launch(attn_fwd_kernel, dim3((v.nq + 63) / 64, EG_H, B), 64, att_lds(),
           AttnArgs{w(x.qkv), w(x.att), w(x.stat), nullptr, nullptr, nullptr, S, v.q0, v.site, drop});
    fwd(p.out, w(x.att) + o, v.r64, w(x.x1pre) + o, v.r64, v.M, drop_res(xof(l) + o, v.site + 1, v.q0));
    ln_fwd(v, w(x.x1pre) + o, w(x.x1) + o, p.n1);
    fwd(p.l1, w(x.x1) + o, v.r64, w(x.gel) + of, v.rff, v.M, gelu_drop(w(x.hpre) + of, v.site + 2, v.q0));
    fwd(p.l2, w(x.gel) + of, v.rff, w(x.x2pre) + o, v.r64, v.M, drop_res(w(x.x1) + o, v.site + 3, v.q0));
    ln_fwd(v, w(x.x2pre) + o, xof(l + 1) + o, p.n2);
  }
  void forward_head_and_loss() {
    const HeadWs& h = c->head;
    fwd(c->p0, cls_rows(), one(), w(h.h1), flat(D), B, silu(w(h.h1pre)));
    fwd(c->p2, w(h.h1), flat(D), w(h.h2), flat(D), B, silu(w(h.h2pre)));
    fwd(c->p4, w(h.h2), flat(D), io.act, flat(n.F), B);
    launch(ce_kernel, 1, 256, 0, io.act, io.labels, B, n.F, w(c->g.lb), w(c->g.dact), io.loss);
  }
  void backward_head() {
    const HeadWs& h = c->head;
    const GradWs& g = c->g;
    wgrad(c->p4, w(g.dact), flat(n.F), w(h.h2), flat(D), B);
    dgrad(c->p4, w(g.dact), flat(n.F), w(g.dh2), flat(D), B, bwd_silu(w(h.h2pre)));
    wgrad(c->p2, w(g.dh2), flat(D), w(h.h1), flat(D), B);
    dgrad(c->p2, w(g.dh2), flat(D), w(g.dh1), flat(D), B, bwd_silu(w(h.h1pre)));
    wgrad(c->p0, w(g.dh1), flat(D), cls_rows(), one(), B);
    dgrad(c->p0, w(g.dh1), flat(D), w(g.dx) + (long)(S - 1) * D, one(), B);
  }
  void backward_layer(int l) {
    const LayerWs& x = c->lw[l];
    const LayerP& p = c->lp[l];
    const GradWs& g = c->g;
    const LayerView v = layer_view(l);
    const long o = v.o64, of = v.off;
    // LayerNorm 2, the feed-forward block
    ln_bwd(v, g.dx, x.x2pre, p.n2, v.site + 3);
    wgrad(p.l2, w(g.dym) + o, v.r64, w(x.gel) + of, v.rff, v.M);
    dgrad(p.l2, w(g.dym) + o, v.r64, w(g.dh) + of, v.rff, v.M, bwd_gelu_drop(w(x.hpre) + of, v.site + 2, v.q0));
    wgrad(p.l1, w(g.dh) + of, v.rff, w(x.x1) + o, v.r64, v.M);
    dgrad(p.l1, w(g.dh) + of, v.rff, w(g.dx1) + o, v.r64, v.M, bwd_res(w(g.dz) + o));
    // LayerNorm 1, out-projection, attention, in-projection
    ln_bwd(v, g.dx1, x.x1pre, p.n1, v.site + 1);
    wgrad(p.out, w(g.dym) + o, v.r64, w(x.att) + o, v.r64, v.M);
    dgrad(p.out, w(g.dym) + o, v.r64, w(g.datt) + o, v.r64, v.M);
    const AttnArgs a{w(x.qkv), nullptr, w(x.stat), w(g.datt), w(g.dqkv), w(g.delta), S, v.q0, v.site, drop};
    launch(attn_bwd_q_kernel, dim3((S + 63) / 64, EG_H, B), 64, att_lds(), a);
    launch(attn_bwd_kv_kernel, dim3((S + 63) / 64, EG_H, B), 64, att_lds(), a);
    wgrad(p.inproj, w(g.dqkv), flat(3 * D), xof(l), flat(D), n.R);
    dgrad(p.inproj, w(g.dqkv), flat(3 * D), w(g.dx), rows(S, D), n.R, bwd_res_q0(w(g.dz), v.q0));
  }
  void backward_input() {
    const InputWs& x = c->in;
    const GradWs& g = c->g;
    launch(assemble_kernel, blocks(n.R * D, 256), 256, 0, w(x.pre), c->pe->p, nullptr, w(g.dx), w(g.dpre), B, S, drop);
    wgrad(c->shape, w(g.dpre) + 1 * D, one(), w(x.shm), flat(n.sd), B);
    wgrad(c->obj, w(g.dpre) + 2 * D, one(), w(x.oem), flat(n.od), B);
    const float* dfr = w(g.dpre) + ENC_P * D;
    wgrad(c->m2, dfr, frames(), w(x.z), flat(D), n.BT);
    dgrad(c->m2, dfr, frames(), w(g.dzin), flat(D), n.BT, bwd_silu(w(x.zpre)));
    wgrad(c->m0, w(g.dzin), flat(D), w(x.cat), flat(2 * D), n.BT);
    dgrad(c->m0, w(g.dzin), flat(D), w(g.dcat), flat(2 * D), n.BT);
    wgrad(c->pose, w(g.dcat), flat(2 * D), io.pose, flat(n.F), n.BT);
    wgrad(c->traj, w(g.dcat) + D, flat(2 * D), w(x.trm), flat(n.qd), n.BT);
  }
};

}  // namespace

extern "C" {

const char* tamf_enctrain_last_error(void) { return g_error.c_str(); }

int tamf_enctrain_create(const tamf_arch* arch, int32_t max_batch, int32_t max_frames, int32_t device, tamf_enctrain_ctx** out) {
  if (!arch || !out) return fail(TAMF_ERR_INVALID, "null argument");
  *out = nullptr;
  if (arch->latent_dim != ENC_D || arch->num_heads != EG_H)
    return fail(TAMF_ERR_INVALID, "the encoder training step supports latent_dim 64 with 4 heads, got latent_dim " + std::to_string(arch->latent_dim) +
                                      " with " + std::to_string(arch->num_heads) + " heads");
  if (arch->ff_size < 16 || arch->ff_size > 512 || arch->ff_size % 16)
    return fail(TAMF_ERR_INVALID, "ff_size must be a multiple of 16 in [16, 512], got " + std::to_string(arch->ff_size));
  if (arch->num_layers < 1 || arch->num_layers > 64) return fail(TAMF_ERR_INVALID, "num_layers must be in [1, 64], got " + std::to_string(arch->num_layers));
  if (arch->input_dim < 1 || arch->input_dim > 4096 || arch->obj_input_dim < 1 || arch->obj_input_dim > 4096 || arch->hand_shape_dim < 1 ||
      arch->hand_shape_dim > 4096 || arch->obj_embed_dim < 1 || arch->obj_embed_dim > 4096)
    return fail(TAMF_ERR_INVALID, "input_dim, obj_input_dim, hand_shape_dim and obj_embed_dim must be in [1, 4096]");
  if (max_frames < 1 || max_frames > EG_MAX_S - ENC_P - 1)
    return fail(TAMF_ERR_INVALID, "max_frames must be in [1, " + std::to_string(EG_MAX_S - ENC_P - 1) + "] (one head's keys and values in 64 KiB of LDS), got " +
                                      std::to_string(max_frames));
  if (max_batch < 1 || max_batch > 65535) return fail(TAMF_ERR_INVALID, "max_batch must be in [1, 65535], got " + std::to_string(max_batch));
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return fail(TAMF_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));

  tamf_enctrain_ctx* c = new (std::nothrow) tamf_enctrain_ctx(*arch, max_batch, max_frames, device);
  if (!c) return fail(TAMF_ERR_NOMEM, "out of host memory");
  declare_model(c);
  const Dims n = dims(*arch, max_batch, max_frames);
  Carver cv;
  c->in = carve_input(cv, n);
  for (int l = 0; l < arch->num_layers; ++l) c->lw.push_back(carve_layer(cv, n.R, D, EG_H, n.ff));
  c->head = carve_head(cv, n);
  c->g = carve_grads(cv, n, c->tab.slab_nk);
  if (int rc = alloc_buffers(c, cv)) {
    tamf_enctrain_destroy(c);
    return rc;
  }
  *out = c;
  return 0;
}

void tamf_enctrain_destroy(tamf_enctrain_ctx* c) {
  if (!c) return;
  free_buffers(c);
  delete c;
}

int tamf_enctrain_bind(tamf_enctrain_ctx* c, const char* name, const float* param_dev, float* grad_dev, const int64_t* shape, int32_t ndim) {
  return bind_declared(c ? &c->tab : nullptr, name, param_dev, grad_dev, shape, ndim);
}

int tamf_enctrain_step(tamf_enctrain_ctx* c, int32_t B, int32_t T, int32_t nobj, const int32_t* obj_num_host, const float* pose_dev,
                       const float* shape_dev, const uint8_t* hand_side_dev, const float* obj_emb_dev, const float* obj_traj_dev,
                       const int64_t* labels_dev, const int64_t* clip_id_host, float dropout_p, uint64_t seed, uint32_t step,
                       float* loss_out_dev, float* activation_out_dev, void* stream) {
  if (!c || !pose_dev || !shape_dev || !hand_side_dev || !obj_emb_dev || !obj_traj_dev || !labels_dev || !loss_out_dev || !activation_out_dev)
    return fail(TAMF_ERR_INVALID, "null argument");
  if (int rc = check_call(c, B, T, nobj, dropout_p, obj_num_host)) return rc;
  if (int rc = stage_call(c, B, obj_num_host, clip_id_host, (hipStream_t)stream)) return rc;

  Step s;
  s.c = c;
  s.st = (hipStream_t)stream;
  s.ws = c->ws, s.lw = &c->lw, s.xlast = c->head.xlast;
  s.n = dims(c->arch, B, T);
  s.B = B, s.T = T, s.S = T + ENC_P + 1, s.D = D;
  s.io = Batch{pose_dev, shape_dev, obj_emb_dev, obj_traj_dev, hand_side_dev, obj_num_host ? c->cnt : nullptr, (const long long*)labels_dev, loss_out_dev, activation_out_dev, nobj};
  s.drop = make_drop(seed, step, dropout_p, clip_id_host ? c->clip : nullptr);
  const int L = c->arch.num_layers;
  s.forward_input();
  for (int l = 0; l < L; ++l) s.forward_layer(l);
  s.forward_head_and_loss();
  s.backward_head();
  for (int l = L - 1; l >= 0; --l) s.backward_layer(l);
  s.backward_input();
  return s.status();
}

int tamf_enctrain_dropout_mask(uint64_t seed, uint32_t step, int64_t clip_id, int32_t site, int32_t rows, int32_t cols, float p,
                               uint8_t* out_dev, void* stream) {
  return dropout_mask(seed, step, clip_id, site, rows, cols, p, out_dev, stream);
}

}  // extern "C"
