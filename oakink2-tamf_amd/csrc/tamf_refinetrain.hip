// libtamf_refinetrain.so (include/tamf_refinetrain.h): the host side of the SegmentRefineModel training step - the declared tensors,
// the workspace and the launch sequences of the kernels of tamf_trunk_grad.h, on the host code of tamf_train_host.h (the table, the
// context base, the call checks, the launcher) and tamf_trunk_host.h (the layer stack, shared with libtamf_mdmtrain.so).  Host
// conventions of tamf_weights.h: an int status, a thread-local last-error string, nothing thrown across the ABI.
//
// The layer stack (TrunkStep::forward_layer / backward_layer) sees token rows [B][S][d] and nothing of the model around it; the refiner
// is its input stage (3 prefix rows, frames merged from pose | object trajectory | hand->object distance) and its head (x_in + poseFinal).
//
// Row counts of the workspace structs below: R = B (T + 3) token rows, BT = B T frame rows; the context carves them for (max_batch,
// max_frames), a call addresses them with its own B and T.
#include "tamf_trunk_host.h"

#include "../../include/tamf_refinetrain.h"

namespace {

constexpr int PREFIX = 3;

struct Dims {
  long B, BT, R;
  int D, H, F, ff, sd, od, qd, hd;
};
Dims dims(const tamf_arch& a, long B, long T) {
  return {B, B * T, B * (T + PREFIX), a.latent_dim, a.num_heads, a.input_dim, a.ff_size, a.hand_shape_dim, a.obj_embed_dim, a.obj_input_dim, a.h2o_dim};
}

// ---- the workspace (offsets in floats): what the forward keeps for the backward, then the backward's own buffers ----
struct InputWs {
  long shm, oem, trm, cat, zpre, z, pre;
};
InputWs carve_input(Carver& cv, const Dims& n) {
  InputWs x;
  x.shm = cv.take(n.B * n.sd);            // [B][sd]     the hand shape, mean over the frames
  x.oem = cv.take(n.B * n.od);            // [B][od]     the object embedding, mean over the objects
  x.trm = cv.take(n.BT * n.qd);           // [BT][qd]    the object trajectory, mean over the objects
  x.cat = cv.take(n.BT * 3 * n.D);        // [BT][3 d]   pose | trajectory | distance embeddings
  x.zpre = cv.take(n.BT * n.D);           // [BT][d]     the first merge map before ...
  x.z = cv.take(n.BT * n.D);              //             ... and after SiLU
  x.pre = cv.take(n.R * n.D);             // [R][d]      token rows before nan_to_num and PE
  return x;
}
struct HeadWs {
  long xlast, outpre;
};
HeadWs carve_head(Carver& cv, const Dims& n) {
  HeadWs x;
  x.xlast = cv.take(n.R * n.D);           // [R][d]   the last layer's output
  x.outpre = cv.take(n.BT * n.F);         // [BT][F]  x_in + poseFinal(...) before nan_to_num
  return x;
}
struct GradWs {  // the gradients of the refiner's own buffers, between the layer stack's (TrunkGrads) and the slab
  long dpre, dzin, dcat, dout;
};
GradWs carve_grads(Carver& cv, const Dims& n) {
  GradWs x;
  x.dpre = cv.take(n.R * n.D);            // [R][d]     of InputWs::pre,
  x.dzin = cv.take(n.BT * n.D);           // [BT][d]    zpre,
  x.dcat = cv.take(n.BT * 3 * n.D);       // [BT][3 d]  cat
  x.dout = cv.take(n.BT * n.F);           // [BT][F]    of HeadWs::outpre
  return x;
}

// the caller's tensors of one forward (device memory; cnt is the context's copy of obj_num or null)
struct Batch {
  const float *pose, *dist, *shape, *oemb, *traj;
  const uint8_t* side;
  const int* cnt;
  float* out;
  int nobj;
};

}  // namespace

struct tamf_refinetrain_ctx : TrainCtx {
  using TrainCtx::TrainCtx;
  const Bound *rh, *lh, *pe;
  Lin shape, obj, pose, traj, dist, m0, m2, head;
  std::vector<LayerP> lp;
  InputWs in;
  std::vector<LayerWs> lw;
  HeadWs hw;
  TrunkGrads tg;
  GradWs g;
  // the forward whose activations the workspace holds
  bool have_forward = false;
  int B = 0, T = 0;
  Profile profile;  // tamf_refinetrain_set_profile / tamf_refinetrain_get_profile
  Batch io{};
  Drop drop{};
};

namespace {

// every tensor of the state dict, in its order
void declare_model(tamf_refinetrain_ctx* c) {
  const tamf_arch& a = c->arch;
  ParamTable& t = c->tab;
  const int D = a.latent_dim;
  c->rh = t.declare("hand_side_process.rh_embed", {D}, false);
  c->lh = t.declare("hand_side_process.lh_embed", {D}, false);
  c->shape = t.declare_linear("hand_shape_process.shape_embed", D, a.hand_shape_dim);
  c->obj = t.declare_linear("obj_embed_process.embedding", D, a.obj_embed_dim);
  c->pose = t.declare_linear("input_process.poseEmbedding", D, a.input_dim);
  c->traj = t.declare_linear("obj_input_process.poseEmbedding", D, a.obj_input_dim);
  c->dist = t.declare_linear("h2o_dist_input_process.poseEmbedding", D, a.h2o_dim);
  c->m0 = t.declare_linear("input_merge.0", D, 3 * D);
  c->m2 = t.declare_linear("input_merge.2", D, D);
  c->pe = t.declare("sequence_pos_encoder.pe", {5000, 1, D}, false);
  for (int l = 0; l < a.num_layers; ++l) c->lp.push_back(t.declare_layer(l, D, a.ff_size));
  c->head = t.declare_linear("output_process.poseFinal", a.input_dim, D);
}

// ---- the input stage: means, the hand-side row, x0 = drop(nan_to_num(pre) + PE), the output mask ----
struct PrepArgs {
  const float *shape, *oemb, *traj;  // (B,T,sd) (B,nobj,od) (B,nobj,T,qd)
  const unsigned char* side;         // [B] 0 = rh, 1 = lh
  const int* cnt;                    // [B] or null
  const float *rh, *lh;              // [d] each
  float *shm, *oem, *trm, *pre;      // [B][sd] [B][od] [B*T][qd]; pre [B][S][d]: row 0 is written here
  int B, T, D, nobj, sd, od, qd;
};
__global__ void prep_kernel(const PrepArgs a) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int S = a.T + PREFIX;
  const long n0 = (long)a.B * a.sd, n1 = n0 + (long)a.B * a.od, n2 = n1 + (long)a.B * a.T * a.qd, n3 = n2 + (long)a.B * a.D;
  if (e < n0) {
    const int b = (int)(e / a.sd), c = (int)(e % a.sd);
    double s = 0.0;  // (T terms of one sign: a float32 running sum would lose log2(T) bits of the hand-shape row)
    for (int t = 0; t < a.T; ++t) s += (double)a.shape[((long)b * a.T + t) * a.sd + c];
    a.shm[e] = (float)(s / (double)a.T);
  } else if (e < n1) {
    const long i = e - n0;
    const int b = (int)(i / a.od), c = (int)(i % a.od);
    const int n = a.cnt ? max(1, min(a.cnt[b], a.nobj)) : a.nobj;
    float s = 0.f;
    for (int o = 0; o < n; ++o) s += a.oemb[((long)b * a.nobj + o) * a.od + c];
    a.oem[i] = s / (float)n;
  } else if (e < n2) {
    const long i = e - n1;
    const int c = (int)(i % a.qd);
    const long bt = i / a.qd;
    const int b = (int)(bt / a.T), t = (int)(bt % a.T);
    const int n = a.cnt ? max(1, min(a.cnt[b], a.nobj)) : a.nobj;
    float s = 0.f;
    for (int o = 0; o < n; ++o) s += a.traj[(((long)b * a.nobj + o) * a.T + t) * a.qd + c];
    a.trm[i] = s / (float)n;
  } else if (e < n3) {
    const long i = e - n2;
    const int b = (int)(i / a.D), c = (int)(i % a.D);
    a.pre[(long)b * S * a.D + c] = (a.side[b] ? a.lh : a.rh)[c];
  }
}
struct Step : TrunkStep<Step> {
  static constexpr int MAX_HD = 64;  // (tamf_refinetrain_create refuses another head dimension)
  tamf_refinetrain_ctx* c = nullptr;
  Dims n{};
  Batch io{};

  // the shared launch, between a pair of events when the context's profile is on
  template <class K, class... A>
  void launch(K kernel, dim3 grid, int block, size_t lds, A... args) {
    c->profile.around(tag, st, [&] { Launcher::launch(kernel, grid, block, lds, args...); });
  }

  // ---- the refiner around it ----
  void forward_input() {
    const InputWs& x = c->in;
    const PrepArgs a{io.shape, io.oemb, io.traj, io.side, io.cnt, c->rh->p, c->lh->p, w(x.shm), w(x.oem), w(x.trm), w(x.pre),
                     B, T, D, io.nobj, n.sd, n.od, n.qd};
    tag = "input stage (elementwise)";
    launch(prep_kernel, blocks(n.B * n.sd + n.B * n.od + n.BT * n.qd + n.B * D, 256), 256, 0, a);
    fwd(c->shape, w(x.shm), flat(n.sd), w(x.pre) + 1 * D, one(), B);
    fwd(c->obj, w(x.oem), flat(n.od), w(x.pre) + 2 * D, one(), B);
    fwd(c->pose, io.pose, flat(n.F), w(x.cat), flat(3 * D), (int)n.BT);
    fwd(c->traj, w(x.trm), flat(n.qd), w(x.cat) + D, flat(3 * D), (int)n.BT);
    fwd(c->dist, io.dist, flat(n.hd), w(x.cat) + 2 * D, flat(3 * D), (int)n.BT);
    fwd(c->m0, w(x.cat), flat(3 * D), w(x.z), flat(D), (int)n.BT, silu(w(x.zpre)));
    fwd(c->m2, w(x.z), flat(D), w(x.pre) + PREFIX * D, frames(), (int)n.BT);
    tag = "input stage (elementwise)";
    launch(assemble_kernel, blocks(n.R * D, 256), 256, 0, w(x.pre), c->pe->p, xof(0), nullptr, nullptr, B, S, D, drop);
  }
  void forward_head() {
    const float* fr = xof((int)c->lw.size()) + PREFIX * D;
    Epi e{TG_HEAD_RES, w(c->hw.outpre), io.pose};
    fwd(c->head, fr, frames(), io.out, flat(n.F), (int)n.BT, e);
  }
  void backward_head(const float* gout) {
    const GradWs& g = c->g;
    const float* fr = xof((int)c->lw.size()) + PREFIX * D;
    tag = "input stage (elementwise)";
    launch(finite_mask_kernel, blocks(n.BT * n.F, 256), 256, 0, w(c->hw.outpre), gout, w(g.dout), n.BT * n.F);
    wgrad(c->head, w(g.dout), flat(n.F), fr, frames(), (int)n.BT);
    if (err == hipSuccess) err = hipMemsetAsync(w(tg.dx), 0, n.R * D * sizeof(float), st);  // (the prefix rows feed no output row)
    dgrad(c->head, w(g.dout), flat(n.F), w(tg.dx) + PREFIX * D, frames(), (int)n.BT);
  }
  void backward_input() {
    const InputWs& x = c->in;
    const GradWs& g = c->g;
    tag = "input stage (elementwise)";
    launch(assemble_kernel, blocks(n.R * D, 256), 256, 0, w(x.pre), c->pe->p, nullptr, w(tg.dx), w(g.dpre), B, S, D, drop);
    wgrad(c->shape, w(g.dpre) + 1 * D, one(), w(x.shm), flat(n.sd), B);
    wgrad(c->obj, w(g.dpre) + 2 * D, one(), w(x.oem), flat(n.od), B);
    const float* dfr = w(g.dpre) + PREFIX * D;
    wgrad(c->m2, dfr, frames(), w(x.z), flat(D), (int)n.BT);
    dgrad(c->m2, dfr, frames(), w(g.dzin), flat(D), (int)n.BT, bwd_silu(w(x.zpre)));
    wgrad(c->m0, w(g.dzin), flat(D), w(x.cat), flat(3 * D), (int)n.BT);
    dgrad(c->m0, w(g.dzin), flat(D), w(g.dcat), flat(3 * D), (int)n.BT);
    wgrad(c->pose, w(g.dcat), flat(3 * D), io.pose, flat(n.F), (int)n.BT);
    wgrad(c->traj, w(g.dcat) + D, flat(3 * D), w(x.trm), flat(n.qd), (int)n.BT);
    wgrad(c->dist, w(g.dcat) + 2 * D, flat(3 * D), io.dist, flat(n.hd), (int)n.BT);
  }
};

Step make_step(tamf_refinetrain_ctx* c, hipStream_t st) {
  Step s;
  s.c = c;
  s.st = st;
  s.ws = c->ws, s.lw = &c->lw, s.xlast = c->hw.xlast;
  s.n = dims(c->arch, c->B, c->T);
  s.B = c->B, s.T = c->T, s.S = c->T + PREFIX, s.D = c->arch.latent_dim;
  s.lp = &c->lp, s.tg = c->tg, s.R = s.n.R, s.H = s.n.H, s.ff = s.n.ff;
  s.io = c->io;
  s.drop = c->drop;
  return s;
}

}  // namespace

extern "C" {

const char* tamf_refinetrain_last_error(void) { return g_error.c_str(); }

int tamf_refinetrain_create(const tamf_arch* arch, int32_t max_batch, int32_t max_frames, int32_t device, tamf_refinetrain_ctx** out) {
  if (!arch || !out) return fail(TAMF_ERR_INVALID, "null argument");
  *out = nullptr;
  if (arch->num_heads < 1 || arch->num_heads > TG_MAXC) return fail(TAMF_ERR_INVALID, range("num_heads", arch->num_heads, 1, TG_MAXC));
  if (arch->latent_dim != TG_HD * arch->num_heads)
    return fail(TAMF_ERR_INVALID, "the head dimension must be 64: latent_dim = 64 * num_heads, got latent_dim " + std::to_string(arch->latent_dim) +
                                      " with " + std::to_string(arch->num_heads) + " heads");
  if (arch->ff_size < 16 || arch->ff_size > 4096 || arch->ff_size % 16)
    return fail(TAMF_ERR_INVALID, "ff_size must be a multiple of 16 in [16, 4096], got " + std::to_string(arch->ff_size));
  if (arch->num_layers < 1 || arch->num_layers > 64) return fail(TAMF_ERR_INVALID, range("num_layers", arch->num_layers, 1, 64));
  const std::pair<const char*, int> widths[] = {{"input_dim", arch->input_dim}, {"obj_input_dim", arch->obj_input_dim}, {"hand_shape_dim", arch->hand_shape_dim},
                                                {"obj_embed_dim", arch->obj_embed_dim}, {"h2o_dim", arch->h2o_dim}};
  for (const auto& kv : widths)
    if (kv.second < 1 || kv.second > 4096) return fail(TAMF_ERR_INVALID, range(kv.first, kv.second, 1, 4096));
  if (max_frames < 1 || max_frames > MAX_S - PREFIX) return fail(TAMF_ERR_INVALID, range("max_frames", max_frames, 1, MAX_S - PREFIX));
  if (max_batch < 1 || max_batch > 65535) return fail(TAMF_ERR_INVALID, range("max_batch", max_batch, 1, 65535));
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return fail(TAMF_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));

  tamf_refinetrain_ctx* c = new (std::nothrow) tamf_refinetrain_ctx(*arch, max_batch, max_frames, device);
  if (!c) return fail(TAMF_ERR_NOMEM, "out of host memory");
  declare_model(c);
  const Dims n = dims(*arch, max_batch, max_frames);
  Carver cv;
  c->in = carve_input(cv, n);
  for (int l = 0; l < arch->num_layers; ++l) c->lw.push_back(carve_layer(cv, n.R, n.D, n.H, n.ff));
  c->hw = carve_head(cv, n);
  c->tg = carve_trunk_grads(cv, n.R, n.D, n.H, n.ff);
  c->g = carve_grads(cv, n);
  c->tg.slab = carve_slab(cv, c->tab.slab_nk);
  if (int rc = alloc_buffers(c, cv)) {
    tamf_refinetrain_destroy(c);
    return rc;
  }
  *out = c;
  return 0;
}

void tamf_refinetrain_destroy(tamf_refinetrain_ctx* c) {
  if (!c) return;
  c->profile.clear();
  free_buffers(c);
  delete c;
}

int tamf_refinetrain_bind(tamf_refinetrain_ctx* c, const char* name, const float* param_dev, float* grad_dev, const int64_t* shape, int32_t ndim) {
  return bind_declared(c ? &c->tab : nullptr, name, param_dev, grad_dev, shape, ndim);
}

int tamf_refinetrain_forward(tamf_refinetrain_ctx* c, int32_t B, int32_t T, int32_t nobj, const int32_t* obj_num_host,
                             const float* sample_pose_dev, const float* h2o_dist_dev, const float* shape_dev, const uint8_t* hand_side_dev,
                             const float* obj_emb_dev, const float* obj_traj_dev, const int64_t* clip_id_host, float dropout_p, uint64_t seed,
                             uint32_t step, float* refine_pose_out_dev, void* stream) {
  if (!c || !sample_pose_dev || !h2o_dist_dev || !shape_dev || !hand_side_dev || !obj_emb_dev || !obj_traj_dev || !refine_pose_out_dev)
    return fail(TAMF_ERR_INVALID, "null argument");
  if (int rc = check_call(c, B, T, nobj, dropout_p, obj_num_host)) return rc;
  c->have_forward = false;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = stage_call(c, B, obj_num_host, clip_id_host, st)) return rc;

  c->B = B, c->T = T;
  c->io = Batch{sample_pose_dev, h2o_dist_dev, shape_dev, obj_emb_dev, obj_traj_dev, hand_side_dev, obj_num_host ? c->cnt : nullptr, refine_pose_out_dev, nobj};
  c->drop = make_drop(seed, step, dropout_p, clip_id_host ? c->clip : nullptr);
  Step s = make_step(c, st);
  s.forward_input();
  for (int l = 0; l < c->arch.num_layers; ++l) s.forward_layer(l);
  s.forward_head();
  c->have_forward = s.err == hipSuccess;
  return s.status();
}

int tamf_refinetrain_backward(tamf_refinetrain_ctx* c, const float* grad_refine_pose_dev, void* stream) {
  if (!c || !grad_refine_pose_dev) return fail(TAMF_ERR_INVALID, "null argument");
  if (!c->have_forward) return fail(TAMF_ERR_STATE, "tamf_refinetrain_backward needs a preceding tamf_refinetrain_forward on this context (a forward serves one backward)");
  if (int rc = c->tab.require_bound()) return rc;
  if (int rc = use_device(c)) return rc;
  c->have_forward = false;
  Step s = make_step(c, (hipStream_t)stream);
  s.backward_head(grad_refine_pose_dev);
  for (int l = c->arch.num_layers - 1; l >= 0; --l) s.backward_layer(l);
  s.backward_input();
  return s.status();
}

int tamf_refinetrain_set_profile(tamf_refinetrain_ctx* c, int32_t on) {
  if (!c) return fail(TAMF_ERR_INVALID, "null argument");
  c->profile.on = on != 0;
  return 0;
}

int tamf_refinetrain_get_profile(tamf_refinetrain_ctx* c, char* out, int64_t size) {
  if (!c || !out || size < 1) return fail(TAMF_ERR_INVALID, "null argument");
  return c->profile.report(out, size);
}

int tamf_refinetrain_dropout_mask(uint64_t seed, uint32_t step, int64_t clip_id, int32_t site, int32_t rows, int32_t cols, float p,
                                  uint8_t* out_dev, void* stream) {
  return dropout_mask(seed, step, clip_id, site, rows, cols, p, out_dev, stream);
}

}  // extern "C"
