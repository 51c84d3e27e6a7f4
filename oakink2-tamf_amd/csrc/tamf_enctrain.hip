// libtamf_enctrain.so (include/tamf_enctrain.h): the host side of the SegmentEncoder training step - the table of bound tensors, the
// workspace and the launch sequence of the kernels of tamf_encoder_grad.h.  Host conventions of tamf_weights.h: an int status, a
// thread-local last-error string, nothing thrown across the ABI.
//
// Workspace (floats; R = max_batch * (max_frames + 4) token rows, BT = max_batch * max_frames frame rows), kept from the forward for
// the backward:
//   input stage   shm [B][sd], oem [B][od], trm [BT][qd] (means over frames / objects), cat [BT][128] (hand | object embedding),
//                 zpre, z [BT][64] (input_merge.0 before / after SiLU), pre [R][64] (token rows before nan_to_num and PE)
//   per layer     x [R][64] (its input; x[L] is the output), qkv [R][192], stat [B][4][S][2] (softmax max, sum), att [R][64],
//                 x1pre, x1, x2pre [R][64] (LayerNorm inputs / output), hpre, gel [R][ff] (linear1 output, dropped-out GELU)
//   head          h1pre, h1, h2pre, h2 [B][64]
// and the transient gradients of the backward (dx, dz, dym, tt, dx1, datt [R][64], dqkv [R][192], dh [R][ff], delta, dpre, dzin, dcat,
// dact, dh1, dh2, the per-clip losses) and the slab of weight-gradient partial sums [<= 64 splits][N][K + 1].
#include "tamf_weights.h"

#include "../../include/tamf_enctrain.h"
#include "tamf_encoder_grad.h"

namespace {

constexpr int MAX_SPLIT = 64, SPLIT_ROWS = 128;

struct Bound {
  std::vector<int64_t> shape;
  bool trainable = true;
  const float* p = nullptr;
  float* g = nullptr;
};

struct LayerWs {
  long x, qkv, stat, att, x1pre, x1, x2pre, hpre, gel;
};

// one bound (weight, bias) pair with its gradients - a linear map, or the gain and bias of a LayerNorm
struct Lin {
  const float *w = nullptr, *b = nullptr;
  float *gw = nullptr, *gb = nullptr;
};
struct LayerP {
  Lin inproj, out, l1, l2, n1, n2;
};

}  // namespace

struct tamf_enctrain_ctx {
  tamf_arch arch;
  int maxB, maxT, device;
  std::vector<std::string> order;
  std::map<std::string, Bound> t;
  float* ws = nullptr;
  int* cnt = nullptr;           // [maxB]
  long long* clip = nullptr;    // [maxB]
  // offsets in floats
  long shm, oem, trm, cat, zpre, z, pre, xlast, h1pre, h1, h2pre, h2;
  long dx, dz, dym, tt, dx1, datt, dqkv, dh, delta, dpre, dzin, dcat, dact, dh1, dh2, lb, slab;
  std::vector<LayerWs> lw;
  // the bound pointers, looked up once after a bind (resolve()), not per launch
  bool resolved = false;
  const float *rh = nullptr, *lh = nullptr, *cls = nullptr, *pe = nullptr;
  Lin shape, obj, pose, traj, m0, m2, p0, p2, p4;
  std::vector<LayerP> lp;
};

namespace {

void declare(tamf_enctrain_ctx* c, const std::string& k, std::vector<int64_t> shape, bool trainable = true) {
  c->order.push_back(k);
  Bound& b = c->t[k];
  b.shape = std::move(shape);
  b.trainable = trainable;
}
void declare_linear(tamf_enctrain_ctx* c, const std::string& k, int64_t o, int64_t i) {
  declare(c, k + ".weight", {o, i});
  declare(c, k + ".bias", {o});
}

Lin lin_of(tamf_enctrain_ctx* c, const std::string& wk, const std::string& bk) {
  const Bound &w = c->t.at(wk), &b = c->t.at(bk);
  Lin l;
  l.w = w.p;
  l.b = b.p;
  l.gw = w.g;
  l.gb = b.g;
  return l;
}
Lin lin_of(tamf_enctrain_ctx* c, const std::string& k) { return lin_of(c, k + ".weight", k + ".bias"); }
void resolve(tamf_enctrain_ctx* c) {
  c->rh = c->t.at("hand_side_process.rh_embed").p;
  c->lh = c->t.at("hand_side_process.lh_embed").p;
  c->cls = c->t.at("classification_token").p;
  c->pe = c->t.at("sequence_pos_encoder.pe").p;
  c->shape = lin_of(c, "hand_shape_process.shape_embed");
  c->obj = lin_of(c, "obj_embed_process.embedding");
  c->pose = lin_of(c, "input_process.poseEmbedding");
  c->traj = lin_of(c, "obj_input_process.poseEmbedding");
  c->m0 = lin_of(c, "input_merge.0");
  c->m2 = lin_of(c, "input_merge.2");
  c->p0 = lin_of(c, "output_process.poseFinal.0");
  c->p2 = lin_of(c, "output_process.poseFinal.2");
  c->p4 = lin_of(c, "output_process.poseFinal.4");
  c->lp.resize(c->arch.num_layers);
  for (int l = 0; l < c->arch.num_layers; ++l) {
    const std::string p = "seqTransEncoder.layers." + std::to_string(l) + ".";
    LayerP& x = c->lp[l];
    x.inproj = lin_of(c, p + "self_attn.in_proj_weight", p + "self_attn.in_proj_bias");
    x.out = lin_of(c, p + "self_attn.out_proj");
    x.l1 = lin_of(c, p + "linear1");
    x.l2 = lin_of(c, p + "linear2");
    x.n1 = lin_of(c, p + "norm1");
    x.n2 = lin_of(c, p + "norm2");
  }
  c->resolved = true;
}

RowMap flat(long ld) { return RowMap{1 << 30, 0, ld}; }

struct Step {
  tamf_enctrain_ctx* c;
  hipStream_t st;
  int B, T, S;
  Drop d;
  hipError_t err = hipSuccess;

  float* w(long off) const { return c->ws + off; }
  RowMap rows(int nq, long ld) const { return RowMap{nq, (long)S * ld, ld}; }  // nq rows of every clip inside [B][S][ld]
  void check() {
    if (err == hipSuccess) err = hipGetLastError();
  }

  void lin(LinArgs a) {
    a.d = d;
    const long tiles = (long)((a.M + 15) / 16) * ((a.N + 15) / 16);
    lin_kernel<<<blocks(tiles, 4), 256, 0, st>>>(a);
    check();
  }
  // dW (N, K) and db (N) of a linear map from its output gradient Y and its input A over R rows
  void wgrad(const float* Y, RowMap ym, const float* A, RowMap am, int R, int N, int K, const Lin& lin) {
    const int nsplit = std::max(1, std::min(MAX_SPLIT, (R + SPLIT_ROWS - 1) / SPLIT_ROWS));
    const int chunk = ((R + nsplit - 1) / nsplit + 3) / 4 * 4;
    WgradArgs a{Y, ym, A, am, w(c->slab), R, N, K, nsplit, chunk};
    const long tiles = (long)((N + 15) / 16) * ((K + 1 + 15) / 16) * nsplit;
    wgrad_kernel<<<blocks(tiles, 4), 256, 0, st>>>(a);
    check();
    reduce_kernel<<<blocks((long)N * (K + 1), 256), 256, 0, st>>>(w(c->slab), nsplit, N, K + 1, K, lin.gw, lin.gb);
    check();
  }
  void colsum(const float* X, RowMap xm, int R, float* out) {
    const int nsplit = std::max(1, std::min(MAX_SPLIT, (R + SPLIT_ROWS - 1) / SPLIT_ROWS));
    const int chunk = (R + nsplit - 1) / nsplit;
    colsum_kernel<<<nsplit, ENC_D, 0, st>>>(X, xm, R, chunk, w(c->slab));
    check();
    reduce_kernel<<<1, ENC_D, 0, st>>>(w(c->slab), nsplit, 1, ENC_D, ENC_D, out, nullptr);
    check();
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

  tamf_enctrain_ctx* c = new (std::nothrow) tamf_enctrain_ctx();
  if (!c) return fail(TAMF_ERR_NOMEM, "out of host memory");
  c->arch = *arch;
  c->maxB = max_batch;
  c->maxT = max_frames;
  c->device = device;
  const int d = ENC_D, F = arch->input_dim, ff = arch->ff_size, L = arch->num_layers, sd = arch->hand_shape_dim, od = arch->obj_embed_dim,
            qd = arch->obj_input_dim;
  declare(c, "hand_side_process.rh_embed", {d}, false);
  declare(c, "hand_side_process.lh_embed", {d}, false);
  declare_linear(c, "hand_shape_process.shape_embed", d, sd);
  declare_linear(c, "obj_embed_process.embedding", d, od);
  declare(c, "classification_token", {1, 1, d}, false);
  declare_linear(c, "input_process.poseEmbedding", d, F);
  declare_linear(c, "obj_input_process.poseEmbedding", d, qd);
  declare_linear(c, "input_merge.0", d, 2 * d);
  declare_linear(c, "input_merge.2", d, d);
  declare(c, "sequence_pos_encoder.pe", {5000, 1, d}, false);
  for (int l = 0; l < L; ++l) {
    const std::string p = "seqTransEncoder.layers." + std::to_string(l) + ".";
    declare(c, p + "self_attn.in_proj_weight", {3 * d, d});
    declare(c, p + "self_attn.in_proj_bias", {3 * d});
    declare_linear(c, p + "self_attn.out_proj", d, d);
    declare_linear(c, p + "linear1", ff, d);
    declare_linear(c, p + "linear2", d, ff);
    declare(c, p + "norm1.weight", {d});
    declare(c, p + "norm1.bias", {d});
    declare(c, p + "norm2.weight", {d});
    declare(c, p + "norm2.bias", {d});
  }
  declare_linear(c, "output_process.poseFinal.0", d, d);
  declare_linear(c, "output_process.poseFinal.2", d, d);
  declare_linear(c, "output_process.poseFinal.4", F, d);

  const long Bm = max_batch, R = Bm * (max_frames + ENC_P + 1), BT = Bm * max_frames;
  Carver cv;
  c->shm = cv.take(Bm * sd);
  c->oem = cv.take(Bm * od);
  c->trm = cv.take(BT * qd);
  c->cat = cv.take(BT * 2 * d);
  c->zpre = cv.take(BT * d);
  c->z = cv.take(BT * d);
  c->pre = cv.take(R * d);
  c->lw.resize(L);
  for (int l = 0; l < L; ++l) {
    LayerWs& x = c->lw[l];
    x.x = cv.take(R * d);
    x.qkv = cv.take(R * 3 * d);
    x.stat = cv.take(R * EG_H * 2);
    x.att = cv.take(R * d);
    x.x1pre = cv.take(R * d);
    x.x1 = cv.take(R * d);
    x.x2pre = cv.take(R * d);
    x.hpre = cv.take(R * ff);
    x.gel = cv.take(R * ff);
  }
  c->xlast = cv.take(R * d);
  c->h1pre = cv.take(Bm * d);
  c->h1 = cv.take(Bm * d);
  c->h2pre = cv.take(Bm * d);
  c->h2 = cv.take(Bm * d);
  c->dx = cv.take(R * d);
  c->dz = cv.take(R * d);
  c->dym = cv.take(R * d);
  c->tt = cv.take(R * d);
  c->dx1 = cv.take(R * d);
  c->datt = cv.take(R * d);
  c->dqkv = cv.take(R * 3 * d);
  c->dh = cv.take(R * ff);
  c->delta = cv.take(R * EG_H);
  c->dpre = cv.take(R * d);
  c->dzin = cv.take(BT * d);
  c->dcat = cv.take(BT * 2 * d);
  c->dact = cv.take(Bm * F);
  c->dh1 = cv.take(Bm * d);
  c->dh2 = cv.take(Bm * d);
  c->lb = cv.take(Bm);
  long nk = 0;  // the largest N * (K + 1) of a linear map
  for (long v : {(long)d * (sd + 1), (long)d * (od + 1), (long)d * (F + 1), (long)d * (qd + 1), (long)d * (2 * d + 1), (long)3 * d * (d + 1), (long)ff * (d + 1),
                 (long)d * (ff + 1), (long)F * (d + 1)})
    nk = std::max(nk, v);
  c->slab = cv.take(nk * MAX_SPLIT);
  e = hipMalloc((void**)&c->ws, cv.total * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&c->cnt, Bm * sizeof(int));
  if (e == hipSuccess) e = hipMalloc((void**)&c->clip, Bm * sizeof(long long));
  if (e != hipSuccess) {
    const std::string msg = std::string("hipMalloc of the workspace (") + std::to_string(cv.total * sizeof(float)) + " bytes): " + hipGetErrorString(e);
    tamf_enctrain_destroy(c);
    return fail(e == hipErrorOutOfMemory ? TAMF_ERR_NOMEM : TAMF_ERR_HIP, msg);
  }
  *out = c;
  return 0;
}

void tamf_enctrain_destroy(tamf_enctrain_ctx* c) {
  if (!c) return;
  if (c->ws) (void)hipFree(c->ws);
  if (c->cnt) (void)hipFree(c->cnt);
  if (c->clip) (void)hipFree(c->clip);
  delete c;
}

int tamf_enctrain_bind(tamf_enctrain_ctx* c, const char* name, const float* param_dev, float* grad_dev, const int64_t* shape, int32_t ndim) {
  if (!c || !name || !param_dev || ndim < 0 || (ndim > 0 && !shape)) return fail(TAMF_ERR_INVALID, "null argument");
  auto it = c->t.find(name);
  if (it == c->t.end()) return fail(TAMF_ERR_INVALID, std::string("unknown key '") + name + "'");
  Bound& b = it->second;
  if ((size_t)ndim != b.shape.size() || !std::equal(b.shape.begin(), b.shape.end(), shape))
    return fail(TAMF_ERR_INVALID, std::string(name) + ": expected shape " + shape_str(b.shape.data(), (int)b.shape.size()) + ", got " + shape_str(shape, ndim));
  if (b.trainable && !grad_dev) return fail(TAMF_ERR_INVALID, std::string(name) + ": a trainable tensor needs a gradient buffer");
  if (!b.trainable && grad_dev) return fail(TAMF_ERR_INVALID, std::string(name) + ": a buffer takes no gradient");
  b.p = param_dev;
  b.g = grad_dev;
  c->resolved = false;
  return 0;
}

int tamf_enctrain_step(tamf_enctrain_ctx* c, int32_t B, int32_t T, int32_t nobj, const int32_t* obj_num_host, const float* pose_dev,
                       const float* shape_dev, const uint8_t* hand_side_dev, const float* obj_emb_dev, const float* obj_traj_dev,
                       const int64_t* labels_dev, const int64_t* clip_id_host, float dropout_p, uint64_t seed, uint32_t step,
                       float* loss_out_dev, float* activation_out_dev, void* stream) {
  if (!c || !pose_dev || !shape_dev || !hand_side_dev || !obj_emb_dev || !obj_traj_dev || !labels_dev || !loss_out_dev || !activation_out_dev)
    return fail(TAMF_ERR_INVALID, "null argument");
  if (B < 1 || B > c->maxB) return fail(TAMF_ERR_INVALID, "B = " + std::to_string(B) + " outside [1, max_batch = " + std::to_string(c->maxB) + "]");
  if (T < 1 || T > c->maxT) return fail(TAMF_ERR_INVALID, "T = " + std::to_string(T) + " outside [1, max_frames = " + std::to_string(c->maxT) + "]");
  if (nobj < 1 || nobj > 4096) return fail(TAMF_ERR_INVALID, "nobj = " + std::to_string(nobj) + " outside [1, 4096]");
  if (!(dropout_p >= 0.f && dropout_p < 1.f)) return fail(TAMF_ERR_INVALID, "dropout_p must be in [0, 1)");
  if (obj_num_host)
    for (int b = 0; b < B; ++b)
      if (obj_num_host[b] < 1 || obj_num_host[b] > nobj)
        return fail(TAMF_ERR_INVALID, "obj_num[" + std::to_string(b) + "] = " + std::to_string(obj_num_host[b]) + " outside [1, nobj = " + std::to_string(nobj) + "]");
  if (!c->resolved) {  // (the first step after a bind: every tensor has to be there, then the pointers are looked up once)
    for (const std::string& k : c->order)
      if (!c->t[k].p) return fail(TAMF_ERR_MISSING, "missing binding '" + k + "'");
    resolve(c);
  }
  hipError_t e = hipSetDevice(c->device);
  if (e != hipSuccess) return fail(TAMF_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));

  Step s;
  s.c = c;
  s.st = (hipStream_t)stream;
  s.B = B;
  s.T = T;
  s.S = T + ENC_P + 1;
  const int S = s.S, d = ENC_D, F = c->arch.input_dim, ff = c->arch.ff_size, L = c->arch.num_layers, sd = c->arch.hand_shape_dim,
            od = c->arch.obj_embed_dim, qd = c->arch.obj_input_dim, BT = B * T, BS = B * S;
  hipStream_t st = s.st;
  if (obj_num_host) {
    e = hipMemcpyAsync(c->cnt, obj_num_host, B * sizeof(int), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return fail(TAMF_ERR_HIP, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
  }
  if (clip_id_host) {
    e = hipMemcpyAsync(c->clip, clip_id_host, B * sizeof(long long), hipMemcpyHostToDevice, st);
    if (e != hipSuccess) return fail(TAMF_ERR_HIP, std::string("hipMemcpyAsync: ") + hipGetErrorString(e));
  }
  s.d.k0 = (uint32_t)(seed & 0xFFFFFFFFu);
  s.d.k1 = (uint32_t)(seed >> 32);
  s.d.step = step;
  s.d.thr = (uint32_t)std::min(4294967295.0, std::floor((double)dropout_p * 4294967296.0));
  s.d.scale = 1.0f / (1.0f - dropout_p);
  s.d.clip = clip_id_host ? c->clip : nullptr;
  const Drop& dr = s.d;
  auto w = [&](long off) { return c->ws + off; };
  const size_t att_lds = (size_t)S * ENC_HD * 2 * sizeof(float);

  // ---------------- forward ----------------
  {
    PrepArgs a{shape_dev, obj_emb_dev, obj_traj_dev, hand_side_dev, obj_num_host ? c->cnt : nullptr, c->rh, c->lh, c->cls, w(c->shm), w(c->oem), w(c->trm), w(c->pre), B, T, nobj, sd, od, qd};
    const long n = (long)B * sd + (long)B * od + (long)BT * qd + (long)B * 2 * d;
    prep_kernel<<<blocks(n, 256), 256, 0, st>>>(a);
    s.check();
  }
  const RowMap one = RowMap{1, (long)S * d, d};  // one row of every clip inside [B][S][64]
  auto base_lin = [&](const float* A, RowMap am, const Lin& lin, float* C, RowMap cm, int M, int N, int K) {
    LinArgs a{};
    a.A = A;
    a.am = am;
    a.W = lin.w;
    a.swn = K;
    a.swk = 1;
    a.bias = lin.b;
    a.C = C;
    a.cm = cm;
    a.rm = cm;
    a.M = M;
    a.N = N;
    a.K = K;
    a.mode = EG_LIN;
    return a;
  };
  // the data gradient of the same map: dA (M, K) = dY (M, N) . W
  auto base_dgrad = [&](const float* dY, RowMap ym, const Lin& lin, int N, int K, float* C, RowMap cm, int M) {
    LinArgs a{};
    a.A = dY;
    a.am = ym;
    a.W = lin.w;
    a.swn = 1;
    a.swk = K;
    a.C = C;
    a.cm = cm;
    a.rm = cm;
    a.M = M;
    a.N = K;
    a.K = N;
    a.mode = EG_LIN;
    return a;
  };
  s.lin(base_lin(w(c->shm), flat(sd), c->shape, w(c->pre) + 1 * d, one, B, d, sd));
  s.lin(base_lin(w(c->oem), flat(od), c->obj, w(c->pre) + 2 * d, one, B, d, od));
  s.lin(base_lin(pose_dev, flat(F), c->pose, w(c->cat), flat(2 * d), BT, d, F));
  s.lin(base_lin(w(c->trm), flat(qd), c->traj, w(c->cat) + d, flat(2 * d), BT, d, qd));
  {
    LinArgs a = base_lin(w(c->cat), flat(2 * d), c->m0, w(c->z), flat(d), BT, d, 2 * d);
    a.mode = EG_SILU;
    a.C2 = w(c->zpre);
    s.lin(a);
  }
  const RowMap frames = RowMap{T, (long)S * d, d};
  s.lin(base_lin(w(c->z), flat(d), c->m2, w(c->pre) + ENC_P * d, frames, BT, d, d));
  const float* pe = c->pe;
  auto xof = [&](int l) { return w(l < L ? c->lw[l].x : c->xlast); };
  assemble_kernel<<<blocks((long)BS * d, 256), 256, 0, st>>>(w(c->pre), pe, xof(0), nullptr, nullptr, B, S, dr);
  s.check();

  for (int l = 0; l < L; ++l) {
    const LayerWs& x = c->lw[l];
    const LayerP& lp = c->lp[l];
    const int q0 = l == L - 1 ? S - 1 : 0, nq = S - q0, M = B * nq, site = 1 + 4 * l;
    const RowMap r64 = s.rows(nq, d), rff = s.rows(nq, ff);
    const long o64 = (long)q0 * d, off = (long)q0 * ff;
    s.lin(base_lin(xof(l), flat(d), lp.inproj, w(x.qkv), flat(3 * d), BS, 3 * d, d));
    {
      AttnArgs a{w(x.qkv), w(x.att), w(x.stat), nullptr, nullptr, nullptr, S, q0, site, dr};
      attn_fwd_kernel<<<dim3((nq + 63) / 64, EG_H, B), 64, att_lds, st>>>(a);
      s.check();
    }
    {
      LinArgs a = base_lin(w(x.att) + o64, r64, lp.out, w(x.x1pre) + o64, r64, M, d, d);
      a.mode = EG_DROP_RES;
      a.R = xof(l) + o64;
      a.site = site + 1;
      a.q0 = q0;
      s.lin(a);
    }
    ln_fwd_kernel<<<blocks(M, 4), 256, 0, st>>>(w(x.x1pre) + o64, r64, w(x.x1) + o64, r64, lp.n1.w, lp.n1.b, M);
    s.check();
    {
      LinArgs a = base_lin(w(x.x1) + o64, r64, lp.l1, w(x.gel) + off, rff, M, ff, d);
      a.mode = EG_GELU_DROP;
      a.C2 = w(x.hpre) + off;
      a.site = site + 2;
      a.q0 = q0;
      s.lin(a);
    }
    {
      LinArgs a = base_lin(w(x.gel) + off, rff, lp.l2, w(x.x2pre) + o64, r64, M, d, ff);
      a.mode = EG_DROP_RES;
      a.R = w(x.x1) + o64;
      a.site = site + 3;
      a.q0 = q0;
      s.lin(a);
    }
    ln_fwd_kernel<<<blocks(M, 4), 256, 0, st>>>(w(x.x2pre) + o64, r64, xof(l + 1) + o64, r64, lp.n2.w, lp.n2.b, M);
    s.check();
  }
  const float* enc = xof(L) + (long)(S - 1) * d;  // the classification rows, at `one`
  {
    LinArgs a = base_lin(enc, one, c->p0, w(c->h1), flat(d), B, d, d);
    a.mode = EG_SILU;
    a.C2 = w(c->h1pre);
    s.lin(a);
    a = base_lin(w(c->h1), flat(d), c->p2, w(c->h2), flat(d), B, d, d);
    a.mode = EG_SILU;
    a.C2 = w(c->h2pre);
    s.lin(a);
    s.lin(base_lin(w(c->h2), flat(d), c->p4, activation_out_dev, flat(F), B, F, d));
  }
  ce_kernel<<<1, 256, 0, st>>>(activation_out_dev, (const long long*)labels_dev, B, F, w(c->lb), w(c->dact), loss_out_dev);
  s.check();

  // ---------------- backward ----------------
  s.wgrad(w(c->dact), flat(F), w(c->h2), flat(d), B, F, d, c->p4);
  {
    LinArgs a = base_dgrad(w(c->dact), flat(F), c->p4, F, d, w(c->dh2), flat(d), B);
    a.mode = EG_BWD_SILU;
    a.R = w(c->h2pre);
    s.lin(a);
    s.wgrad(w(c->dh2), flat(d), w(c->h1), flat(d), B, d, d, c->p2);
    a = base_dgrad(w(c->dh2), flat(d), c->p2, d, d, w(c->dh1), flat(d), B);
    a.mode = EG_BWD_SILU;
    a.R = w(c->h1pre);
    s.lin(a);
    s.wgrad(w(c->dh1), flat(d), enc, one, B, d, d, c->p0);
    s.lin(base_dgrad(w(c->dh1), flat(d), c->p0, d, d, w(c->dx) + (long)(S - 1) * d, one, B));
  }
  for (int l = L - 1; l >= 0; --l) {
    const LayerWs& x = c->lw[l];
    const LayerP& lp = c->lp[l];
    const int q0 = l == L - 1 ? S - 1 : 0, nq = S - q0, M = B * nq, site = 1 + 4 * l;
    const RowMap r64 = s.rows(nq, d), rff = s.rows(nq, ff);
    const long o64 = (long)q0 * d, off = (long)q0 * ff;
    // LayerNorm 2, linear2, GELU, linear1
    ln_bwd_kernel<<<blocks(M, 4), 256, 0, st>>>(w(c->dx) + o64, w(x.x2pre) + o64, r64, lp.n2.w, w(c->dz) + o64, w(c->dym) + o64,
                                                w(c->tt) + o64, M, q0, site + 3, dr);
    s.check();
    s.colsum(w(c->tt) + o64, r64, M, lp.n2.gw);
    s.colsum(w(c->dx) + o64, r64, M, lp.n2.gb);
    s.wgrad(w(c->dym) + o64, r64, w(x.gel) + off, rff, M, d, ff, lp.l2);
    {
      LinArgs a = base_dgrad(w(c->dym) + o64, r64, lp.l2, d, ff, w(c->dh) + off, rff, M);
      a.mode = EG_BWD_GELU_DROP;
      a.R = w(x.hpre) + off;
      a.site = site + 2;
      a.q0 = q0;
      s.lin(a);
    }
    s.wgrad(w(c->dh) + off, rff, w(x.x1) + o64, r64, M, ff, d, lp.l1);
    {
      LinArgs a = base_dgrad(w(c->dh) + off, rff, lp.l1, ff, d, w(c->dx1) + o64, r64, M);
      a.mode = EG_BWD_RES;
      a.R = w(c->dz) + o64;
      s.lin(a);
    }
    // LayerNorm 1, out-projection, attention, in-projection
    ln_bwd_kernel<<<blocks(M, 4), 256, 0, st>>>(w(c->dx1) + o64, w(x.x1pre) + o64, r64, lp.n1.w, w(c->dz) + o64, w(c->dym) + o64,
                                                w(c->tt) + o64, M, q0, site + 1, dr);
    s.check();
    s.colsum(w(c->tt) + o64, r64, M, lp.n1.gw);
    s.colsum(w(c->dx1) + o64, r64, M, lp.n1.gb);
    s.wgrad(w(c->dym) + o64, r64, w(x.att) + o64, r64, M, d, d, lp.out);
    s.lin(base_dgrad(w(c->dym) + o64, r64, lp.out, d, d, w(c->datt) + o64, r64, M));
    {
      AttnArgs a{w(x.qkv), nullptr, w(x.stat), w(c->datt), w(c->dqkv), w(c->delta), S, q0, site, dr};
      attn_bwd_q_kernel<<<dim3((S + 63) / 64, EG_H, B), 64, att_lds, st>>>(a);
      s.check();
      attn_bwd_kv_kernel<<<dim3((S + 63) / 64, EG_H, B), 64, att_lds, st>>>(a);
      s.check();
    }
    s.wgrad(w(c->dqkv), flat(3 * d), xof(l), flat(d), BS, 3 * d, d, lp.inproj);
    {
      LinArgs a = base_dgrad(w(c->dqkv), flat(3 * d), lp.inproj, 3 * d, d, w(c->dx), s.rows(S, d), BS);
      a.mode = EG_BWD_RES_Q0;
      a.R = w(c->dz);
      a.rq0 = q0;
      s.lin(a);
    }
  }
  // input stage
  assemble_kernel<<<blocks((long)BS * d, 256), 256, 0, st>>>(w(c->pre), pe, nullptr, w(c->dx), w(c->dpre), B, S, dr);
  s.check();
  s.wgrad(w(c->dpre) + 1 * d, one, w(c->shm), flat(sd), B, d, sd, c->shape);
  s.wgrad(w(c->dpre) + 2 * d, one, w(c->oem), flat(od), B, d, od, c->obj);
  const float* dfr = w(c->dpre) + ENC_P * d;
  s.wgrad(dfr, frames, w(c->z), flat(d), BT, d, d, c->m2);
  {
    LinArgs a = base_dgrad(dfr, frames, c->m2, d, d, w(c->dzin), flat(d), BT);
    a.mode = EG_BWD_SILU;
    a.R = w(c->zpre);
    s.lin(a);
  }
  s.wgrad(w(c->dzin), flat(d), w(c->cat), flat(2 * d), BT, d, 2 * d, c->m0);
  s.lin(base_dgrad(w(c->dzin), flat(d), c->m0, d, 2 * d, w(c->dcat), flat(2 * d), BT));
  s.wgrad(w(c->dcat), flat(2 * d), pose_dev, flat(F), BT, d, F, c->pose);
  s.wgrad(w(c->dcat) + d, flat(2 * d), w(c->trm), flat(qd), BT, d, qd, c->traj);

  if (s.err != hipSuccess) return fail(TAMF_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(s.err));
  return 0;
}

int tamf_enctrain_dropout_mask(uint64_t seed, uint32_t step, int64_t clip_id, int32_t site, int32_t rows, int32_t cols, float p,
                               uint8_t* out_dev, void* stream) {
  if (!out_dev) return fail(TAMF_ERR_INVALID, "null argument");
  if (rows < 1 || cols < 1 || (long)rows * cols > 0xFFFFFFFFL) return fail(TAMF_ERR_INVALID, "rows * cols must be in [1, 2^32)");
  if (site < 0) return fail(TAMF_ERR_INVALID, "site must be >= 0");
  if (!(p >= 0.f && p < 1.f)) return fail(TAMF_ERR_INVALID, "p must be in [0, 1)");
  Drop d;
  d.k0 = (uint32_t)(seed & 0xFFFFFFFFu);
  d.k1 = (uint32_t)(seed >> 32);
  d.step = step;
  d.thr = (uint32_t)std::min(4294967295.0, std::floor((double)p * 4294967296.0));
  d.scale = 1.0f / (1.0f - p);
  d.clip = nullptr;
  const long n = (long)rows * cols;
  dropout_mask_kernel<<<blocks(n, 256), 256, 0, (hipStream_t)stream>>>(d, site, (unsigned long long)clip_id, n, out_dev);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(TAMF_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
  return 0;
}

}  // extern "C"
