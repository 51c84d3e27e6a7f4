// libtamf_hip.so - host side of the C-ABI declared in include/tamf_hip.h: context, weight repacking,
// step-invariant conditioning precompute, the per-step kernel sequence and its hipGraph replay loop.
// gfx950 (MI355X) only.
#include "../../include/tamf_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "tamf_attn.h"
#include "tamf_gemm.h"
#include "tamf_gemm_clip.h"
#include "tamf_gemm_deep.h"
#include "tamf_geom.h"
#include "tamf_misc.h"
#include "tamf_encoder.h"
#include "tamf_spectrum.h"
#include "tamf_shapes.h"       // host only: the shape arithmetic
#include "tamf_weight_prep.h"  // host only: what is uploaded as a weight, before it is uploaded

// run EXPR with `Op` bound to the operand traits of arithmetic mode `prec` (tamf_precision)
#define TAMF_WITH_OP(prec, EXPR)                                         \
  switch (prec) {                                                        \
    case TAMF_PREC_F32: { typedef OpF32 Op; EXPR; } break;               \
    case TAMF_PREC_BF16: { typedef OpBF16 Op; EXPR; } break;             \
    case TAMF_PREC_BF16X3: { typedef OpBF16X3 Op; EXPR; } break;         \
    default: { typedef OpF16X3 Op; EXPR; } break;                        \
  }

// ------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_noctx_err;  // context-free failures of the calling thread (tamf_last_error(NULL))

struct OperandBuf {
  void* p = nullptr;
  float inv_scale = 1.0f;  // f16x3 weights are stored scaled by a power of two (upload_operand); this is its inverse, applied by the epilogue
};

struct LayerW {
  OperandBuf Win, Wout, W1, W2;
  // deferred LayerNorm (tamf_device.h): Win / W1 hold W diag(gamma) (I - 1 1^T / d), the consumers take c2 = W beta + b
  // in place of the bias, the residual adds take (gamma, beta + bias) of the LayerNorm their residual passes through
  float *c2_in = nullptr, *c2_ff = nullptr;
  float *g_att = nullptr, *bb_att = nullptr, *g_ffn = nullptr, *bb_ffn = nullptr;
};

// What a captured step sequence depends on.  Seed, clip range, noise / dump tensors are NOT part of it: the kernels read
// them from the device-side LoopParams block, so one executable graph serves every loop of the same shape.
struct GraphKey {
  int B = -1, T = -1, n_steps = -1, steps_per_graph = 0;
  bool operator==(const GraphKey& o) const {
    return B == o.B && T == o.T && n_steps == o.n_steps && steps_per_graph == o.steps_per_graph;
  }
};

// Guard-band mode, for tests only (GPU AddressSanitizer is not available for gfx950 here): with tamf_test_set_guard_bytes(n > 0) every
// device allocation of contexts created afterwards is n bytes longer at both ends, the margins are filled with GUARD_BYTE, and
// tamf_test_check_guards() verifies them - a kernel that stores below or beyond its buffer (the V^T overrun of round 4) changes a margin
// instead of a neighbouring live buffer, where a later kernel would have overwritten the evidence.
struct GuardRec {
  char* base;
  size_t bytes, guard;
  const char* tag;
  bool ws;
};
static constexpr unsigned char GUARD_BYTE = 0xA5;
static std::atomic<size_t> g_guard_bytes{0};
static thread_local const char* g_alloc_tag = "";

// Everything dimensioned by (max_batch, max_frames), i.e. what alloc_workspaces / enc_alloc_workspaces fill.  tamf_ctx_resize moves this
// sub-object out of the context and back as a whole (ws_take / ws_put): a member added here is saved and restored with the rest.
struct Workspaces {
  int Bmax = 0, Tmax = 0;
  long Mmax = 0;
  float *xs = nullptr, *cobj = nullptr, *X = nullptr, *pstatic = nullptr;
  OperandBuf xs_op, h1_op, X_op, QK_op, Vt_op, A_op, H_op;
  // f32: an fp32 operand matrix [rows][ld] is byte for byte the fp32 tensor, so the residual stream X and the sampler state xs ARE
  // their own operands (X_op.p = X, xs_op.p = xs) and the kernels that used to write both copies write one (X_st / xs_st = null):
  // 27 MB less per LayerNorm at B = 64 (round 4)
  void *X_st = nullptr, *xs_st = nullptr;
  int* tcur = nullptr;
  unsigned* status = nullptr;  // this context's sticky status word (tamf_device.h): written by its kernels only
  unsigned char* side_dev = nullptr;
  int* objnum_dev = nullptr;  // per-clip object counts of tamf_set_cond_ragged
  // deferred LayerNorm: partial row statistics of the residual stream after the attention / feed-forward sublayer, [Mmax][d / 32]
  float2 *stat_att = nullptr, *stat_ffn = nullptr;
  LoopParams* loop_params = nullptr;
  std::vector<void*> ws_allocs;  // the allocations behind the pointers above
};

struct tamf_ctx : Workspaces {
  tamf_arch arch{};
  int prec = 0, device = 0;
  int d = 0, ff = 0, L = 0, H = 0, hd = 0, P = 0, F = 0, has_t = 0;
  int XK = 0;   // padded K of the fused input GEMM
  int XN = 128; // padded N of the output head
  int EB = 4;  // bytes per logical operand element (f32 4, bf16 2, bf16x3 4 = hi + lo)
  std::string err;
  std::vector<void*> allocs;     // weights, tables, schedule: live as long as the context (the workspaces: Workspaces::ws_allocs)
  bool alloc_ws = false;         // dev_alloc files its allocation under ws_allocs
  std::vector<GuardRec> guards;  // guard-band mode (tamf_test_set_guard_bytes): one record per allocation
  std::map<std::string, std::vector<int64_t>> expected;  // checkpoint key -> shape (expected_shapes), until the weights are finalised
  std::map<std::string, std::vector<float>> raw;
  bool finalized = false, cond_set = false;
  int n_t = 0;  // rows of the timestep table
  // schedule
  int n_steps = 0;
  std::vector<float> h_c1, h_c2, h_sigma;
  float *c1 = nullptr, *c2 = nullptr, *sigma = nullptr;
  // weights
  std::vector<LayerW> layers;
  OperandBuf Wfused, Wm2, Wf;
  float *bm2 = nullptr, *bf = nullptr;
  float* pe = nullptr;    // [5000][d]
  float* temb = nullptr;  // [n_t][d]
  // respaced sampling (tamf_set_timestep_map): row i = temb[map[i]], i = the loop's own step index; the loop's kernels read this table
  // instead of temb while a map is set (a single evaluation - tamf_denoise - always indexes temb with the caller's timesteps)
  float* temb_loop = nullptr;
  int temb_loop_cap = 0;
  bool tmap_on = false, in_loop = false;
  int tmap_max = -1;
  OperandBuf Wt1_f32, Wt2_f32;
  float *bt1 = nullptr, *bt2 = nullptr;
  // conditioning (tamf_misc.h, prefix_rows_kernel / cobj_kernel): transposed weights W^T [K][d]; WcT / bc = input_merge.0[:, d:2d] composed with
  // obj_input_process.poseEmbedding (and the fused bias of input_merge.0)
  float *WtxtT = nullptr, *btxt = nullptr, *WshapeT = nullptr, *bshape = nullptr, *WobjT = nullptr, *bobj = nullptr;
  float *WcT = nullptr, *bc = nullptr, *rh = nullptr, *lh = nullptr;
  // shape of the conditioning in force (the activations themselves: Workspaces)
  int B = 0, T = 0, S = 0, Sp = 0, Skp = 0, M = 0;
  float* enc_w = nullptr;  // SegmentEncoder (TAMF_KIND_E, tamf_encoder.h): packed weights; its prefix rows live in pstatic [Bmax][3][d]
  int enc_kin = 0;         // ... and the K of its fused input linear map (input_dim + obj_input_dim, padded to 4)
  unsigned host_status = 0;  // status bits raised on the host (TAMF_STATUS_F16_WEIGHT_RANGE at tamf_finalize_weights); never cleared
  std::string weight_note;   // ... and which tensor raised it
  // graph
  hipStream_t cap_stream = nullptr;
  hipGraph_t graph = nullptr;
  hipGraphExec_t graph_exec = nullptr;
  GraphKey graph_key;
  hipEvent_t graph_done = nullptr;  // recorded after the last launch of graph_exec: waited for before it is destroyed
  bool graph_in_flight = false;
  int sched_cap = 0;  // allocated length of c1 / c2 / sigma
  int graph_captures = 0, graph_launches_last_loop = 0;  // tamf_loop_stats
  int step_kernels = 0;
  // per-launch profiling (tamf_step_profile)
  bool prof_on = false;
  std::vector<hipEvent_t> prof_ev;
  std::vector<std::string> prof_names;
  std::vector<double> prof_flops;
};

static std::vector<tamf_ctx*> g_live_ctx;  // contexts of this process (tamf_set_gemm_tuning retires their captured graphs)
static std::mutex g_live_mu;                // (contexts may be created / destroyed from different threads)
// The tuning / selection words (g_krot, g_sel) are process-global and a captured graph has them baked in.  Every entry point that
// enqueues kernels or touches a context's graph holds this lock for its (host-side, microseconds) duration, and so does
// tamf_set_gemm_tuning: a thread inside loop_impl never sees a half-updated selection or a graph being destroyed under it.
static std::recursive_mutex g_launch_mu;
// Round 6: that serialisation exists ONLY in the hooks build (-DTAMF_TEST_HOOKS), where tamf_set_gemm_tuning can change the words.  The
// product library has no setter - g_krot / g_sel are constants there - so its entry points take no process-wide lock: contexts are
// independent (one thread per context, as the header says), the lazily set per-device "kernel attributes prepared" flags and the
// workgroup-slot table are atomics, and the list of live contexts has its own mutex.  Context creation still serialises (TAMF_STATE_LOCK).
#ifdef TAMF_TEST_HOOKS
#define TAMF_LAUNCH_LOCK std::lock_guard<std::recursive_mutex> launch_lock_(g_launch_mu)
#else
#define TAMF_LAUNCH_LOCK ((void)0)
#endif
#define TAMF_STATE_LOCK std::lock_guard<std::recursive_mutex> state_lock_(g_launch_mu)

static int fail(tamf_ctx* ctx, int code, const std::string& msg) {
  if (ctx) ctx->err = msg;
  else g_noctx_err = msg;
  return code;
}
// what a context-free entry point returns after its launches
static int launched() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : fail(nullptr, TAMF_ERR_HIP, hipGetErrorString(e));
}
// Kind gating of the entry points: `mask` holds the kinds (KIND_G | ...) that `func` serves.  A null context is TAMF_ERR_INVALID, a
// context of another kind TAMF_ERR_STATE.
enum : unsigned { KIND_G = 1u << TAMF_KIND_G, KIND_R = 1u << TAMF_KIND_R, KIND_E = 1u << TAMF_KIND_E };
static int need_kind(tamf_ctx* ctx, const char* func, unsigned mask) {
  if (!ctx) return fail(ctx, TAMF_ERR_INVALID, std::string(func) + ": null ctx");
  if (mask & (1u << ctx->arch.kind)) return 0;
  if (ctx->arch.kind == TAMF_KIND_E) return fail(ctx, TAMF_ERR_STATE, std::string(func) + ": not available on a SegmentEncoder (TAMF_KIND_E) context");
  return fail(ctx, TAMF_ERR_STATE, std::string(func) + (mask == KIND_E   ? " needs a SegmentEncoder (TAMF_KIND_E) context"
                                                        : mask == KIND_G ? " needs a G context"
                                                        : mask == KIND_R ? " needs an R context"
                                                                         : " needs a G or R context"));
}
#define HIPCHK(ctx, call)                                                                                         \
  do {                                                                                                            \
    hipError_t e_ = (call);                                                                                       \
    if (e_ != hipSuccess)                                                                                         \
      return fail(ctx, TAMF_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_) + " (" + __FILE__ + ":" +  \
                                         std::to_string(__LINE__) + ")");                                        \
  } while (0)
#define TRY(expr)           \
  do {                      \
    int rc_ = (expr);       \
    if (rc_ != 0) return rc_; \
  } while (0)

static inline dim3 grid1d(long n, int bs = 256) { return dim3((unsigned)((n + bs - 1) / bs)); }

static std::atomic<int> g_fail_alloc_in{-1};  // test hook (tamf_test_fail_alloc_after): the n-th device allocation from now fails
static int dev_alloc(tamf_ctx* ctx, void** p, size_t bytes, bool zero = false) {
  if (bytes == 0) bytes = 16;
  const size_t guard = g_guard_bytes.load();
  if (g_fail_alloc_in.load() >= 0 && g_fail_alloc_in.fetch_sub(1) == 0)
    return fail(ctx, TAMF_ERR_NOMEM, "hipMalloc failed: injected by tamf_test_fail_alloc_after");
  hipError_t e = hipMalloc(p, bytes + 2 * guard);
  if (e != hipSuccess) return fail(ctx, TAMF_ERR_NOMEM, std::string("hipMalloc failed: ") + hipGetErrorString(e));
  (ctx->alloc_ws ? ctx->ws_allocs : ctx->allocs).push_back(*p);
  if (guard) {
    char* base = (char*)*p;
    HIPCHK(ctx, hipMemset(base, GUARD_BYTE, guard));
    HIPCHK(ctx, hipMemset(base + guard + bytes, GUARD_BYTE, guard));
    ctx->guards.push_back(GuardRec{base, bytes, guard, g_alloc_tag, ctx->alloc_ws});
    *p = base + guard;
  }
  if (zero) HIPCHK(ctx, hipMemset(*p, 0, bytes));
  return 0;
}
template <class T>
static int dev_upload(tamf_ctx* ctx, T** p, const T* host, size_t n) {
  TRY(dev_alloc(ctx, (void**)p, n * sizeof(T)));
  HIPCHK(ctx, hipMemcpy(*p, host, n * sizeof(T), hipMemcpyHostToDevice));
  return 0;
}

// upload host fp32 [N][K] as an operand matrix [N][ldk] in precision `prec`: packed on the host (pack_operand, tamf_weight_prep.h), its
// refusal or weight-range note recorded in the context, then uploaded
static int upload_operand(tamf_ctx* ctx, int prec, const float* w, int N, int K, int ldk, OperandBuf* out, const char* what) {
  const PackedOperand po = pack_operand(prec, w, N, K, ldk);
  if (po.refused) return fail(ctx, po.error_code(), po.error_message(what));
  out->inv_scale = po.inv_scale;
  if (po.small_share_noted()) {
    ctx->host_status |= TAMF_STATUS_F16_WEIGHT_RANGE;
    if (ctx->weight_note.empty()) ctx->weight_note = po.range_note(what);
  }
  return dev_upload(ctx, (unsigned char**)&out->p, po.image.data(), po.image.size());
}
static int upload_vec(tamf_ctx* ctx, float** p, const std::vector<float>& v) { return dev_upload(ctx, p, v.data(), v.size()); }

#include "tamf_launch.h"

// ------------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------------
extern "C" const char* tamf_last_error(const tamf_ctx* ctx) { return ctx ? ctx->err.c_str() : g_noctx_err.c_str(); }

static int alloc_operand(tamf_ctx* ctx, OperandBuf* ob, long elems, bool zero = false) {
  return dev_alloc(ctx, &ob->p, (size_t)elems * ctx->EB, zero);
}

// the kernels address operands with 32-bit byte offsets and int element indices: refuse shapes beyond them
static int check_dims(const tamf_arch* arch, int max_batch, int max_frames) {
  if (max_batch <= 0 || max_frames <= 0 || max_frames > 4990) return fail(nullptr, TAMF_ERR_INVALID, "bad max_batch/max_frames");
  if (!dims_fit_32bit_offsets(max_batch, max_frames, arch->ff_size, arch->latent_dim))
    return fail(nullptr, TAMF_ERR_INVALID, "max_batch x max_frames too large for one context (32-bit operand offsets): split the batch");
  return 0;
}

// The views of the hidden operand's allocation (scratch_layout, tamf_shapes.h): addresses that depend on (max_batch, max_frames) alone,
// never on the batch of a call - a captured graph stays valid between calls.  Guard-band mode: the margins between the views get the
// pattern and a record each, so that tamf_test_check_guards verifies them like an allocation's.
static int place_scratch_views(tamf_ctx* ctx, const ScratchLayout& sl) {
  char* host = (char*)ctx->H_op.p;
  ctx->QK_op.p = host + sl.qk_off;
  ctx->A_op.p = host + sl.a_off;
  ctx->h1_op.p = host + sl.h1_off;
  const size_t guard = g_guard_bytes.load();
  if (!guard) return 0;
  const struct { size_t off, bytes; const char* tag; } views[3] = {{(size_t)sl.qk_off, (size_t)sl.qk_bytes, "view QK_op of H_op's allocation"},
                                                                  {(size_t)sl.a_off, (size_t)sl.a_bytes, "view A_op of H_op's allocation"},
                                                                  {(size_t)sl.h1_off, (size_t)sl.h1_bytes, "view h1_op of H_op's allocation"}};
  for (const auto& v : views) {
    HIPCHK(ctx, hipMemset(host + v.off - guard, GUARD_BYTE, guard));  // (the margin behind a view is the one below the next, or the allocation's own)
    ctx->guards.push_back(GuardRec{host + v.off - guard, v.bytes, guard, v.tag, true});
  }
  return 0;
}

// every buffer whose size depends on (max_batch, max_frames): sampler state, token rows, operand planes, V^T, scratch
static int alloc_workspaces(tamf_ctx* ctx, int max_batch, int max_frames) {
  const int d = ctx->d;
  const SeqShape smax = seq_shape_max(max_frames, ctx->P);  // (Skp >= vt_row_keys of every shape)
  const long BT = (long)max_batch * max_frames;
  const long Mmax = (long)max_batch * smax.Sp;
  ctx->Mmax = Mmax;
  ctx->Bmax = max_batch;
  ctx->Tmax = max_frames;
  ctx->alloc_ws = true;
  int rc = 0;
#define A(call)             \
  do {                      \
    g_alloc_tag = #call;    \
    if (rc == 0) rc = call; \
  } while (0)
  A(dev_alloc(ctx, (void**)&ctx->xs, BT * ctx->XK * 4, true));
  if (ctx->prec == TAMF_PREC_F32) ctx->xs_op.p = ctx->xs;
  else { A(alloc_operand(ctx, &ctx->xs_op, BT * ctx->XK, true)); ctx->xs_st = ctx->xs_op.p; }
  A(dev_alloc(ctx, (void**)&ctx->cobj, BT * d * 4));
  // Q | K, the attention output and the input-merge rows: views of the hidden operand's allocation where they fit (scratch_layout)
  const ScratchLayout sl = scratch_layout(Mmax, BT, d, ctx->ff, ctx->EB, g_guard_bytes.load());
  if (!sl.alias) A(alloc_operand(ctx, &ctx->h1_op, BT * d));
  A(dev_alloc(ctx, (void**)&ctx->X, Mmax * d * 4, true));
  if (ctx->prec == TAMF_PREC_F32) ctx->X_op.p = ctx->X;
  else { A(alloc_operand(ctx, &ctx->X_op, Mmax * d, true)); ctx->X_st = ctx->X_op.p; }
  if (!sl.alias) A(alloc_operand(ctx, &ctx->QK_op, Mmax * 2 * d, true));
  A(alloc_operand(ctx, &ctx->Vt_op, (long)max_batch * d * smax.Skp, true));
  if (!sl.alias) A(alloc_operand(ctx, &ctx->A_op, Mmax * d, true));
  if (!sl.alias) A(alloc_operand(ctx, &ctx->H_op, Mmax * ctx->ff, true));
  else {
    A(dev_alloc(ctx, &ctx->H_op.p, sl.host_bytes, true));
    A(place_scratch_views(ctx, sl));
  }
  A(dev_alloc(ctx, (void**)&ctx->pstatic, (long)max_batch * ctx->P * d * 4, true));
  A(dev_alloc(ctx, (void**)&ctx->tcur, (long)max_batch * 4, true));
  A(dev_alloc(ctx, (void**)&ctx->status, 16, true));
  A(dev_alloc(ctx, (void**)&ctx->side_dev, max_batch, true));
  A(dev_alloc(ctx, (void**)&ctx->objnum_dev, (long)max_batch * 4, true));
  A(dev_alloc(ctx, (void**)&ctx->stat_att, Mmax * (d / 32) * 8, true));  // block statistics of the residual stream (deferred LayerNorm)
  A(dev_alloc(ctx, (void**)&ctx->stat_ffn, Mmax * (d / 32) * 8, true));
  A(dev_alloc(ctx, (void**)&ctx->loop_params, sizeof(LoopParams), true));
#undef A
  g_alloc_tag = "(weights / tables)";
  ctx->alloc_ws = false;
  return rc;
}

// ---- SegmentEncoder contexts (TAMF_KIND_E): their own shape set, their own (small) workspaces ----
static int enc_max_frames(int ff, int kin) {  // the longest clip whose token rows fit the LDS of one CU (tamf_encoder.h)
  int t = 0;
  while (t < 5000 && enc_lds_bytes(t + 1 + ENC_P + 1, ff, kin) <= ENC_LDS_BYTES) ++t;
  return t;
}
static int enc_check_shape(const tamf_arch* a, int max_batch, int max_frames) {
  if (a->latent_dim != ENC_D || a->num_heads != 4)
    return fail(nullptr, TAMF_ERR_INVALID, "SegmentEncoder (TAMF_KIND_E): latent_dim must be 64 with num_heads 4 (head dim 16)");
  if (a->ff_size < 16 || a->ff_size > 512 || a->ff_size % 16)
    return fail(nullptr, TAMF_ERR_INVALID, "SegmentEncoder (TAMF_KIND_E): ff_size must be a multiple of 16 in [16, 512]");
  if (a->num_layers < 1 || a->num_layers > 64) return fail(nullptr, TAMF_ERR_INVALID, "SegmentEncoder (TAMF_KIND_E): num_layers must be in [1, 64]");
  if (a->input_dim < 1 || a->input_dim > 128 || a->obj_input_dim < 1 || a->obj_input_dim > 16 || a->hand_shape_dim < 1 ||
      a->hand_shape_dim > 64 || a->obj_embed_dim < 1 || a->obj_embed_dim > 4096)
    return fail(nullptr, TAMF_ERR_INVALID, "SegmentEncoder (TAMF_KIND_E): input_dim must be in [1, 128], obj_input_dim in [1, 16], "
                                           "hand_shape_dim in [1, 64], obj_embed_dim in [1, 4096]");
  if (max_batch <= 0 || max_batch > (1 << 20) || max_frames <= 0) return fail(nullptr, TAMF_ERR_INVALID, "bad max_batch/max_frames");
  const int tmax = enc_max_frames(a->ff_size, round_up(a->input_dim + a->obj_input_dim, 4));
  if (max_frames > tmax)
    return fail(nullptr, TAMF_ERR_INVALID, "SegmentEncoder (TAMF_KIND_E): max_frames " + std::to_string(max_frames) + " exceeds the limit of " +
                                               std::to_string(tmax) + " frames (a clip's token rows live in the 160 KiB LDS of one CU)");
  return 0;
}
static int enc_alloc_workspaces(tamf_ctx* ctx, int max_batch, int max_frames) {
  ctx->Bmax = max_batch;
  ctx->Tmax = max_frames;
  ctx->alloc_ws = true;
  g_alloc_tag = "encoder workspaces";
  int rc = dev_alloc(ctx, (void**)&ctx->pstatic, (size_t)max_batch * ENC_P * ctx->d * 4, true);
  if (rc == 0) rc = dev_alloc(ctx, (void**)&ctx->objnum_dev, (size_t)max_batch * 4, true);
  g_alloc_tag = "(weights / tables)";
  ctx->alloc_ws = false;
  return rc;
}
static int alloc_workspaces_of_kind(tamf_ctx* ctx, int max_batch, int max_frames) {
  return ctx->arch.kind == TAMF_KIND_E ? enc_alloc_workspaces(ctx, max_batch, max_frames) : alloc_workspaces(ctx, max_batch, max_frames);
}

// ---- what tamf_ctx_create does per kind: the checks on the architecture, and the device-side preparation before the workspaces ----
static int enc_check_create(const tamf_arch* arch, int max_batch, int max_frames, int precision) {
  if (precision != TAMF_PREC_F32) return fail(nullptr, TAMF_ERR_INVALID, "SegmentEncoder (TAMF_KIND_E) runs in fp32 only (TAMF_PREC_F32)");
  return enc_check_shape(arch, max_batch, max_frames);
}
static int gr_check_arch(const tamf_arch* arch, int precision) {  // (check_dims follows the device checks)
  const int d = arch->latent_dim;
  if (!(d == 128 || d == 256 || d == 512)) return fail(nullptr, TAMF_ERR_INVALID, "latent_dim must be 128, 256 or 512");
  if (arch->num_heads <= 0 || d % arch->num_heads) return fail(nullptr, TAMF_ERR_INVALID, "bad num_heads");
  const int hd = d / arch->num_heads;
  if (!(hd == 64 || hd == 128)) return fail(nullptr, TAMF_ERR_INVALID, "head dim (latent_dim/num_heads) must be 64 or 128");
  if (arch->ff_size <= 0 || arch->ff_size % 128) return fail(nullptr, TAMF_ERR_INVALID, "ff_size must be a multiple of 128");
  if (arch->num_layers <= 0 || arch->num_layers > 64) return fail(nullptr, TAMF_ERR_INVALID, "bad num_layers");
  if (arch->input_dim <= 0 || arch->input_dim > 128) return fail(nullptr, TAMF_ERR_INVALID, "input_dim must be in [1,128]");
  if (precision < 0 || precision > TAMF_PREC_F16X3) return fail(nullptr, TAMF_ERR_INVALID, "unknown precision");
  if (arch->kind != TAMF_KIND_G && arch->kind != TAMF_KIND_R) return fail(nullptr, TAMF_ERR_INVALID, "unknown model kind");
  return 0;
}
static int enc_prepare(tamf_ctx* ctx) {
  hipError_t e = lds_once<encoder_kernel>((int)ENC_LDS_BYTES);
  if (e != hipSuccess) return fail(ctx, TAMF_ERR_HIP, std::string("encoder kernel attribute setup failed: ") + hipGetErrorString(e));
  return 0;
}
static int gr_prepare(tamf_ctx* ctx) {  // workgroup slots of the device, kernel attributes, the capture stream
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device) == hipSuccess && cus > 0)
      g_wg_slots_dev[ctx->device & 63].store(2 * cus, std::memory_order_relaxed);
  }
  hipError_t pe;
  {
    TAMF_STATE_LOCK;  // (one context at a time sets the kernel attributes of a device: they are idempotent, this only avoids the duplicate work)
    pe = prepare_all<OpF32>();
    if (pe == hipSuccess && ctx->prec != TAMF_PREC_F32) TAMF_WITH_OP(ctx->prec, pe = prepare_all<Op>());
  }
  if (pe != hipSuccess) return fail(ctx, TAMF_ERR_HIP, std::string("kernel attribute setup failed: ") + hipGetErrorString(pe));
  if (hipStreamCreateWithFlags(&ctx->cap_stream, hipStreamNonBlocking) != hipSuccess) return fail(ctx, TAMF_ERR_HIP, "hipStreamCreate failed");
  return 0;
}

extern "C" int tamf_ctx_create(const tamf_arch* arch, int32_t max_batch, int32_t max_frames, int32_t precision,
                               int32_t device, tamf_ctx** out) {
  if (!arch || !out) return fail(nullptr, TAMF_ERR_INVALID, "null argument");
  *out = nullptr;
  const bool enc = arch->kind == TAMF_KIND_E;
  if (int rc = enc ? enc_check_create(arch, max_batch, max_frames, precision) : gr_check_arch(arch, precision)) return rc;
  int ndev = 0;
  hipError_t de = hipGetDeviceCount(&ndev);
  if (de != hipSuccess || ndev <= 0)
    return fail(nullptr, TAMF_ERR_HIP, std::string("no HIP device visible (") + hipGetErrorString(de) +
                                           "): libtamf_hip has no CPU fallback");
  if (device < 0 || device >= ndev) return fail(nullptr, TAMF_ERR_INVALID, "device index out of range");
  if (!enc)
    if (int rc = check_dims(arch, max_batch, max_frames)) return rc;

  tamf_ctx* ctx = new tamf_ctx();
  ctx->arch = *arch;
  ctx->prec = precision;
  ctx->device = device;
  ctx->d = arch->latent_dim;
  ctx->ff = arch->ff_size;
  ctx->L = arch->num_layers;
  ctx->H = arch->num_heads;
  ctx->hd = arch->latent_dim / arch->num_heads;
  ctx->F = arch->input_dim;
  ctx->has_t = arch->kind == TAMF_KIND_G ? 1 : 0;
  ctx->EB = precision == TAMF_PREC_BF16 ? 2 : 4;
  if (enc) {
    ctx->P = ENC_P;
    ctx->enc_kin = round_up(arch->input_dim + arch->obj_input_dim, 4);
  } else {
    ctx->P = arch->kind == TAMF_KIND_G ? PREFIX_ROWS_G : PREFIX_ROWS_R;
    ctx->XK = arch->kind == TAMF_KIND_G ? 128 : round_up(arch->input_dim + arch->h2o_dim, 64);
    ctx->layers.resize(ctx->L);
  }
  ctx->expected = expected_shapes(ctx->arch);

  auto bail = [&](int rc) {
    std::string e = ctx->err;
    tamf_ctx_destroy(ctx);
    g_noctx_err = e;
    return rc;
  };
  if (hipSetDevice(device) != hipSuccess) return bail(fail(ctx, TAMF_ERR_HIP, "hipSetDevice failed"));
  if (int rc = enc ? enc_prepare(ctx) : gr_prepare(ctx)) return bail(rc);
  if (int rc = alloc_workspaces_of_kind(ctx, max_batch, max_frames)) return bail(rc);
  if (!enc && hipEventCreateWithFlags(&ctx->graph_done, hipEventDisableTiming) != hipSuccess)
    return bail(fail(ctx, TAMF_ERR_HIP, "hipEventCreate failed"));
  {
    std::lock_guard<std::mutex> lk(g_live_mu);
    g_live_ctx.push_back(ctx);
  }
  *out = ctx;
  return 0;
}

extern "C" void tamf_ctx_destroy(tamf_ctx* ctx) {
  if (!ctx) return;
  TAMF_LAUNCH_LOCK;
  {
    std::lock_guard<std::mutex> lk(g_live_mu);
    g_live_ctx.erase(std::remove(g_live_ctx.begin(), g_live_ctx.end(), ctx), g_live_ctx.end());
  }
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  if (ctx->graph_done) (void)hipEventDestroy(ctx->graph_done);
  if (ctx->graph_exec) (void)hipGraphExecDestroy(ctx->graph_exec);
  if (ctx->graph) (void)hipGraphDestroy(ctx->graph);
  if (ctx->cap_stream) (void)hipStreamDestroy(ctx->cap_stream);
  for (void* p : ctx->allocs) (void)hipFree(p);
  for (void* p : ctx->ws_allocs) (void)hipFree(p);
  delete ctx;
}

static int retire_graph(tamf_ctx* ctx);

// a context's workspace set, moved out of it (ws_take): the sub-object and the guard records of its allocations
struct TakenWorkspaces {
  Workspaces ws;
  std::vector<GuardRec> guards;
};
static TakenWorkspaces ws_take(tamf_ctx* c) {  // (the context is left with no workspaces: null pointers, empty lists)
  TakenWorkspaces t;
  std::swap(t.ws, static_cast<Workspaces&>(*c));
  const auto first_ws = std::stable_partition(c->guards.begin(), c->guards.end(), [](const GuardRec& g) { return !g.ws; });
  t.guards.assign(first_ws, c->guards.end());
  c->guards.erase(first_ws, c->guards.end());
  return t;
}
static void ws_put(tamf_ctx* c, TakenWorkspaces& t) {  // (into a context without workspaces; their guard records go to the end of the list)
  std::swap(t.ws, static_cast<Workspaces&>(*c));
  c->guards.insert(c->guards.end(), t.guards.begin(), t.guards.end());
}
static void ws_free(const TakenWorkspaces& t) {
  for (void* p : t.ws.ws_allocs) (void)hipFree(p);
}

// Transactional: the new workspaces are allocated FIRST, beside the old ones; only when every allocation has succeeded
// are the old ones freed.  On failure (the likely one: a larger batch that does not fit) the partial new set is freed, the old set -
// pointers, dimensions, conditioning - is put back and the context keeps working at its old size; the captured graph is gone either
// way (it holds the old pointers' kernels: harmless, but it is re-captured on the next loop).  The sticky status word travels with
// the context: bits raised and not yet read survive the resize.  A SegmentEncoder context has no graph, conditioning or status word:
// only its prefix rows and object counts are dimensioned.
extern "C" int tamf_ctx_resize(tamf_ctx* ctx, int32_t max_batch, int32_t max_frames) {
  TAMF_LAUNCH_LOCK;
  if (!ctx) return fail(ctx, TAMF_ERR_INVALID, "null ctx");
  const bool enc = ctx->arch.kind == TAMF_KIND_E;
  if (int rc = enc ? enc_check_shape(&ctx->arch, max_batch, max_frames) : check_dims(&ctx->arch, max_batch, max_frames)) {
    ctx->err = g_noctx_err;
    return rc;
  }
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipDeviceSynchronize());
  if (!enc) TRY(retire_graph(ctx));
  TakenWorkspaces old = ws_take(ctx);
  int rc = alloc_workspaces_of_kind(ctx, max_batch, max_frames);
  if (rc == 0 && old.ws.status && ctx->status &&
      hipMemcpy(ctx->status, old.ws.status, 16, hipMemcpyDeviceToDevice) != hipSuccess)
    rc = fail(ctx, TAMF_ERR_HIP, "tamf_ctx_resize: carrying the status word over failed");
  if (rc != 0) {
    const std::string why = ctx->err;
    ws_free(ws_take(ctx));  // whatever the allocator got before it failed
    ws_put(ctx, old);
    ctx->err = "tamf_ctx_resize(" + std::to_string(max_batch) + ", " + std::to_string(max_frames) + ") failed, the context keeps its " +
               std::to_string(ctx->Bmax) + " x " + std::to_string(ctx->Tmax) + " workspaces: " + why;
    return rc;
  }
  ws_free(old);
  if (!enc) {
    ctx->cond_set = false;
    ctx->B = ctx->T = ctx->S = ctx->Sp = ctx->Skp = ctx->M = 0;
  }
  return 0;
}

// ------------------------------------------------------------------------------------------------
// weights
// ------------------------------------------------------------------------------------------------
extern "C" int tamf_load_weight(tamf_ctx* ctx, const char* name, const float* host_data, const int64_t* shape,
                                int32_t ndim) {
  if (!ctx || !name || !host_data || !shape || ndim <= 0) return fail(ctx, TAMF_ERR_INVALID, "null/invalid argument");
  if (ctx->finalized) return fail(ctx, TAMF_ERR_STATE, "weights already finalised");
  const auto it = ctx->expected.find(name);
  if (it == ctx->expected.end()) return 0;  // strict=False: unexpected keys are ignored (e.g. clip_model.*, aliased pe buffer)
  std::vector<int64_t> shp(shape, shape + ndim);
  if (shp != it->second) return fail(ctx, TAMF_ERR_INVALID, std::string("shape mismatch for ") + name);
  int64_t n = 1;
  for (auto v : shp) n *= v;
  ctx->raw[name].assign(host_data, host_data + n);
  return 0;
}

static int upload_f32(tamf_ctx* ctx, const std::string& name, float** p) {
  const auto& v = ctx->raw.at(name);
  return dev_upload(ctx, p, v.data(), v.size());
}
static int upload_T(tamf_ctx* ctx, const std::string& name, int N, int K, float** p) {  // W [N][K] -> W^T [K][N] (prefix_rows_kernel)
  return upload_vec(ctx, p, transposed(ctx->raw.at(name).data(), N, K));
}
// the tables of the prefix rows that every kind has (prefix_rows_kernel): hand shape, object embedding, hand side
static int upload_prefix_tables(tamf_ctx* ctx) {
  const int d = ctx->d;
  TRY(upload_T(ctx, "hand_shape_process.shape_embed.weight", d, ctx->arch.hand_shape_dim, &ctx->WshapeT));
  TRY(upload_f32(ctx, "hand_shape_process.shape_embed.bias", &ctx->bshape));
  TRY(upload_T(ctx, "obj_embed_process.embedding.weight", d, ctx->arch.obj_embed_dim, &ctx->WobjT));
  TRY(upload_f32(ctx, "obj_embed_process.embedding.bias", &ctx->bobj));
  TRY(upload_f32(ctx, "hand_side_process.rh_embed", &ctx->rh));
  return upload_f32(ctx, "hand_side_process.lh_embed", &ctx->lh);
}
// SegmentEncoder weights -> the packed layout of tamf_encoder.h (EncHeadOff, then one EncLayerOff block per layer) + the prefix-row
// tables of prefix_rows_kernel.  The input linear maps are composed in float64 as for G / R: W_in = [W_m1[:, :d] W_p | W_m1[:, d:] W_q].
static int enc_finalize(tamf_ctx* ctx) {
  const int d = ctx->d, ff = ctx->ff, F = ctx->F, qd = ctx->arch.obj_input_dim, kin = ctx->enc_kin, hd = ctx->hd, H = ctx->H;
  auto R = [&](const std::string& n) -> const float* { return ctx->raw.at(n).data(); };
  const EncHeadOff ho = enc_head_off(kin, F);
  const EncLayerOff lo = enc_layer_off(ff);
  std::vector<float> w((size_t)(ho.layers + (long)ctx->L * lo.stride), 0.f);
  auto put = [&](long off, const std::string& n, size_t cnt) { memcpy(w.data() + off, R(n), cnt * 4); };
  put(ho.cls, "classification_token", d);
  {
    const float *Wm1 = R("input_merge.0.weight"), *bm1 = R("input_merge.0.bias");
    const float *Wp = R("input_process.poseEmbedding.weight"), *bp = R("input_process.poseEmbedding.bias");
    const float *Wq = R("obj_input_process.poseEmbedding.weight"), *bq = R("obj_input_process.poseEmbedding.bias");
    input_bias_two_terms_per_column(Wm1, d, bm1, bp, bq, w.data() + ho.bin);
    compose_block(Wm1, 2 * d, 0, d, Wp, F, w.data() + ho.win, kin, 1);
    compose_block(Wm1, 2 * d, d, d, Wq, qd, w.data() + ho.win + F, kin, 1);
  }
  put(ho.wm2, "input_merge.2.weight", (size_t)d * d);
  put(ho.bm2, "input_merge.2.bias", d);
  put(ho.p0, "output_process.poseFinal.0.weight", (size_t)d * d);
  put(ho.pb0, "output_process.poseFinal.0.bias", d);
  put(ho.p2, "output_process.poseFinal.2.weight", (size_t)d * d);
  put(ho.pb2, "output_process.poseFinal.2.bias", d);
  put(ho.p4, "output_process.poseFinal.4.weight", (size_t)F * d);
  put(ho.pb4, "output_process.poseFinal.4.bias", F);
  for (int l = 0; l < ctx->L; ++l) {
    const std::string p = "seqTransEncoder.layers." + std::to_string(l);
    const long base = ho.layers + (long)l * lo.stride;
    const float *Win = R(p + ".self_attn.in_proj_weight"), *bin = R(p + ".self_attn.in_proj_bias");
    for (int h = 0; h < H; ++h)  // rows grouped per head: [q_h | k_h | v_h]
      for (int part = 0; part < 3; ++part)
        for (int j = 0; j < hd; ++j) {
          const int dst = h * 3 * hd + part * hd + j, src = part * d + h * hd + j;
          memcpy(w.data() + base + lo.wqkv + (long)dst * d, Win + (size_t)src * d, (size_t)d * 4);
          w[base + lo.bqkv + dst] = bin[src];
        }
    put(base + lo.wo, p + ".self_attn.out_proj.weight", (size_t)d * d);
    put(base + lo.bo, p + ".self_attn.out_proj.bias", d);
    put(base + lo.w1, p + ".linear1.weight", (size_t)ff * d);
    put(base + lo.b1, p + ".linear1.bias", ff);
    put(base + lo.w2, p + ".linear2.weight", (size_t)d * ff);
    put(base + lo.b2, p + ".linear2.bias", d);
    put(base + lo.g1, p + ".norm1.weight", d);
    put(base + lo.be1, p + ".norm1.bias", d);
    put(base + lo.g2, p + ".norm2.weight", d);
    put(base + lo.be2, p + ".norm2.bias", d);
  }
  TRY(dev_upload(ctx, &ctx->enc_w, w.data(), w.size()));
  TRY(upload_f32(ctx, "sequence_pos_encoder.pe", &ctx->pe));
  return upload_prefix_tables(ctx);
}

extern "C" int tamf_finalize_weights(tamf_ctx* ctx, int32_t max_timesteps, void* stream) {
  TAMF_LAUNCH_LOCK;
  if (!ctx) return fail(ctx, TAMF_ERR_INVALID, "null ctx");
  if (ctx->finalized) return fail(ctx, TAMF_ERR_STATE, "weights already finalised");
  if (max_timesteps <= 0 || max_timesteps > 5000) return fail(ctx, TAMF_ERR_INVALID, "max_timesteps must be in [1,5000]");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  for (const auto& kv : ctx->expected)
    if (!ctx->raw.count(kv.first)) return fail(ctx, TAMF_ERR_MISSING, "missing checkpoint tensor: " + kv.first);
  auto done = [&]() {
    ctx->raw.clear();
    ctx->expected.clear();
    ctx->finalized = true;
    if (!ctx->weight_note.empty()) ctx->err = ctx->weight_note;  // (readable through tamf_last_error after the successful call)
    return 0;
  };
  if (ctx->arch.kind == TAMF_KIND_E) {
    TRY(enc_finalize(ctx));
    return done();
  }
  const int d = ctx->d, ff = ctx->ff, F = ctx->F, prec = ctx->prec;
  auto R = [&](const std::string& n) -> const float* { return ctx->raw.at(n).data(); };
  // a linear map [N][d] behind a deferred LayerNorm (gamma g, beta be; null: none): the folded weight as an operand of Npad rows, c2 in
  // place of its bias (fold_layernorm, tamf_weight_prep.h)
  auto upload_folded = [&](const std::string& weight, const std::string& bias, int N, int Npad, const float* g, const float* be, OperandBuf* ob,
                           float** c2) -> int {
    const FoldedLinear f = fold_layernorm(R(weight), R(bias), N, Npad, d, g, be);
    TRY(upload_operand(ctx, prec, f.w.data(), Npad, d, d, ob, weight.c_str()));
    return upload_vec(ctx, c2, f.c2);
  };
  // what the residual add behind a block takes: gamma, beta + the bias of the block's last linear map (residual_ln)
  auto upload_residual_ln = [&](const float* g, const float* be, const std::string& bias, float** g_dev, float** bb_dev) -> int {
    const ResidualLn r = residual_ln(g, be, R(bias), d);
    TRY(upload_vec(ctx, g_dev, r.g));
    return upload_vec(ctx, bb_dev, r.bb);
  };

  for (int l = 0; l < ctx->L; ++l) {
    const std::string p = "seqTransEncoder.layers." + std::to_string(l);
    LayerW& w = ctx->layers[l];
    {
      const std::string pp = "seqTransEncoder.layers." + std::to_string(l - 1);
      const float* g_in = l ? R(pp + ".norm2.weight") : nullptr;   // LayerNorm in front of this layer's attention block
      const float* be_in = l ? R(pp + ".norm2.bias") : nullptr;
      const float* g1 = R(p + ".norm1.weight");                    // ... in front of its feed-forward block
      const float* be1 = R(p + ".norm1.bias");
      TRY(upload_folded(p + ".self_attn.in_proj_weight", p + ".self_attn.in_proj_bias", 3 * d, 3 * d, g_in, be_in, &w.Win, &w.c2_in));
      TRY(upload_folded(p + ".linear1.weight", p + ".linear1.bias", ff, ff, g1, be1, &w.W1, &w.c2_ff));
      TRY(upload_residual_ln(g_in, be_in, p + ".self_attn.out_proj.bias", &w.g_att, &w.bb_att));
      TRY(upload_residual_ln(g1, be1, p + ".linear2.bias", &w.g_ffn, &w.bb_ffn));
    }
    TRY(upload_operand(ctx, prec, R(p + ".self_attn.out_proj.weight"), d, d, d, &w.Wout, (p + ".self_attn.out_proj.weight").c_str()));
    TRY(upload_operand(ctx, prec, R(p + ".linear2.weight"), d, ff, ff, &w.W2, (p + ".linear2.weight").c_str()));
  }
  {  // fused input weight: input_merge.0[:, :d] . poseEmbedding (and, for R, input_merge.0[:, 2d:] . h2o embedding), its object half, its bias
    const bool isR = ctx->arch.kind == TAMF_KIND_R;
    const FusedInput fi = fuse_input(d, F, ctx->arch.obj_input_dim, ctx->arch.h2o_dim, ctx->XK, R("input_merge.0.weight"), R("input_merge.0.bias"),
                                     R("input_process.poseEmbedding.weight"), R("input_process.poseEmbedding.bias"),
                                     R("obj_input_process.poseEmbedding.weight"), R("obj_input_process.poseEmbedding.bias"),
                                     isR ? R("h2o_dist_input_process.poseEmbedding.weight") : nullptr,
                                     isR ? R("h2o_dist_input_process.poseEmbedding.bias") : nullptr);
    TRY(upload_operand(ctx, prec, fi.w.data(), d, ctx->XK, ctx->XK, &ctx->Wfused, "input_merge.0.weight x poseEmbedding.weight (fused)"));
    TRY(upload_vec(ctx, &ctx->WcT, fi.wct));
    TRY(upload_vec(ctx, &ctx->bc, fi.bias));
  }
  TRY(upload_operand(ctx, prec, R("input_merge.2.weight"), d, d, d, &ctx->Wm2, "input_merge.2.weight"));
  TRY(upload_f32(ctx, "input_merge.2.bias", &ctx->bm2));
  {  // the encoder's last LayerNorm, deferred into the head: W_f diag(gamma) (I - 1 1^T / d), c2 = W_f beta + b_f; XN rows, zero beyond F
    const std::string pl = "seqTransEncoder.layers." + std::to_string(ctx->L - 1);
    TRY(upload_folded("output_process.poseFinal.weight", "output_process.poseFinal.bias", F, ctx->XN, R(pl + ".norm2.weight"), R(pl + ".norm2.bias"),
                      &ctx->Wf, &ctx->bf));
  }
  TRY(upload_f32(ctx, "sequence_pos_encoder.pe", &ctx->pe));
  if (ctx->arch.hand_shape_dim > 64 || ctx->arch.obj_input_dim > COBJ_QMAX || d > 1024)
    return fail(ctx, TAMF_ERR_INVALID, "hand_shape_dim > 64, obj_input_dim > 16 or latent_dim > 1024");
  TRY(upload_prefix_tables(ctx));
  if (ctx->has_t) {
    TRY(upload_T(ctx, "embed_text.weight", d, ctx->arch.clip_dim, &ctx->WtxtT));
    TRY(upload_f32(ctx, "embed_text.bias", &ctx->btxt));
    TRY(upload_operand(ctx, TAMF_PREC_F32, R("embed_timestep.time_embed.0.weight"), d, d, d, &ctx->Wt1_f32, "embed_timestep.time_embed.0.weight"));
    TRY(upload_operand(ctx, TAMF_PREC_F32, R("embed_timestep.time_embed.2.weight"), d, d, d, &ctx->Wt2_f32, "embed_timestep.time_embed.2.weight"));
    TRY(upload_f32(ctx, "embed_timestep.time_embed.0.bias", &ctx->bt1));
    TRY(upload_f32(ctx, "embed_timestep.time_embed.2.bias", &ctx->bt2));
    // timestep-embedding table: temb[t] = nan_to_num(W2 silu(W1 pe[t] + b1) + b2) + pe[0]   (exact fp32 MFMA)
    ctx->n_t = max_timesteps;
    float* tmp = nullptr;
    TRY(dev_alloc(ctx, (void**)&ctx->temb, (size_t)ctx->n_t * d * 4));
    TRY(dev_alloc(ctx, (void**)&tmp, (size_t)ctx->n_t * d * 4));
    GemmArgs<OpF32> g1{ctx->pe, d, (const float*)ctx->Wt1_f32.p, d, ctx->n_t, d, d, 0};
    EpiBiasAct<OpF32> e1{ctx->bt1, nullptr, 0, tmp, d, ACT_SILU};
    HIPCHK(ctx, gemm128<OpF32>(g1, e1, st));
    GemmArgs<OpF32> g2{tmp, d, (const float*)ctx->Wt2_f32.p, d, ctx->n_t, d, d, 0};
    EpiSeqRows<OpF32> e2{ctx->bt2, ctx->pe, 0, ctx->temb, nullptr, d, 0x7FFFFFFF, 0, 0, nullptr, nullptr, nullptr, 0, 0, 0};
    HIPCHK(ctx, gemm128<OpF32>(g2, e2, st));
  }
  HIPCHK(ctx, hipStreamSynchronize(st));
  return done();
}

// destroy the executable graph once its last replay has finished (its launches may still be queued on the caller's stream)
static int retire_graph(tamf_ctx* ctx) {
  if (ctx->graph_in_flight) {
    HIPCHK(ctx, hipEventSynchronize(ctx->graph_done));
    ctx->graph_in_flight = false;
  }
  if (ctx->graph_exec) { (void)hipGraphExecDestroy(ctx->graph_exec); ctx->graph_exec = nullptr; }
  if (ctx->graph) { (void)hipGraphDestroy(ctx->graph); ctx->graph = nullptr; }
  ctx->graph_key = GraphKey();
  return 0;
}

extern "C" int tamf_set_schedule(tamf_ctx* ctx, int32_t n_steps, const double* c1, const double* c2, const double* logvar) {
  TAMF_LAUNCH_LOCK;
  TRY(need_kind(ctx, __func__, KIND_G | KIND_R));
  if (!c1 || !c2 || !logvar || n_steps <= 0) return fail(ctx, TAMF_ERR_INVALID, "null/invalid argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  ctx->h_c1.resize(n_steps);
  ctx->h_c2.resize(n_steps);
  ctx->h_sigma.resize(n_steps);
  for (int i = 0; i < n_steps; ++i) {
    ctx->h_c1[i] = (float)c1[i];  // float64 -> float32 cast of _extract_into_tensor (gaussian_diffusion.py:1275)
    ctx->h_c2[i] = (float)c2[i];
    ctx->h_sigma[i] = expf(0.5f * (float)logvar[i]);  // th.exp(0.5 * log_variance) on float32 (:459)
  }
  ctx->n_steps = n_steps;
  if (ctx->tmap_on) {  // a new schedule is a new sampler: its timestep map (if any) is set after it
    TRY(retire_graph(ctx));
    ctx->tmap_on = false;
    ctx->tmap_max = -1;
  }
  if (n_steps > ctx->sched_cap) {  // (re)allocated only when a longer schedule arrives; a captured graph holds these pointers
    TRY(retire_graph(ctx));
    const int cap = std::max(n_steps, 1000);
    TRY(dev_alloc(ctx, (void**)&ctx->c1, (size_t)cap * 4));
    TRY(dev_alloc(ctx, (void**)&ctx->c2, (size_t)cap * 4));
    TRY(dev_alloc(ctx, (void**)&ctx->sigma, (size_t)cap * 4));
    ctx->sched_cap = cap;
  }
  // plain (synchronous) copies: ordered after earlier work on the null stream semantics of hipMemcpy
  HIPCHK(ctx, hipDeviceSynchronize());
  HIPCHK(ctx, hipMemcpy(ctx->c1, ctx->h_c1.data(), (size_t)n_steps * 4, hipMemcpyHostToDevice));
  HIPCHK(ctx, hipMemcpy(ctx->c2, ctx->h_c2.data(), (size_t)n_steps * 4, hipMemcpyHostToDevice));
  HIPCHK(ctx, hipMemcpy(ctx->sigma, ctx->h_sigma.data(), (size_t)n_steps * 4, hipMemcpyHostToDevice));
  return 0;
}

extern "C" int tamf_set_timestep_map(tamf_ctx* ctx, int32_t n_steps, const int32_t* map_host) {
  TAMF_LAUNCH_LOCK;
  TRY(need_kind(ctx, __func__, KIND_G));
  if (!ctx->finalized) return fail(ctx, TAMF_ERR_STATE, "tamf_set_timestep_map needs a G context with finalised weights");
  if (ctx->n_steps <= 0 || n_steps != ctx->n_steps) return fail(ctx, TAMF_ERR_STATE, "tamf_set_timestep_map: set the schedule of the same length first");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  TRY(retire_graph(ctx));  // (a captured loop holds the table pointer of its capture time)
  if (!map_host) {
    ctx->tmap_on = false;
    ctx->tmap_max = -1;
    return 0;
  }
  int mx = -1;
  for (int i = 0; i < n_steps; ++i) {
    if (map_host[i] < 0 || map_host[i] >= ctx->n_t)
      return fail(ctx, TAMF_ERR_INVALID, "timestep map entry " + std::to_string(map_host[i]) + " outside the timestep table (max_timesteps = " + std::to_string(ctx->n_t) + ")");
    if (i && map_host[i] <= map_host[i - 1]) return fail(ctx, TAMF_ERR_INVALID, "timestep map must be strictly increasing (respace.py:76-82)");
    mx = std::max(mx, (int)map_host[i]);
  }
  if (n_steps > ctx->temb_loop_cap) {
    const int cap = std::max(n_steps, 1000);
    TRY(dev_alloc(ctx, (void**)&ctx->temb_loop, (size_t)cap * ctx->d * 4));
    ctx->temb_loop_cap = cap;
  }
  int* map_dev = nullptr;
  HIPCHK(ctx, hipDeviceSynchronize());
  HIPCHK(ctx, hipMalloc((void**)&map_dev, (size_t)n_steps * 4));
  hipError_t e = hipMemcpy(map_dev, map_host, (size_t)n_steps * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(gather_rows_kernel, grid1d((long)n_steps * ctx->d), dim3(256), 0, nullptr, ctx->temb_loop, ctx->temb, map_dev, n_steps, ctx->d);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipDeviceSynchronize();
  (void)hipFree(map_dev);
  HIPCHK(ctx, e);
  ctx->tmap_on = true;
  ctx->tmap_max = mx;
  return 0;
}

// ------------------------------------------------------------------------------------------------
// conditioning (step-invariant precompute, always exact fp32)
// ------------------------------------------------------------------------------------------------
// per-clip object counts (tamf_set_cond_ragged, tamf_encode; null: every clip has nobj objects): checked on the host, then copied to
// the context's objnum_dev, which *cnt names for the kernels
static int check_obj_num(tamf_ctx* ctx, const int32_t* obj_num_host, int B, int nobj) {
  if (obj_num_host)
    for (int b = 0; b < B; ++b)
      if (obj_num_host[b] < 1 || obj_num_host[b] > nobj)
        return fail(ctx, TAMF_ERR_INVALID, "obj_num[" + std::to_string(b) + "] = " + std::to_string(obj_num_host[b]) + " outside [1, nobj]");
  return 0;
}
static int upload_obj_num(tamf_ctx* ctx, const int32_t* obj_num_host, int B, hipStream_t st, const int** cnt) {
  *cnt = nullptr;
  if (!obj_num_host) return 0;
  HIPCHK(ctx, hipMemcpyAsync(ctx->objnum_dev, obj_num_host, sizeof(int32_t) * B, hipMemcpyHostToDevice, st));
  *cnt = ctx->objnum_dev;
  return 0;
}

extern "C" int tamf_set_cond(tamf_ctx* ctx, int32_t B, int32_t T, int32_t nobj, const float* text_emb_dev,
                             const uint8_t* hand_side_host, const float* shape_dev, const float* obj_emb_dev,
                             const float* obj_traj_dev, void* stream) {
  return tamf_set_cond_ragged(ctx, B, T, nobj, nullptr, text_emb_dev, hand_side_host, shape_dev, obj_emb_dev, obj_traj_dev, stream);
}

extern "C" int tamf_set_cond_ragged(tamf_ctx* ctx, int32_t B, int32_t T, int32_t nobj, const int32_t* obj_num_host,
                                    const float* text_emb_dev, const uint8_t* hand_side_host, const float* shape_dev,
                                    const float* obj_emb_dev, const float* obj_traj_dev, void* stream) {
  TAMF_LAUNCH_LOCK;
  TRY(need_kind(ctx, __func__, KIND_G | KIND_R));
  if (!ctx->finalized) return fail(ctx, TAMF_ERR_STATE, "weights not finalised");
  if (B <= 0 || B > ctx->Bmax || T <= 0 || T > ctx->Tmax || nobj <= 0) return fail(ctx, TAMF_ERR_INVALID, "B/T/nobj out of range");
  if (!hand_side_host || !shape_dev || !obj_emb_dev || !obj_traj_dev || (ctx->has_t && !text_emb_dev))
    return fail(ctx, TAMF_ERR_INVALID, "null conditioning tensor");
  for (int b = 0; b < B; ++b)
    if (hand_side_host[b] > 1) return fail(ctx, TAMF_ERR_INVALID, "unexpected hand_side: " + std::to_string(hand_side_host[b]));
  TRY(check_obj_num(ctx, obj_num_host, B, nobj));
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const int* cnt = nullptr;
  TRY(upload_obj_num(ctx, obj_num_host, B, st, &cnt));
  const int d = ctx->d, P = ctx->P, ht = ctx->has_t, nrows = P - ht;
  ctx->B = B;
  ctx->T = T;
  const SeqShape sq = seq_shape(T, P);
  ctx->S = sq.S;
  ctx->Sp = sq.Sp;
  ctx->Skp = sq.Skp;
  ctx->M = B * sq.Sp;
  ctx->cond_set = false;
  HIPCHK(ctx, hipMemcpyAsync(ctx->side_dev, hand_side_host, B, hipMemcpyHostToDevice, st));
  // two launches (tamf_misc.h): the static prefix rows of every clip, and the hoisted object half of input_merge.0 per frame
  const int sd = ctx->arch.hand_shape_dim, od = ctx->arch.obj_embed_dim, qd = ctx->arch.obj_input_dim, cd = ht ? ctx->arch.clip_dim : 0;
  PrefixArgs pa{};
  pa.text = ht ? text_emb_dev : nullptr; pa.WtxtT = ctx->WtxtT; pa.btxt = ctx->btxt;
  pa.side = ctx->side_dev; pa.rh = ctx->rh; pa.lh = ctx->lh;
  pa.shape = shape_dev; pa.WshapeT = ctx->WshapeT; pa.bshape = ctx->bshape;
  pa.oemb = obj_emb_dev; pa.WobjT = ctx->WobjT; pa.bobj = ctx->bobj; pa.cnt = cnt;
  pa.pe = ctx->pe; pa.pstatic = ctx->pstatic;
  pa.B = B; pa.d = d; pa.T = T; pa.sd = sd; pa.nobj = nobj; pa.od = od; pa.clip_dim = cd; pa.nrows = nrows; pa.ht = ht;
  const size_t psm = (size_t)(std::max(std::max(cd, od), sd) + 1024) * sizeof(float);
  hipLaunchKernelGGL(prefix_rows_kernel, dim3(B, nrows), dim3(1024), psm, st, pa);
  hipLaunchKernelGGL(cobj_kernel, dim3((unsigned)(((long)B * T + COBJ_ROWS - 1) / COBJ_ROWS)), dim3(256), 0, st, obj_traj_dev, ctx->WcT, ctx->bc,
                     ctx->cobj, B, nobj, T, qd, d, cnt);
  HIPCHK(ctx, hipGetLastError());
  ctx->cond_set = true;
  return 0;
}

// ------------------------------------------------------------------------------------------------
// one denoiser evaluation = the kernel sequence below (captured into a hipGraph by the sampling loop)
// ------------------------------------------------------------------------------------------------
template <class Op>
static int enqueue_step(tamf_ctx* ctx, hipStream_t st, const EpiHead<Op>& head_in, int t_off = 0) {
  typedef typename Op::elem_t E;
  const int d = ctx->d, ff = ctx->ff, B = ctx->B, T = ctx->T, S = ctx->S, Sp = ctx->Sp, M = ctx->M, P = ctx->P;
  int nk = 0;
  // algorithmic FLOPs of the reference work each launch stands for (true S, not padded rows)
  const double BS = (double)B * S, BT = (double)B * T, dd = d, F = ctx->F;
  auto mark = [&](const char* name, double flops) {
    ++nk;
    if (!ctx->prof_on) return;
    hipEvent_t ev;
    if (hipEventCreate(&ev) != hipSuccess) return;
    (void)hipEventRecord(ev, st);
    ctx->prof_ev.push_back(ev);
    ctx->prof_names.push_back(name);
    ctx->prof_flops.push_back(flops);
  };
  {  // input_merge.0 on [pose | (h2o)] with the hoisted object term, SiLU
    GemmArgs<Op> ga{(const E*)ctx->xs_op.p, ctx->XK, (const E*)ctx->Wfused.p, ctx->XK, B * T, d, ctx->XK, 0};
    EpiBiasAct<Op> ep{nullptr, ctx->cobj, d, (E*)ctx->h1_op.p, d, ACT_SILU, {ctx->Wfused.inv_scale, ctx->status}};
    HIPCHK(ctx, gemm128<Op>(ga, ep, st));
    mark("gemm_input_merge0", BT * (2.0 * F * dd + 2.0 * dd * (ctx->arch.kind == TAMF_KIND_R ? 3 : 2) * dd +
                                    (ctx->arch.kind == TAMF_KIND_R ? 2.0 * ctx->arch.h2o_dim * dd : 0.0)));
  }
  {  // input_merge.2 + nan_to_num + positional rows -> token rows of X
    GemmArgs<Op> ga{(const E*)ctx->h1_op.p, d, (const E*)ctx->Wm2.p, d, B * T, d, d, 0};
    // (+ the prefix and pad rows of every clip, written by the tile that holds the clip's first frame)
    const float* temb_now = (ctx->in_loop && ctx->tmap_on) ? ctx->temb_loop : ctx->temb;
    EpiSeqRows<Op> ep{ctx->bm2, ctx->pe + (long)P * d, d, ctx->X, (E*)ctx->X_st, d, T, Sp, P, ctx->pstatic, temb_now, ctx->tcur, ctx->has_t, S, t_off, {ctx->Wm2.inv_scale, ctx->status}};
    HIPCHK(ctx, launch_rows<Op>(ga, ep, st));
    mark("gemm_input_merge2", BT * 2.0 * dd * dd + (ctx->has_t ? B * 4.0 * dd * dd : 0.0));
  }
  const float qscale = 1.4426950408889634f / sqrtf((float)ctx->hd);
  // Deferred LayerNorm (tamf_device.h): the residual stream X / X_op holds the UN-normalised sums; five launches per layer (f32: six,
  // the QKV projection as two clip launches)
  const int NB = d / 32;
  const float inv_d = 1.0f / (float)d;
  for (int l = 0; l < ctx->L; ++l) {
    LayerW& w = ctx->layers[l];
    const LnStats ln_in{l ? ctx->stat_ffn : nullptr, NB, inv_d, 1e-5f};  // the LayerNorm in front of the attention block (layer 0: none)
    const LnStats ln_ff{ctx->stat_att, NB, inv_d, 1e-5f};               // ... in front of the feed-forward block
    {
      GemmArgs<Op> ga{(const E*)ctx->X_op.p, d, (const E*)w.Win.p, d, M, 3 * d, d, 0};
      EpiQKV<Op, true> ep{w.c2_in, (E*)ctx->QK_op.p, (E*)ctx->Vt_op.p, d, ctx->H, ctx->hd, Sp, ctx->Skp, qscale, {w.Win.inv_scale, ctx->status}, ln_in};
      HIPCHK(ctx, launch_qkv<Op>(ga, ep, B, Sp, st, [&](const char* name, int cols) { mark(name, BS * 2.0 * dd * cols); }));
    }
    {
      AttnArgs<Op> aa{(const E*)ctx->QK_op.p, (const E*)ctx->Vt_op.p, (E*)ctx->A_op.p, S, Sp, ctx->Skp, d, ctx->H, 0};
      HIPCHK(ctx, launch_attn<Op>(aa, B, ctx->hd, st));
      mark("attention", 4.0 * B * (double)S * S * dd);
    }
    {
      GemmArgs<Op> ga{(const E*)ctx->A_op.p, d, (const E*)w.Wout.p, d, M, d, d, 0};
      EpiResid<Op> ep{w.bb_att, w.g_att, ctx->X, (E*)ctx->X_st, d, ctx->stat_att, ACT_NONE, {w.Wout.inv_scale, ctx->status}, ln_in};
      HIPCHK(ctx, launch_resid<Op>(ga, ep, B, Sp, st));
      mark("gemm_outproj", BS * 2.0 * dd * dd);
    }
    {
      GemmArgs<Op> ga{(const E*)ctx->X_op.p, d, (const E*)w.W1.p, d, M, ff, d, 0};
      EpiBiasAct<Op, true> ep{w.c2_ff, nullptr, 0, (E*)ctx->H_op.p, ff, ACT_GELU, {w.W1.inv_scale, ctx->status}, ln_ff};
      HIPCHK(ctx, launch_ffn1<Op>(ga, ep, B, Sp, st));
      mark("gemm_ffn1_gelu", BS * 2.0 * dd * ff);
    }
    {
      GemmArgs<Op> ga{(const E*)ctx->H_op.p, ff, (const E*)w.W2.p, ff, M, d, ff, 0};
      EpiResid<Op> ep{w.bb_ffn, w.g_ffn, ctx->X, (E*)ctx->X_st, d, ctx->stat_ffn, ACT_NONE, {w.W2.inv_scale, ctx->status}, ln_ff};
      HIPCHK(ctx, launch_resid<Op>(ga, ep, B, Sp, st));
      mark("gemm_ffn2", BS * 2.0 * dd * ff);
    }
  }
  {
    GemmArgs<Op> ga{(const E*)ctx->X_op.p, d, (const E*)ctx->Wf.p, d, M, ctx->XN, d, 0};
    EpiHead<Op> head = head_in;
    head.t_off = t_off;
    HIPCHK(ctx, launch_rows<Op>(ga, head, st));
    mark("gemm_head_ddpm", BT * 2.0 * dd * F);
  }
  ctx->step_kernels = nk;
  return 0;
}

template <class Op>
static EpiHead<Op> make_head(tamf_ctx* ctx, int mode) {
  EpiHead<Op> h{};
  h.bias = ctx->bf;
  h.mode = mode;
  h.F = ctx->F;
  h.T = ctx->T;
  h.Sp = ctx->Sp;
  h.P = ctx->P;
  h.XK = ctx->XK;
  h.xs = ctx->xs;
  h.xs_op = (typename Op::elem_t*)ctx->xs_st;
  h.tcur = ctx->tcur;
  h.c1 = ctx->c1;
  h.c2 = ctx->c2;
  h.sigma = ctx->sigma;
  h.n_steps = ctx->n_steps;
  h.lp = ctx->loop_params;
  h.ctl = EpiCtl{ctx->Wf.inv_scale, ctx->status};
  h.ln = LnStats{ctx->stat_ffn, ctx->d / 32, 1.0f / (float)ctx->d, 1e-5f};
  return h;
}

template <class Op>
static int denoise_impl(tamf_ctx* ctx, const float* x, const int64_t* t_dev, float* out, hipStream_t st) {
  typedef typename Op::elem_t E;
  const int B = ctx->B, T = ctx->T;
  hipLaunchKernelGGL((state_in_kernel<Op>), grid1d((long)B * T * (ctx->XK / 8)), dim3(256), 0, st, x, ctx->xs, (E*)ctx->xs_st,
                     B, ctx->F, T, ctx->XK, 0, 0ull, 0ll, ctx->status);
  hipLaunchKernelGGL(set_t_kernel, grid1d(B), dim3(256), 0, st, ctx->tcur, (const long long*)t_dev, 0, B, ctx->n_t > 0 ? ctx->n_t : 1);
  EpiHead<Op> h = make_head<Op>(ctx, HEAD_X0);
  h.x0_out = out;
  TRY(enqueue_step<Op>(ctx, st, h));
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

extern "C" int tamf_denoise(tamf_ctx* ctx, const float* x_dev, const int64_t* t_dev, float* x0_out_dev, void* stream) {
  TAMF_LAUNCH_LOCK;
  TRY(need_kind(ctx, __func__, KIND_G));
  if (!x_dev || !t_dev || !x0_out_dev) return fail(ctx, TAMF_ERR_INVALID, "null argument");
  if (!ctx->cond_set) return fail(ctx, TAMF_ERR_STATE, "conditioning not set");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  TAMF_WITH_OP(ctx->prec, return denoise_impl<Op>(ctx, x_dev, t_dev, x0_out_dev, st));
  return 0;
}

template <class Op>
static int refine_impl(tamf_ctx* ctx, const float* x_in, const float* h2o, float* out, hipStream_t st) {
  typedef typename Op::elem_t E;
  const int B = ctx->B, T = ctx->T;
  hipLaunchKernelGGL((refine_in_kernel<Op>), grid1d((long)B * T * (ctx->XK / 8)), dim3(256), 0, st, x_in, h2o, (E*)ctx->xs_op.p,
                     B * T, ctx->F, ctx->arch.h2o_dim, ctx->XK, ctx->status);
  EpiHead<Op> h = make_head<Op>(ctx, HEAD_RESIDUAL);
  h.x0_out = out;
  h.x_in = x_in;
  TRY(enqueue_step<Op>(ctx, st, h));
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

extern "C" int tamf_refine(tamf_ctx* ctx, const float* sample_pose_repr_dev, const float* h2o_dist_dev, float* out_dev,
                           void* stream) {
  TAMF_LAUNCH_LOCK;
  TRY(need_kind(ctx, __func__, KIND_R));
  if (!sample_pose_repr_dev || !h2o_dist_dev || !out_dev) return fail(ctx, TAMF_ERR_INVALID, "null argument");
  if (!ctx->cond_set) return fail(ctx, TAMF_ERR_STATE, "conditioning not set");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  TAMF_WITH_OP(ctx->prec, return refine_impl<Op>(ctx, sample_pose_repr_dev, h2o_dist_dev, out_dev, st));
  return 0;
}

extern "C" int tamf_ddpm_step(tamf_ctx* ctx, const float* x_t_dev, const float* x0_dev, int32_t t, const float* noise_dev,
                              float* x_out_dev, int64_t n, void* stream) {
  TRY(need_kind(ctx, __func__, KIND_G | KIND_R));
  if (!x_t_dev || !x0_dev || !x_out_dev || n <= 0) return fail(ctx, TAMF_ERR_INVALID, "null/invalid argument");
  if (ctx->n_steps <= 0) return fail(ctx, TAMF_ERR_STATE, "schedule not set");
  if (t < 0 || t >= ctx->n_steps) return fail(ctx, TAMF_ERR_INVALID, "t out of range");
  if (t != 0 && !noise_dev) return fail(ctx, TAMF_ERR_INVALID, "noise required for t != 0");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipLaunchKernelGGL(ddpm_step_kernel, grid1d(n), dim3(256), 0, (hipStream_t)stream, x_t_dev, x0_dev, noise_dev, x_out_dev,
                     (long)n, ctx->h_c1[t], ctx->h_c2[t], ctx->h_sigma[t], t);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

template <class Op>
static int loop_impl(tamf_ctx* ctx, const float* noise, uint64_t seed, int64_t clip_base, float* out, float* dump,
                     int use_graph, hipStream_t st) {
  typedef typename Op::elem_t E;
  const int B = ctx->B, T = ctx->T, N = ctx->n_steps;
  // draw 0 = x_T
  hipLaunchKernelGGL((state_in_kernel<Op>), grid1d((long)B * T * (ctx->XK / 8)), dim3(256), 0, st, noise, ctx->xs,
                     (E*)ctx->xs_st, B, ctx->F, T, ctx->XK, noise ? 0 : 1, (unsigned long long)seed,
                     (long long)clip_base, ctx->status);
  hipLaunchKernelGGL(set_t_kernel, grid1d(B), dim3(256), 0, st, ctx->tcur, (const long long*)nullptr, N - 1, B, ctx->n_t > 0 ? ctx->n_t : 1);
  EpiHead<Op> h = make_head<Op>(ctx, HEAD_DDPM);
  struct InLoop {  // the step's timestep-embedding table is the respaced one (if a map is set) while the LOOP enqueues or captures
    tamf_ctx* c;
    explicit InLoop(tamf_ctx* c_) : c(c_) { c->in_loop = true; }
    ~InLoop() { c->in_loop = false; }
  } in_loop_(ctx);
  hipLaunchKernelGGL(set_loop_params_kernel, dim3(1), dim3(64), 0, st, ctx->loop_params, noise, dump, (long)B * ctx->F * T,
                     (unsigned long long)seed, (long long)clip_base);
  if (!use_graph) {
    for (int i = 0; i < N; ++i) {
      TRY(enqueue_step<Op>(ctx, st, h));
      hipLaunchKernelGGL(advance_t_kernel, grid1d(B), dim3(256), 0, st, ctx->tcur, B, 1);
    }
  } else {
    // G consecutive steps per graph (the largest divisor of N up to 16: 10 for N = 1000 -> 100 graph launches per loop);
    // the sequence is step-agnostic (device-side step counter) and seed-agnostic (LoopParams), so it is captured once per
    // (B, T, N) and replayed by every later loop
    int G = 1;
    for (int g = 2; g <= 16; ++g)
      if (N % g == 0) G = g;
    GraphKey key;
    key.B = B; key.T = T; key.n_steps = N; key.steps_per_graph = G;
    if (!(key == ctx->graph_key) || !ctx->graph_exec) {
      TRY(retire_graph(ctx));
      HIPCHK(ctx, hipStreamBeginCapture(ctx->cap_stream, hipStreamCaptureModeRelaxed));
      int rc = 0;
      // step g of the graph works at t = counter - g (a kernel argument of its input-merge and head GEMMs); the counter itself
      // moves once per graph launch
      for (int g = 0; g < G && rc == 0; ++g) rc = enqueue_step<Op>(ctx, ctx->cap_stream, h, g);
      hipLaunchKernelGGL(advance_t_kernel, grid1d(B), dim3(256), 0, ctx->cap_stream, ctx->tcur, B, G);
      hipError_t ee = hipStreamEndCapture(ctx->cap_stream, &ctx->graph);
      if (rc) return rc;
      HIPCHK(ctx, ee);
      HIPCHK(ctx, hipGraphInstantiate(&ctx->graph_exec, ctx->graph, nullptr, nullptr, 0));
      ctx->graph_key = key;
      ++ctx->graph_captures;
    }
    for (int i = 0; i < N / G; ++i) HIPCHK(ctx, hipGraphLaunch(ctx->graph_exec, st));
    ctx->graph_launches_last_loop = N / G;
    HIPCHK(ctx, hipEventRecord(ctx->graph_done, st));
    ctx->graph_in_flight = true;
  }
  hipLaunchKernelGGL(state_out_kernel, grid1d((long)B * ctx->F * T), dim3(256), 0, st, ctx->xs, out, B, ctx->F, T, ctx->XK);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

extern "C" int tamf_sample_loop(tamf_ctx* ctx, const float* noise_dev, uint64_t seed, int64_t clip_id_base, float* x0_out_dev,
                                float* dump_dev, int32_t use_graph, void* stream) {
  TAMF_LAUNCH_LOCK;
  TRY(need_kind(ctx, __func__, KIND_G));
  if (!x0_out_dev) return fail(ctx, TAMF_ERR_INVALID, "null argument");
  if (!ctx->cond_set) return fail(ctx, TAMF_ERR_STATE, "conditioning not set");
  if (ctx->n_steps <= 0) return fail(ctx, TAMF_ERR_STATE, "schedule not set");
  if (ctx->n_steps > ctx->n_t) return fail(ctx, TAMF_ERR_STATE, "schedule longer than the timestep table (max_timesteps)");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  TAMF_WITH_OP(ctx->prec, return loop_impl<Op>(ctx, noise_dev, seed, clip_id_base, x0_out_dev, dump_dev, use_graph, st));
  return 0;
}

extern "C" int tamf_get_status_flags(tamf_ctx* ctx, uint32_t* flags, int32_t clear, void* stream) {
  TRY(need_kind(ctx, __func__, KIND_G | KIND_R));
  if (!flags) return fail(ctx, TAMF_ERR_INVALID, "null argument");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipStreamSynchronize((hipStream_t)stream));
  // this context's own word (per-context since round 4: another context on the device neither sees nor clears it)
  unsigned v = 0;
  HIPCHK(ctx, hipMemcpy(&v, ctx->status, sizeof(v), hipMemcpyDeviceToHost));
  *flags = v | ctx->host_status;  // (the host-side bits describe the loaded weights: they are not cleared)
  if (clear && v) HIPCHK(ctx, hipMemset(ctx->status, 0, sizeof(v)));
  return 0;
}

extern "C" int tamf_step_kernel_count(const tamf_ctx* ctx) { return ctx ? ctx->step_kernels : 0; }

extern "C" int tamf_loop_stats(const tamf_ctx* ctx, int32_t* graph_captures, int32_t* graph_launches_last_loop) {
  if (!ctx) return TAMF_ERR_INVALID;
  if (graph_captures) *graph_captures = ctx->graph_captures;
  if (graph_launches_last_loop) *graph_launches_last_loop = ctx->graph_launches_last_loop;
  return 0;
}

template <class Op>
static int profile_impl(tamf_ctx* ctx, hipStream_t st) {
  EpiHead<Op> h = make_head<Op>(ctx, HEAD_DDPM);
  hipLaunchKernelGGL(set_loop_params_kernel, dim3(1), dim3(64), 0, st, ctx->loop_params, (const float*)nullptr, (float*)nullptr,
                     (long)ctx->B * ctx->F * ctx->T, 1ull, 0ll);
  return enqueue_step<Op>(ctx, st, h);
}

// Runs `body` (which enqueues launches through enqueue_step) with an event behind every launch and reports per launch: milliseconds,
// algorithmic FLOPs, name.
template <class Body>
static int profile_run(tamf_ctx* ctx, int32_t max_n, float* ms_host, double* flops_host, char* names_host, hipStream_t st, Body body) {
  ctx->prof_ev.clear();
  ctx->prof_names.clear();
  ctx->prof_flops.clear();
  hipEvent_t ev0;
  HIPCHK(ctx, hipEventCreate(&ev0));
  // cost of an event record between two launches: measured on back-to-back records with nothing in between and taken
  // off every interval below, so that the per-launch times agree with the profiler's kernel durations
  hipEvent_t cal[6];
  for (hipEvent_t& e : cal) HIPCHK(ctx, hipEventCreate(&e));
  ctx->prof_on = true;
  for (hipEvent_t& e : cal) (void)hipEventRecord(e, st);
  (void)hipEventRecord(ev0, st);
  int rc = body();
  ctx->prof_on = false;
  hipError_t se = hipStreamSynchronize(st);
  int n = 0;
  if (rc == 0 && se == hipSuccess) {
    float gaps[5];
    for (int i = 0; i < 5; ++i) {
      gaps[i] = 0.f;
      (void)hipEventElapsedTime(&gaps[i], cal[i], cal[i + 1]);
    }
    std::sort(gaps, gaps + 5);
    const float ev_cost = gaps[2];
    hipEvent_t prev = ev0;
    for (size_t i = 0; i < ctx->prof_ev.size() && n < max_n; ++i, ++n) {
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, prev, ctx->prof_ev[i]);
      ms = ms > ev_cost ? ms - ev_cost : ms;
      ms_host[n] = ms;
      flops_host[n] = ctx->prof_flops[i];
      snprintf(names_host + (size_t)n * 48, 48, "%s", ctx->prof_names[i].c_str());
      prev = ctx->prof_ev[i];
    }
  }
  for (hipEvent_t e : ctx->prof_ev) (void)hipEventDestroy(e);
  for (hipEvent_t e : cal) (void)hipEventDestroy(e);
  (void)hipEventDestroy(ev0);
  ctx->prof_ev.clear();
  if (rc) return rc;
  HIPCHK(ctx, se);
  return n;
}

extern "C" int tamf_step_profile(tamf_ctx* ctx, int32_t max_n, float* ms_host, double* flops_host, char* names_host,
                                 void* stream) {
  TAMF_LAUNCH_LOCK;
  TRY(need_kind(ctx, __func__, KIND_G));
  if (!ms_host || !flops_host || !names_host || max_n <= 0) return fail(ctx, TAMF_ERR_INVALID, "null/invalid argument");
  if (!ctx->cond_set || ctx->n_steps <= 0) return fail(ctx, TAMF_ERR_STATE, "conditioning / schedule not set");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(set_t_kernel, grid1d(ctx->B), dim3(256), 0, st, ctx->tcur, (const long long*)nullptr, ctx->n_steps / 2, ctx->B, ctx->n_t > 0 ? ctx->n_t : 1);
  return profile_run(ctx, max_n, ms_host, flops_host, names_host, st, [&]() {
    int rc = 0;
    TAMF_WITH_OP(ctx->prec, rc = profile_impl<Op>(ctx, st));
    return rc;
  });
}

extern "C" int tamf_refine_profile(tamf_ctx* ctx, const float* sample_pose_repr_dev, const float* h2o_dist_dev, float* out_dev,
                                   int32_t max_n, float* ms_host, double* flops_host, char* names_host, void* stream) {
  TAMF_LAUNCH_LOCK;
  TRY(need_kind(ctx, __func__, KIND_R));
  if (!sample_pose_repr_dev || !h2o_dist_dev || !out_dev || !ms_host || !flops_host || !names_host || max_n <= 0)
    return fail(ctx, TAMF_ERR_INVALID, "null/invalid argument");
  if (!ctx->cond_set) return fail(ctx, TAMF_ERR_STATE, "conditioning not set");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  return profile_run(ctx, max_n, ms_host, flops_host, names_host, st, [&]() {
    int rc = 0;
    TAMF_WITH_OP(ctx->prec, rc = refine_impl<Op>(ctx, sample_pose_repr_dev, h2o_dist_dev, out_dev, st));
    return rc;
  });
}

// ------------------------------------------------------------------------------------------------
// SegmentEncoder forward (TAMF_KIND_E): two launches - the prefix rows (prefix_rows_kernel, shared with G / R) and the encoder
// (encoder_kernel, tamf_encoder.h: one workgroup per clip)
// ------------------------------------------------------------------------------------------------
extern "C" int tamf_encode(tamf_ctx* ctx, int32_t B, int32_t T, int32_t nobj, const int32_t* obj_num_host, const float* pose_repr_dev,
                           const float* shape_dev, const uint8_t* hand_side_dev, const float* obj_emb_dev, const float* obj_traj_dev,
                           float* encoding_out_dev, float* activation_out_dev, void* stream) {
  TAMF_LAUNCH_LOCK;
  TRY(need_kind(ctx, __func__, KIND_E));
  if (!ctx->finalized) return fail(ctx, TAMF_ERR_STATE, "weights not finalised");
  if (B <= 0 || B > ctx->Bmax || T <= 0 || T > ctx->Tmax || nobj <= 0)
    return fail(ctx, TAMF_ERR_INVALID, "B/T/nobj out of range (B = " + std::to_string(B) + " of max_batch " + std::to_string(ctx->Bmax) +
                                           ", T = " + std::to_string(T) + " of max_frames " + std::to_string(ctx->Tmax) + ")");
  if (!pose_repr_dev || !shape_dev || !hand_side_dev || !obj_emb_dev || !obj_traj_dev || !encoding_out_dev)
    return fail(ctx, TAMF_ERR_INVALID, "null tensor");
  TRY(check_obj_num(ctx, obj_num_host, B, nobj));
  HIPCHK(ctx, hipSetDevice(ctx->device));
  hipStream_t st = (hipStream_t)stream;
  const int* cnt = nullptr;
  TRY(upload_obj_num(ctx, obj_num_host, B, st, &cnt));
  const int d = ctx->d, sd = ctx->arch.hand_shape_dim, od = ctx->arch.obj_embed_dim;
  PrefixArgs pa{};
  pa.side = hand_side_dev; pa.rh = ctx->rh; pa.lh = ctx->lh;
  pa.shape = shape_dev; pa.WshapeT = ctx->WshapeT; pa.bshape = ctx->bshape;
  pa.oemb = obj_emb_dev; pa.WobjT = ctx->WobjT; pa.bobj = ctx->bobj; pa.cnt = cnt;
  pa.pe = ctx->pe; pa.pstatic = ctx->pstatic;
  pa.B = B; pa.d = d; pa.T = T; pa.sd = sd; pa.nobj = nobj; pa.od = od; pa.clip_dim = 0; pa.nrows = ENC_P; pa.ht = 0;
  hipLaunchKernelGGL(prefix_rows_kernel, dim3(B, ENC_P), dim3(1024), (size_t)(std::max(od, sd) + 1024) * sizeof(float), st, pa);
  EncArgs ea{};
  ea.w = ctx->enc_w; ea.pe = ctx->pe; ea.pstatic = ctx->pstatic; ea.pose = pose_repr_dev; ea.traj = obj_traj_dev; ea.cnt = cnt;
  ea.enc = encoding_out_dev; ea.act = activation_out_dev;
  ea.T = T; ea.nobj = nobj; ea.F = ctx->F; ea.qd = ctx->arch.obj_input_dim; ea.kin = ctx->enc_kin; ea.ff = ctx->ff; ea.L = ctx->L;
  hipLaunchKernelGGL(encoder_kernel, dim3(B), dim3(ENC_NT), (size_t)enc_lds_bytes(T + ENC_P + 1, ctx->ff, ctx->enc_kin), st, ea);
  HIPCHK(ctx, hipGetLastError());
  return 0;
}

extern "C" int tamf_pose_decode(const float* pose_repr_dev, int64_t n_frames, int32_t n_joints, float* tsl_out_dev,
                                float* quat_out_dev, void* stream) {
  if (!pose_repr_dev || !quat_out_dev || n_frames <= 0 || n_joints <= 0) return fail(nullptr, TAMF_ERR_INVALID, "bad argument");
  hipLaunchKernelGGL(pose_decode_kernel, grid1d(n_frames * n_joints), dim3(256), 0, (hipStream_t)stream, pose_repr_dev,
                     tsl_out_dev, quat_out_dev, (long)n_frames, n_joints, 3 + 6 * n_joints);
  return launched();
}

static int h2o_launch(const float* hand_verts_dev, const float* obj_traj_dev, const float* obj_points_dev,
                      const int32_t* obj_num_dev, int32_t B, int32_t T, int32_t V, int32_t nobj, int32_t P, float* h2o_out_dev,
                      float* frame_min_dev, void* stream) {
  if (!hand_verts_dev || !obj_traj_dev || !obj_points_dev || (!h2o_out_dev && !frame_min_dev))
    return fail(nullptr, TAMF_ERR_INVALID, "null argument");
  if (B <= 0 || T <= 0 || V <= 0 || nobj <= 0 || P <= 0) return fail(nullptr, TAMF_ERR_INVALID, "bad shape");
  if (V > 256 * H2O_VPT) return fail(nullptr, TAMF_ERR_INVALID, "at most 1024 hand vertices per frame (MANO has 778)");
  if (B > 65535) return fail(nullptr, TAMF_ERR_INVALID, "batch too large for one launch");
  hipLaunchKernelGGL(h2o_dist_kernel, dim3(T, B), dim3(256), 0, (hipStream_t)stream, hand_verts_dev, obj_traj_dev,
                     obj_points_dev, (const int*)obj_num_dev, h2o_out_dev, frame_min_dev, T, V, nobj, P);
  return launched();
}

extern "C" int tamf_h2o_dist(const float* hand_verts_dev, const float* obj_traj_dev, const float* obj_points_dev,
                             const int32_t* obj_num_dev, int32_t B, int32_t T, int32_t V, int32_t nobj, int32_t P,
                             float* h2o_out_dev, void* stream) {
  if (!h2o_out_dev) return fail(nullptr, TAMF_ERR_INVALID, "null argument");
  return h2o_launch(hand_verts_dev, obj_traj_dev, obj_points_dev, obj_num_dev, B, T, V, nobj, P, h2o_out_dev, nullptr, stream);
}

extern "C" int tamf_contact_min_dist(const float* hand_verts_dev, const float* obj_traj_dev, const float* obj_points_dev,
                                     const int32_t* obj_num_dev, int32_t B, int32_t T, int32_t V, int32_t nobj, int32_t P,
                                     float* min_dist_out_dev, void* stream) {
  if (!min_dist_out_dev) return fail(nullptr, TAMF_ERR_INVALID, "null argument");
  return h2o_launch(hand_verts_dev, obj_traj_dev, obj_points_dev, obj_num_dev, B, T, V, nobj, P, nullptr, min_dist_out_dev, stream);
}

extern "C" int tamf_transform_points(const void* obj_traj_dev, const void* obj_points_dev, int32_t n_obj, int32_t T, int32_t P,
                                     int32_t is_f64, void* out_dev, void* stream) {
  if (!obj_traj_dev || !obj_points_dev || !out_dev) return fail(nullptr, TAMF_ERR_INVALID, "null argument");
  if (n_obj <= 0 || T <= 0 || P <= 0 || n_obj > 65535) return fail(nullptr, TAMF_ERR_INVALID, "bad shape");
  if (is_f64)
    hipLaunchKernelGGL((transform_points_kernel<double>), dim3(T, n_obj), dim3(256), 0, (hipStream_t)stream, (const double*)obj_traj_dev,
                       (const double*)obj_points_dev, (double*)out_dev, T, P);
  else
    hipLaunchKernelGGL((transform_points_kernel<float>), dim3(T, n_obj), dim3(256), 0, (hipStream_t)stream, (const float*)obj_traj_dev,
                       (const float*)obj_points_dev, (float*)out_dev, T, P);
  return launched();
}

extern "C" int tamf_vertex_normals(const float* verts_dev, int64_t n_mesh, int32_t V, const int32_t* csr_off_dev,
                                    const int32_t* csr_ent_dev, float* normals_out_dev, void* stream) {
  if (!verts_dev || !csr_off_dev || !csr_ent_dev || !normals_out_dev) return fail(nullptr, TAMF_ERR_INVALID, "null argument");
  if (n_mesh <= 0 || V <= 0) return fail(nullptr, TAMF_ERR_INVALID, "bad shape");
  hipLaunchKernelGGL(vertex_normals_kernel, grid1d((long)n_mesh * V), dim3(256), 0, (hipStream_t)stream, verts_dev, csr_off_dev,
                     csr_ent_dev, normals_out_dev, (long)n_mesh, V);
  return launched();
}

extern "C" int tamf_mesh_contains(const double* verts_dev, const int32_t* faces_dev, int32_t n_faces, const double* points_dev,
                                  int64_t n_points, const double* scale3, const double* translate3, int32_t resolution,
                                  double* tri_workspace_dev, uint8_t* contains_out_dev, void* stream) {
  if (!verts_dev || !faces_dev || !points_dev || !scale3 || !translate3 || !tri_workspace_dev || !contains_out_dev)
    return fail(nullptr, TAMF_ERR_INVALID, "null argument");
  if (n_faces <= 0 || n_points <= 0 || resolution <= 1) return fail(nullptr, TAMF_ERR_INVALID, "bad shape");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mesh_prepare_kernel, grid1d(n_faces), dim3(256), 0, st, verts_dev, (const int*)faces_dev, n_faces, scale3[0],
                     scale3[1], scale3[2], translate3[0], translate3[1], translate3[2], tri_workspace_dev);
  hipLaunchKernelGGL(mesh_contains_kernel, grid1d(n_points), dim3(256), 0, st, tri_workspace_dev, n_faces, points_dev,
                     (long)n_points, scale3[0], scale3[1], scale3[2], translate3[0], translate3[1], translate3[2],
                     (double)resolution, contains_out_dev);
  return launched();
}

// PSKL-J score, device half (tamf_spectrum.h): one launch per PS_LENS clips - the lengths travel in the kernel arguments - each
// continuing the sums of the one before, which by the kernel's ordered addition is the same arithmetic as one launch over all N
extern "C" int tamf_power_spectrum_sum(const float* joints_dev, const int32_t* len_host, int32_t N, int32_t T, int32_t F,
                                       int32_t accumulate, double* psd_sum_dev, double* psd_clip_dev, void* stream) {
  if (N < 1 || F < 1) return fail(nullptr, TAMF_ERR_INVALID, "bad shape (N = " + std::to_string(N) + ", F = " + std::to_string(F) + ")");
  if (T < 3) return fail(nullptr, TAMF_ERR_INVALID, "T = " + std::to_string(T) + ": the second difference needs at least 3 frames");
  if (T > PS_MAX_T)
    return fail(nullptr, TAMF_ERR_INVALID, "T = " + std::to_string(T) + " above the " + std::to_string(PS_MAX_T) +
                                               " frames whose accelerations and twiddle table fit the LDS");
  if (!joints_dev || !psd_sum_dev) return fail(nullptr, TAMF_ERR_INVALID, "null argument");
  if (len_host)
    for (int n = 0; n < N; ++n)
      if (len_host[n] < 1 || len_host[n] > T)
        return fail(nullptr, TAMF_ERR_INVALID, "len[" + std::to_string(n) + "] = " + std::to_string(len_host[n]) + " outside [1, T]");
  const int L = T - 2, K = L / 2 + 1;
  const size_t lds = ps_lds_bytes(L);
  // the dynamic-LDS ceiling of the kernel is raised once per device, to what the longest accepted clip needs
  const hipError_t e = lds_once<power_spectrum_kernel>((int)ps_lds_bytes(PS_MAX_T - 2));
  if (e != hipSuccess) return fail(nullptr, TAMF_ERR_HIP, std::string("power spectrum kernel attribute setup failed: ") + hipGetErrorString(e));
  const dim3 grid((F + PS_FT - 1) / PS_FT, (K + PS_KT - 1) / PS_KT);
  PsLens lens;  // refilled per launch up to its n; what a longer earlier launch left beyond n is never read (the kernel stops at n)
  memset(&lens, 0, sizeof(lens));
  for (int n0 = 0; n0 < N; n0 += PS_LENS) {
    const int n = std::min(PS_LENS, N - n0);
    if (len_host)
      for (int i = 0; i < n; ++i) lens.v[i] = (uint16_t)len_host[n0 + i];
    hipLaunchKernelGGL(power_spectrum_kernel, grid, dim3(PS_NT), lds, (hipStream_t)stream, joints_dev + (size_t)n0 * T * F, lens,
                       len_host ? 1 : 0, n, T, F, (accumulate || n0 > 0) ? 1 : 0, psd_sum_dev,
                       psd_clip_dev ? psd_clip_dev + (size_t)n0 * L * F : nullptr);
  }
  return launched();
}

#ifdef TAMF_TEST_HOOKS
#include "tamf_hip_hooks.h"
#endif
