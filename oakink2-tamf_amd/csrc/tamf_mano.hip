// libtamf_mano.so: the C-ABI of include/tamf_mano.h - the native MANO hand layer.  One translation unit.
#include "../../include/tamf_mano.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <string>
#include <vector>

#include "tamf_mano.h"

static thread_local std::string g_mano_error;

static int fail(int code, const std::string& msg) {
  g_mano_error = msg;
  return code;
}

extern "C" const char* tamf_mano_last_error(void) { return g_mano_error.c_str(); }

struct tamf_mano_model {
  float* f32 = nullptr;  // one allocation: basis | vt | w | jt | jd
  int* tab = nullptr;
  long off_vt = 0, off_w = 0, off_jt = 0, off_jd = 0;
  int V = 0, Vp = 0, center = -1, maxdepth = 0, m_tiles = 0;
};

static const int32_t kTips[MANO_TIPS] = {745, 317, 444, 556, 673};
static const int32_t kOrder[MANO_NJ] = {0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20};

static bool all_finite(const double* p, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(p[i])) return false;
  return true;
}

extern "C" int tamf_mano_model_create(int32_t V, const double* v_template, const double* shapedirs, const double* posedirs,
                                      const double* J_regressor, const double* weights, const int32_t* parents, const int32_t* tip_ids,
                                      const int32_t* joint_order, int32_t center_idx, tamf_mano_model** model_out) {
  if (!model_out) return fail(TAMF_ERR_INVALID, "model_out is null");
  *model_out = nullptr;  // (on every failure below, a null mandatory pointer included)
  const struct { const char* name; const double* p; size_t per_vertex; } arr[5] = {
      {"v_template", v_template, 3}, {"shapedirs", shapedirs, 3 * MANO_NB}, {"posedirs", posedirs, 3 * MANO_NP},
      {"J_regressor", J_regressor, MANO_J}, {"weights", weights, MANO_J}};
  for (const auto& x : arr)
    if (!x.p) return fail(TAMF_ERR_INVALID, std::string(x.name) + " is null");
  if (!parents) return fail(TAMF_ERR_INVALID, "parents is null");
  if (V < 1 || V > MANO_VMAX) return fail(TAMF_ERR_INVALID, "V = " + std::to_string(V) + " outside [1, 1024]");
  if (center_idx < -1 || center_idx >= MANO_NJ) return fail(TAMF_ERR_INVALID, "center_idx = " + std::to_string(center_idx) + " outside [-1, 21)");
  for (const auto& x : arr)
    if (!all_finite(x.p, (size_t)V * x.per_vertex)) return fail(TAMF_ERR_INVALID, std::string(x.name) + " holds a non-finite value");
  int tab[MANO_T_INTS];
  int maxdepth = 0;
  for (int j = 0; j < MANO_J; ++j) {
    const int p = parents[j];
    if (j == 0 ? p >= 0 : (p < 0 || p >= j))
      return fail(TAMF_ERR_INVALID, "parents[" + std::to_string(j) + "] = " + std::to_string(p) + ": need a tree with root 0 and parents below their children");
    tab[MANO_T_PARENT + j] = j == 0 ? -1 : p;
    tab[MANO_T_DEPTH + j] = j == 0 ? 0 : tab[MANO_T_DEPTH + p] + 1;
    maxdepth = std::max(maxdepth, tab[MANO_T_DEPTH + j]);
  }
  for (int i = 0; i < MANO_TIPS; ++i) {
    const int t = (tip_ids ? tip_ids : kTips)[i];
    if (t < 0 || t >= V) return fail(TAMF_ERR_INVALID, "tip_ids[" + std::to_string(i) + "] = " + std::to_string(t) + " outside [0, V)");
    tab[MANO_T_TIP + i] = t;
  }
  bool seen[MANO_NJ] = {};
  for (int i = 0; i < MANO_NJ; ++i) {
    const int s = (joint_order ? joint_order : kOrder)[i];
    if (s < 0 || s >= MANO_NJ || seen[s]) return fail(TAMF_ERR_INVALID, "joint_order is not a permutation of 0..20");
    seen[s] = true;
    tab[MANO_T_ORDER + i] = s;
  }

  const int Vp = (V + 15) / 16 * 16;
  tamf_mano_model* m = new tamf_mano_model;
  m->V = V, m->Vp = Vp, m->center = center_idx, m->maxdepth = maxdepth;
  const long n_basis = 3L * MANO_KP * Vp;
  m->off_vt = n_basis;
  m->off_w = m->off_vt + 3L * Vp;
  m->off_jt = m->off_w + (long)Vp * MANO_J;
  m->off_jd = m->off_jt + MANO_J * 3;
  const long total = m->off_jd + MANO_J * 3 * MANO_NB;
  std::vector<float> h((size_t)total, 0.f);
  for (int i = 0; i < V; ++i)
    for (int c = 0; c < 3; ++c) {
      float* plane = h.data() + (long)c * MANO_KP * Vp;
      for (int k = 0; k < MANO_NB; ++k) plane[(long)k * Vp + i] = (float)shapedirs[((size_t)i * 3 + c) * MANO_NB + k];
      for (int k = 0; k < MANO_NP; ++k) plane[(long)(MANO_NB + k) * Vp + i] = (float)posedirs[((size_t)i * 3 + c) * MANO_NP + k];
      h[m->off_vt + (long)c * Vp + i] = (float)v_template[i * 3 + c];
    }
  for (int i = 0; i < V; ++i)
    for (int j = 0; j < MANO_J; ++j) h[m->off_w + (long)i * MANO_J + j] = (float)weights[(size_t)i * MANO_J + j];
  // J_template = J_regressor . v_template, J_dirs = J_regressor . shapedirs: float64, vertices in ascending order, then rounded
  for (int j = 0; j < MANO_J; ++j)
    for (int c = 0; c < 3; ++c) {
      double s = 0.0, sd[MANO_NB] = {};
      for (int i = 0; i < V; ++i) {
        const double r = J_regressor[(size_t)j * V + i];
        s += r * v_template[i * 3 + c];
        for (int k = 0; k < MANO_NB; ++k) sd[k] += r * shapedirs[((size_t)i * 3 + c) * MANO_NB + k];
      }
      h[m->off_jt + j * 3 + c] = (float)s;
      for (int k = 0; k < MANO_NB; ++k) h[m->off_jd + (j * 3 + c) * MANO_NB + k] = (float)sd[k];
    }
  hipError_t e = hipMalloc((void**)&m->f32, (size_t)total * sizeof(float));
  if (e == hipSuccess) e = hipMalloc((void**)&m->tab, sizeof(tab));
  if (e != hipSuccess) {
    (void)hipFree(m->f32);
    delete m;
    return fail(e == hipErrorOutOfMemory ? TAMF_ERR_NOMEM : TAMF_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
  }
  e = hipMemcpy(m->f32, h.data(), (size_t)total * sizeof(float), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(m->tab, tab, sizeof(tab), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(m->f32);
    (void)hipFree(m->tab);
    delete m;
    return fail(TAMF_ERR_HIP, std::string("hipMemcpy: ") + hipGetErrorString(e));
  }
  *model_out = m;
  return 0;
}

extern "C" int tamf_mano_model_destroy(tamf_mano_model* m) {
  if (!m) return 0;
  hipError_t e = hipFree(m->f32);
  hipError_t e2 = hipFree(m->tab);
  delete m;
  if (e != hipSuccess || e2 != hipSuccess) return fail(TAMF_ERR_HIP, std::string("hipFree: ") + hipGetErrorString(e != hipSuccess ? e : e2));
  return 0;
}

extern "C" int tamf_mano_model_set_tiles(tamf_mano_model* m, int32_t m_tiles) {
  if (!m) return fail(TAMF_ERR_INVALID, "null argument");
  if (m_tiles != 0 && m_tiles != 1 && m_tiles != 2 && m_tiles != 4) return fail(TAMF_ERR_INVALID, "m_tiles must be 0, 1, 2 or 4");
  m->m_tiles = m_tiles;
  return 0;
}

template <int MT>
static hipError_t launch(const ManoArgs& a, dim3 grid, hipStream_t st) {
  const size_t lds = (size_t)MT * MANO_L_FLOATS * sizeof(float);
  if (lds > 64 * 1024) {  // (kernel attributes are per device; setting it again costs a host call, no device work)
    hipError_t e = hipFuncSetAttribute((const void*)mano_forward_kernel<MT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((mano_forward_kernel<MT>), grid, dim3(MANO_NT), lds, st, a);
  return hipGetLastError();
}

// Frame tiles per workgroup when the caller has not set one, and the split of the vertex tiles over blockIdx.y: enough workgroups
// to fill the device (256 CUs, a few workgroups each) before a workgroup takes more than one round of vertex tiles per wave.
// Neither enters the arithmetic.  One tile per workgroup: measured fastest at every shape (tools/mano_bench.py, DESIGN section 4 -
// with 2 or 4 tiles the kernel needs 256 VGPRs + accumulators, one wave per SIMD, and runs at about half the rate).
constexpr int MANO_DEFAULT_TILES = 1;
constexpr long MANO_TARGET_WGS = 1024;

extern "C" int tamf_mano_forward(const tamf_mano_model* m, const float* quat_dev, const float* betas_dev, int64_t N, float* verts_out_dev,
                                 float* joints_out_dev, void* stream) {
  if (!m) return fail(TAMF_ERR_INVALID, "null argument");
  if (N < 0) return fail(TAMF_ERR_INVALID, "N = " + std::to_string(N) + " is negative");
  if (N == 0) return 0;
  if (!quat_dev || !betas_dev || !verts_out_dev) return fail(TAMF_ERR_INVALID, "null argument");
  if ((uintptr_t)quat_dev & 15) return fail(TAMF_ERR_INVALID, "quat must be 16-byte aligned");
  if (N > (1LL << 31) - 64) return fail(TAMF_ERR_INVALID, "N too large for one call: split the batch");
  int mt = m->m_tiles;
  if (mt == 0) mt = MANO_DEFAULT_TILES;
  const long nx = (N + 16L * mt - 1) / (16L * mt);
  const int ntiles = m->Vp / 16;
  long gy = (MANO_TARGET_WGS + nx - 1) / nx;
  gy = std::max(1L, std::min(gy, (long)(ntiles + 3) / 4));
  const int tpg = (int)((ntiles + gy - 1) / gy);
  gy = (ntiles + tpg - 1) / tpg;
  ManoArgs a;
  a.basis = m->f32;
  a.vt = m->f32 + m->off_vt;
  a.w = m->f32 + m->off_w;
  a.jt = m->f32 + m->off_jt;
  a.jd = m->f32 + m->off_jd;
  a.tab = m->tab;
  a.quat = quat_dev;
  a.betas = betas_dev;
  a.verts = verts_out_dev;
  a.joints = joints_out_dev;
  a.N = (int)N, a.V = m->V, a.Vp = m->Vp, a.center = m->center, a.maxdepth = m->maxdepth, a.tiles_per_group = tpg;
  const dim3 grid((unsigned)nx, (unsigned)gy);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = mt == 1 ? launch<1>(a, grid, st) : mt == 2 ? launch<2>(a, grid, st) : launch<4>(a, grid, st);
  if (e != hipSuccess) return fail(TAMF_ERR_HIP, hipGetErrorString(e));
  return 0;
}

extern "C" int tamf_mano_backward(const tamf_mano_model* m, const float* quat_dev, const float* betas_dev, int64_t N, const float* dverts_dev,
                                  const float* djoints_dev, float* dquat_out_dev, float* dbetas_out_dev, void* stream) {
  if (!m) return fail(TAMF_ERR_INVALID, "null argument");
  if (N < 0) return fail(TAMF_ERR_INVALID, "N = " + std::to_string(N) + " is negative");
  if (N == 0) return 0;
  if (!quat_dev || !betas_dev || !dquat_out_dev) return fail(TAMF_ERR_INVALID, "null argument");
  if (!dverts_dev && !djoints_dev) return fail(TAMF_ERR_INVALID, "no upstream gradient: dverts and djoints are both null");
  if (((uintptr_t)quat_dev | (uintptr_t)dquat_out_dev) & 15) return fail(TAMF_ERR_INVALID, "quat and dquat_out must be 16-byte aligned");
  if (N > (1LL << 31) - 64) return fail(TAMF_ERR_INVALID, "N too large for one call: split the batch");
  ManoGradArgs ga;
  ManoArgs& a = ga.f;
  a.basis = m->f32;
  a.vt = m->f32 + m->off_vt;
  a.w = m->f32 + m->off_w;
  a.jt = m->f32 + m->off_jt;
  a.jd = m->f32 + m->off_jd;
  a.tab = m->tab;
  a.quat = quat_dev;
  a.betas = betas_dev;
  a.verts = nullptr;
  a.joints = nullptr;
  a.N = (int)N, a.V = m->V, a.Vp = m->Vp, a.center = m->center, a.maxdepth = m->maxdepth, a.tiles_per_group = 0;
  ga.dverts = dverts_dev;
  ga.djoints = djoints_dev;
  ga.dquat = dquat_out_dev;
  ga.dbetas = dbetas_out_dev;
  // one workgroup per 16 frames, whatever m_tiles says: the launch enters no operation's operands or order
  const size_t lds = (size_t)MANO_GL_FLOATS * sizeof(float);
  hipError_t e = hipFuncSetAttribute((const void*)mano_backward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return fail(TAMF_ERR_HIP, hipGetErrorString(e));
  hipLaunchKernelGGL(mano_backward_kernel, dim3((unsigned)((N + 15) / 16)), dim3(MANO_NT), lds, (hipStream_t)stream, ga);
  e = hipGetLastError();
  if (e != hipSuccess) return fail(TAMF_ERR_HIP, hipGetErrorString(e));
  return 0;
}
