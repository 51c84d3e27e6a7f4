// libtamf_sdfgrid.so: the C-ABI of include/tamf_sdfgrid.h - the SDF-lattice sampler of the training losses' `pen` term.  One translation unit.
#include "../../include/tamf_sdfgrid.h"

#include <hip/hip_runtime.h>

#include <string>

#include "tamf_sdfgrid.h"

static_assert(SG_MIN_RES == TAMF_SDFGRID_MIN_RES && SG_MAX_RES == TAMF_SDFGRID_MAX_RES, "the header's constants are the kernels'");

static thread_local std::string g_sdfgrid_error;

static int fail(int code, const std::string& msg) {
  g_sdfgrid_error = msg;
  return code;
}

extern "C" const char* tamf_sdfgrid_last_error(void) { return g_sdfgrid_error.c_str(); }

extern "C" int tamf_sdfgrid_forward(const float* values, const int64_t* grid_off, const int32_t* res, const double* origin, const double* step,
                                    int32_t G, const float* hand, const float* traj, const int32_t* grid_id, const int32_t* obj_num, int32_t B,
                                    int32_t T, int32_t V, int32_t nobj, float* depth, int32_t* cell, void* stream) {
  std::string bad = sg_bad_pointers(values, grid_off, res, origin, step, hand, traj, grid_id, depth, "depth_out");
  if (bad.empty()) bad = sg_bad_shape(G, B, T, V, nobj);
  if (!bad.empty()) return fail(TAMF_ERR_INVALID, bad);
  int32_t fc, nchunks;
  sg_chunks(T, 1, fc, nchunks);
  const SgSet S = {values, (const long long*)grid_off, (const int*)res, origin, step, G};
  hipLaunchKernelGGL(sdfgrid_forward_kernel, dim3(nchunks, B * nobj), dim3(SG_NT), 0, (hipStream_t)stream, S, hand, traj, (const int*)grid_id,
                     (const int*)obj_num, depth, (int*)cell, T, V, nobj, fc);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(TAMF_ERR_HIP, hipGetErrorString(e));
  return 0;
}

extern "C" int tamf_sdfgrid_backward(const float* values, const int64_t* grid_off, const int32_t* res, const double* origin, const double* step,
                                     int32_t G, const float* hand, const float* traj, const int32_t* grid_id, const int32_t* obj_num, int32_t B,
                                     int32_t T, int32_t V, int32_t nobj, const float* g_depth, float* g_hand, void* stream) {
  std::string bad = sg_bad_pointers(values, grid_off, res, origin, step, hand, traj, grid_id, g_hand, "g_hand_out");
  if (bad.empty() && !g_depth) bad = "null argument: g_depth is required";
  if (bad.empty()) bad = sg_bad_shape(G, B, T, V, nobj);
  if (!bad.empty()) return fail(TAMF_ERR_INVALID, bad);
  int32_t fc, nchunks;
  sg_chunks(T, nobj, fc, nchunks);
  const SgSet S = {values, (const long long*)grid_off, (const int*)res, origin, step, G};
  hipLaunchKernelGGL(sdfgrid_backward_kernel, dim3(nchunks, B), dim3(SG_NT), 0, (hipStream_t)stream, S, hand, traj, (const int*)grid_id,
                     (const int*)obj_num, g_depth, g_hand, T, V, nobj, fc);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(TAMF_ERR_HIP, hipGetErrorString(e));
  return 0;
}
