// libtamf_contact.so: the C-ABI of include/tamf_contact.h - the contact-distance kernels of the training losses.  One translation unit.
#include "../../include/tamf_contact.h"

#include <hip/hip_runtime.h>

#include <string>

#include "tamf_contact.h"

static thread_local std::string g_contact_error;

static int fail(int code, const std::string& msg) {
  g_contact_error = msg;
  return code;
}

extern "C" const char* tamf_contact_last_error(void) { return g_contact_error.c_str(); }

constexpr long CT_GRID_YZ = 65535;

// the limits of include/tamf_contact.h; "" when the shape is accepted
static std::string bad_shape(int B, int T, int V, int nobj, int P) {
  const std::string dims = "B = " + std::to_string(B) + ", T = " + std::to_string(T) + ", V = " + std::to_string(V) + ", nobj = " +
                           std::to_string(nobj) + ", P = " + std::to_string(P);
  if (B < 1 || T < 1 || nobj < 1 || P < 1) return "B, T, nobj and P must be at least 1 (" + dims + ")";
  if (V < 1 || V > CT_VMAX) return "V outside [1, " + std::to_string(CT_VMAX) + "] (" + dims + ")";
  if ((long)B * nobj > CT_GRID_YZ) return "B * nobj above " + std::to_string(CT_GRID_YZ) + ": split the batch (" + dims + ")";
  if (((long)P + CT_CHUNK - 1) / CT_CHUNK > CT_GRID_YZ) return "P above " + std::to_string(CT_GRID_YZ * CT_CHUNK) + " (" + dims + ")";
  return "";
}

extern "C" int tamf_contact_forward(const float* hand, const float* normals, const float* traj, const float* pts, const int32_t* obj_num,
                                    int32_t B, int32_t T, int32_t V, int32_t nobj, int32_t P, float* h2o, int32_t* h2o_idx, float* o2h,
                                    int32_t* o2h_idx, void* stream) {
  if (!hand || !traj || !pts) return fail(TAMF_ERR_INVALID, "null argument: hand_verts, obj_traj and obj_points are required");
  if (!h2o != !h2o_idx || !o2h != !o2h_idx) return fail(TAMF_ERR_INVALID, "an output pair needs both pointers (distance and index), or neither");
  if (!h2o && !o2h) return fail(TAMF_ERR_INVALID, "null argument: both output pairs are null, nothing to compute");
  const std::string bad = bad_shape(B, T, V, nobj, P);
  if (!bad.empty()) return fail(TAMF_ERR_INVALID, bad);
  hipStream_t st = (hipStream_t)stream;
  if (h2o) hipLaunchKernelGGL(contact_h2o_kernel, dim3(T, B * nobj), dim3(CT_NT), 0, st, hand, traj, pts, (const int*)obj_num, h2o,
                              (int*)h2o_idx, T, V, nobj, P);
  if (o2h) hipLaunchKernelGGL(contact_o2h_kernel, dim3(T, B * nobj, (P + CT_CHUNK - 1) / CT_CHUNK), dim3(CT_NT), 0, st, hand, normals, traj,
                              pts, (const int*)obj_num, o2h, (int*)o2h_idx, T, V, nobj, P);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(TAMF_ERR_HIP, hipGetErrorString(e));
  return 0;
}

extern "C" int tamf_contact_backward(const float* hand, const float* traj, const float* pts, const int32_t* obj_num, int32_t B, int32_t T,
                                     int32_t V, int32_t nobj, int32_t P, const int32_t* h2o_idx, const float* g_h2o, const float* o2h_signed,
                                     const int32_t* o2h_idx, const float* g_o2h, float* g_hand, void* stream) {
  if (!hand || !traj || !pts || !g_hand) return fail(TAMF_ERR_INVALID, "null argument: hand_verts, obj_traj, obj_points and g_hand_out are required");
  if (!g_h2o && !g_o2h) return fail(TAMF_ERR_INVALID, "no upstream gradient: g_h2o and g_o2h are both null");
  if (g_h2o && !h2o_idx) return fail(TAMF_ERR_INVALID, "null argument: g_h2o needs h2o_idx");
  if (g_o2h && (!o2h_signed || !o2h_idx)) return fail(TAMF_ERR_INVALID, "null argument: g_o2h needs o2h_signed and o2h_idx");
  const std::string bad = bad_shape(B, T, V, nobj, P);
  if (!bad.empty()) return fail(TAMF_ERR_INVALID, bad);
  hipLaunchKernelGGL(contact_backward_kernel, dim3(T, B), dim3(CT_NT), 0, (hipStream_t)stream, hand, traj, pts, (const int*)obj_num,
                     (const int*)h2o_idx, g_h2o, o2h_signed, (const int*)o2h_idx, g_o2h, g_hand, T, V, nobj, P);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(TAMF_ERR_HIP, hipGetErrorString(e));
  return 0;
}
