// libtamf_surface.so: the C-ABI of include/tamf_surface.h - the bit-defined surface sampler.  One translation unit.
#include "../../include/tamf_surface.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "tamf_surface.h"

static_assert(SURF_SCAN_BLOCK == TAMF_SURFACE_SCAN_BLOCK && SURF_ITEMS == TAMF_SURFACE_SCAN_ITEMS, "the header's summation order is the kernels'");

static thread_local std::string g_surface_error;

static int fail(int code, const std::string& msg) {
  g_surface_error = msg;
  return code;
}

static int hip_fail(const char* what, hipError_t e) { return fail(TAMF_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }

extern "C" const char* tamf_surface_last_error(void) { return g_surface_error.c_str(); }

// workspace: [cdf: F doubles | block carries: n_blocks doubles | total: 1 double], rounded up to 16 bytes
static inline int64_t scan_blocks(int64_t F) { return (F + SURF_SCAN_BLOCK - 1) / SURF_SCAN_BLOCK; }

extern "C" int64_t tamf_surface_workspace_bytes(int32_t F) {
  if (F < 1 || F > TAMF_SURFACE_MAX_FACES)
    return fail(TAMF_ERR_INVALID, "F = " + std::to_string(F) + " outside [1, " + std::to_string(TAMF_SURFACE_MAX_FACES) + "]");
  return (((int64_t)F + scan_blocks(F) + 1) * (int64_t)sizeof(double) + 15) & ~(int64_t)15;
}

extern "C" int tamf_surface_sample(const float* verts_dev, const int32_t* faces_dev, int32_t V, int32_t F, int64_t M, uint64_t seed, uint64_t key,
                                   int64_t first_sample, float* points_out_dev, float* normals_out_dev, int32_t* face_out_dev,
                                   void* workspace_dev, int64_t workspace_bytes, void* stream) {
  if (!verts_dev || !faces_dev || !points_out_dev || !workspace_dev) return fail(TAMF_ERR_INVALID, "null argument");
  if (V < 1 || F < 1 || F > TAMF_SURFACE_MAX_FACES || M < 1 || M > TAMF_SURFACE_MAX_SAMPLES)
    return fail(TAMF_ERR_INVALID, "bad shape (V = " + std::to_string(V) + ", F = " + std::to_string(F) + ", M = " + std::to_string(M) +
                                      "): V >= 1, 1 <= F <= 2^26, 1 <= M <= 2^31 - 1");
  if (first_sample < 0 || first_sample > INT64_MAX - M)
    return fail(TAMF_ERR_INVALID, "first_sample = " + std::to_string(first_sample) + ": the samples must lie in [0, 2^63)");
  const int64_t need = tamf_surface_workspace_bytes(F);
  if (workspace_bytes < need)
    return fail(TAMF_ERR_INVALID, "workspace too small: " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(need) + " needed for F = " + std::to_string(F));
  if ((uintptr_t)workspace_dev & 15) return fail(TAMF_ERR_INVALID, "workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int nb = (int)scan_blocks(F);
  double* cdf = (double*)workspace_dev;
  double* block_sum = cdf + F;
  hipLaunchKernelGGL(surface_area_scan_kernel, dim3((unsigned)nb), dim3(SURF_NT), 0, st, verts_dev, V, (const int*)faces_dev, F, cdf, block_sum);
  hipLaunchKernelGGL(surface_carry_kernel, dim3(1), dim3(64), 0, st, block_sum, nb);
  hipLaunchKernelGGL(surface_add_carry_kernel, dim3((unsigned)((F + SURF_NT - 1) / SURF_NT)), dim3(SURF_NT), 0, st, cdf, (const double*)block_sum, F);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail("the CDF launches", e);
  double total = 0.0;
  e = hipMemcpyAsync(&total, block_sum + nb, sizeof(double), hipMemcpyDeviceToHost, st);
  if (e != hipSuccess) return hip_fail("copy of the total area", e);
  e = hipStreamSynchronize(st);
  if (e != hipSuccess) return hip_fail("hipStreamSynchronize", e);
  if (!(total > 0.0) || !std::isfinite(total))
    return fail(TAMF_ERR_INVALID, total == 0.0 ? "the mesh has no face of positive area (total area 0): nothing to sample"
                                               : "the total area is not finite: scale the mesh");
  hipLaunchKernelGGL(surface_sample_kernel, dim3((unsigned)((M + SURF_NT - 1) / SURF_NT)), dim3(SURF_NT), 0, st, verts_dev, V, (const int*)faces_dev, F,
                     (const double*)cdf, total, (long)M, seed, key, (uint64_t)first_sample, points_out_dev, normals_out_dev, face_out_dev);
  e = hipGetLastError();
  if (e != hipSuccess) return hip_fail("the sampling launch", e);
  return 0;
}
