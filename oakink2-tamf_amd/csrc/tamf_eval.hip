// libtamf_eval.so: the C-ABI of include/tamf_eval.h - evaluation kernels without a context (the SIV score).  One translation unit.
#include "../../include/tamf_eval.h"

#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "tamf_voxel.h"

static thread_local std::string g_eval_error;

static int fail(int code, const std::string& msg) {
  g_eval_error = msg;
  return code;
}

extern "C" const char* tamf_eval_last_error(void) { return g_eval_error.c_str(); }

static inline dim3 grid1d(long n, int block = 256) { return dim3((unsigned)((n + block - 1) / block)); }

extern "C" int tamf_voxelize_lattice(const double* verts_dev, const int32_t* faces_dev, int32_t n_faces, const double* ticks_dev,
                                     int32_t R, const double* scale3, const double* translate3, int32_t hash_resolution,
                                     double* tri_workspace_dev, uint8_t* mask_out_dev, void* stream) {
  if (!verts_dev || !faces_dev || !ticks_dev || !scale3 || !translate3 || !tri_workspace_dev || !mask_out_dev)
    return fail(TAMF_ERR_INVALID, "null argument");
  if (R < 2 || R > 512) return fail(TAMF_ERR_INVALID, "R = " + std::to_string(R) + " outside [2, 512]");
  if (n_faces < 1 || hash_resolution < 2)
    return fail(TAMF_ERR_INVALID, "bad shape (F = " + std::to_string(n_faces) + ", hash_resolution = " + std::to_string(hash_resolution) + ")");
  hipStream_t st = (hipStream_t)stream;
  const double sx = scale3[0], sy = scale3[1], sz = scale3[2], tx = translate3[0], ty = translate3[1], tz = translate3[2];
  hipLaunchKernelGGL(mesh_prepare_kernel, grid1d(n_faces), dim3(256), 0, st, verts_dev, (const int*)faces_dev, n_faces, sx, sy, sz, tx, ty,
                     tz, tri_workspace_dev);
  const dim3 grid((unsigned)(((long)R * R + VOX_COLS - 1) / VOX_COLS));
  if (R <= 128)
    hipLaunchKernelGGL((voxelize_lattice_kernel<2>), grid, dim3(256), 0, st, (const double*)tri_workspace_dev, n_faces, ticks_dev, R, sx, sy,
                       sz, tx, ty, tz, (double)hash_resolution, mask_out_dev);
  else
    hipLaunchKernelGGL((voxelize_lattice_kernel<8>), grid, dim3(256), 0, st, (const double*)tri_workspace_dev, n_faces, ticks_dev, R, sx, sy,
                       sz, tx, ty, tz, (double)hash_resolution, mask_out_dev);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(TAMF_ERR_HIP, hipGetErrorString(e));
  return 0;
}

// workspace of tamf_mesh_contains_count: [M boxes | M * F triangle records | J job records]
static inline int64_t count_ws_box(int64_t M) { return M * CNT_BOX * (int64_t)sizeof(double); }
static inline int64_t count_ws_tc(int64_t M, int64_t F) { return M * F * MESH_TC * (int64_t)sizeof(double); }

extern "C" int64_t tamf_mesh_contains_count_workspace(int32_t M, int32_t F, int32_t J) {
  if (M < 1 || F < 1 || J < 1) return fail(TAMF_ERR_INVALID, "bad shape");
  return count_ws_box(M) + count_ws_tc(M, F) + (int64_t)J * (int64_t)sizeof(CountJob);
}

// The job records are packed on the host and copied with one hipMemcpyAsync from pageable memory: the runtime has read the source
// when the call returns, so the calling thread's buffer can be reused by its next call.  (Such a copy is stream-ordered: the runtime
// may hold the host until the work queued earlier on `stream` has drained.  The device is not synchronised.)
static thread_local std::vector<CountJob> g_jobs;

extern "C" int tamf_mesh_contains_count(const float* verts_dev, int32_t M, int32_t V, const int32_t* faces_dev, int32_t F,
                                        const double* points_dev, int64_t P_total, int32_t J, const int32_t* mesh_id_host,
                                        const double* transf_host, const int64_t* pt_off_host, const int64_t* pt_len_host,
                                        int32_t hash_resolution, void* workspace_dev, int64_t workspace_bytes, int64_t* count_out_dev,
                                        void* stream) {
  if (!verts_dev || !faces_dev || !mesh_id_host || !transf_host || !pt_off_host || !pt_len_host || !workspace_dev || !count_out_dev)
    return fail(TAMF_ERR_INVALID, "null argument");
  if (M < 1 || M > 65535 || V < 1 || F < 1 || J < 1 || P_total < 0 || hash_resolution < 2)
    return fail(TAMF_ERR_INVALID, "bad shape (M = " + std::to_string(M) + ", V = " + std::to_string(V) + ", F = " + std::to_string(F) +
                                      ", J = " + std::to_string(J) + ", P_total = " + std::to_string(P_total) + ")");
  if (P_total > 0 && !points_dev) return fail(TAMF_ERR_INVALID, "null argument");
  if (workspace_bytes < tamf_mesh_contains_count_workspace(M, F, J)) return fail(TAMF_ERR_INVALID, "workspace too small");
  if ((uintptr_t)workspace_dev & 15) return fail(TAMF_ERR_INVALID, "workspace must be 16-byte aligned");
  long long nblk = 0;
  for (int j = 0; j < J; ++j) {
    if (mesh_id_host[j] < 0 || mesh_id_host[j] >= M)
      return fail(TAMF_ERR_INVALID, "mesh_id[" + std::to_string(j) + "] = " + std::to_string(mesh_id_host[j]) + " outside [0, M)");
    const int64_t off = pt_off_host[j], len = pt_len_host[j];
    if (off < 0 || len < 0 || off > P_total || len > P_total - off)
      return fail(TAMF_ERR_INVALID, "slice of job " + std::to_string(j) + " [" + std::to_string(off) + ", +" + std::to_string(len) +
                                        ") leaves the " + std::to_string(P_total) + " points");
    nblk += (len + CNT_CHUNK - 1) / CNT_CHUNK;
  }
  if (nblk > 0x7fffffffLL) return fail(TAMF_ERR_INVALID, "too many points for one call: split the jobs");
  g_jobs.resize((size_t)J);
  CountJob* rec = g_jobs.data();
  const size_t job_bytes = (size_t)J * sizeof(CountJob);
  long long b0 = 0;
  for (int j = 0; j < J; ++j) {
    std::memcpy(rec[j].tr, transf_host + (size_t)j * 12, 12 * sizeof(double));
    rec[j].off = pt_off_host[j];
    rec[j].len = pt_len_host[j];
    rec[j].blk0 = b0;
    rec[j].mesh = mesh_id_host[j];
    rec[j].pad = 0;
    b0 += (pt_len_host[j] + CNT_CHUNK - 1) / CNT_CHUNK;
  }
  hipStream_t st = (hipStream_t)stream;
  double* box = (double*)workspace_dev;
  double* tc = (double*)((char*)workspace_dev + count_ws_box(M));
  CountJob* jobs = (CountJob*)((char*)workspace_dev + count_ws_box(M) + count_ws_tc(M, F));
  hipError_t e = hipMemcpyAsync(jobs, rec, job_bytes, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return fail(TAMF_ERR_HIP, std::string("job copy: ") + hipGetErrorString(e));
  e = hipMemsetAsync(count_out_dev, 0, (size_t)J * sizeof(int64_t), st);
  if (e != hipSuccess) return fail(TAMF_ERR_HIP, std::string("hipMemsetAsync: ") + hipGetErrorString(e));
  if (nblk == 0) return 0;
  hipLaunchKernelGGL(mesh_box_kernel, dim3(M), dim3(256), 0, st, verts_dev, V, (const int*)faces_dev, F, (double)hash_resolution, box);
  hipLaunchKernelGGL(mesh_prepare_batched_kernel, dim3((F + 255) / 256, M), dim3(256), 0, st, verts_dev, V, (const int*)faces_dev, F,
                     (const double*)box, tc);
  hipLaunchKernelGGL(mesh_contains_count_kernel, dim3((unsigned)nblk), dim3(256), 0, st, (const double*)box, (const double*)tc, F,
                     (const CountJob*)jobs, J, points_dev, (double)hash_resolution, (unsigned long long*)count_out_dev);
  e = hipGetLastError();
  if (e != hipSuccess) return fail(TAMF_ERR_HIP, hipGetErrorString(e));
  return 0;
}
