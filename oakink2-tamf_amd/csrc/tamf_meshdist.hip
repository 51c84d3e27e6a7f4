// libtamf_meshdist.so: the C-ABI of include/tamf_meshdist.h - the exact point-to-mesh distance.  One translation unit.
#include "../../include/tamf_meshdist.h"

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "tamf_meshdist.h"

static_assert(MD_TILE == TAMF_MESHDIST_TILE && MD_MARGIN == TAMF_MESHDIST_BOX_MARGIN, "the header's constants are the kernels'");
static_assert(MD_TC == MESH_TC, "the inside test's record");

static thread_local std::string g_meshdist_error;

static int fail(int code, const std::string& msg) {
  g_meshdist_error = msg;
  return code;
}

static int hip_fail(const char* what, hipError_t e) { return fail(TAMF_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }

extern "C" const char* tamf_meshdist_last_error(void) { return g_meshdist_error.c_str(); }

extern "C" int64_t tamf_meshdist_workspace(int32_t M, const int64_t* vert_off_host, const int64_t* face_off_host, const int64_t* perm_off_host) {
  MdLayout L;
  const std::string err = md_layout(M, vert_off_host, face_off_host, perm_off_host, L);
  if (!err.empty()) return fail(TAMF_ERR_INVALID, err);
  return L.bytes;
}

// Packed on the host and copied with one hipMemcpyAsync from pageable memory: the runtime has read the source when the call returns,
// so the calling thread's buffer can be reused by its next call (the copy is stream-ordered; the device is not synchronised).
static thread_local std::vector<unsigned char> g_pack;
static thread_local std::vector<MdJob> g_jobs;

extern "C" int tamf_meshdist_prepare(const double* verts_host, const int32_t* faces_host, int32_t M, const int64_t* vert_off_host,
                                     const int64_t* face_off_host, const int32_t* perm_host, const int64_t* perm_off_host,
                                     const double* scale3_host, const double* translate3_host, int32_t hash_resolution, void* workspace_dev,
                                     int64_t workspace_bytes, void* stream) {
  MdLayout L;
  std::string err = md_layout(M, vert_off_host, face_off_host, perm_off_host, L);
  if (!err.empty()) return fail(TAMF_ERR_INVALID, err);
  if (!workspace_dev) return fail(TAMF_ERR_INVALID, "null argument");
  if (workspace_bytes < L.bytes)
    return fail(TAMF_ERR_INVALID, "workspace too small: " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(L.bytes) + " needed");
  if ((uintptr_t)workspace_dev & 15) return fail(TAMF_ERR_INVALID, "workspace must be 16-byte aligned");
  err = md_pack(L, verts_host, faces_host, vert_off_host, face_off_host, perm_host, perm_off_host, scale3_host, translate3_host, hash_resolution, g_pack);
  if (!err.empty()) return fail(TAMF_ERR_INVALID, err);
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(workspace_dev, g_pack.data(), (size_t)L.upload_bytes, hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return hip_fail("copy of the packed meshes", e);
  for (int m = 0; m < M; ++m) {
    const int F = (int)(face_off_host[m + 1] - face_off_host[m]);
    hipLaunchKernelGGL(md_inside_prepare_kernel, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, st, (char*)workspace_dev, m);
  }
  e = hipGetLastError();
  if (e != hipSuccess) return hip_fail("the prepare launches", e);
  return 0;
}

extern "C" int64_t tamf_meshdist_points_workspace(int32_t J) {
  if (J < 1) return fail(TAMF_ERR_INVALID, "J = " + std::to_string(J) + " < 1");
  return (int64_t)J * (int64_t)sizeof(MdJob);
}

extern "C" int tamf_meshdist_points(const void* prepared_dev, int32_t M, const float* points_dev, int64_t P_total, int32_t J,
                                    const int32_t* mesh_id_host, const double* transf_host, const int64_t* pt_off_host,
                                    const int64_t* pt_len_host, uint32_t flags, void* jobs_workspace_dev, int64_t jobs_workspace_bytes,
                                    double* dist_out_dev, int32_t* face_out_dev, uint8_t* inside_out_dev, void* stream) {
  if (!prepared_dev || !jobs_workspace_dev || !dist_out_dev || !face_out_dev || (P_total > 0 && !points_dev))
    return fail(TAMF_ERR_INVALID, "null argument");
  if (flags & ~TAMF_MESHDIST_NO_CULL) return fail(TAMF_ERR_INVALID, "unknown flags " + std::to_string(flags));
  long long nblk = 0, n_out = 0;
  const std::string err = md_jobs(M, P_total, J, mesh_id_host, transf_host, pt_off_host, pt_len_host, g_jobs, nblk, n_out);
  if (!err.empty()) return fail(TAMF_ERR_INVALID, err);
  if (jobs_workspace_bytes < (int64_t)J * (int64_t)sizeof(MdJob)) return fail(TAMF_ERR_INVALID, "jobs workspace too small");
  if ((uintptr_t)jobs_workspace_dev & 15) return fail(TAMF_ERR_INVALID, "jobs workspace must be 16-byte aligned");
  if (nblk == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(jobs_workspace_dev, g_jobs.data(), (size_t)J * sizeof(MdJob), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return hip_fail("job copy", e);
  hipLaunchKernelGGL(meshdist_points_kernel, dim3((unsigned)nblk), dim3(MD_NT), 0, st, (const char*)prepared_dev, (const MdJob*)jobs_workspace_dev, J,
                     points_dev, flags, dist_out_dev, (int*)face_out_dev, inside_out_dev);
  e = hipGetLastError();
  if (e != hipSuccess) return hip_fail("the points launch", e);
  return 0;
}

extern "C" int tamf_meshdist_lattice(const void* prepared_dev, int32_t M, int32_t mesh, const double* ticks_dev, int32_t R, uint32_t flags,
                                     double* dist_out_dev, void* stream) {
  if (!prepared_dev || !ticks_dev || !dist_out_dev) return fail(TAMF_ERR_INVALID, "null argument");
  if (M < 1 || M > TAMF_MESHDIST_MAX_MESHES || mesh < 0 || mesh >= M)
    return fail(TAMF_ERR_INVALID, "mesh = " + std::to_string(mesh) + " outside [0, M = " + std::to_string(M) + ")");
  if (R < 2 || R > 512) return fail(TAMF_ERR_INVALID, "R = " + std::to_string(R) + " outside [2, 512]");
  if (flags & ~TAMF_MESHDIST_NO_CULL) return fail(TAMF_ERR_INVALID, "unknown flags " + std::to_string(flags));
  const long nb = (long)((R + MD_BI - 1) / MD_BI) * ((R + MD_BJ - 1) / MD_BJ) * ((R + MD_BK - 1) / MD_BK);
  hipLaunchKernelGGL(meshdist_lattice_kernel, dim3((unsigned)nb), dim3(MD_NT), 0, (hipStream_t)stream, (const char*)prepared_dev, mesh, ticks_dev, R, flags,
                     dist_out_dev);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail("the lattice launch", e);
  return 0;
}
