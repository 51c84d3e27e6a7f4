// libtamf_winding.so: the C-ABI of include/tamf_winding.h - the generalized winding number of a triangle mesh.  One translation unit.
//
// A work group is 256 points that lie together - a brick of 8 x 8 x 4 lattice points, or a run of 256 points of one job - one point
// per lane.  Face records (9 doubles: a, b, c) go through LDS WN_TILE at a time; every lane reads the same record at the same time (an
// LDS broadcast, no bank conflicts) and keeps its running sum in a register.  A chunk's partial is always formed by wn_chunk_sum, in
// index order from +0; the lattice kernel and the looped points kernel add the partials in a register, the spread points kernel
// writes its one partial to memory and wn_reduce_kernel adds them in the same order: the same tree, the same bits.
#include "../../include/tamf_winding.h"

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "tamf_winding_host.h"

static_assert(WN_CHUNK == TAMF_WINDING_CHUNK && WN_FORCE_LOOP == TAMF_WINDING_FORCE_LOOP && WN_FORCE_SPREAD == TAMF_WINDING_FORCE_SPREAD,
              "the header's constants are the kernels'");

#pragma clang fp contract(off)

#define WN_DEV static __device__ __forceinline__

WN_DEV double wn_dot(double ux, double uy, double uz, double vx, double vy, double vz) { return (ux * vx + uy * vy) + uz * vz; }

// omega of one record at p (van Oosterom and Strackee)
WN_DEV double wn_omega(double px, double py, double pz, const double* __restrict__ r) {
  const double ax = r[0] - px, ay = r[1] - py, az = r[2] - pz;
  const double bx = r[3] - px, by = r[4] - py, bz = r[5] - pz;
  const double cx = r[6] - px, cy = r[7] - py, cz = r[8] - pz;
  const double la = __dsqrt_rn(wn_dot(ax, ay, az, ax, ay, az)), lb = __dsqrt_rn(wn_dot(bx, by, bz, bx, by, bz)), lc = __dsqrt_rn(wn_dot(cx, cy, cz, cx, cy, cz));
  const double det = wn_dot(ax, ay, az, by * cz - bz * cy, bz * cx - bx * cz, bx * cy - by * cx);
  const double den = ((la * lb) * lc + wn_dot(ax, ay, az, bx, by, bz) * lc) + (wn_dot(bx, by, bz, cx, cy, cz) * la + wn_dot(cx, cy, cz, ax, ay, az) * lb);
  return 2.0 * atan2(det, den);
}

// The partial of `count` records starting at `recs` (global memory), for this lane's point: the serial sum in index order from +0.
// Called by every thread of the work group (the barriers), whether its point is real or a copy of a neighbour's.
WN_DEV double wn_chunk_sum(const double* __restrict__ recs, int count, double px, double py, double pz, double* __restrict__ sh) {
  double part = 0.0;
  for (int t0 = 0; t0 < count; t0 += WN_TILE) {
    const int n = count - t0 < WN_TILE ? count - t0 : WN_TILE;
    __syncthreads();  // (the previous tile has been read by every lane)
    for (int i = threadIdx.x; i < n * WN_REC; i += WN_NT) sh[i] = recs[(long long)t0 * WN_REC + i];
    __syncthreads();
    for (int j = 0; j < n; ++j) part = part + wn_omega(px, py, pz, sh + j * WN_REC);
  }
  return part;
}

WN_DEV void wn_store(double total, long long o, double* __restrict__ w_out, unsigned char* __restrict__ inside_out) {
  const double w = total / TAMF_WINDING_FOUR_PI;
  w_out[o] = w;
  if (inside_out) inside_out[o] = (unsigned char)(fabs(w) > 0.5);  // (false for a NaN)
}

// ---- J jobs.  SPREAD: work group = (block of 256 points, chunk), the partial goes to memory.  Otherwise: every chunk in turn. ----------
template <bool SPREAD>
__global__ __launch_bounds__(WN_NT) void winding_points_kernel(const char* __restrict__ base, const WnJob* __restrict__ jobs, int J,
                                                               const float* __restrict__ pts, int max_chunks, long long n_out,
                                                               double* __restrict__ partial, double* __restrict__ w_out,
                                                               unsigned char* __restrict__ inside_out) {
  __shared__ double sh[WN_TILE * WN_REC];
  const long long b = SPREAD ? (long long)(blockIdx.x / (unsigned)max_chunks) : (long long)blockIdx.x;
  const int chunk = SPREAD ? (int)(blockIdx.x % (unsigned)max_chunks) : 0;
  int jl = 0, jh = J - 1;  // the last job whose first block is <= b (it is never an empty one)
  while (jl < jh) {
    const int mid = (jl + jh + 1) >> 1;
    if (jobs[mid].blk0 <= b) jl = mid;
    else jh = mid - 1;
  }
  const WnJob* jb = jobs + jl;
  const WnMesh* m = (const WnMesh*)base + jb->mesh;
  const int K = m->K, nchunks = m->nchunks;
  if (SPREAD && chunk >= nchunks) return;  // (uniform: before any barrier)
  const double* recs = (const double*)(base + m->rec_off);
  const long long first = (b - jb->blk0) * WN_NT, len = jb->len;
  const bool active = first + threadIdx.x < len;
  const long long idx = active ? first + threadIdx.x : first;  // (first < len: the block exists because of it)
  const float* pp = pts + (jb->off + idx) * 3;
  const double x = (double)pp[0], y = (double)pp[1], z = (double)pp[2];
  const double px = ((jb->tr[0] * x + jb->tr[1] * y) + jb->tr[2] * z) + jb->tr[3];
  const double py = ((jb->tr[4] * x + jb->tr[5] * y) + jb->tr[6] * z) + jb->tr[7];
  const double pz = ((jb->tr[8] * x + jb->tr[9] * y) + jb->tr[10] * z) + jb->tr[11];
  const long long o = jb->out0 + idx;
  if (SPREAD) {
    const long long f0 = (long long)chunk * WN_CHUNK;
    const int count = K - f0 < WN_CHUNK ? (int)(K - f0) : WN_CHUNK;
    const double part = wn_chunk_sum(recs + f0 * WN_REC, count, px, py, pz, sh);
    if (active) partial[(long long)chunk * n_out + o] = part;
  } else {
    double total = 0.0;
    for (int c = 0; c < nchunks; ++c) {
      const long long f0 = (long long)c * WN_CHUNK;
      const int count = K - f0 < WN_CHUNK ? (int)(K - f0) : WN_CHUNK;
      total = total + wn_chunk_sum(recs + f0 * WN_REC, count, px, py, pz, sh);
    }
    if (active) wn_store(total, o, w_out, inside_out);
  }
}

// the second launch of the spread route: one thread per output adds its partials in chunk order from +0
__global__ __launch_bounds__(WN_NT) void winding_reduce_kernel(const char* __restrict__ base, const WnJob* __restrict__ jobs, int J, int max_chunks,
                                                               long long n_out, const double* __restrict__ partial, double* __restrict__ w_out,
                                                               unsigned char* __restrict__ inside_out) {
  const long long o = (long long)blockIdx.x * WN_NT + threadIdx.x;
  if (o >= n_out) return;
  int jl = 0, jh = J - 1;  // the last job whose first output is <= o (it is never an empty one)
  while (jl < jh) {
    const int mid = (jl + jh + 1) >> 1;
    if (jobs[mid].out0 <= o) jl = mid;
    else jh = mid - 1;
  }
  const WnMesh* m = (const WnMesh*)base + jobs[jl].mesh;
  const int nchunks = m->nchunks < max_chunks ? m->nchunks : max_chunks;
  double total = 0.0;
  for (int c = 0; c < nchunks; ++c) total = total + partial[(long long)c * n_out + o];
  wn_store(total, o, w_out, inside_out);
}

// ---- one mesh on an R^3 lattice: bricks of 8 x 8 x 4 points, every chunk in turn ------------------------------------------------------
constexpr int WN_BI = 8, WN_BJ = 8, WN_BK = 4;
static_assert(WN_BI * WN_BJ * WN_BK == WN_NT, "one lattice point per lane");

__global__ __launch_bounds__(WN_NT) void winding_lattice_kernel(const char* __restrict__ base, int mesh, const double* __restrict__ ticks, int R,
                                                                double* __restrict__ w_out, unsigned char* __restrict__ inside_out) {
  __shared__ double sh[WN_TILE * WN_REC];
  const WnMesh* m = (const WnMesh*)base + mesh;
  const int K = m->K, nchunks = m->nchunks;
  const double* recs = (const double*)(base + m->rec_off);
  const int nbj = (R + WN_BJ - 1) / WN_BJ, nbk = (R + WN_BK - 1) / WN_BK;
  const int bk = blockIdx.x % nbk, bj = (blockIdx.x / nbk) % nbj, bi = blockIdx.x / (nbk * nbj);
  const int i = bi * WN_BI + (threadIdx.x >> 5), j = bj * WN_BJ + ((threadIdx.x >> 2) & 7), k = bk * WN_BK + (threadIdx.x & 3);
  const bool active = i < R && j < R && k < R;
  const double px = ticks[(i < R ? i : R - 1) * 3 + 0], py = ticks[(j < R ? j : R - 1) * 3 + 1], pz = ticks[(k < R ? k : R - 1) * 3 + 2];
  double total = 0.0;
  for (int c = 0; c < nchunks; ++c) {
    const long long f0 = (long long)c * WN_CHUNK;
    const int count = K - f0 < WN_CHUNK ? (int)(K - f0) : WN_CHUNK;
    total = total + wn_chunk_sum(recs + f0 * WN_REC, count, px, py, pz, sh);
  }
  if (active) wn_store(total, ((long long)i * R + j) * R + k, w_out, inside_out);
}

#pragma clang fp contract(fast)

// ---- the C-ABI ---------------------------------------------------------------------------------------------------------------------
static thread_local std::string g_winding_error;

static int fail(int code, const std::string& msg) {
  g_winding_error = msg;
  return code;
}

static int hip_fail(const char* what, hipError_t e) { return fail(TAMF_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }

extern "C" const char* tamf_winding_last_error(void) { return g_winding_error.c_str(); }

extern "C" int64_t tamf_winding_workspace(int32_t M, const int64_t* vert_off_host, const int64_t* face_off_host, const int64_t* valid_off_host) {
  WnLayout L;
  const std::string err = wn_layout(M, vert_off_host, face_off_host, valid_off_host, L);
  if (!err.empty()) return fail(TAMF_ERR_INVALID, err);
  return L.bytes;
}

// Packed on the host and copied with one hipMemcpyAsync from pageable memory: the runtime has read the source when the call returns,
// so the calling thread's buffer can be reused by its next call (the copy is stream-ordered; the device is not synchronised).
static thread_local std::vector<unsigned char> g_pack;
static thread_local std::vector<WnJob> g_jobs;

extern "C" int tamf_winding_prepare(const double* verts_host, const int32_t* faces_host, int32_t M, const int64_t* vert_off_host,
                                    const int64_t* face_off_host, const int32_t* valid_host, const int64_t* valid_off_host, void* workspace_dev,
                                    int64_t workspace_bytes, void* stream) {
  WnLayout L;
  std::string err = wn_layout(M, vert_off_host, face_off_host, valid_off_host, L);
  if (!err.empty()) return fail(TAMF_ERR_INVALID, err);
  if (!workspace_dev) return fail(TAMF_ERR_INVALID, "null argument");
  if (workspace_bytes < L.bytes)
    return fail(TAMF_ERR_INVALID, "workspace too small: " + std::to_string(workspace_bytes) + " bytes, " + std::to_string(L.bytes) + " needed");
  if ((uintptr_t)workspace_dev & 15) return fail(TAMF_ERR_INVALID, "workspace must be 16-byte aligned");
  err = wn_pack(L, verts_host, faces_host, vert_off_host, face_off_host, valid_host, valid_off_host, g_pack);
  if (!err.empty()) return fail(TAMF_ERR_INVALID, err);
  const hipError_t e = hipMemcpyAsync(workspace_dev, g_pack.data(), (size_t)L.bytes, hipMemcpyHostToDevice, (hipStream_t)stream);
  if (e != hipSuccess) return hip_fail("copy of the packed meshes", e);
  return 0;
}

extern "C" int64_t tamf_winding_points_workspace(int32_t J, int32_t M, const int32_t* mesh_id_host, const int64_t* pt_len_host,
                                                 const int64_t* valid_off_host, uint32_t flags) {
  long long nblk = 0, n_out = 0;
  int max_chunks = 1;
  std::string err = wn_sizes(M, J, mesh_id_host, pt_len_host, valid_off_host, nblk, n_out, max_chunks);
  if (!err.empty()) return fail(TAMF_ERR_INVALID, err);
  WnPlan P;
  err = wn_plan(J, nblk, n_out, max_chunks, flags, P);
  if (!err.empty()) return fail(TAMF_ERR_INVALID, err);
  return P.bytes;
}

extern "C" int tamf_winding_points(const void* prepared_dev, int32_t M, const float* points_dev, int64_t P_total, int32_t J,
                                   const int32_t* mesh_id_host, const double* transf_host, const int64_t* pt_off_host, const int64_t* pt_len_host,
                                   const int64_t* valid_off_host, uint32_t flags, void* jobs_workspace_dev, int64_t jobs_workspace_bytes,
                                   double* w_out_dev, uint8_t* inside_out_dev, void* stream) {
  if (!prepared_dev || !jobs_workspace_dev || !w_out_dev || (P_total > 0 && !points_dev)) return fail(TAMF_ERR_INVALID, "null argument");
  long long nblk = 0, n_out = 0;
  int max_chunks = 1;
  std::string err = wn_sizes(M, J, mesh_id_host, pt_len_host, valid_off_host, nblk, n_out, max_chunks);
  if (!err.empty()) return fail(TAMF_ERR_INVALID, err);
  err = wn_jobs(M, P_total, J, mesh_id_host, transf_host, pt_off_host, pt_len_host, valid_off_host, g_jobs);
  if (!err.empty()) return fail(TAMF_ERR_INVALID, err);
  WnPlan P;
  err = wn_plan(J, nblk, n_out, max_chunks, flags, P);
  if (!err.empty()) return fail(TAMF_ERR_INVALID, err);
  if (jobs_workspace_bytes < P.bytes)
    return fail(TAMF_ERR_INVALID, "jobs workspace too small: " + std::to_string(jobs_workspace_bytes) + " bytes, " + std::to_string(P.bytes) + " needed");
  if ((uintptr_t)jobs_workspace_dev & 15) return fail(TAMF_ERR_INVALID, "jobs workspace must be 16-byte aligned");
  if (nblk == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemcpyAsync(jobs_workspace_dev, g_jobs.data(), (size_t)J * sizeof(WnJob), hipMemcpyHostToDevice, st);
  if (e != hipSuccess) return hip_fail("job copy", e);
  const WnJob* jobs = (const WnJob*)jobs_workspace_dev;
  double* partial = (double*)((char*)jobs_workspace_dev + P.partial_off);
  if (P.spread) {
    hipLaunchKernelGGL(winding_points_kernel<true>, dim3((unsigned)P.groups), dim3(WN_NT), 0, st, (const char*)prepared_dev, jobs, J, points_dev,
                       P.max_chunks, n_out, partial, w_out_dev, inside_out_dev);
    hipLaunchKernelGGL(winding_reduce_kernel, dim3((unsigned)((n_out + WN_NT - 1) / WN_NT)), dim3(WN_NT), 0, st, (const char*)prepared_dev, jobs, J,
                       P.max_chunks, n_out, (const double*)partial, w_out_dev, inside_out_dev);
  } else {
    hipLaunchKernelGGL(winding_points_kernel<false>, dim3((unsigned)P.groups), dim3(WN_NT), 0, st, (const char*)prepared_dev, jobs, J, points_dev,
                       P.max_chunks, n_out, partial, w_out_dev, inside_out_dev);
  }
  e = hipGetLastError();
  if (e != hipSuccess) return hip_fail("the points launch", e);
  return 0;
}

extern "C" int tamf_winding_lattice(const void* prepared_dev, int32_t M, int32_t mesh, const double* ticks_dev, int32_t R, double* w_out_dev,
                                    uint8_t* inside_out_dev, void* stream) {
  if (!prepared_dev || !ticks_dev || !w_out_dev) return fail(TAMF_ERR_INVALID, "null argument");
  if (M < 1 || M > TAMF_WINDING_MAX_MESHES || mesh < 0 || mesh >= M)
    return fail(TAMF_ERR_INVALID, "mesh = " + std::to_string(mesh) + " outside [0, M = " + std::to_string(M) + ")");
  if (R < 2 || R > 512) return fail(TAMF_ERR_INVALID, "R = " + std::to_string(R) + " outside [2, 512]");
  const long nb = (long)((R + WN_BI - 1) / WN_BI) * ((R + WN_BJ - 1) / WN_BJ) * ((R + WN_BK - 1) / WN_BK);
  hipLaunchKernelGGL(winding_lattice_kernel, dim3((unsigned)nb), dim3(WN_NT), 0, (hipStream_t)stream, (const char*)prepared_dev, mesh, ticks_dev, R,
                     w_out_dev, inside_out_dev);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail("the lattice launch", e);
  return 0;
}
