// Kernels of the Solid Intersection Volume score (libtamf_eval.so, include/tamf_eval.h): the inside test of tamf_geom.h's
// mesh_contains_kernel in two other work decompositions.  Same 16-double triangle records (tamf_mesh.h), same float64 expressions
// per (point, triangle), no fused multiply-adds: the booleans are those of mesh_contains_kernel.
//
//   voxelize_lattice_kernel      points of an R^3 lattice: the 2D test and the intersection depth depend on the column (i, j) only,
//                                so a wave's lanes sweep the triangles once per column and only the rare hits touch the R points
//   mesh_contains_count_kernel   J jobs (hand mesh, rigid transform, slice of object points) in one launch, reduced to counts
#pragma once
#include "tamf_mesh.h"

#pragma clang fp contract(off)

// ---- lattice ----------------------------------------------------------------------------------------------------------------
// Work group: 4 waves, VOX_CPW columns per wave (col = i * R + j; 16 consecutive columns per group).  Triangle records are staged
// VOX_TILE at a time, field-major: field k of triangle j at tile[k * VOX_LD + j].  VOX_LD = VOX_TILE + 2 doubles puts the 16 fields
// of one triangle 4 banks apart and neighbouring triangles 2 banks apart, so the staging writes (consecutive record doubles per
// lane) and the sweep's reads (consecutive triangles per lane) are both free of bank conflicts.  Per 64 triangles a lane holds the 8
// doubles of ITS triangle's 2D test in registers and tests them against the wave's columns; the hits of a column come back as a
// ballot, and for every set bit all lanes read the hit's depth fields at one address (an LDS broadcast), evaluate the depth once
// and flip the above / below parity of their points k = lane + 64 s.  No atomics; a column's result does not depend on the tiling.
constexpr int VOX_TILE = 256;
constexpr int VOX_LD = VOX_TILE + 2;
constexpr int VOX_CPW = 4;
constexpr int VOX_COLS = 4 * VOX_CPW;

template <int KS>  // points per lane along k: R <= 64 * KS
__global__ __launch_bounds__(256) void voxelize_lattice_kernel(const double* __restrict__ tc, int F, const double* __restrict__ ticks,
                                                               int R, double sx, double sy, double sz, double tx, double ty,
                                                               double tz, double res, unsigned char* __restrict__ out) {
  __shared__ double tile[MESH_TC * VOX_LD];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long ncol = (long)R * R;
  const long col0 = (long)blockIdx.x * VOX_COLS + wave * VOX_CPW;
  double qx[VOX_CPW], qy[VOX_CPW];
  bool lcol[VOX_CPW];
#pragma unroll
  for (int c = 0; c < VOX_CPW; ++c) {
    const long col = col0 + c;
    const bool ok = col < ncol;
    const int i = ok ? (int)(col / R) : 0, j = ok ? (int)(col % R) : 0;
    qx[c] = sx * ticks[i * 3 + 0] + tx;
    qy[c] = sy * ticks[j * 3 + 1] + ty;
    // the column's share of mesh_contains_kernel's `live`: inside the rescaled box and inside the hash grid
    lcol[c] = ok && qx[c] >= 0.0 && qx[c] <= res && qy[c] >= 0.0 && qy[c] <= res && qx[c] < res && qy[c] < res;
  }
  double qz[KS];
  bool lz[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int k = lane + 64 * s;
    qz[s] = sz * ticks[(k < R ? k : 0) * 3 + 2] + tz;
    lz[s] = k < R && qz[s] >= 0.0 && qz[s] <= res;
  }
  unsigned par[VOX_CPW];  // bit s: parity of the intersections at or above point s; bit 16 + s: of those below
#pragma unroll
  for (int c = 0; c < VOX_CPW; ++c) par[c] = 0u;

  for (int f0 = 0; f0 < F; f0 += VOX_TILE) {
    const int nt = F - f0 < VOX_TILE ? F - f0 : VOX_TILE;
    __syncthreads();
    for (int e = threadIdx.x; e < nt * MESH_TC; e += 256) tile[(e & (MESH_TC - 1)) * VOX_LD + (e >> 4)] = tc[(long)f0 * MESH_TC + e];
    __syncthreads();
    for (int sub = 0; sub < nt; sub += 64) {
      const bool has = sub + lane < nt;
      const double* cj = tile + (has ? sub + lane : 0);
      const double c0 = cj[0], c1 = cj[VOX_LD], c2 = cj[2 * VOX_LD], c3 = cj[3 * VOX_LD], c4 = cj[4 * VOX_LD], c5 = cj[5 * VOX_LD],
                   c6 = cj[6 * VOX_LD], adet = cj[7 * VOX_LD];
#pragma unroll
      for (int c = 0; c < VOX_CPW; ++c) {
        const double y0 = qx[c] - c0, y1 = qy[c] - c1;
        const double u = (c5 * y0 - c3 * y1) * c6;
        const double v = (-c4 * y0 + c2 * y1) * c6;
        const double s = u + v;
        const bool hit = has && lcol[c] && adet != 0.0 && 0.0 < u && u < adet && 0.0 < v && v < adet && 0.0 < s && s < adet;
        unsigned long long m = __ballot(hit);
        while (m) {  // (uniform: every lane walks the same hits)
          const double* ch = tile + sub + (__ffsll((long long)m) - 1);
          m &= m - 1;
          const double an = ch[11 * VOX_LD];
          if (an == 0.0) continue;
          const double alpha = ch[8 * VOX_LD] * (ch[12 * VOX_LD] - qx[c]) + ch[9 * VOX_LD] * (ch[13 * VOX_LD] - qy[c]);
          const double depth = ch[14 * VOX_LD] + alpha * ch[10 * VOX_LD];
#pragma unroll
          for (int s2 = 0; s2 < KS; ++s2) {
            const double zq = qz[s2] * an;
            if (depth >= zq) par[c] ^= 1u << s2;
            else if (depth < zq) par[c] ^= 0x10000u << s2;
          }
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < VOX_CPW; ++c) {
    const long col = col0 + c;
    if (col >= ncol) continue;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int k = lane + 64 * s;
      if (k < R) out[col * R + k] = (unsigned char)(lcol[c] && lz[s] && ((par[c] >> s) & 1u) && ((par[c] >> (16 + s)) & 1u));
    }
  }
}

// ---- batched counts ---------------------------------------------------------------------------------------------------------
// per mesh: scale3 | translate3 of the rescaling to the hash grid, over the vertices the faces reference (inside_mesh.py:20-24).
// min / max are exact whatever the order; the f32 -> f64 conversion is exact; the division is IEEE.
constexpr int CNT_BOX = 8;  // doubles per mesh: sx sy sz tx ty tz - -
__global__ __launch_bounds__(256) void mesh_box_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                                       double res, double* __restrict__ box) {
  __shared__ double red[6][4];
  const int m = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* v = verts + (long)m * V * 3;
  double lo[3] = {__builtin_inf(), __builtin_inf(), __builtin_inf()}, hi[3] = {-__builtin_inf(), -__builtin_inf(), -__builtin_inf()};
  for (int e = threadIdx.x; e < 3 * F; e += 256) {
    const float* p = v + (long)faces[e] * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const double x = (double)p[k];
      lo[k] = x < lo[k] ? x : lo[k];
      hi[k] = x > hi[k] ? x : hi[k];
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    for (int d = 32; d; d >>= 1) {
      const double a = __shfl_xor(lo[k], d), b = __shfl_xor(hi[k], d);
      lo[k] = a < lo[k] ? a : lo[k];
      hi[k] = b > hi[k] ? b : hi[k];
    }
    if (lane == 0) { red[k][wave] = lo[k]; red[3 + k][wave] = hi[k]; }
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int k = threadIdx.x;
    double a = red[k][0], b = red[3 + k][0];
    for (int w = 1; w < 4; ++w) {
      a = red[k][w] < a ? red[k][w] : a;
      b = red[3 + k][w] > b ? red[3 + k][w] : b;
    }
    const double scale = (res - 1.0) / (b - a);
    box[(long)m * CNT_BOX + k] = scale;
    box[(long)m * CNT_BOX + 3 + k] = 0.5 - scale * a;
  }
}

// mesh_prepare_kernel for M float32 meshes sharing `faces`, the rescaling read from `box`: grid (ceil(F / 256), M)
__global__ void mesh_prepare_batched_kernel(const float* __restrict__ verts, int V, const int* __restrict__ faces, int F,
                                            const double* __restrict__ box, double* __restrict__ tc) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x, m = blockIdx.y;
  if (f >= F) return;
  const double* bx = box + (long)m * CNT_BOX;
  double t[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float* v = verts + ((long)m * V + faces[f * 3 + k]) * 3;
    t[k][0] = bx[0] * (double)v[0] + bx[3];
    t[k][1] = bx[1] * (double)v[1] + bx[4];
    t[k][2] = bx[2] * (double)v[2] + bx[5];
  }
  mesh_record(t, tc + ((long)m * F + f) * MESH_TC);
}

// One job = (mesh, rigid transform, slice of the object-frame points); the host lays the jobs' chunks of CNT_CHUNK points end to
// end over the grid: blk0 = first work group of the job (an empty job shares its successor's).
struct CountJob {
  double tr[12];  // rows of [R | t]
  long long off, len, blk0;
  int mesh, pad;
};
static_assert(sizeof(CountJob) == 128, "job record layout");
constexpr int CNT_PPT = 2;  // points per thread: one LDS broadcast of a triangle serves both
constexpr int CNT_CHUNK = 256 * CNT_PPT;
constexpr int CNT_TILE = 64;

__global__ __launch_bounds__(256) void mesh_contains_count_kernel(const double* __restrict__ box, const double* __restrict__ tc_all,
                                                                  int F, const CountJob* __restrict__ jobs, int J,
                                                                  const double* __restrict__ pts, double res,
                                                                  unsigned long long* __restrict__ count) {
  __shared__ double tile[CNT_TILE * MESH_TC];
  const long long b = blockIdx.x;
  int jl = 0, jh = J - 1;  // the last job whose first work group is <= b (it is never an empty one)
  while (jl < jh) {
    const int mid = (jl + jh + 1) >> 1;
    if (jobs[mid].blk0 <= b) jl = mid;
    else jh = mid - 1;
  }
  const CountJob* jb = jobs + jl;
  const long long base = (b - jb->blk0) * CNT_CHUNK, len = jb->len;
  const double* bx = box + (long)jb->mesh * CNT_BOX;
  const double* tc = tc_all + (long)jb->mesh * F * MESH_TC;
  double qx[CNT_PPT], qy[CNT_PPT], qz[CNT_PPT];
  bool live[CNT_PPT];
  bool any = false;
#pragma unroll
  for (int p = 0; p < CNT_PPT; ++p) {
    const long long idx = base + threadIdx.x + 256 * p;
    qx[p] = qy[p] = qz[p] = 0.0;
    live[p] = false;
    if (idx < len) {
      const double* pp = pts + (jb->off + idx) * 3;
      const double x = pp[0], y = pp[1], z = pp[2];
      const double wx = ((jb->tr[0] * x + jb->tr[1] * y) + jb->tr[2] * z) + jb->tr[3];
      const double wy = ((jb->tr[4] * x + jb->tr[5] * y) + jb->tr[6] * z) + jb->tr[7];
      const double wz = ((jb->tr[8] * x + jb->tr[9] * y) + jb->tr[10] * z) + jb->tr[11];
      qx[p] = bx[0] * wx + bx[3];
      qy[p] = bx[1] * wy + bx[4];
      qz[p] = bx[2] * wz + bx[5];
      live[p] = qx[p] >= 0.0 && qx[p] <= res && qy[p] >= 0.0 && qy[p] <= res && qz[p] >= 0.0 && qz[p] <= res && qx[p] < res && qy[p] < res;
    }
    any = any || live[p];
  }
  // most object points of a frame lie outside the hand's box: a work group without a live point reads no triangle
  if (!__syncthreads_or(any)) return;
  unsigned above[CNT_PPT], below[CNT_PPT];
#pragma unroll
  for (int p = 0; p < CNT_PPT; ++p) above[p] = below[p] = 0u;
  for (int f0 = 0; f0 < F; f0 += CNT_TILE) {
    const int nt = F - f0 < CNT_TILE ? F - f0 : CNT_TILE;
    __syncthreads();
    for (int k = threadIdx.x; k < nt * MESH_TC; k += 256) tile[k] = tc[(long)f0 * MESH_TC + k];
    __syncthreads();
    if (!any) continue;
    for (int j = 0; j < nt; ++j) {
      const double* c = tile + j * MESH_TC;
      const double adet = c[7];
      if (adet == 0.0) continue;
#pragma unroll
      for (int p = 0; p < CNT_PPT; ++p) {
        if (!live[p]) continue;
        const double y0 = qx[p] - c[0], y1 = qy[p] - c[1];
        const double u = (c[5] * y0 - c[3] * y1) * c[6];
        const double v = (-c[4] * y0 + c[2] * y1) * c[6];
        const double s = u + v;
        if (!(0.0 < u && u < adet && 0.0 < v && v < adet && 0.0 < s && s < adet)) continue;
        const double an = c[11];
        if (an == 0.0) continue;
        const double alpha = c[8] * (c[12] - qx[p]) + c[9] * (c[13] - qy[p]);
        const double depth = c[14] + alpha * c[10];
        const double zq = qz[p] * an;
        if (depth >= zq) ++above[p];
        else if (depth < zq) ++below[p];
      }
    }
  }
  unsigned n = 0;
#pragma unroll
  for (int p = 0; p < CNT_PPT; ++p) n += (unsigned)__popcll(__ballot(live[p] && (above[p] & 1u) && (below[p] & 1u)));
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(count + jl, (unsigned long long)n);  // integer: order-independent
}

#pragma clang fp contract(fast)
