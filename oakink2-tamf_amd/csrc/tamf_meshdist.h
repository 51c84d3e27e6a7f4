// Kernels of libtamf_meshdist.so (include/tamf_meshdist.h holds the definition): the exact point-to-mesh distance in float64, and
// the inside test of tamf_geom.h's mesh_contains_kernel for the same query points (the 16-double records of tamf_mesh.h).
//
// A work group is 256 points that lie together - a brick of 8 x 8 x 4 lattice points, or a run of 256 points of one job - one point
// per lane.  Triangle tiles of MD_TILE records (10 doubles: a, b, c, original index) go through LDS one at a time; every lane reads
// the same record at the same time (an LDS broadcast) and keeps its (d2, f) in registers.  The region logic of the closest point is
// written with selects: the six region predicates give one region code, the code picks one numerator / denominator pair (one IEEE
// division per pair, not four), one base and one direction, so lanes in different regions run the same instructions.
// Culling (the header's bound) is decided per work group on values made uniform with readfirstlane: a skipped tile costs its box
// (six scalar loads) and ten flops; the largest best of the group is taken again only after a tile was swept.
#pragma once
#include "tamf_mesh.h"
#include "tamf_meshdist_host.h"

#pragma clang fp contract(off)

TAMF_DEV double md_dot(double ux, double uy, double uz, double vx, double vy, double vz) { return (ux * vx + uy * vy) + uz * vz; }

// (d2, f) of one record against the running best
TAMF_DEV void md_tri(double px, double py, double pz, const double* __restrict__ r, double& best, int& bestf) {
  const double ax = r[0], ay = r[1], az = r[2], bx = r[3], by = r[4], bz = r[5], cx = r[6], cy = r[7], cz = r[8];
  const int f = (int)__double_as_longlong(r[9]);
  const double abx = bx - ax, aby = by - ay, abz = bz - az, acx = cx - ax, acy = cy - ay, acz = cz - az;
  const double apx = px - ax, apy = py - ay, apz = pz - az;
  const double d1 = md_dot(abx, aby, abz, apx, apy, apz), d2 = md_dot(acx, acy, acz, apx, apy, apz);
  const double bpx = px - bx, bpy = py - by, bpz = pz - bz;
  const double d3 = md_dot(abx, aby, abz, bpx, bpy, bpz), d4 = md_dot(acx, acy, acz, bpx, bpy, bpz);
  const double cpx = px - cx, cpy = py - cy, cpz = pz - cz;
  const double d5 = md_dot(abx, aby, abz, cpx, cpy, cpz), d6 = md_dot(acx, acy, acz, cpx, cpy, cpz);
  const double vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
  const double e43 = d4 - d3, e56 = d5 - d6;
  // the first region that applies: 0 A, 1 B, 2 AB, 3 C, 4 AC, 5 BC, 6 interior
  int k = 6;
  k = (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0) ? 5 : k;
  k = (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) ? 4 : k;
  k = (d6 >= 0.0 && d5 <= d6) ? 3 : k;
  k = (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) ? 2 : k;
  k = (d3 >= 0.0 && d4 <= d3) ? 1 : k;
  k = (d1 <= 0.0 && d2 <= 0.0) ? 0 : k;
  const double num = k == 2 ? d1 : k == 4 ? d2 : k == 5 ? e43 : 1.0;
  const double den = k == 2 ? d1 - d3 : k == 4 ? d2 - d6 : k == 5 ? e43 + e56 : (va + vb) + vc;
  const double t = num / den;
  const double t1 = k == 6 ? vb * t : t, t2 = vc * t;
  const bool on_ac = k == 4, on_bc = k == 5, in = k == 6;
  const double ox = on_bc ? bx : ax, oy = on_bc ? by : ay, oz = on_bc ? bz : az;
  const double ex = on_ac ? acx : on_bc ? cx - bx : abx, ey = on_ac ? acy : on_bc ? cy - by : aby, ez = on_ac ? acz : on_bc ? cz - bz : abz;
  double qx = ox + ex * t1, qy = oy + ey * t1, qz = oz + ez * t1;
  const double ix = qx + acx * t2, iy = qy + acy * t2, iz = qz + acz * t2;
  qx = in ? ix : qx; qy = in ? iy : qy; qz = in ? iz : qz;
  qx = k == 0 ? ax : k == 1 ? bx : k == 3 ? cx : qx;
  qy = k == 0 ? ay : k == 1 ? by : k == 3 ? cy : qy;
  qz = k == 0 ? az : k == 1 ? bz : k == 3 ? cz : qz;
  const double dx = px - qx, dy = py - qy, dz = pz - qz;
  const double dd = md_dot(dx, dy, dz, dx, dy, dz);
  const bool win = dd < best || (dd == best && f < bestf);
  best = win ? dd : best;
  bestf = win ? f : bestf;
}

// the same value in every lane -> a scalar
TAMF_DEV double md_uniform(double v) {
  const long long b = __double_as_longlong(v);
  const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)b), hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(b >> 32));
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

// max / min over the work group's 256 lanes (exact, any order); `red` = 4 doubles of LDS.  Every lane gets the result, as a scalar.
template <bool MAX>
TAMF_DEV double md_group_reduce(double v, double* red) {
  for (int d = 32; d; d >>= 1) {
    const double o = __shfl_xor(v, d);
    v = MAX ? (o > v ? o : v) : (o < v ? o : v);
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double r = red[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) r = MAX ? (red[w] > r ? red[w] : r) : (red[w] < r ? red[w] : r);
  return md_uniform(r);
}

// the header's lower bound of d2 between the group's box and a tile's box, before the factor (1 - 2^-40)
TAMF_DEV double md_gap2(const double* __restrict__ bx, const double (&plo)[3], const double (&phi)[3]) {
  double g[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double u = bx[k] - phi[k], w = plo[k] - bx[3 + k];
    double m = u > w ? u : w;
    g[k] = m > 0.0 ? m : (m <= 0.0 ? 0.0 : m);  // (a NaN stays a NaN: the tile is never skipped)
  }
  return (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
}

struct MdShared {
  alignas(16) double tile[MD_TILE * MD_REC];
  double red[4];
  int redi[4];
};

TAMF_DEV void md_sweep_tile(const double* __restrict__ tiles, int t, double px, double py, double pz, double& best, int& bestf, MdShared& sh) {
  __syncthreads();
  const double* src = tiles + (long)t * (MD_TILE * MD_REC);
  for (int e = threadIdx.x; e < MD_TILE * MD_REC; e += MD_NT) sh.tile[e] = src[e];
  __syncthreads();
#pragma unroll 2
  for (int j = 0; j < MD_TILE; ++j) md_tri(px, py, pz, sh.tile + j * MD_REC, best, bestf);
}

// (d2, f) of the lane's point over all tiles of mesh `m`.  Every lane of the group calls this (an inactive lane carries a copy of an
// active lane's point or any finite point and is left out of the box and of the largest best).
TAMF_DEV void md_sweep(const char* __restrict__ base, const MdMesh* __restrict__ m, double px, double py, double pz, bool active, bool cull,
                       double& best, int& bestf, MdShared& sh) {
  const double* tiles = (const double*)(base + m->tiles_off);
  const double* boxes = (const double*)(base + m->boxes_off);
  const int nt = __builtin_amdgcn_readfirstlane(m->ntiles);
  best = __builtin_inf();
  bestf = 0x7fffffff;
  if (!cull) {
    for (int t = 0; t < nt; ++t) md_sweep_tile(tiles, t, px, py, pz, best, bestf, sh);
    return;
  }
  const double inf = __builtin_inf();
  double plo[3], phi[3];
  plo[0] = md_group_reduce<false>(active ? px : inf, sh.red);
  plo[1] = md_group_reduce<false>(active ? py : inf, sh.red);
  plo[2] = md_group_reduce<false>(active ? pz : inf, sh.red);
  phi[0] = md_group_reduce<true>(active ? px : -inf, sh.red);
  phi[1] = md_group_reduce<true>(active ? py : -inf, sh.red);
  phi[2] = md_group_reduce<true>(active ? pz : -inf, sh.red);
  // the seed: the tile whose box is nearest to the group's (the lowest index among equals; a NaN bound is never nearest)
  double sg = inf;
  int st = 0x7fffffff;
  for (int t = threadIdx.x; t < nt; t += MD_NT) {
    const double g = md_gap2(boxes + (long)t * MD_BOX, plo, phi);
    if (g < sg) { sg = g; st = t; }
  }
  const double gmin = md_group_reduce<false>(sg, sh.red);
  int cand = (sg == gmin) ? st : 0x7fffffff;
  for (int d = 32; d; d >>= 1) {
    const int o = __shfl_xor(cand, d);
    cand = o < cand ? o : cand;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh.redi[threadIdx.x >> 6] = cand;
  __syncthreads();
  int seed = sh.redi[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) seed = sh.redi[w] < seed ? sh.redi[w] : seed;
  seed = __builtin_amdgcn_readfirstlane(seed);
  if (seed < 0 || seed >= nt) seed = 0;  // (every bound a NaN)
  md_sweep_tile(tiles, seed, px, py, pz, best, bestf, sh);
  double gmax = md_group_reduce<true>(active ? best : 0.0, sh.red);
  for (int t = 0; t < nt; ++t) {
    if (t == seed) continue;
    const double lb = md_gap2(boxes + (long)t * MD_BOX, plo, phi) * (1.0 - 0x1p-40);
    if (lb > gmax) continue;  // (uniform: scalars on both sides)
    md_sweep_tile(tiles, t, px, py, pz, best, bestf, sh);
    gmax = md_group_reduce<true>(active ? best : 0.0, sh.red);
  }
}

// ---- the records of the inside test, one mesh per launch: mesh_prepare_kernel of tamf_mesh.h, with a face that has an index outside
// [0, V) left as a record of zeros (|det| = 0: the test passes it over) ---------------------------------------------------------------
__global__ void md_inside_prepare_kernel(char* __restrict__ base, int mesh) {
  const MdMesh* m = (const MdMesh*)base + mesh;
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= m->F) return;
  const double* verts = (const double*)(base + m->verts_off);
  const int* faces = (const int*)(base + m->faces_off);
  double* o = (double*)(base + m->tc_off) + (long)f * MESH_TC;
  const int i0 = faces[f * 3], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2], V = m->V;
  if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V) {
#pragma unroll
    for (int k = 0; k < MESH_TC; ++k) o[k] = 0.0;
    return;
  }
  const int idx[3] = {i0, i1, i2};
  double t[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double* v = verts + (long)idx[k] * 3;
    t[k][0] = m->sc[0] * v[0] + m->tr[0];
    t[k][1] = m->sc[1] * v[1] + m->tr[1];
    t[k][2] = m->sc[2] * v[2] + m->tr[2];
  }
  mesh_record(t, o);
}

// mesh_contains_kernel's test of the lane's point against all F records of the mesh; the group leaves together when no point is live
TAMF_DEV bool md_inside(const char* __restrict__ base, const MdMesh* __restrict__ m, double wx, double wy, double wz, bool active, MdShared& sh) {
  constexpr int TILE = MD_TILE * MD_REC / MESH_TC;  // records of the inside test that fit the distance tile's LDS: 40
  const double res = m->res;
  const double qx = m->sc[0] * wx + m->tr[0], qy = m->sc[1] * wy + m->tr[1], qz = m->sc[2] * wz + m->tr[2];
  const bool live = active && qx >= 0.0 && qx <= res && qy >= 0.0 && qy <= res && qz >= 0.0 && qz <= res && qx < res && qy < res;
  if (!__syncthreads_or(live)) return false;
  const double* tc = (const double*)(base + m->tc_off);
  const int F = __builtin_amdgcn_readfirstlane(m->F);
  unsigned above = 0, below = 0;
  for (int f0 = 0; f0 < F; f0 += TILE) {
    const int nt = F - f0 < TILE ? F - f0 : TILE;
    __syncthreads();
    for (int k = threadIdx.x; k < nt * MESH_TC; k += MD_NT) sh.tile[k] = tc[(long)f0 * MESH_TC + k];
    __syncthreads();
    if (!live) continue;
    for (int j = 0; j < nt; ++j) {
      const double* c = sh.tile + j * MESH_TC;
      const double adet = c[7];
      if (adet == 0.0) continue;
      const double y0 = qx - c[0], y1 = qy - c[1];
      const double u = (c[5] * y0 - c[3] * y1) * c[6];
      const double v = (-c[4] * y0 + c[2] * y1) * c[6];
      const double s = u + v;
      if (!(0.0 < u && u < adet && 0.0 < v && v < adet && 0.0 < s && s < adet)) continue;
      const double an = c[11];
      if (an == 0.0) continue;
      const double alpha = c[8] * (c[12] - qx) + c[9] * (c[13] - qy);
      const double depth = c[14] + alpha * c[10];
      const double zq = qz * an;
      if (depth >= zq) ++above;
      else if (depth < zq) ++below;
    }
  }
  return live && (above & 1u) && (below & 1u);
}

// ---- J jobs in one launch ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MD_NT) void meshdist_points_kernel(const char* __restrict__ base, const MdJob* __restrict__ jobs, int J,
                                                                const float* __restrict__ pts, unsigned flags, double* __restrict__ dist_out,
                                                                int* __restrict__ face_out, unsigned char* __restrict__ inside_out) {
  __shared__ MdShared sh;
  const long long b = blockIdx.x;
  int jl = 0, jh = J - 1;  // the last job whose first work group is <= b (it is never an empty one)
  while (jl < jh) {
    const int mid = (jl + jh + 1) >> 1;
    if (jobs[mid].blk0 <= b) jl = mid;
    else jh = mid - 1;
  }
  const MdJob* jb = jobs + jl;
  const MdMesh* m = (const MdMesh*)base + jb->mesh;
  const long long first = (b - jb->blk0) * MD_NT, len = jb->len;
  const bool active = first + threadIdx.x < len;
  const long long idx = active ? first + threadIdx.x : first;  // (first < len: the group exists because of it)
  const float* pp = pts + (jb->off + idx) * 3;
  const double x = (double)pp[0], y = (double)pp[1], z = (double)pp[2];
  const double wx = ((jb->tr[0] * x + jb->tr[1] * y) + jb->tr[2] * z) + jb->tr[3];
  const double wy = ((jb->tr[4] * x + jb->tr[5] * y) + jb->tr[6] * z) + jb->tr[7];
  const double wz = ((jb->tr[8] * x + jb->tr[9] * y) + jb->tr[10] * z) + jb->tr[11];
  double best;
  int bestf;
  md_sweep(base, m, wx, wy, wz, active, !(flags & 1u), best, bestf, sh);
  const long long o = jb->out0 + idx;
  if (active) {
    dist_out[o] = __dsqrt_rn(best);
    face_out[o] = bestf == 0x7fffffff ? -1 : bestf;
  }
  if (inside_out) {  // (uniform)
    const bool in = md_inside(base, m, wx, wy, wz, active, sh);
    if (active) inside_out[o] = (unsigned char)in;
  }
}

// ---- one mesh on an R^3 lattice: bricks of 8 x 8 x 4 points ---------------------------------------------------------------------------
constexpr int MD_BI = 8, MD_BJ = 8, MD_BK = 4;
static_assert(MD_BI * MD_BJ * MD_BK == MD_NT, "one lattice point per lane");

__global__ __launch_bounds__(MD_NT) void meshdist_lattice_kernel(const char* __restrict__ base, int mesh, const double* __restrict__ ticks,
                                                                 int R, unsigned flags, double* __restrict__ dist_out) {
  __shared__ MdShared sh;
  const MdMesh* m = (const MdMesh*)base + mesh;
  const int nbj = (R + MD_BJ - 1) / MD_BJ, nbk = (R + MD_BK - 1) / MD_BK;
  const int bk = blockIdx.x % nbk, bj = (blockIdx.x / nbk) % nbj, bi = blockIdx.x / (nbk * nbj);
  const int i = bi * MD_BI + (threadIdx.x >> 5), j = bj * MD_BJ + ((threadIdx.x >> 2) & 7), k = bk * MD_BK + (threadIdx.x & 3);
  const bool active = i < R && j < R && k < R;
  const double px = ticks[(i < R ? i : R - 1) * 3 + 0], py = ticks[(j < R ? j : R - 1) * 3 + 1], pz = ticks[(k < R ? k : R - 1) * 3 + 2];
  double best;
  int bestf;
  md_sweep(base, m, px, py, pz, active, !(flags & 1u), best, bestf, sh);
  if (active) dist_out[((long)i * R + j) * R + k] = __dsqrt_rn(best);
}

#pragma clang fp contract(fast)
