// SDF-lattice sampler of the training losses' `pen` term (include/tamf_sdfgrid.h): the pose transform into the object frame and a
// trilinear read of the object's signed distance lattice, for every clip, object, frame and hand vertex in one launch, and the backward
// with respect to the hand vertices.  float64 arithmetic on widened float32 inputs, compiled with -ffp-contract=off: every expression
// below is the header's, operation by operation, and tests/sdfgrid_restatement.py states it again in numpy.
//
// A work group owns up to SG_FC consecutive frames: their poses (two square roots and six divisions each) are computed once into LDS,
// one thread per pose, and the threads then run over the chunk's frames x vertices, which are contiguous in every tensor.  The eight
// corners are gathered straight from global memory (a 100^3 float32 lattice is 4 MB: it stays in L2 / Infinity Cache).
// The forward owns one object per work group; the backward owns a clip and sums over its objects in the thread that owns the vertex,
// so nothing here uses an atomic: every output element has one writer and every sum a fixed order.
#pragma once
#include <hip/hip_runtime.h>

#include "tamf_sdfgrid_host.h"

#define SG_DEV __device__ __forceinline__

constexpr double SG_EPS = 1.1920928955078125e-07;  // 2^-23, float32's eps: the guard of the Gram-Schmidt (metrics/siv.tslrot6d_to_transf)

struct SgSet {
  const float* values;
  const long long* off;
  const int* res;
  const double* origin;
  const double* step;
  int G;
};

// P[0..8] = the rows b1, b2, b3 of R, P[9..11] = t, from one obj_traj row (tsl | rot6d)
SG_DEV void sg_pose(const float* __restrict__ tr, double (&P)[12]) {
  const double a0 = (double)tr[3], a1 = (double)tr[4], a2 = (double)tr[5], a3 = (double)tr[6], a4 = (double)tr[7], a5 = (double)tr[8];
  double n1 = __dsqrt_rn((a0 * a0 + a1 * a1) + a2 * a2);
  n1 = n1 > SG_EPS ? n1 : SG_EPS;
  const double b1x = a0 / n1, b1y = a1 / n1, b1z = a2 / n1;
  const double dp = (b1x * a3 + b1y * a4) + b1z * a5;
  double b2x = a3 - dp * b1x, b2y = a4 - dp * b1y, b2z = a5 - dp * b1z;
  double n2 = __dsqrt_rn((b2x * b2x + b2y * b2y) + b2z * b2z);
  n2 = n2 > SG_EPS ? n2 : SG_EPS;
  b2x = b2x / n2, b2y = b2y / n2, b2z = b2z / n2;
  P[0] = b1x, P[1] = b1y, P[2] = b1z;
  P[3] = b2x, P[4] = b2y, P[5] = b2z;
  P[6] = b1y * b2z - b1z * b2y;
  P[7] = b1z * b2x - b1x * b2z;
  P[8] = b1x * b2y - b1y * b2x;
  P[9] = (double)tr[0], P[10] = (double)tr[1], P[11] = (double)tr[2];
}

// the lattice of object (b, o), or -1: a padded object, one without a lattice, or an id / resolution outside the set's ranges
SG_DEV int sg_grid_of(const SgSet& S, const int* __restrict__ grid_id, const int* __restrict__ obj_num, int b, int o, int nobj, int& R) {
  R = 0;
  if (obj_num && o >= obj_num[b]) return -1;
  const int g = grid_id[(long)b * nobj + o];
  if (g < 0 || g >= S.G) return -1;
  R = S.res[g];
  if (R < SG_MIN_RES || R > SG_MAX_RES) return -1;
  return g;
}

// The depth s of the vertex (x, y, z) in lattice g of resolution R under pose P; false (and nothing written) unless s > 0.
// GRAD: also the world gradient w of s with respect to the vertex.
template <bool GRAD>
SG_DEV bool sg_sample(const SgSet& S, int g, int R, const double (&P)[12], float x, float y, float z, double& s, int& cell, double (&w)[3]) {
  const double* __restrict__ og = S.origin + (long)g * 3;
  const double* __restrict__ st = S.step + (long)g * 3;
  const double d0 = (double)x - P[9], d1 = (double)y - P[10], d2 = (double)z - P[11];
  const double p0 = (P[0] * d0 + P[3] * d1) + P[6] * d2;
  const double p1 = (P[1] * d0 + P[4] * d1) + P[7] * d2;
  const double p2 = (P[2] * d0 + P[5] * d1) + P[8] * d2;
  const double st0 = st[0], st1 = st[1], st2 = st[2];
  const double u0 = (p0 - og[0]) / st0, u1 = (p1 - og[1]) / st1, u2 = (p2 - og[2]) / st2;
  const double hi = (double)(R - 1);
  if (!(u0 >= 0.0 && u0 <= hi && u1 >= 0.0 && u1 <= hi && u2 >= 0.0 && u2 <= hi)) return false;  // (false for a NaN as well)
  const int i0 = min((int)floor(u0), R - 2), i1 = min((int)floor(u1), R - 2), i2 = min((int)floor(u2), R - 2);  // in [0, R - 2]
  const double fx = u0 - (double)i0, fy = u1 - (double)i1, fz = u2 - (double)i2;
  const int c = (i0 * R + i1) * R + i2;  // < 512^3 = 2^27; the farthest corner is c + R^2 + R + 1 <= R^3 - 1
  const float* __restrict__ v = S.values + S.off[g] + c;
  const int RR = R * R;
  const double s000 = (double)v[0], s001 = (double)v[1], s010 = (double)v[R], s011 = (double)v[R + 1];
  const double s100 = (double)v[RR], s101 = (double)v[RR + 1], s110 = (double)v[RR + R], s111 = (double)v[RR + R + 1];
  const double d00 = s001 - s000, d01 = s011 - s010, d10 = s101 - s100, d11 = s111 - s110;
  const double c00 = s000 + d00 * fz, c01 = s010 + d01 * fz, c10 = s100 + d10 * fz, c11 = s110 + d11 * fz;
  const double e0 = c01 - c00, e1 = c11 - c10;
  const double c0 = c00 + e0 * fy, c1 = c10 + e1 * fy;
  const double gx = c1 - c0;
  const double sv = c0 + gx * fx;
  if (!(sv > 0.0)) return false;
  s = sv;
  cell = c;
  if (GRAD) {
    const double gy = e0 + (e1 - e0) * fx;
    const double m0 = d00 + (d01 - d00) * fy, m1 = d10 + (d11 - d10) * fy;
    const double gz = m0 + (m1 - m0) * fx;
    const double q0 = gx / st0, q1 = gy / st1, q2 = gz / st2;
    w[0] = (P[0] * q0 + P[1] * q1) + P[2] * q2;
    w[1] = (P[3] * q0 + P[4] * q1) + P[5] * q2;
    w[2] = (P[6] * q0 + P[7] * q1) + P[8] * q2;
  }
  return true;
}

// depth[b, o, t, v] and cell[b, o, t, v].  grid (frame chunks, B * nobj); a work group owns object (b, o) over nf <= fc <= SG_FC frames.
__global__ __launch_bounds__(SG_NT) void sdfgrid_forward_kernel(SgSet S, const float* __restrict__ hand, const float* __restrict__ traj,
                                                                const int* __restrict__ grid_id, const int* __restrict__ obj_num,
                                                                float* __restrict__ depth, int* __restrict__ cell, int T, int V, int nobj,
                                                                int fc) {
  __shared__ double pose[SG_FC][12];
  const int tid = threadIdx.x, bo = blockIdx.y;
  const int b = bo / nobj, o = bo - b * nobj;
  const int t0 = blockIdx.x * fc, nf = min(fc, T - t0);
  const int n = nf * V;  // <= T * V < 2^31
  const long ob = ((long)bo * T + t0) * V;
  int R;
  const int g = sg_grid_of(S, grid_id, obj_num, b, o, nobj, R);  // (uniform over the work group)
  if (g < 0) {
    for (int i = tid; i < n; i += SG_NT) {
      depth[ob + i] = 0.f;
      if (cell) cell[ob + i] = -1;
    }
    return;
  }
  if (tid < nf) {
    double P[12];
    sg_pose(traj + ((long)bo * T + t0 + tid) * 9, P);
#pragma unroll
    for (int k = 0; k < 12; ++k) pose[tid][k] = P[k];
  }
  __syncthreads();
  const float* hv = hand + ((long)b * T + t0) * V * 3;
  for (int i = tid; i < n; i += SG_NT) {
    const int f = i / V;
    double P[12], s = 0.0, w[3];
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = pose[f][k];
    int c = -1;
    const bool in = sg_sample<false>(S, g, R, P, hv[(long)i * 3 + 0], hv[(long)i * 3 + 1], hv[(long)i * 3 + 2], s, c, w);
    depth[ob + i] = in ? (float)s : 0.f;
    if (cell) cell[ob + i] = in ? c : -1;
  }
}

// g_hand[b, t, v] = sum over the real objects o with a lattice and s > 0, ascending, of g_depth[b, o, t, v] * w.  grid (frame chunks, B);
// a work group owns clip b over nf <= fc frames and keeps the poses of the first `per` = min(nobj, SG_POSES) objects of each of them
// (fc * per <= SG_POSES); the pose of an object beyond them is computed where it is used.
__global__ __launch_bounds__(SG_NT) void sdfgrid_backward_kernel(SgSet S, const float* __restrict__ hand, const float* __restrict__ traj,
                                                                 const int* __restrict__ grid_id, const int* __restrict__ obj_num,
                                                                 const float* __restrict__ g_depth, float* __restrict__ g_hand, int T, int V,
                                                                 int nobj, int fc) {
  __shared__ double pose[SG_POSES][12];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int t0 = blockIdx.x * fc, nf = min(fc, T - t0);
  const int n = nf * V;
  const int per = min(nobj, SG_POSES);
  const int nreal = obj_num ? min(obj_num[b], nobj) : nobj;
  for (int i = tid; i < nf * per; i += SG_NT) {  // (nf * per <= SG_POSES)
    const int f = i / per, o = i - f * per;
    int R;
    if (o < nreal && sg_grid_of(S, grid_id, obj_num, b, o, nobj, R) >= 0) {
      double P[12];
      sg_pose(traj + (((long)b * nobj + o) * T + t0 + f) * 9, P);
#pragma unroll
      for (int k = 0; k < 12; ++k) pose[i][k] = P[k];
    }
  }
  __syncthreads();
  const float* hv = hand + ((long)b * T + t0) * V * 3;
  float* go = g_hand + ((long)b * T + t0) * V * 3;
  for (int i = tid; i < n; i += SG_NT) {
    const int f = i / V;
    const float x = hv[(long)i * 3 + 0], y = hv[(long)i * 3 + 1], z = hv[(long)i * 3 + 2];
    double ax = 0.0, ay = 0.0, az = 0.0;
    for (int o = 0; o < nreal; ++o) {
      int R;
      const int g = sg_grid_of(S, grid_id, obj_num, b, o, nobj, R);  // (uniform over the work group)
      if (g < 0) continue;
      const long bo = (long)b * nobj + o;
      double P[12], s, w[3];
      if (o < per) {
#pragma unroll
        for (int k = 0; k < 12; ++k) P[k] = pose[f * per + o][k];
      } else {
        sg_pose(traj + (bo * T + t0 + f) * 9, P);
      }
      int c;
      if (!sg_sample<true>(S, g, R, P, x, y, z, s, c, w)) continue;
      const double gd = (double)g_depth[(bo * T + t0) * V + i];
      ax += gd * w[0], ay += gd * w[1], az += gd * w[2];
    }
    go[(long)i * 3 + 0] = (float)ax, go[(long)i * 3 + 1] = (float)ay, go[(long)i * 3 + 2] = (float)az;
  }
}
