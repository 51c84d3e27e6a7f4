// Contact-distance kernels of the training losses (include/tamf_contact.h): brute-force nearest neighbour in both directions between
// a frame's hand vertices and one object's points, WITH the index of the nearest, and the backward with respect to the hand vertices
// (model/loss/chamfer_distance.py:4-64 point2point_signed as model/interaction_segment_extra_loss.py:146-178 calls it).  fp32, VALU-bound.
// The layout is h2o_dist_kernel's (tamf_geom.h); object points are moved to the frame's pose on the fly with its expressions, so
// the minimum over the objects of h2o equals that kernel's output bit for bit.
//
// Both forward directions are one scan: every thread keeps up to CT_QPT queries in registers, the candidates stream through LDS in
// tiles of 256 float4 and are read back as 16-byte broadcasts (one ds_read_b128 per 4 x 9 VALU operations).  The nearest is the
// smallest squared distance; a strict `<` over ascending candidates leaves the LOWEST index on an exact tie.
// Nothing here uses an atomic: every output element has one writer and every sum a fixed order.
#pragma once
#include "tamf_geom.h"

constexpr int CT_NT = 256;   // threads of a workgroup = candidates of a tile
constexpr int CT_QPT = 4;    // queries a thread keeps: V <= CT_NT * CT_QPT
constexpr int CT_VMAX = CT_NT * CT_QPT;
constexpr int CT_CHUNK = CT_NT * CT_QPT;  // object points of one o2h workgroup

struct ContactPose {
  float R[9], tx, ty, tz;
};

TAMF_DEV ContactPose contact_pose(const float* __restrict__ tr) {
  ContactPose p;
  float a[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) a[k] = tr[3 + k];
  gs_rows(a, p.R);
  p.tx = tr[0], p.ty = tr[1], p.tz = tr[2];
  return p;
}

// R p + t, the expressions of h2o_dist_kernel
TAMF_DEV float4 contact_move(const ContactPose& q, const float* __restrict__ p) {
  const float px = p[0], py = p[1], pz = p[2];
  float4 r;
  r.x = fmaf(q.R[2], pz, fmaf(q.R[1], py, q.R[0] * px)) + q.tx;
  r.y = fmaf(q.R[5], pz, fmaf(q.R[4], py, q.R[3] * px)) + q.ty;
  r.z = fmaf(q.R[8], pz, fmaf(q.R[7], py, q.R[6] * px)) + q.tz;
  r.w = 0.f;
  return r;
}

TAMF_DEV void contact_scan(const float4* tile, int nt, int base, const float (&qx)[CT_QPT], const float (&qy)[CT_QPT],
                           const float (&qz)[CT_QPT], float (&best)[CT_QPT], int (&bidx)[CT_QPT]) {
#pragma unroll 8
  for (int k = 0; k < nt; ++k) {
    const float4 c = tile[k];
#pragma unroll
    for (int i = 0; i < CT_QPT; ++i) {
      const float dx = qx[i] - c.x, dy = qy[i] - c.y, dz = qz[i] - c.z;
      const float d = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
      const bool lt = d < best[i];
      best[i] = lt ? d : best[i];
      bidx[i] = lt ? base + k : bidx[i];
    }
  }
}

TAMF_DEV float contact_sign(float v) { return (float)((v > 0.f) - (v < 0.f)); }

// h2o[b, o, t, v] = || hand[b,t,v] - nearest point of object o at frame t ||, h2o_idx = that point's index.
// grid (T, B * nobj); the queries are the frame's hand vertices, v = tid + 256 i.
__global__ __launch_bounds__(CT_NT) void contact_h2o_kernel(const float* __restrict__ hand, const float* __restrict__ traj,
                                                            const float* __restrict__ pts, const int* __restrict__ obj_num,
                                                            float* __restrict__ h2o, int* __restrict__ h2o_idx, int T, int V, int nobj,
                                                            int P) {
  __shared__ float4 tile[CT_NT];
  const int t = blockIdx.x, bo = blockIdx.y, tid = threadIdx.x;
  const int b = bo / nobj, o = bo - b * nobj;
  const long ob = ((long)bo * T + t) * V;
  if (obj_num && o >= obj_num[b]) {  // a padded object (uniform over the workgroup)
    for (int v = tid; v < V; v += CT_NT) h2o[ob + v] = 0.f, h2o_idx[ob + v] = -1;
    return;
  }
  const float* hv = hand + ((long)b * T + t) * V * 3;
  float qx[CT_QPT], qy[CT_QPT], qz[CT_QPT], best[CT_QPT];
  int bidx[CT_QPT];
#pragma unroll
  for (int i = 0; i < CT_QPT; ++i) {
    const int v = tid + CT_NT * i;
    const bool ok = v < V;
    qx[i] = ok ? hv[v * 3 + 0] : 0.f;
    qy[i] = ok ? hv[v * 3 + 1] : 0.f;
    qz[i] = ok ? hv[v * 3 + 2] : 0.f;
    best[i] = 3.0e38f;
    bidx[i] = 0;
  }
  const ContactPose pose = contact_pose(traj + ((long)bo * T + t) * 9);
  const float* pp = pts + (long)bo * P * 3;
  for (int p0 = 0; p0 < P; p0 += CT_NT) {
    const int j = p0 + tid;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < P) q = contact_move(pose, pp + (long)j * 3);
    __syncthreads();
    tile[tid] = q;
    __syncthreads();
    contact_scan(tile, min(CT_NT, P - p0), p0, qx, qy, qz, best, bidx);
  }
#pragma unroll
  for (int i = 0; i < CT_QPT; ++i) {
    const int v = tid + CT_NT * i;
    if (v < V) h2o[ob + v] = sqrtf(best[i]), h2o_idx[ob + v] = bidx[i];
  }
}

// o2h[b, o, t, j] = || y_j - nearest hand vertex || * sign(n . (y_j - x_near)) (unsigned when normals is null), o2h_idx = that vertex.
// grid (T, B * nobj, ceil(P / CT_CHUNK)); the queries are CT_CHUNK object points in the frame's pose, the candidates the hand vertices.
__global__ __launch_bounds__(CT_NT) void contact_o2h_kernel(const float* __restrict__ hand, const float* __restrict__ normals,
                                                            const float* __restrict__ traj, const float* __restrict__ pts,
                                                            const int* __restrict__ obj_num, float* __restrict__ o2h,
                                                            int* __restrict__ o2h_idx, int T, int V, int nobj, int P) {
  __shared__ float4 tile[CT_NT];
  const int t = blockIdx.x, bo = blockIdx.y, tid = threadIdx.x;
  const int b = bo / nobj, o = bo - b * nobj;
  const long j0 = (long)blockIdx.z * CT_CHUNK;
  const long ob = ((long)bo * T + t) * P;
  if (obj_num && o >= obj_num[b]) {
    for (long j = j0 + tid; j < P && j < j0 + CT_CHUNK; j += CT_NT) o2h[ob + j] = 0.f, o2h_idx[ob + j] = -1;
    return;
  }
  const ContactPose pose = contact_pose(traj + ((long)bo * T + t) * 9);
  const float* pp = pts + (long)bo * P * 3;
  float qx[CT_QPT], qy[CT_QPT], qz[CT_QPT], best[CT_QPT];
  int bidx[CT_QPT];
#pragma unroll
  for (int i = 0; i < CT_QPT; ++i) {
    const long j = j0 + tid + CT_NT * i;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < P) q = contact_move(pose, pp + j * 3);
    qx[i] = q.x, qy[i] = q.y, qz[i] = q.z;
    best[i] = 3.0e38f;
    bidx[i] = 0;
  }
  const float* hv = hand + ((long)b * T + t) * V * 3;
  for (int v0 = 0; v0 < V; v0 += CT_NT) {
    const int v = v0 + tid;
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (v < V) q = make_float4(hv[v * 3 + 0], hv[v * 3 + 1], hv[v * 3 + 2], 0.f);
    __syncthreads();
    tile[tid] = q;
    __syncthreads();
    contact_scan(tile, min(CT_NT, V - v0), v0, qx, qy, qz, best, bidx);
  }
  const float* nv = normals ? normals + ((long)b * T + t) * V * 3 : nullptr;
#pragma unroll
  for (int i = 0; i < CT_QPT; ++i) {
    const long j = j0 + tid + CT_NT * i;
    if (j >= P) continue;
    const int v = bidx[i];  // in [0, V): starts at 0 and only takes candidate indices
    float d = sqrtf(best[i]);
    if (nv) {
      const float dot = nv[v * 3 + 0] * (qx[i] - hv[v * 3 + 0]) + nv[v * 3 + 1] * (qy[i] - hv[v * 3 + 1]) + nv[v * 3 + 2] * (qz[i] - hv[v * 3 + 2]);
      d *= contact_sign(dot);
    }
    o2h[ob + j] = d;
    o2h_idx[ob + j] = v;
  }
}

// g_hand[b, t, v] = sum over the real objects o, ascending, of
//     g_h2o[b,o,t,v] * u(x_v - y_near)                                                       (y_near = point h2o_idx[b,o,t,v] of object o)
//   + sum over the points j, ascending, with o2h_idx[b,o,t,j] == v of  g_o2h[b,o,t,j] * sign(o2h_signed[b,o,t,j]) * u(x_v - y_j)
// with u(d) = d / |d| and u(0) = 0.  grid (T, B); a thread owns the vertices v = tid + 256 i.  The scatter of the second sum is a
// gather: a tile of 256 points is prepared once as (coefficient * unit vector, index) and every thread adds the entries that name one
// of its vertices, in the tile's order.  The terms are float32; their sums are kept in float64 and rounded once at the end (a vertex
// that is nearest to thousands of points would otherwise carry the rounding of every partial sum).  An index outside its range (a padded row's -1, or a caller's mistake) contributes nothing.
__global__ __launch_bounds__(CT_NT) void contact_backward_kernel(const float* __restrict__ hand, const float* __restrict__ traj,
                                                                 const float* __restrict__ pts, const int* __restrict__ obj_num,
                                                                 const int* __restrict__ h2o_idx, const float* __restrict__ g_h2o,
                                                                 const float* __restrict__ o2h_signed, const int* __restrict__ o2h_idx,
                                                                 const float* __restrict__ g_o2h, float* __restrict__ g_hand, int T, int V,
                                                                 int nobj, int P) {
  __shared__ float4 tile[CT_NT];
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const float* hv = hand + ((long)b * T + t) * V * 3;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  float qx[CT_QPT], qy[CT_QPT], qz[CT_QPT];
  double ax[CT_QPT], ay[CT_QPT], az[CT_QPT];  // float64 sums of float32 terms: a vertex may collect thousands of them
#pragma unroll
  for (int i = 0; i < CT_QPT; ++i) {
    const int v = tid + CT_NT * i;
    const bool ok = v < V;
    qx[i] = ok ? hv[v * 3 + 0] : 0.f;
    qy[i] = ok ? hv[v * 3 + 1] : 0.f;
    qz[i] = ok ? hv[v * 3 + 2] : 0.f;
    ax[i] = ay[i] = az[i] = 0.0;
  }
  const int n = obj_num ? min(obj_num[b], nobj) : nobj;
  for (int o = 0; o < n; ++o) {
    const long bo = (long)b * nobj + o;
    const ContactPose pose = contact_pose(traj + (bo * T + t) * 9);
    const float* pp = pts + bo * P * 3;
    if (g_h2o) {
      const long rb = (bo * T + t) * V;
#pragma unroll
      for (int i = 0; i < CT_QPT; ++i) {
        const int v = tid + CT_NT * i;
        if (v >= V) continue;
        const int j = h2o_idx[rb + v];
        if (j < 0 || j >= P) continue;
        const float4 y = contact_move(pose, pp + (long)j * 3);
        const float dx = qx[i] - y.x, dy = qy[i] - y.y, dz = qz[i] - y.z;
        const float len = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
        if (len > 0.f) {
          const float c = g_h2o[rb + v] / len;
          ax[i] += (double)(c * dx), ay[i] += (double)(c * dy), az[i] += (double)(c * dz);
        }
      }
    }
    if (g_o2h) {
      const long rb = (bo * T + t) * P;
      for (int p0 = 0; p0 < P; p0 += CT_NT) {
        const int j = p0 + tid;
        float4 e = make_float4(0.f, 0.f, 0.f, as_f(-1));
        if (j < P) {
          const int v = o2h_idx[rb + j];
          if (v >= 0 && v < V) {
            const float4 y = contact_move(pose, pp + (long)j * 3);
            const float dx = hv[v * 3 + 0] - y.x, dy = hv[v * 3 + 1] - y.y, dz = hv[v * 3 + 2] - y.z;
            const float len = sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
            const float s = contact_sign(o2h_signed[rb + j]);
            if (len > 0.f && s != 0.f) {
              const float c = g_o2h[rb + j] * s / len;
              e = make_float4(c * dx, c * dy, c * dz, as_f(v));
            }
          }
        }
        __syncthreads();
        tile[tid] = e;
        __syncthreads();
        const int nt = min(CT_NT, P - p0);
        for (int k = 0; k < nt; ++k) {
          const float4 c = tile[k];
          // every lane read the same entry, so its vertex id is uniform: the three waves that do not own the vertex skip the entry
          // on the scalar unit, the fourth adds it in the owner's lane (0.0 elsewhere) to the accumulator of the owner's slot
          const int v = __builtin_amdgcn_readfirstlane(as_i(c.w));
          if (v < 0 || ((v >> 6) & 3) != wave) continue;
          const bool hit = (v & 63) == lane;
          const double ex = hit ? (double)c.x : 0.0, ey = hit ? (double)c.y : 0.0, ez = hit ? (double)c.z : 0.0;
          switch (v >> 8) {
            case 0: ax[0] += ex, ay[0] += ey, az[0] += ez; break;
            case 1: ax[1] += ex, ay[1] += ey, az[1] += ez; break;
            case 2: ax[2] += ex, ay[2] += ey, az[2] += ez; break;
            default: ax[3] += ex, ay[3] += ey, az[3] += ez; break;
          }
        }
      }
    }
  }
  float* go = g_hand + ((long)b * T + t) * V * 3;
#pragma unroll
  for (int i = 0; i < CT_QPT; ++i) {
    const int v = tid + CT_NT * i;
    if (v < V) go[v * 3 + 0] = (float)ax[i], go[v * 3 + 1] = (float)ay[i], go[v * 3 + 2] = (float)az[i];
  }
}
