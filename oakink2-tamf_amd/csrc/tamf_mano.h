// MANO hand layer forward (libtamf_mano.so, include/tamf_mano.h) - linear blend skinning as published for SMPL / MANO
// (Loper et al. 2015, eq. 2-10; Romero et al. 2017, section 3), quaternion input, no PCA, flat hand mean; fp32 throughout.
//
// Per hand frame n (quat (16,4) in (w,x,y,z) order as tamf_pose_decode writes it, betas (10)):
//   1  q <- q / max(|q|, 1e-12);  R_j = the rotation matrix of q_j
//   2  pose feature = (R_1..R_15 - I), row-major, 135 values
//   3  v_posed = v_template + [shapedirs | posedirs] . [betas | pose feature]      ONE contraction over K = 145 (148 with padding) on
//      v_mfma_f32_16x16x4_f32: M = 16 frames, N = 16 vertices, the stacked basis in three planes (x / y / z) so that a lane holds
//      the three coordinates of ITS vertex for ITS four frames; the accumulators start at v_template
//   4  J = J_template + J_dirs . betas;  G_0 = [R_0 | J_0],  G_j = G_parent(j) . [R_j | J_j - J_parent(j)];  A_j = [R_Gj | t_j - R_Gj J_j]
//   5  verts[v] = sum_j weights[v, j] (A_j [v_posed[v]; 1]), the 16 weights in ascending j
//   6  joints = (16 chain joints t_j | verts[tip_ids]) permuted by joint_order
//   7  center_idx >= 0: verts, joints -= joints[center_idx]
//
// Launch: grid (frame groups of 16 * MT frames, vertex-tile groups), 256 threads.  Every workgroup first computes steps 1, 2, 4 of ITS
// frames into LDS - thread (f, j) of a 16-frame tile owns joint j of frame f, the chain goes level by level of the tree (MANO: 4
// levels) - then, where needed (a centre that is a fingertip; the workgroup that writes the joints), runs the five tip vertices as a
// 16-column tile of their own through mano_tile(), the same code the main pass runs: a vertex's value is one column of the MFMA (a
// k-ordered fp32 chain over that column alone) followed by per-lane arithmetic, so the tip tile gives the bits of the main pass.
// Then each wave takes 16-vertex tiles of the group round-robin: K loop (basis fragments through L2, MT frame tiles per fragment),
// skinning in the epilogue from the transforms in LDS, centre subtracted, stores.
//
// A frame's output bits depend on nothing but its own inputs and the model: the K order is fixed, nothing is reduced across lanes,
// there are no atomics, and neither MT nor the grid enters any operation's operands or order.
//
// LDS per 16-frame tile (floats): feat [148][16] (k-major: a wave's A fragment read touches every bank twice) | A [16][16][12]
// ([R row-major | t]) | jpos [16][16][3] | tipv [16][5][3] | cen [16][3]  = 6 496 floats = 25.4 KiB.
#pragma once
#include "tamf_device.h"

constexpr int MANO_J = 16, MANO_NB = 10, MANO_NP = 135, MANO_K = MANO_NB + MANO_NP, MANO_KP = 148, MANO_NT = 256;
constexpr int MANO_TIPS = 5, MANO_NJ = MANO_J + MANO_TIPS, MANO_VMAX = 1024;
constexpr int MANO_L_FEAT = 0, MANO_L_A = MANO_L_FEAT + MANO_KP * 16, MANO_L_JPOS = MANO_L_A + 16 * MANO_J * 12;
constexpr int MANO_L_TIP = MANO_L_JPOS + 16 * MANO_J * 3, MANO_L_CEN = MANO_L_TIP + 16 * MANO_TIPS * 3, MANO_L_FLOATS = MANO_L_CEN + 16 * 3;
// int table of a model (device): parents | depth | tip_ids | joint_order
constexpr int MANO_T_PARENT = 0, MANO_T_DEPTH = 16, MANO_T_TIP = 32, MANO_T_ORDER = 37, MANO_T_INTS = 58;

struct ManoArgs {
  const float* basis;  // [3][148][Vp]  plane c, row k: shapedirs[v][c][k] (k < 10), posedirs[v][c][k - 10] (k < 145), 0
  const float* vt;     // [3][Vp]       v_template planes
  const float* w;      // [Vp][16]      skinning weights
  const float* jt;     // [16][3]       J_regressor . v_template
  const float* jd;     // [16][3][10]   J_regressor . shapedirs
  const int* tab;      // [58]
  const float* quat;   // [N][16][4]
  const float* betas;  // [N][10]
  float* verts;        // [N][V][3]
  float* joints;       // [N][21][3] or null
  int N, V, Vp, center, maxdepth, tiles_per_group;
};

// One 16-vertex tile for the MT frame tiles of the workgroup: this lane (r = lane & 15, g = lane >> 4) computes vertex `vid`
// (< Vp; columns past V hold zeros) of frames 4g..4g+3 of every tile: steps 3 and 5.  emit(mt, i, x, y, z) receives the skinned
// vertex of frame 4g + i of tile mt, not centred.  The frame loop of the epilogue is a real loop (the accumulators rotate through
// element 0): unrolled, the compiler hoists the 192 * MT transform reads of a lane above the K loop and spills them.
template <int MT, class Emit>
TAMF_DEV void mano_tile(const ManoArgs& a, const float* lds, int vid, Emit emit) {
  const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
  const long Vp = a.Vp, plane = (long)MANO_KP * Vp;
  const float* __restrict__ bp = a.basis + (long)g * Vp + vid;
  f32x4 acc[MT][3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float t = a.vt[c * Vp + vid];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt][c] = f32x4{t, t, t, t};
  }
  const float* fp = lds + MANO_L_FEAT + g * 16 + r;
#pragma unroll 2
  for (int k = 0; k < MANO_KP; k += 4) {
    const float bx = bp[k * Vp], by = bp[plane + k * Vp], bz = bp[2 * plane + k * Vp];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const float af = fp[mt * MANO_L_FLOATS + k * 16];
      acc[mt][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, bx, acc[mt][0], 0, 0, 0);
      acc[mt][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, by, acc[mt][1], 0, 0, 0);
      acc[mt][2] = __builtin_amdgcn_mfma_f32_16x16x4f32(af, bz, acc[mt][2], 0, 0, 0);
    }
  }
  float w[MANO_J];
  {
    const float4* wp = reinterpret_cast<const float4*>(a.w + (long)vid * MANO_J);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 t = wp[q];
      w[4 * q] = t.x, w[4 * q + 1] = t.y, w[4 * q + 2] = t.z, w[4 * q + 3] = t.w;
    }
  }
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) {
    f32x4 X = acc[mt][0], Y = acc[mt][1], Z = acc[mt][2];
#pragma unroll 1
    for (int i = 0; i < 4; ++i) {
      const float4* ap = reinterpret_cast<const float4*>(lds + mt * MANO_L_FLOATS + MANO_L_A + (4 * g + i) * MANO_J * 12);
      const float px = X[0], py = Y[0], pz = Z[0];
      float ox = 0.f, oy = 0.f, oz = 0.f;
#pragma unroll
      for (int j = 0; j < MANO_J; ++j) {
        const float4 a0 = ap[3 * j], a1 = ap[3 * j + 1], a2 = ap[3 * j + 2];  // R00 R01 R02 R10 | R11 R12 R20 R21 | R22 t0 t1 t2
        const float tx = fmaf(a0.z, pz, fmaf(a0.y, py, fmaf(a0.x, px, a2.y)));
        const float ty = fmaf(a1.y, pz, fmaf(a1.x, py, fmaf(a0.w, px, a2.z)));
        const float tz = fmaf(a2.x, pz, fmaf(a1.w, py, fmaf(a1.z, px, a2.w)));
        ox = fmaf(w[j], tx, ox);
        oy = fmaf(w[j], ty, oy);
        oz = fmaf(w[j], tz, oz);
      }
      emit(mt, i, ox, oy, oz);
      X = f32x4{X[1], X[2], X[3], X[0]}, Y = f32x4{Y[1], Y[2], Y[3], Y[0]}, Z = f32x4{Z[1], Z[2], Z[3], Z[0]};
    }
  }
}

// steps 1, 2, 4 of one 16-frame tile (frames n0..n0+15; frames past N run as the identity pose with zero betas and are never
// stored): thread (f = tid >> 4, j = tid & 15).  Ends with the tile's feat, A and jpos complete and the workgroup synchronised.
TAMF_DEV void mano_frames(const ManoArgs& a, float* lds, long n0) {
  const int tid = threadIdx.x, f = tid >> 4, j = tid & 15, lane = tid & 63;
  const long n = n0 + f;
  const bool live = n < a.N;
  float qw = 1.f, qx = 0.f, qy = 0.f, qz = 0.f;
  float b[MANO_NB];
  if (live) {
    const float4 q = reinterpret_cast<const float4*>(a.quat)[n * MANO_J + j];
    qw = q.x, qx = q.y, qy = q.z, qz = q.w;
  }
#pragma unroll
  for (int i = 0; i < MANO_NB; ++i) b[i] = live ? a.betas[n * MANO_NB + i] : 0.f;
  const float inv = 1.0f / fmaxf(sqrtf(fmaf(qz, qz, fmaf(qy, qy, fmaf(qx, qx, qw * qw)))), 1e-12f);
  qw *= inv, qx *= inv, qy *= inv, qz *= inv;
  float R[9];
  R[0] = 1.f - 2.f * (qy * qy + qz * qz), R[1] = 2.f * (qx * qy - qw * qz), R[2] = 2.f * (qx * qz + qw * qy);
  R[3] = 2.f * (qx * qy + qw * qz), R[4] = 1.f - 2.f * (qx * qx + qz * qz), R[5] = 2.f * (qy * qz - qw * qx);
  R[6] = 2.f * (qx * qz - qw * qy), R[7] = 2.f * (qy * qz + qw * qx), R[8] = 1.f - 2.f * (qx * qx + qy * qy);
  float* feat = lds + MANO_L_FEAT;
  // (static indices only: b[] and R[] stay in registers)
#pragma unroll
  for (int i = 0; i < MANO_NB; ++i)
    if (j == i) feat[i * 16 + f] = b[i];
  if (j >= 1) {
#pragma unroll
    for (int e = 0; e < 9; ++e) feat[(MANO_NB + (j - 1) * 9 + e) * 16 + f] = R[e] - ((e & 3) == 0 ? 1.f : 0.f);
  } else {
#pragma unroll
    for (int k = MANO_K; k < MANO_KP; ++k) feat[k * 16 + f] = 0.f;
  }
  float Jr[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float s = a.jt[j * 3 + c];
#pragma unroll
    for (int i = 0; i < MANO_NB; ++i) s = fmaf(a.jd[(j * 3 + c) * MANO_NB + i], b[i], s);
    Jr[c] = s;
  }
  const int par = a.tab[MANO_T_PARENT + j], dep = a.tab[MANO_T_DEPTH + j];
  // the parent's rest joint: same frame, same wave (a wave holds 4 frames x 16 joints)
  const int psrc = (lane & 48) | (par < 0 ? j : par);
  float d[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) d[c] = Jr[c] - __shfl(Jr[c], psrc, 64);
  float* Aj = lds + MANO_L_A + (f * MANO_J + j) * 12;
  float G[12];
  for (int lv = 0; lv <= a.maxdepth; ++lv) {
    if (dep == lv) {
      if (par < 0) {
#pragma unroll
        for (int e = 0; e < 9; ++e) G[e] = R[e];
#pragma unroll
        for (int c = 0; c < 3; ++c) G[9 + c] = Jr[c];
      } else {
        float P[12];
        const float* Ap = lds + MANO_L_A + (f * MANO_J + par) * 12;
#pragma unroll
        for (int e = 0; e < 12; ++e) P[e] = Ap[e];
#pragma unroll
        for (int rr = 0; rr < 3; ++rr) {
#pragma unroll
          for (int cc = 0; cc < 3; ++cc)
            G[rr * 3 + cc] = fmaf(P[rr * 3 + 2], R[6 + cc], fmaf(P[rr * 3 + 1], R[3 + cc], P[rr * 3] * R[cc]));
          G[9 + rr] = fmaf(P[rr * 3 + 2], d[2], fmaf(P[rr * 3 + 1], d[1], fmaf(P[rr * 3], d[0], P[9 + rr])));
        }
      }
#pragma unroll
      for (int e = 0; e < 12; ++e) Aj[e] = G[e];
    }
    __syncthreads();
  }
  // every G is complete and read: posed joints out, translation -> t - R_G J
  float* jp = lds + MANO_L_JPOS + (f * MANO_J + j) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    jp[c] = G[9 + c];
    Aj[9 + c] = G[9 + c] - fmaf(G[c * 3 + 2], Jr[2], fmaf(G[c * 3 + 1], Jr[1], G[c * 3] * Jr[0]));
  }
  __syncthreads();
}

template <int MT>
__global__ __launch_bounds__(MANO_NT) void mano_forward_kernel(const ManoArgs a) {
  extern __shared__ float4 mano_lds4[];
  float* lds = reinterpret_cast<float*>(mano_lds4);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4;
  const long n0 = (long)blockIdx.x * (16 * MT);
  for (int mt = 0; mt < MT; ++mt) mano_frames(a, lds + mt * MANO_L_FLOATS, n0 + mt * 16);

  // ---- fingertips first, where something needs them before the vertex stores ----
  const int cj = a.center >= 0 ? a.tab[MANO_T_ORDER + a.center] : -1;  // what the centre is: chain joint (< 16), tip (>= 16), none
  const bool writes_joints = a.joints != nullptr && blockIdx.y == 0;
  if (cj >= MANO_J || writes_joints) {
    if (wave == 0) {
      mano_tile<MT>(a, lds, r < MANO_TIPS ? a.tab[MANO_T_TIP + r] : 0, [&](int mt, int i, float x, float y, float z) {
        if (r < MANO_TIPS) {
          float* tp = lds + mt * MANO_L_FLOATS + MANO_L_TIP + ((4 * g + i) * MANO_TIPS + r) * 3;
          tp[0] = x, tp[1] = y, tp[2] = z;
        }
      });
    }
    __syncthreads();
  }
  for (int e = tid; e < MT * 48; e += MANO_NT) {
    const int mt = e / 48, fc = e % 48, f = fc / 3, c = fc % 3;
    const float* L = lds + mt * MANO_L_FLOATS;
    L = cj < MANO_J ? L + MANO_L_JPOS + (f * MANO_J + (cj < 0 ? 0 : cj)) * 3 : L + MANO_L_TIP + (f * MANO_TIPS + (cj - MANO_J)) * 3;
    lds[mt * MANO_L_FLOATS + MANO_L_CEN + fc] = cj < 0 ? 0.f : L[c];
  }
  __syncthreads();
  if (writes_joints) {
    for (int e = tid; e < MT * 16 * MANO_NJ * 3; e += MANO_NT) {
      const int mt = e / (16 * MANO_NJ * 3), rem = e % (16 * MANO_NJ * 3), f = rem / (MANO_NJ * 3), slot = rem % (MANO_NJ * 3) / 3, c = rem % 3;
      const long n = n0 + mt * 16 + f;
      if (n < a.N) {
        const int src = a.tab[MANO_T_ORDER + slot];
        const float* L = lds + mt * MANO_L_FLOATS;
        const float v = src < MANO_J ? L[MANO_L_JPOS + (f * MANO_J + src) * 3 + c] : L[MANO_L_TIP + (f * MANO_TIPS + (src - MANO_J)) * 3 + c];
        a.joints[(n * MANO_NJ + slot) * 3 + c] = v - L[MANO_L_CEN + f * 3 + c];
      }
    }
  }

  // ---- vertices ----
  const int ntiles = a.Vp >> 4, t0 = blockIdx.y * a.tiles_per_group, t1 = min(t0 + a.tiles_per_group, ntiles);
  for (int t = t0 + wave; t < t1; t += MANO_NT / 64) {
    const int vid = t * 16 + r;
    mano_tile<MT>(a, lds, vid, [&](int mt, int i, float x, float y, float z) {
      const int f = 4 * g + i;
      const long n = n0 + mt * 16 + f;
      if (vid < a.V && n < a.N) {
        const float* cen = lds + mt * MANO_L_FLOATS + MANO_L_CEN + f * 3;
        float* dst = a.verts + (n * a.V + vid) * 3;
        dst[0] = x - cen[0], dst[1] = y - cen[1], dst[2] = z - cen[2];
      }
    });
  }
}
