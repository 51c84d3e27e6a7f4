// MANO hand layer, forward and (second half of this file) backward (libtamf_mano.so, include/tamf_mano.h) - linear blend skinning as
// published for SMPL / MANO
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
// step 3 for the lane's vertex `vid` and its four frames of every tile: acc[mt][c] = v_posed, coordinate c (shared with the backward)
template <int MT>
TAMF_DEV void mano_vposed(const ManoArgs& a, const float* lds, int vid, f32x4 (&acc)[MT][3]) {
  const int lane = threadIdx.x & 63, r = lane & 15, g = lane >> 4;
  const long Vp = a.Vp, plane = (long)MANO_KP * Vp;
  const float* __restrict__ bp = a.basis + (long)g * Vp + vid;
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
}

template <int MT, class Emit>
TAMF_DEV void mano_tile(const ManoArgs& a, const float* lds, int vid, Emit emit) {
  const int lane = threadIdx.x & 63, g = lane >> 4;
  f32x4 acc[MT][3];
  mano_vposed<MT>(a, lds, vid, acc);
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
struct ManoLocal {
  float q[4], nrm, R[9], Jr[3], d[3];  // normalised quaternion, |q| of the input, local rotation, rest joint, rest offset from the parent
  int par, dep;
};

TAMF_DEV void mano_frames(const ManoArgs& a, float* lds, long n0, ManoLocal& L) {
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
  L.nrm = sqrtf(fmaf(qz, qz, fmaf(qy, qy, fmaf(qx, qx, qw * qw))));
  const float inv = 1.0f / fmaxf(L.nrm, 1e-12f);
  qw *= inv, qx *= inv, qy *= inv, qz *= inv;
  L.q[0] = qw, L.q[1] = qx, L.q[2] = qy, L.q[3] = qz;
  float (&R)[9] = L.R;
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
  float (&Jr)[3] = L.Jr;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float s = a.jt[j * 3 + c];
#pragma unroll
    for (int i = 0; i < MANO_NB; ++i) s = fmaf(a.jd[(j * 3 + c) * MANO_NB + i], b[i], s);
    Jr[c] = s;
  }
  const int par = L.par = a.tab[MANO_T_PARENT + j], dep = L.dep = a.tab[MANO_T_DEPTH + j];
  // the parent's rest joint: same frame, same wave (a wave holds 4 frames x 16 joints)
  const int psrc = (lane & 48) | (par < 0 ? j : par);
  float (&d)[3] = L.d;
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
  for (int mt = 0; mt < MT; ++mt) {
    ManoLocal unused;
    mano_frames(a, lds + mt * MANO_L_FLOATS, n0 + mt * 16, unused);
  }

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

// ================================================================================================================================
// Backward (tamf_mano_backward): the vector-Jacobian product of steps 1-7 for upstream dverts (N,V,3) and / or djoints (N,21,3) ->
// dquat (N,16,4), with respect to the UN-normalised input, and dbetas (N,10).  Nothing is kept from a forward call: a workgroup
// recomputes steps 1, 2, 4 of its 16 frames with mano_frames() and v_posed with mano_vposed(), the forward's own code.
//
// Grid: one workgroup of 256 threads per 16-frame tile, whatever the model's tile setting.  Phases:
//   P  centre (step 7): gcen = -(sum of all upstream rows of the frame).  Thread (f, s) sums the vertices v = s mod 16 in ascending
//      order, thread (f, c) then the 16 partial sums and the 21 joint rows.  It is added to the upstream of the centre's source (a
//      chain joint or a fingertip vertex).  The upstream of the fingertip rows goes to tipg: it is added to dV of those vertices.
//   V  per wave, 16-vertex tiles round-robin; lane (r, g) owns vertex 16 t + r of frames 4 g .. 4 g + 3 as in the forward:
//        a  v_posed: mano_vposed, K = 148 on the MFMA
//           dvp = sum_j w[v,j] RG_j^T dV per lane; dV, v_posed, dvp go through a per-wave LDS stage (they change owner: the MFMAs
//           below contract over the VERTEX, which has to sit on the k lanes)
//        b  dA[f][j][c][d] += sum_v w[v,j] dV[f][v][c] [v_posed[f][v]; 1][d]:  M = 16 joints, K = 16 vertices (4 steps),
//           N = 16 frames, one accumulator per (c, d): 12
//        c  dfeat[f][k] += sum_c sum_v dvp[f][v][c] basis[c][k][v]:  M = 16 frames, K = 3 * 16, N = 148 in 10 column tiles
//      each tile's products are summed from zero (48 resp. 48 terms per element) and then added to the wave's running sum (12 or 13
//      tiles); the four waves' sums are added in the order ((0 + 1) + 2) + 3.  No accumulation chain is longer than that.
//   C  thread (f, j) again: dRG_j, dtG_j from dA (t_A = t_G - RG J), the chain from the deepest level to the root - a joint gathers
//      from its children in ascending order what each of them left in LDS (dRG_c R_c^T + dtG_c (x) d_c | dtG_c) -, then
//      dR_j = RG_p^T dRG_j + dfeat rows, dJ, rotation matrix -> quaternion -> normalisation; thread (f, i) dbetas[i] = dfeat[i] +
//      J_dirs . dJ over (joint, coordinate) in ascending order.
// No atomics; every sum has a fixed order that depends on the model alone, so a frame's gradient bits depend on its own inputs and
// the model - not on N, the frame's position or the launch.  Frames past N run with zero upstream and are never stored.
//
// LDS (floats): the forward's tile (6 496) | stage 4 waves x 10 planes [16 frames][17] (dV 3, v_posed 3 + a plane of ones, dvp 3;
// after the vertex loop the same floats hold the waves' partial sums) | dA [16][16][12] | dfeat [148][16] | tipg [16][5][3] |
// part [16][16][3] | cen [16][3] | up [16][16][12] | dd [16][16][3] | dJ [16][16][3]  = 28 480 floats = 111.3 KiB.
constexpr int MANO_G_ROW = 17, MANO_G_PLANE = 16 * MANO_G_ROW, MANO_G_SDV = 0, MANO_G_SVP = 3 * MANO_G_PLANE, MANO_G_SDVP = 7 * MANO_G_PLANE;
constexpr int MANO_G_STAGE = 10 * MANO_G_PLANE, MANO_G_NB = 12, MANO_G_NC = (MANO_KP + 15) / 16;
constexpr int MANO_GL_STAGE = MANO_L_FLOATS, MANO_GL_DA = MANO_GL_STAGE + 4 * MANO_G_STAGE, MANO_GL_DF = MANO_GL_DA + 16 * MANO_J * 12;
constexpr int MANO_GL_TIPG = MANO_GL_DF + MANO_KP * 16, MANO_GL_PART = MANO_GL_TIPG + 16 * MANO_TIPS * 3, MANO_GL_CEN = MANO_GL_PART + 16 * 16 * 3;
constexpr int MANO_GL_UP = MANO_GL_CEN + 16 * 3, MANO_GL_DD = MANO_GL_UP + 16 * MANO_J * 12, MANO_GL_DJ = MANO_GL_DD + 16 * MANO_J * 3;
constexpr int MANO_GL_FLOATS = MANO_GL_DJ + 16 * MANO_J * 3;
static_assert((MANO_G_NB + MANO_G_NC) * 4 * 64 <= 4 * MANO_G_STAGE, "the waves' partial sums must fit in the stage");

struct ManoGradArgs {
  ManoArgs f;            // the forward's arguments; verts / joints unused
  const float* dverts;   // [N][V][3] or null
  const float* djoints;  // [N][21][3] or null
  float* dquat;          // [N][16][4]
  float* dbetas;         // [N][10] or null
};

__global__ __launch_bounds__(MANO_NT) void mano_backward_kernel(const ManoGradArgs ga) {
  extern __shared__ float4 mano_lds4[];
  float* lds = reinterpret_cast<float*>(mano_lds4);
  const ManoArgs& a = ga.f;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, g = lane >> 4, f = tid >> 4, j = tid & 15;
  const long n0 = (long)blockIdx.x * 16, n = n0 + f;
  const bool live = n < a.N;
  ManoLocal L;
  mano_frames(a, lds, n0, L);

  // ---- P: the centre's gradient, the upstream of this thread's chain joint and of the fingertips ----
  const int cj = a.center >= 0 ? a.tab[MANO_T_ORDER + a.center] : -1;
  {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    if (cj >= 0 && live && ga.dverts) {
      const float* p = ga.dverts + n * a.V * 3;
      for (int v = j; v < a.V; v += 16) s0 += p[v * 3], s1 += p[v * 3 + 1], s2 += p[v * 3 + 2];
    }
    float* part = lds + MANO_GL_PART + (f * 16 + j) * 3;
    part[0] = s0, part[1] = s1, part[2] = s2;
  }
  __syncthreads();
  if (j < 3) {
    float s = 0.f;
    for (int k = 0; k < 16; ++k) s += lds[MANO_GL_PART + (f * 16 + k) * 3 + j];
    if (cj >= 0 && live && ga.djoints)
      for (int slot = 0; slot < MANO_NJ; ++slot) s += ga.djoints[(n * MANO_NJ + slot) * 3 + j];
    lds[MANO_GL_CEN + f * 3 + j] = cj >= 0 ? -s : 0.f;
  }
  __syncthreads();
  float dtG[3] = {0.f, 0.f, 0.f};  // upstream of t_G of joint j: its output row, and the centre's when it is the centre
  {
    // the output rows of chain joint j and of fingertip j: joint_order is a permutation of 0..20 (checked by tamf_mano_model_create),
    // so each is found exactly once (slot_t is used for j < 5 only)
    int slot_j = 0, slot_t = 0;
    for (int slot = 0; slot < MANO_NJ; ++slot) {
      const int src = a.tab[MANO_T_ORDER + slot];
      if (src == j) slot_j = slot;
      if (src == MANO_J + j) slot_t = slot;
    }
    const float* cen = lds + MANO_GL_CEN + f * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (live && ga.djoints) dtG[c] = ga.djoints[(n * MANO_NJ + slot_j) * 3 + c];
      if (cj == j) dtG[c] += cen[c];
      if (j < MANO_TIPS) {
        float t = live && ga.djoints ? ga.djoints[(n * MANO_NJ + slot_t) * 3 + c] : 0.f;
        if (cj == MANO_J + j) t += cen[c];
        lds[MANO_GL_TIPG + (f * MANO_TIPS + j) * 3 + c] = t;
      }
    }
  }
  float* st = lds + MANO_GL_STAGE + wave * MANO_G_STAGE;
  for (int e = lane; e < MANO_G_PLANE; e += 64) st[MANO_G_SVP + 3 * MANO_G_PLANE + e] = 1.f;
  __syncthreads();

  // ---- V: the vertex loop ----
  int tipv[MANO_TIPS];
#pragma unroll
  for (int i = 0; i < MANO_TIPS; ++i) tipv[i] = a.tab[MANO_T_TIP + i];
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};
  f32x4 accB[MANO_G_NB], accC[MANO_G_NC];
#pragma unroll
  for (int i = 0; i < MANO_G_NB; ++i) accB[i] = zero4;
#pragma unroll
  for (int i = 0; i < MANO_G_NC; ++i) accC[i] = zero4;
  const int ntiles = a.Vp >> 4;
  const long Vp = a.Vp, plane = (long)MANO_KP * Vp;
  for (int t0 = 0; t0 < ntiles; t0 += MANO_NT / 64) {
    const int t = t0 + wave;
    const bool act = t < ntiles;  // (wave-uniform; the barriers below are reached by every wave)
    if (act) {
      const int vid = t * 16 + r;
      f32x4 acc[1][3];
      mano_vposed<1>(a, lds, vid, acc);
      float w[MANO_J];
      {
        const float4* wp = reinterpret_cast<const float4*>(a.w + (long)vid * MANO_J);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const float4 x = wp[q];
          w[4 * q] = x.x, w[4 * q + 1] = x.y, w[4 * q + 2] = x.z, w[4 * q + 3] = x.w;
        }
      }
      f32x4 X = acc[0][0], Y = acc[0][1], Z = acc[0][2];
#pragma unroll 1
      for (int i = 0; i < 4; ++i) {
        const int fr = 4 * g + i;
        const long nn = n0 + fr;
        float gx = 0.f, gy = 0.f, gz = 0.f;
        if (vid < a.V && nn < a.N) {
          if (ga.dverts) {
            const float* p = ga.dverts + (nn * a.V + vid) * 3;
            gx = p[0], gy = p[1], gz = p[2];
          }
#pragma unroll
          for (int ti = 0; ti < MANO_TIPS; ++ti)
            if (tipv[ti] == vid) {
              const float* tp = lds + MANO_GL_TIPG + (fr * MANO_TIPS + ti) * 3;
              gx += tp[0], gy += tp[1], gz += tp[2];
            }
        }
        const float4* ap = reinterpret_cast<const float4*>(lds + MANO_L_A + fr * MANO_J * 12);
        float dx = 0.f, dy = 0.f, dz = 0.f;
#pragma unroll
        for (int jj = 0; jj < MANO_J; ++jj) {
          const float4 a0 = ap[3 * jj], a1 = ap[3 * jj + 1], a2 = ap[3 * jj + 2];  // R00 R01 R02 R10 | R11 R12 R20 R21 | R22 t0 t1 t2
          const float tx = fmaf(a1.z, gz, fmaf(a0.w, gy, a0.x * gx));              // RG^T dV
          const float ty = fmaf(a1.w, gz, fmaf(a1.x, gy, a0.y * gx));
          const float tz = fmaf(a2.x, gz, fmaf(a1.y, gy, a0.z * gx));
          dx = fmaf(w[jj], tx, dx);
          dy = fmaf(w[jj], ty, dy);
          dz = fmaf(w[jj], tz, dz);
        }
        float* o = st + fr * MANO_G_ROW + r;
        o[MANO_G_SDV] = gx, o[MANO_G_SDV + MANO_G_PLANE] = gy, o[MANO_G_SDV + 2 * MANO_G_PLANE] = gz;
        o[MANO_G_SVP] = X[0], o[MANO_G_SVP + MANO_G_PLANE] = Y[0], o[MANO_G_SVP + 2 * MANO_G_PLANE] = Z[0];
        o[MANO_G_SDVP] = dx, o[MANO_G_SDVP + MANO_G_PLANE] = dy, o[MANO_G_SDVP + 2 * MANO_G_PLANE] = dz;
        X = f32x4{X[1], X[2], X[3], X[0]}, Y = f32x4{Y[1], Y[2], Y[3], Y[0]}, Z = f32x4{Z[1], Z[2], Z[3], Z[0]};
      }
    }
    __syncthreads();
    if (act) {
      // b: A operand w[vertex 4 s + g][joint r], B operand dV_c * [v_posed; 1]_d of (vertex 4 s + g, frame r)
      {
        f32x4 lb[MANO_G_NB];
#pragma unroll
        for (int i = 0; i < MANO_G_NB; ++i) lb[i] = zero4;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const float wa = a.w[(long)(t * 16 + 4 * s + g) * MANO_J + r];
          const float* o = st + r * MANO_G_ROW + 4 * s + g;
          float dv[3], vp[4];
#pragma unroll
          for (int c = 0; c < 3; ++c) dv[c] = o[MANO_G_SDV + c * MANO_G_PLANE];
#pragma unroll
          for (int d = 0; d < 4; ++d) vp[d] = o[MANO_G_SVP + d * MANO_G_PLANE];
#pragma unroll
          for (int c = 0; c < 3; ++c)
#pragma unroll
            for (int d = 0; d < 4; ++d) lb[c * 4 + d] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa, dv[c] * vp[d], lb[c * 4 + d], 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < MANO_G_NB; ++i) accB[i] += lb[i];
      }
      // c: A operand dvp_c of (frame r, vertex 4 s + g), B operand basis[c][16 nt + r][vertex 4 s + g]
      {
        f32x4 lc[MANO_G_NC];
#pragma unroll
        for (int i = 0; i < MANO_G_NC; ++i) lc[i] = zero4;
#pragma unroll 1
        for (int c = 0; c < 3; ++c) {
#pragma unroll 1
          for (int s = 0; s < 4; ++s) {
            const float dvp = st[MANO_G_SDVP + c * MANO_G_PLANE + r * MANO_G_ROW + 4 * s + g];
            const float* __restrict__ bp = a.basis + c * plane + (t * 16 + 4 * s + g);
#pragma unroll
            for (int nt = 0; nt < MANO_G_NC; ++nt) {
              const int kk = nt * 16 + r;
              const float bv = kk < MANO_KP ? bp[kk * Vp] : 0.f;
              lc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(dvp, bv, lc[nt], 0, 0, 0);
            }
          }
        }
#pragma unroll
        for (int i = 0; i < MANO_G_NC; ++i) accC[i] += lc[i];
      }
    }
    __syncthreads();
  }

  // the four waves' sums, ((0 + 1) + 2) + 3; the last wave leaves dA[f = r][joint 4 g + i][c d] and dfeat[k = 16 nt + r][f = 4 g + i]
  {
    float* comb = lds + MANO_GL_STAGE;
    for (int wv = 0; wv < MANO_NT / 64; ++wv) {
      if (wave == wv) {
#pragma unroll
        for (int nt = 0; nt < MANO_G_NB + MANO_G_NC; ++nt)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int idx = (nt * 4 + i) * 64 + lane;
            float v = nt < MANO_G_NB ? accB[nt < MANO_G_NB ? nt : 0][i] : accC[nt >= MANO_G_NB ? nt - MANO_G_NB : 0][i];
            if (wv > 0) v = comb[idx] + v;
            if (wv < MANO_NT / 64 - 1) {
              comb[idx] = v;
            } else if (nt < MANO_G_NB) {
              lds[MANO_GL_DA + (r * MANO_J + 4 * g + i) * 12 + nt] = v;
            } else {
              const int kk = (nt - MANO_G_NB) * 16 + r;
              if (kk < MANO_KP) lds[MANO_GL_DF + kk * 16 + 4 * g + i] = v;
            }
          }
      }
      __syncthreads();
    }
  }

  // ---- C: the chain backwards; thread (f, j) ----
  const float* dA = lds + MANO_GL_DA + (f * MANO_J + j) * 12;
  const float dtA[3] = {dA[3], dA[7], dA[11]};
  float dRG[9];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int d = 0; d < 3; ++d) dRG[c * 3 + d] = fmaf(-dtA[c], L.Jr[d], dA[c * 4 + d]);  // t_A = t_G - RG J
    dtG[c] += dtA[c];
  }
  unsigned children = 0;
  for (int c = j + 1; c < MANO_J; ++c)
    if (a.tab[MANO_T_PARENT + c] == j) children |= 1u << c;
  for (int lv = a.maxdepth; lv >= 0; --lv) {
    if (L.dep == lv) {
#pragma unroll 1
      for (int c = j + 1; c < MANO_J; ++c)
        if (children >> c & 1) {
          const float* u = lds + MANO_GL_UP + (f * MANO_J + c) * 12;
#pragma unroll
          for (int e = 0; e < 9; ++e) dRG[e] += u[e];
#pragma unroll
          for (int e = 0; e < 3; ++e) dtG[e] += u[9 + e];
        }
      if (L.par >= 0) {  // RG_j = RG_p R_j, t_G_j = RG_p d_j + t_G_p: what the parent receives
        float* u = lds + MANO_GL_UP + (f * MANO_J + j) * 12;
#pragma unroll
        for (int rr = 0; rr < 3; ++rr) {
#pragma unroll
          for (int cc = 0; cc < 3; ++cc)
            u[rr * 3 + cc] = fmaf(dtG[rr], L.d[cc], fmaf(dRG[rr * 3 + 2], L.R[cc * 3 + 2], fmaf(dRG[rr * 3 + 1], L.R[cc * 3 + 1], dRG[rr * 3] * L.R[cc * 3])));
          u[9 + rr] = dtG[rr];
        }
      }
    }
    __syncthreads();
  }
  float dR[9], dd[3] = {0.f, 0.f, 0.f};
  if (L.par >= 0) {
    const float* P = lds + MANO_L_A + (f * MANO_J + L.par) * 12;
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
#pragma unroll
      for (int cc = 0; cc < 3; ++cc) dR[rr * 3 + cc] = fmaf(P[6 + rr], dRG[6 + cc], fmaf(P[3 + rr], dRG[3 + cc], P[rr] * dRG[cc]));
      dd[rr] = fmaf(P[6 + rr], dtG[2], fmaf(P[3 + rr], dtG[1], P[rr] * dtG[0]));
    }
  } else {
#pragma unroll
    for (int e = 0; e < 9; ++e) dR[e] = dRG[e];
  }
  {
    float* o = lds + MANO_GL_DD + (f * MANO_J + j) * 3;
    o[0] = dd[0], o[1] = dd[1], o[2] = dd[2];
  }
  __syncthreads();
  {
    const float* G = lds + MANO_L_A + (f * MANO_J + j) * 12;
    float dJ[3];
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) dJ[rr] = dd[rr] - fmaf(G[6 + rr], dtA[2], fmaf(G[3 + rr], dtA[1], G[rr] * dtA[0]));
#pragma unroll 1
    for (int c = j + 1; c < MANO_J; ++c)
      if (children >> c & 1) {
        const float* u = lds + MANO_GL_DD + (f * MANO_J + c) * 3;
        dJ[0] -= u[0], dJ[1] -= u[1], dJ[2] -= u[2];
      }
    if (L.par < 0) dJ[0] += dtG[0], dJ[1] += dtG[1], dJ[2] += dtG[2];  // t_G of the root is J_0
    float* o = lds + MANO_GL_DJ + (f * MANO_J + j) * 3;
    o[0] = dJ[0], o[1] = dJ[1], o[2] = dJ[2];
  }
  if (j >= 1) {
#pragma unroll
    for (int e = 0; e < 9; ++e) dR[e] += lds[MANO_GL_DF + (MANO_NB + (j - 1) * 9 + e) * 16 + f];
  }
  {
    const float qw = L.q[0], qx = L.q[1], qy = L.q[2], qz = L.q[3];
    float gq[4];
    gq[0] = 2.f * (qz * (dR[3] - dR[1]) + qy * (dR[2] - dR[6]) + qx * (dR[7] - dR[5]));
    gq[1] = 2.f * (qy * (dR[1] + dR[3]) + qz * (dR[2] + dR[6]) + qw * (dR[7] - dR[5]) - 2.f * qx * (dR[4] + dR[8]));
    gq[2] = 2.f * (qx * (dR[1] + dR[3]) + qw * (dR[2] - dR[6]) + qz * (dR[5] + dR[7]) - 2.f * qy * (dR[0] + dR[8]));
    gq[3] = 2.f * (qw * (dR[3] - dR[1]) + qx * (dR[2] + dR[6]) + qy * (dR[5] + dR[7]) - 2.f * qz * (dR[0] + dR[4]));
    // q / max(|q|, 1e-12): above the clamp the component along q is removed, below it the denominator is a constant
    const float inv = 1.0f / fmaxf(L.nrm, 1e-12f);
    const float along = L.nrm >= 1e-12f ? qw * gq[0] + qx * gq[1] + qy * gq[2] + qz * gq[3] : 0.f;
    if (live) reinterpret_cast<float4*>(ga.dquat)[n * MANO_J + j] = make_float4(inv * (gq[0] - qw * along), inv * (gq[1] - qx * along),
                                                                                inv * (gq[2] - qy * along), inv * (gq[3] - qz * along));
  }
  __syncthreads();
  if (ga.dbetas && live && j < MANO_NB) {
    float s = 0.f;
    for (int jj = 0; jj < MANO_J; ++jj)
#pragma unroll
      for (int c = 0; c < 3; ++c) s = fmaf(a.jd[(jj * 3 + c) * MANO_NB + j], lds[MANO_GL_DJ + (f * MANO_J + jj) * 3 + c], s);
    ga.dbetas[n * MANO_NB + j] = s + lds[MANO_GL_DF + j * 16 + f];
  }
}
