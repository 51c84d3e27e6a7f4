/*
 * tamf_sdfgrid.h - C-ABI of the SDF-lattice sampler (libtamf_sdfgrid.so): how deep every hand vertex of every clip, frame and object
 * lies inside the object, read from the object's precomputed signed distance lattice (the SDFData file script/process_object_sdf.sh
 * writes) by a trilinear lookup, and the backward of that depth with respect to the hand vertices.  It is what the `pen` term of the
 * training losses is built on (model/interaction_loss.py).  The term is this package's own: the reference has no such loss.
 *
 * Conventions: those of tamf_contact.h.  Plain C types; every function returns 0 or a negative tamf_status (tamf_hip.h, included for
 * that enum only); the message of the calling thread's last failure is tamf_sdfgrid_last_error().  Every pointer is C-contiguous device
 * memory owned by the caller, on the current device; `stream` is a hipStream_t passed as void*.  Nothing synchronises, nothing
 * allocates, no state is kept between calls.  Invalid arguments launch nothing.
 *
 * THE GRID SET (G lattices, packed by the caller; sdfgrid.SdfGridSet does it):
 *   values   (grid_off[G],) f32   the lattices end to end.  Value (i R + j) R + k of grid g is the SDF at the object-frame point
 *                                 origin_g + (i, j, k) * step_g.  POSITIVE INSIDE (SDFData.sdf's "negative outside").
 *   grid_off (G+1,) int64         grid g owns values [grid_off[g], grid_off[g] + R_g^3)
 *   res      (G,)   int32         R_g in [2, 512]
 *   origin   (G,3)  f64           step (G,3) f64, every entry > 0
 * INPUTS, in the layouts of tamf_contact_forward:
 *   hand_verts (B,T,V,3) f32      obj_traj (B,nobj,T,9) f32 = tsl | rot6d      obj_num (B) int32 or NULL: the first obj_num[b] objects
 *   grid_id    (B,nobj) int32     the lattice of object o of clip b; -1: this object has no lattice         of clip b are real
 *
 * THE DEFINITION.  Everything is float64 from exactly widened float32 inputs, without fused multiply-adds (fp contract off), IEEE
 * division and a correctly rounded sqrt; a result is rounded ONCE to float32.   dot(u, v) = (u0 v0 + u1 v1) + u2 v2.
 *
 *   Pose.   t = tr[0..2], a1 = tr[3..5], a2 = tr[6..8] of the object's obj_traj row at the frame, eps = 2^-23 (float32's):
 *             n1 = sqrt(dot(a1, a1)), n1 = n1 > eps ? n1 : eps, b1 = a1 / n1 (per coordinate)
 *             dp = dot(b1, a2), b2 = a2 - dp b1, n2 = sqrt(dot(b2, b2)), n2 = n2 > eps ? n2 : eps, b2 = b2 / n2
 *             b3 = (b1y b2z - b1z b2y, b1z b2x - b1x b2z, b1x b2y - b1y b2x)
 *           R has the ROWS b1, b2, b3: the rotation tamf_contact_forward and tamf_transform_points build from the row (y = R p + t; the
 *           Gram-Schmidt of metrics/siv.tslrot6d_to_transf), here in float64.
 *           Object-frame point of the vertex x:  d = x - t,  p_k = (R_0k d_0 + R_1k d_1) + R_2k d_2   (R transposed).
 *   Cell.   u_k = (p_k - origin_k) / step_k.  If any u_k fails 0 <= u_k <= R - 1 the depth is 0 and the gradient is 0 (a comparison
 *           with a NaN is false: a NaN vertex or pose lands here).  Otherwise i_k = min(floor(u_k), R - 2), f_k = u_k - i_k (so
 *           u_k = R - 1 belongs to the last cell, with f_k = 1), and cell = (i_x R + i_y) R + i_z.
 *   Trilinear, z first.  s_abc = the value at corner (i_x + a, i_y + b, i_z + c):
 *             c_ab = s_ab0 + (s_ab1 - s_ab0) f_z        c_a = c_a0 + (c_a1 - c_a0) f_y        s = c_0 + (c_1 - c_0) f_x
 *           depth = s when s > 0, else 0.
 *   Gradient, non-zero only where s > 0:
 *             gx = c_1 - c_0
 *             gy = e_0 + (e_1 - e_0) f_x,   e_a = c_a1 - c_a0
 *             gz = m_0 + (m_1 - m_0) f_x,   m_a = d_a0 + (d_a1 - d_a0) f_y,   d_ab = s_ab1 - s_ab0
 *             q_k = g_k / step_k,   world gradient w_r = (R_r0 q_0 + R_r1 q_1) + R_r2 q_2
 *           g_hand[b,t,v] = the sum, from 0.0, over the real objects o with a lattice and s > 0, ascending, of g_depth[b,o,t,v] * w,
 *           in float64, rounded once.
 *
 * Determinism: no atomics, one writer per output element, every sum in a fixed order.  The same call gives the same bits, and the rows
 * of a clip depend on that clip's inputs only - not on B or on the clip's place in the batch.
 *
 * Limits (anything else is TAMF_ERR_INVALID with a message, and nothing is launched): B, T, V, nobj >= 1; B * nobj <= 65535;
 * T * V <= 2^31 - 1; G >= 1; a null mandatory pointer.  What lies in DEVICE memory cannot be read by a call that does not synchronise:
 * that every grid_id is in [-1, G), every R_g in [2, 512] and every step > 0 is the caller's word (sdfgrid.py checks all three on the
 * host before it uploads them).  The kernels never read outside the set for it: an object whose grid_id is outside [0, G), or whose
 * R_g is outside [2, 512], is treated as one without a lattice.
 */
#ifndef TAMF_SDFGRID_H
#define TAMF_SDFGRID_H

#include <stdint.h>

#include "tamf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TAMF_SDFGRID_MIN_RES 2
#define TAMF_SDFGRID_MAX_RES 512

/* message of the last failure of a call made by THIS thread ("" when none) */
const char* tamf_sdfgrid_last_error(void);

/* One launch on `stream` over all clips, objects, frames and vertices:
 *   depth_out (B,nobj,T,V) f32   the depth of THE DEFINITION
 *   cell_out  (B,nobj,T,V) i32 or NULL: the flat index of the cell's low corner in its lattice, -1 where the depth is 0
 * Rows of padded objects (o >= obj_num[b]) and of objects without a lattice are written as 0 (and -1 for cell). */
int tamf_sdfgrid_forward(const float* values_dev, const int64_t* grid_off_dev, const int32_t* res_dev, const double* origin_dev,
                         const double* step_dev, int32_t G, const float* hand_verts_dev, const float* obj_traj_dev,
                         const int32_t* grid_id_dev, const int32_t* obj_num_dev, int32_t B, int32_t T, int32_t V, int32_t nobj,
                         float* depth_out_dev, int32_t* cell_out_dev, void* stream);

/* The vector-Jacobian product of depth with respect to hand_verts, recomputed from the inputs (nothing saved by the forward is needed):
 *   g_depth (B,nobj,T,V) f32: the upstream gradient          g_hand_out (B,T,V,3) f32: overwritten, every element
 * There is no gradient for the trajectory or the lattice: they are data. */
int tamf_sdfgrid_backward(const float* values_dev, const int64_t* grid_off_dev, const int32_t* res_dev, const double* origin_dev,
                          const double* step_dev, int32_t G, const float* hand_verts_dev, const float* obj_traj_dev,
                          const int32_t* grid_id_dev, const int32_t* obj_num_dev, int32_t B, int32_t T, int32_t V, int32_t nobj,
                          const float* g_depth_dev, float* g_hand_out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TAMF_SDFGRID_H */
