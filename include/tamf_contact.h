/*
 * tamf_contact.h - C-ABI of the contact-distance kernels (libtamf_contact.so): the signed nearest-neighbour distances between a
 * frame's hand vertices and an object's points, in both directions and WITH the indices of the nearest, and their backward with
 * respect to the hand vertices.  They are what the training losses' `dist_h` / `dist_o` terms are built on (the reference's
 * model/loss/chamfer_distance.py:4-64 point2point_signed as model/interaction_segment_extra_loss.py:146-178 calls it).
 *
 * Layout: that of tamf_h2o_dist (tamf_hip.h), everything fp32, C-contiguous device memory owned by the caller:
 *   hand_verts (B,T,V,3)     hand_normals (B,T,V,3) or NULL     obj_traj (B,nobj,T,9) = tsl | rot6d
 *   obj_points (B,nobj,P,3) in the object frame, moved to the frame's pose on the fly (y = R p + t, R from the Gram-Schmidt of rot6d)
 *   obj_num (B) int32 or NULL: the first obj_num[b] objects of clip b are real.  The caller keeps it inside [1, nobj].
 *
 * The nearest is the candidate with the smallest squared distance dx^2 + dy^2 + dz^2 (fp32); on an exact tie the LOWEST index wins
 * (a strict `<` scan in ascending order).  This is this package's own convention: it is what torch.argmin gives on the CPU.  The
 * reference takes its indices from the external chamfer_distance CUDA package, whose source was not available to this project, so
 * its tie rule could not be confirmed.
 *
 * Limits (anything else is TAMF_ERR_INVALID with a message, and nothing is launched): 1 <= V <= 1024; B, T, nobj, P >= 1;
 * B * nobj <= 65535; P <= 67107840 (65535 chunks of 1024); a null mandatory pointer.  Non-finite inputs are outside the contract
 * (the indices still stay inside their ranges).
 *
 * Determinism: no atomics, one writer per output element, every sum in a fixed order.  The same call gives the same bits, and the
 * rows of a clip depend on that clip's inputs only - not on B or on the clip's place in the batch.
 *
 * Conventions: those of tamf_hip.h (included for the tamf_status enum only).  Every function returns 0 or a negative tamf_status;
 * the message of the calling thread's last failure is tamf_contact_last_error().  `stream` is a hipStream_t passed as void*.
 * Nothing synchronises.
 */
#ifndef TAMF_CONTACT_H
#define TAMF_CONTACT_H

#include <stdint.h>

#include "tamf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* message of the last failure of a call made by THIS thread ("" when none) */
const char* tamf_contact_last_error(void);

/* Per object (NOT merged over the objects), enqueued on `stream`:
 *   h2o        (B,nobj,T,V) f32: distance of every hand vertex to its nearest point of object o
 *   h2o_idx    (B,nobj,T,V) i32: that point's index in [0, P)
 *   o2h_signed (B,nobj,T,P) f32: distance of every object point y to its nearest hand vertex x, times sign(n . (y - x)) with n the
 *                                hand normal at x; the sign is -1, 0 or +1 as torch.sign gives it.  Unsigned when hand_normals is NULL.
 *   o2h_idx    (B,nobj,T,P) i32: that vertex's index in [0, V)
 * Each direction is an output PAIR: both pointers, or both NULL to skip the direction; skipping both is TAMF_ERR_INVALID.
 * Rows of padded objects (o >= obj_num[b]) are written as 0, with index -1.
 * The minimum over a clip's real objects of h2o equals tamf_h2o_dist's output bit for bit. */
int tamf_contact_forward(const float* hand_verts_dev, const float* hand_normals_dev, const float* obj_traj_dev, const float* obj_points_dev,
                         const int32_t* obj_num_dev, int32_t B, int32_t T, int32_t V, int32_t nobj, int32_t P, float* h2o_out_dev,
                         int32_t* h2o_idx_out_dev, float* o2h_signed_out_dev, int32_t* o2h_idx_out_dev, void* stream);

/* The vector-Jacobian product with respect to hand_verts of what tamf_contact_forward computes (the indices and the signs are
 * piecewise constant, so they carry no derivative; the reference sends none through the normals either: they only enter a sign).
 * With u(d) = d / |d| and u(0) = 0 (a zero distance gives a zero gradient, as torch's norm backward does):
 *   g_hand[b,t,v] = sum over the real objects o, ascending, of
 *         g_h2o[b,o,t,v] * u(x_v - y_near)                                           y_near = point h2o_idx[b,o,t,v] of object o
 *       + sum over the points j, ascending, with o2h_idx[b,o,t,j] == v of
 *         g_o2h[b,o,t,j] * sign(o2h_signed[b,o,t,j]) * u(x_v - y_j)
 *   h2o_idx, o2h_signed, o2h_idx: the forward's outputs for the same inputs (the sign is read from o2h_signed: no normals needed)
 *   g_h2o (B,nobj,T,V) or NULL, g_o2h (B,nobj,T,P) or NULL: the upstream gradients; NULL means zeros and the direction's saved
 *         tensors may then be NULL too; both NULL is TAMF_ERR_INVALID
 *   g_hand_out (B,T,V,3): overwritten
 * There is no gradient for the trajectory or the points: the reference treats them as data.  An index outside its range (-1 of a
 * padded row) contributes nothing. */
int tamf_contact_backward(const float* hand_verts_dev, const float* obj_traj_dev, const float* obj_points_dev, const int32_t* obj_num_dev,
                          int32_t B, int32_t T, int32_t V, int32_t nobj, int32_t P, const int32_t* h2o_idx_dev, const float* g_h2o_dev,
                          const float* o2h_signed_dev, const int32_t* o2h_idx_dev, const float* g_o2h_dev, float* g_hand_out_dev,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TAMF_CONTACT_H */
