"""The reconstruction part of the reference's two training losses on differentiable MANO layers: the `rec_joint`, `rec_vert` and
`edge_len` terms of InteractionSegmentExtraLoss (model/interaction_segment_extra_loss.py:85-144, 183-197) and the `rec_joint` /
`rec_vert` terms of SegmentRefineModelLoss (model/segment_refine_model_loss.py:40-62), with the reference's semantics and key names.

The hot path is the MANO layer (mano.HipManoLayer(differentiable=True): HIP forward and backward); everything here is plumbing in
plain torch ops that autograd carries - the pose decode works on 16 small matrices per frame, the reductions on what the layer
returned.  Where the reference loops over the clips of a batch in Python and calls its layer twice per clip, `forward` makes one
differentiable layer call per hand side over all of that side's predicted frames, and one inference call for their ground truth.

Every loss term is reduced in float64 and returned as a float64 scalar, whatever the inputs' dtype (the reference returns the inputs'
dtype): a float32 sum over up to T * E * 3 values would add its own rounding to the layer's.  The gradients that reach the model output
are in its dtype.

Not here: the contact-distance terms `dist_h` / `dist_o`; this class refuses a positive coefficient for them with
NotImplementedError.  They are model/interaction_loss.HandInteractionLoss, a subclass, on the nearest-neighbour kernels of contact.py.
(They need the backward of the signed nearest-neighbour distance with respect to the hand vertices only, not one of the vertex normals
as the refusal's message still says: the normals enter through a sign, which has a zero derivative.)"""
from __future__ import annotations

import torch


def _unit(v: torch.Tensor) -> torch.Tensor:
    return v / torch.linalg.vector_norm(v, dim=-1, keepdim=True).clamp_min(1e-12)


def rot6d_to_rotmat(d6: torch.Tensor) -> torch.Tensor:
    """(..., 6) -> (..., 3, 3), the continuous 6-D representation of Zhou et al. 2019 (section B): the two 3-vectors are
    orthonormalised (Gram-Schmidt) into the first two ROWS, the third row is their cross product.  A zero vector gives a zero row."""
    first, second = d6.unflatten(-1, (2, 3)).unbind(-2)
    row0 = _unit(first)
    row1 = _unit(second - row0 * torch.linalg.vecdot(row0, second).unsqueeze(-1))
    return torch.stack([row0, row1, torch.linalg.cross(row0, row1)], dim=-2)


def rotmat_to_quat(rotmat: torch.Tensor) -> torch.Tensor:
    """(..., 3, 3) -> (..., 4) in (w, x, y, z), w >= 0, by the pivoting method of Shepperd (1978): with sq = (4 w^2, 4 x^2, 4 y^2, 4 z^2)
    = (1 + tr, 1 + 2 m_kk - tr), the symmetric table

        [ sq_0        m21 - m12   m02 - m20   m10 - m01 ]
        [ .           sq_1        m01 + m10   m02 + m20 ]  =  4 q q^T
        [ .           .           sq_2        m12 + m21 ]
        [ .           .           .           sq_3      ]

    holds 4 q_k q in row k; the row of the largest sq_k is the best conditioned and is divided by 2 sqrt(sq_k).  The divisor is floored
    at 0.2, which only matters for an input that is no rotation (for a rotation the largest sq_k is at least 1)."""
    m, mt = rotmat, rotmat.transpose(-1, -2)
    diag = torch.diagonal(m, dim1=-2, dim2=-1)
    tr = diag.sum(-1, keepdim=True)
    sq = torch.cat([1.0 + tr, 1.0 + 2.0 * diag - tr], dim=-1).clamp_min(0.0)
    skew = m - mt
    vec = torch.stack([skew[..., 2, 1], skew[..., 0, 2], skew[..., 1, 0]], dim=-1)
    lower = m + mt + torch.diag_embed(sq[..., 1:] - 2.0 * diag)
    table = torch.cat([torch.cat([sq[..., :1], vec], dim=-1).unsqueeze(-2), torch.cat([vec.unsqueeze(-1), lower], dim=-1)], dim=-2)
    k = sq.argmax(dim=-1, keepdim=True)
    row = torch.take_along_dim(table, k.unsqueeze(-1), dim=-2).squeeze(-2)
    q = row / (2.0 * torch.sqrt(torch.take_along_dim(sq, k, dim=-1).clamp_min(0.01)))
    return torch.where(q[..., :1] < 0, -q, q)


def decode_pose_repr(pose_repr: torch.Tensor):
    """(..., 3 + 6 J) -> tsl (..., 3), quat (..., J, 4): what geometry.pose_repr_to_quat computes, in torch ops that carry autograd"""
    F = pose_repr.shape[-1]
    J = (F - 3) // 6
    if 3 + 6 * J != F:
        raise ValueError(f"pose representation must be 3 + 6 J wide, got {F}")
    rot6d = pose_repr[..., 3:].reshape(pose_repr.shape[:-1] + (J, 6))
    return pose_repr[..., :3], rotmat_to_quat(rot6d_to_rotmat(rot6d))


class HandReconstructionLoss(torch.nn.Module):
    """`layer_rh`, `layer_lh`: objects with the layer contract (`layer(pose_coeffs=(N,16,4), betas=(N,10)) -> .verts, .joints`)
    through which autograd passes - mano.make_mano_differentiable's layers, or any torch layer.  `vpe` (E, 2) integer vertex pairs
    (the reference's `verts_per_edge` file) and `v_weights` (V,) per-vertex weights (its `rhand_weight` file) are the user's arrays:
    the reference ships neither.  The coefficients are those of the reference's config/loss_param*.yml."""

    def __init__(self, layer_rh, layer_lh, vpe, v_weights, coef_rec_joint_loss, coef_rec_vert_loss, coef_edge_len_loss=0.0,
                 coef_dist_h_loss=0.0, coef_dist_o_loss=0.0):
        super().__init__()
        if coef_dist_h_loss > 0.0 or coef_dist_o_loss > 0.0:
            raise NotImplementedError("dist_h / dist_o are not built: they need the backward of the signed nearest-neighbour distance "
                                      "(tamf_h2o_dist) and of the vertex normals (tamf_vertex_normals), which do not exist yet; "
                                      "set coef_dist_h_loss and coef_dist_o_loss to 0")
        self.layers = {"rh": layer_rh, "lh": layer_lh}  # (a dict: the layers are not modules and hold no parameters)
        vpe = torch.as_tensor(vpe)
        if vpe.dim() != 2 or vpe.shape[1] != 2 or vpe.dtype.is_floating_point:
            raise ValueError(f"vpe: expected an integer (E, 2) array, got {vpe.dtype} {tuple(vpe.shape)}")
        v_weights = torch.as_tensor(v_weights)
        if v_weights.dim() != 1:
            raise ValueError(f"v_weights: expected (V,), got {tuple(v_weights.shape)}")
        if vpe.numel() and not 0 <= int(vpe.min()) <= int(vpe.max()) < v_weights.shape[0]:
            raise ValueError("vpe: vertex ids outside [0, V)")
        self.register_buffer("vpe", vpe.to(torch.long))
        self.register_buffer("v_weights", v_weights.to(torch.get_default_dtype() if not v_weights.dtype.is_floating_point else v_weights.dtype))
        self.coef_rec_joint_loss, self.coef_rec_vert_loss = float(coef_rec_joint_loss), float(coef_rec_vert_loss)
        self.coef_edge_len_loss = float(coef_edge_len_loss)
        self.coef_dist_h_loss = self.coef_dist_o_loss = 0.0

    @staticmethod
    def _mask_coef(mask):
        """(B, T) -> (B,): T / sum(mask), outside the graph; a clip without a valid frame is an error (the reference divides by zero)"""
        with torch.no_grad():
            total = mask.sum(dim=1)
            if bool((total <= 0).any()):
                raise ValueError("mask: a clip has no valid frame")
            return float(mask.shape[1]) / total

    def _terms(self, verts_pred, joints_pred, verts_gt, joints_gt, mask, edges: bool):
        """per-clip terms, (B,) float64 each (0.0 when disabled), of (B, T, V | 21, 3) tensors and the (B, T) mask"""
        # The means run in float64 whatever the inputs' dtype: B * T * V values once per step is not a hot path, and the reported terms
        # then carry the layer's rounding only, not that of a float32 sum over up to T * E * 3 values.
        f64 = torch.float64
        coef = self._mask_coef(mask).to(f64)
        rec_joint = rec_vert = edge_len = 0.0
        if self.coef_rec_joint_loss > 0.0:
            d = ((joints_pred - joints_gt) ** 2).sum(-1).to(f64) * mask.unsqueeze(-1)
            rec_joint = coef * d.mean(dim=(-2, -1))
        if self.coef_rec_vert_loss > 0.0:
            d = ((verts_pred - verts_gt) ** 2).sum(-1).to(f64) * mask.unsqueeze(-1)
            rec_vert = coef * (d * self.v_weights.to(f64) ** 2).mean(dim=(-2, -1))
        if edges and self.coef_edge_len_loss > 0.0:
            e_pred = verts_pred[:, :, self.vpe[:, 0]] - verts_pred[:, :, self.vpe[:, 1]]
            e_gt = verts_gt[:, :, self.vpe[:, 0]] - verts_gt[:, :, self.vpe[:, 1]]
            edge_len = coef * ((e_pred - e_gt).abs().to(f64) * mask[:, :, None, None]).mean(dim=(-3, -2, -1))
        return rec_joint, rec_vert, edge_len

    def _per_side(self, model_output, batch):
        """The decode + MANO calls of `forward`, per hand side present in the batch: yields (layer, idx, verts_pred, joints_pred, verts_gt,
        joints_gt, mask[idx]) with idx the side's clips (a LongTensor) and (nb, T, V | 21, 3) tensors in the model output's dtype.  One
        differentiable layer call per side over all of its predicted frames, one inference call for their ground truth."""
        B, T = model_output.shape[0], model_output.shape[3]
        pred = model_output.squeeze(2).permute(0, 2, 1)  # (B, T, 99)
        gt, shape, mask, sides = batch["pose_repr"], batch["shape"], batch["mask"], list(batch["hand_side"])
        if len(sides) != B or any(s not in self.layers for s in sides):
            raise ValueError(f"unexpected hand_side: {sides}")
        mask = mask.to(pred.dtype)
        for side, layer in self.layers.items():
            rows = [i for i, s in enumerate(sides) if s == side]
            if not rows:
                continue
            idx = torch.as_tensor(rows, device=pred.device)
            nb = len(rows)
            tsl_p, quat_p = decode_pose_repr(pred[idx])
            with torch.no_grad():
                tsl_g, quat_g = decode_pose_repr(gt[idx].to(pred.dtype))
            betas = shape[idx].to(pred.dtype).reshape(nb * T, -1)
            out = layer(pose_coeffs=quat_p.reshape(nb * T, -1, 4), betas=betas)
            with torch.no_grad():  # (the ground truth needs no backward: an inference call)
                out_g = layer(pose_coeffs=quat_g.reshape(nb * T, -1, 4), betas=betas)
            verts_p = out.verts.reshape(nb, T, -1, 3).to(pred.dtype) + tsl_p.unsqueeze(2)
            joints_p = out.joints.reshape(nb, T, -1, 3).to(pred.dtype) + tsl_p.unsqueeze(2)
            verts_g = out_g.verts.reshape(nb, T, -1, 3).to(pred.dtype) + tsl_g.unsqueeze(2)
            joints_g = out_g.joints.reshape(nb, T, -1, 3).to(pred.dtype) + tsl_g.unsqueeze(2)
            yield layer, idx, verts_p, joints_p, verts_g, joints_g, mask[idx]

    def forward(self, model_output, batch):
        """model_output (B, 99, 1, T): the generator's predicted pose representation; batch: `hand_side` (B strings "rh" / "lh"),
        `shape` (B, T, 10), `mask` (B, T), `pose_repr` (B, T, 99) the ground truth.  -> (loss, loss_dict) with the reference's keys;
        every term is summed over the clips, as in the reference, and is a float64 scalar (see _terms)."""
        total = {"rec_joint": 0.0, "rec_vert": 0.0, "edge_len": 0.0}
        for _, _, verts_p, joints_p, verts_g, joints_g, mask in self._per_side(model_output, batch):
            for key, term in zip(("rec_joint", "rec_vert", "edge_len"), self._terms(verts_p, joints_p, verts_g, joints_g, mask, True)):
                if torch.is_tensor(term):
                    total[key] = total[key] + term.sum()
        loss = (self.coef_rec_joint_loss * total["rec_joint"] + self.coef_rec_vert_loss * total["rec_vert"]
                + self.coef_edge_len_loss * total["edge_len"])
        return loss, {"loss": loss, **total, "dist_h": 0.0, "dist_o": 0.0}

    def refine_terms(self, output, batch):
        """SegmentRefineModelLoss's reconstruction terms on already decoded tensors: output `refine_hand_joints` / `target_hand_joints`
        (B, T, 21, 3), `refine_hand_verts` / `target_hand_verts` (B, T, V, 3); batch `mask` (B, T).  Every term is the mean over the
        clips.  -> (loss, loss_dict) with the reference's keys."""
        mask = batch["mask"].to(output["refine_hand_verts"].dtype)
        rec_joint, rec_vert, _ = self._terms(output["refine_hand_verts"], output["refine_hand_joints"], output["target_hand_verts"],
                                             output["target_hand_joints"], mask, False)
        rec_joint = rec_joint.mean() if torch.is_tensor(rec_joint) else rec_joint
        rec_vert = rec_vert.mean() if torch.is_tensor(rec_vert) else rec_vert
        loss = self.coef_rec_joint_loss * rec_joint + self.coef_rec_vert_loss * rec_vert
        return loss, {"loss": loss, "rec_joint": rec_joint, "rec_vert": rec_vert, "dist_h": 0.0}


__all__ = ["HandReconstructionLoss", "decode_pose_repr", "rot6d_to_rotmat", "rotmat_to_quat"]
