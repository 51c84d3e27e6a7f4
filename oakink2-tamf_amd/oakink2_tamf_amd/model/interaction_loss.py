"""The reference's two training losses WITH their contact-distance terms: HandReconstructionLoss (model/reconstruction_loss.py) plus
`dist_h` / `dist_o` of InteractionSegmentExtraLoss (model/interaction_segment_extra_loss.py:146-178) and `dist_h` of
SegmentRefineModelLoss (model/segment_refine_model_loss.py:64-72), with the reference's semantics and key names.

The hot path is the brute-force nearest neighbour between the hand's vertices and the objects' points, in both directions, per clip,
object and frame, for the prediction and for the ground truth: contact.signed_contact_distance (HIP forward and backward).  The
reference calls it per clip and per object in Python; `forward` makes one differentiable call per hand side for the prediction and
one forward-only call for the ground truth.  The hand normals come from geometry.vertex_normals outside the graph: they enter the
distance through a sign only, which has a zero derivative, so the reference's own autograd sends nothing through them either.

Like the other terms, the two are reduced in float64 and summed over the clips.

`pen` (coef_pen_loss) is this package's own term, not the reference's: how much deeper the predicted hand's vertices lie inside the
objects than the ground truth's do, the depth read from the objects' signed distance lattices (sdfgrid.penetration_depth: HIP forward
and backward).  With its coefficient at 0, the default, nothing of it runs and the loss dict has no `pen` key."""
from __future__ import annotations

import numpy as np
import torch

from .reconstruction_loss import HandReconstructionLoss

# The reference builds its per-point weights as a float32 tensor whatever the inputs' dtype, so its 0.1 is float32's.
W_FAR, W_PENETRATION = float(np.float32(0.1)), 1.5
NEAR_BELOW, NEAR_ABOVE = 0.01, -0.005  # the window of the ground truth's signed distance inside which a point keeps weight 1


class HandInteractionLoss(HandReconstructionLoss):
    """HandReconstructionLoss that accepts positive `coef_dist_h_loss` / `coef_dist_o_loss` (the reference's config/loss_param.yml:
    0.1 / 1.0).  `contact_fn(hand_verts, hand_normals, obj_traj, obj_points, obj_num, want_o2h=...)` -> (o2h_signed, h2o, o2h_idx) per
    object defaults to contact.signed_contact_distance, `normals_fn(verts, faces)` to geometry.vertex_normals; the faces are the
    layers' `th_faces`.  `v_weights` should be given as the reference loads it, float32: its power 1 / 2.5 is taken in that dtype.
    A positive `coef_pen_loss` needs `sdf_grids` (an sdfgrid.SdfGridSet on the device) or `pen_fn(hand_verts, obj_traj, grid_id,
    obj_num) -> depth (B, nobj, T, V)`, which defaults to the set's penetration_depth; the batch then carries `sdf_grid_id` (B, nobj)."""

    def __init__(self, layer_rh, layer_lh, vpe, v_weights, coef_rec_joint_loss, coef_rec_vert_loss, coef_edge_len_loss=0.0,
                 coef_dist_h_loss=0.0, coef_dist_o_loss=0.0, contact_fn=None, normals_fn=None, coef_pen_loss=0.0, sdf_grids=None, pen_fn=None):
        super().__init__(layer_rh, layer_lh, vpe, v_weights, coef_rec_joint_loss, coef_rec_vert_loss, coef_edge_len_loss)
        if coef_dist_h_loss < 0.0 or coef_dist_o_loss < 0.0:
            raise ValueError("coef_dist_h_loss and coef_dist_o_loss must not be negative")
        self.coef_dist_h_loss, self.coef_dist_o_loss = float(coef_dist_h_loss), float(coef_dist_o_loss)
        self.register_buffer("v_weights2", torch.pow(self.v_weights, 1.0 / 2.5))
        self._contact_fn, self._normals_fn = contact_fn, normals_fn
        if coef_pen_loss < 0.0:
            raise ValueError("coef_pen_loss must not be negative")
        if coef_pen_loss > 0.0 and sdf_grids is None and pen_fn is None:
            raise ValueError("coef_pen_loss > 0 needs the objects' signed distance lattices: pass sdf_grids (sdfgrid.SdfGridSet) or a pen_fn")
        self.coef_pen_loss = float(coef_pen_loss)
        self._pen_fn = pen_fn if pen_fn is not None or sdf_grids is None else sdf_grids.penetration_depth

    def _pen_term(self, verts_p, verts_g, mask, obj_traj, grid_id, obj_num):
        """per-clip `pen`, (nb,) float64: e = relu(depth(prediction) - depth(ground truth)), the excess over what the ground truth
        itself penetrates (mocap data does, a little), reduced as `dist_h` is in _dist_terms but without vertex weights: masked frames,
        _mask_coef, the mean over frames and vertices, the mean over the clip's real objects."""
        f64 = torch.float64
        with torch.no_grad():
            depth_g = self._pen_fn(verts_g, obj_traj, grid_id, obj_num)  # (forward only)
        depth_p = self._pen_fn(verts_p, obj_traj, grid_id, obj_num)
        nobj = depth_p.shape[1]
        num = torch.as_tensor([int(n) for n in obj_num], device=depth_p.device)
        real = (torch.arange(nobj, device=depth_p.device)[None, :] < num[:, None]).to(f64)  # (nb, nobj)
        coef = self._mask_coef(mask).to(f64) / num.to(f64)
        e = torch.relu(depth_p - depth_g).to(f64) * mask.to(f64)[:, None, :, None]
        return coef * (e.mean(dim=(-2, -1)) * real).sum(dim=1)

    def _fns(self):
        contact_fn, normals_fn = self._contact_fn, self._normals_fn
        if contact_fn is None:
            from ..contact import signed_contact_distance as contact_fn
        if normals_fn is None:
            from ..geometry import vertex_normals as normals_fn
        return contact_fn, normals_fn

    def _dist_terms(self, layer, verts_p, verts_g, mask, obj_traj, obj_points, obj_num):
        """per-clip `dist_h`, `dist_o`, (nb,) float64 each (0.0 when disabled), of one hand side's (nb, T, V, 3) vertices, its (nb, T)
        mask, obj_traj (nb, nobj, T, 9), obj_points (nb, nobj, P, 3) and obj_num (nb ints)"""
        f64 = torch.float64
        contact_fn, normals_fn = self._fns()
        want_o2h = self.coef_dist_o_loss > 0.0
        nobj = obj_points.shape[1]
        with torch.no_grad():
            faces = layer.th_faces
            n_p = normals_fn(verts_p.detach(), faces) if want_o2h else None
            n_g = normals_fn(verts_g, faces) if want_o2h else None
            o2h_g, h2o_g, _ = contact_fn(verts_g, n_g, obj_traj, obj_points, obj_num, want_o2h=want_o2h)  # (forward only)
        o2h, h2o, _ = contact_fn(verts_p, n_p, obj_traj, obj_points, obj_num, want_o2h=want_o2h)
        num = torch.as_tensor([int(n) for n in obj_num], device=h2o.device)
        real = (torch.arange(nobj, device=h2o.device)[None, :] < num[:, None]).to(f64)  # (nb, nobj)
        coef = self._mask_coef(mask).to(f64) / num.to(f64)
        m = mask.to(f64)[:, None, :, None]
        dist_h = dist_o = 0.0
        if self.coef_dist_h_loss > 0.0:
            d = (h2o.abs() - h2o_g.abs()).abs().to(f64) * self.v_weights2.to(f64) * m
            dist_h = coef * (d.mean(dim=(-2, -1)) * real).sum(dim=1)
        if want_o2h:
            with torch.no_grad():
                w = torch.ones_like(o2h_g, dtype=f64)
                w[~((o2h_g < NEAR_BELOW) & (o2h_g > NEAR_ABOVE))] = W_FAR  # less weight for far away points
                w[o2h.detach() < 0.0] = W_PENETRATION  # more weight for penetration
            d = (o2h - o2h_g).abs().to(f64) * w * m
            dist_o = coef * (d.mean(dim=(-2, -1)) * real).sum(dim=1)
        return dist_h, dist_o

    def forward(self, model_output, batch):
        """HandReconstructionLoss.forward's inputs plus batch `obj_traj` (B, nobj, T, 9) = tsl | rot6d, `obj_points` (B, nobj, P, 3) in
        the object frame and `obj_num` (B counts in [1, nobj]; None: all nobj are real).  -> (loss, loss_dict) with the reference's
        keys; every term is summed over the clips and is a float64 scalar.  With a positive coef_pen_loss the batch also carries
        `sdf_grid_id` (B, nobj) integers (-1: no lattice), the loss gains coef_pen_loss * pen and the dict the key `pen`."""
        dist = self.coef_dist_h_loss > 0.0 or self.coef_dist_o_loss > 0.0
        pen = self.coef_pen_loss > 0.0
        total = {"rec_joint": 0.0, "rec_vert": 0.0, "edge_len": 0.0, "dist_h": 0.0, "dist_o": 0.0}
        B = model_output.shape[0]
        if dist:
            obj_traj, obj_points = batch["obj_traj"], batch["obj_points"]
            if obj_traj.dim() != 4 or obj_points.dim() != 4 or obj_traj.shape[0] != B or obj_points.shape[0] != B:
                raise ValueError(f"obj_traj / obj_points: expected (B, nobj, T, 9) and (B, nobj, P, 3) with B = {B}, got "
                                 f"{tuple(obj_traj.shape)} and {tuple(obj_points.shape)}")
        if pen:
            total["pen"] = 0.0
            obj_traj, grid_id = batch["obj_traj"], torch.as_tensor(batch["sdf_grid_id"])
            if obj_traj.dim() != 4 or obj_traj.shape[0] != B or tuple(grid_id.shape) != (B, obj_traj.shape[1]):
                raise ValueError(f"obj_traj / sdf_grid_id: expected (B, nobj, T, 9) and (B, nobj) with B = {B}, got "
                                 f"{tuple(obj_traj.shape)} and {tuple(grid_id.shape)}")
        if dist or pen:
            obj_num = batch.get("obj_num")
            obj_num = [int(obj_points.shape[1] if dist else obj_traj.shape[1])] * B if obj_num is None else [int(n) for n in obj_num]
            if len(obj_num) != B:
                raise ValueError(f"obj_num: expected {B} counts, got {len(obj_num)}")
        for layer, idx, verts_p, joints_p, verts_g, joints_g, mask in self._per_side(model_output, batch):
            terms = dict(zip(("rec_joint", "rec_vert", "edge_len"), self._terms(verts_p, joints_p, verts_g, joints_g, mask, True)))
            if dist:
                dev = verts_p.device
                terms["dist_h"], terms["dist_o"] = self._dist_terms(layer, verts_p, verts_g, mask, obj_traj.to(dev)[idx], obj_points.to(dev)[idx],
                                                                    [obj_num[int(i)] for i in idx])
            if pen:
                dev = verts_p.device
                terms["pen"] = self._pen_term(verts_p, verts_g, mask, obj_traj.to(dev)[idx], grid_id.to(dev)[idx], [obj_num[int(i)] for i in idx])
            for key, term in terms.items():
                if torch.is_tensor(term):
                    total[key] = total[key] + term.sum()
        loss = (self.coef_rec_joint_loss * total["rec_joint"] + self.coef_rec_vert_loss * total["rec_vert"]
                + self.coef_edge_len_loss * total["edge_len"] + self.coef_dist_h_loss * total["dist_h"] + self.coef_dist_o_loss * total["dist_o"])
        if pen:
            loss = loss + self.coef_pen_loss * total["pen"]
        return loss, {"loss": loss, **total}

    def refine_terms(self, output, batch):
        """HandReconstructionLoss.refine_terms plus SegmentRefineModelLoss's `dist_h` on output `refine_h2o_dist` / `target_h2o_dist`
        (B, T, V), the merged hand-to-object distances (contact.merged_h2o_dist carries the gradient), and, with a positive
        coef_pen_loss, `pen` on output `refine_hand_verts` / `target_hand_verts` with batch `obj_traj`, `sdf_grid_id` and `obj_num`.
        Every term is the mean over the clips."""
        loss, d = super().refine_terms(output, batch)
        if self.coef_dist_h_loss > 0.0:
            f64 = torch.float64
            r, t = output["refine_h2o_dist"], output["target_h2o_dist"]
            mask = batch["mask"].to(r.dtype)
            e = (r.abs() - t.abs()).abs().to(f64) * mask.to(f64).unsqueeze(-1) * self.v_weights2.to(f64)
            dist_h = (self._mask_coef(mask).to(f64) * e.mean(dim=(-2, -1))).mean()
            loss = loss + self.coef_dist_h_loss * dist_h
            d = {**d, "loss": loss, "dist_h": dist_h}
        if self.coef_pen_loss > 0.0:
            r = output["refine_hand_verts"]
            traj, grid_id = batch["obj_traj"], torch.as_tensor(batch["sdf_grid_id"])
            obj_num = batch.get("obj_num")
            obj_num = [int(traj.shape[1])] * r.shape[0] if obj_num is None else [int(n) for n in obj_num]
            pen = self._pen_term(r, output["target_hand_verts"], batch["mask"].to(r.dtype), traj.to(r.device), grid_id.to(r.device), obj_num).mean()
            loss = loss + self.coef_pen_loss * pen
            d = {**d, "loss": loss, "pen": pen}
        return loss, d


__all__ = ["HandInteractionLoss"]
