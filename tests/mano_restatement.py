"""Plain-torch restatement of the MANO layer (steps 1-7 of csrc/tamf_mano.h), written from the published definition (SMPL eq. 2-10,
MANO section 3) - dtype-generic: float64 is the yardstick, float32 is the arithmetic a torch MANO layer would run (the skinning
transforms are blended first and applied once, as such layers do).  Not the code under test."""
import torch


def to_torch(arrays, dtype, device="cpu"):
    """ManoArrays (or a dict of numpy arrays) -> dict of tensors in `dtype`"""
    get = (lambda k: getattr(arrays, k)) if not isinstance(arrays, dict) else arrays.__getitem__
    out = {k: torch.as_tensor(get(k)).to(device=device, dtype=dtype) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights")}
    out["parents"] = [int(p) for p in get("parents")]
    out["tip_ids"] = [int(t) for t in get("tip_ids")]
    out["joint_order"] = [int(t) for t in get("joint_order")]
    return out


def quat_to_rotmat(q):
    """(..., 4) in (w, x, y, z), normalised as q / max(|q|, 1e-12) -> (..., 3, 3)"""
    q = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    w, x, y, z = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=-1)
    return R.reshape(q.shape[:-1] + (3, 3))


def mano_forward(m, quat, betas, center_idx=0):
    """m: to_torch(...); quat (N,16,4), betas (N,10) in m's dtype -> verts (N,V,3), joints (N,21,3), chain joints (N,16,3) uncentred"""
    N = quat.shape[0]
    R = quat_to_rotmat(quat)                                                      # 1
    eye = torch.eye(3, dtype=R.dtype, device=R.device)
    feat = (R[:, 1:] - eye).reshape(N, 135)                                       # 2
    v_shaped = m["v_template"] + torch.einsum("vck,nk->nvc", m["shapedirs"], betas)
    v_posed = v_shaped + torch.einsum("vck,nk->nvc", m["posedirs"], feat)         # 3
    J = torch.einsum("jv,nvc->njc", m["J_regressor"], v_shaped)                   # 4
    RG, tG = [R[:, 0]], [J[:, 0]]
    for j in range(1, 16):
        p = m["parents"][j]
        RG.append(RG[p] @ R[:, j])
        tG.append((RG[p] @ (J[:, j] - J[:, p]).unsqueeze(-1)).squeeze(-1) + tG[p])
    RG, tG = torch.stack(RG, dim=1), torch.stack(tG, dim=1)                        # (N,16,3,3), (N,16,3)
    tA = tG - (RG @ J.unsqueeze(-1)).squeeze(-1)
    Rb = torch.einsum("vj,njab->nvab", m["weights"], RG)                          # 5
    tb = torch.einsum("vj,nja->nva", m["weights"], tA)
    # (element-wise, not a batched matmul: N * V products of 3 x 3 by 3 x 1 is a batch count in the hundreds of thousands)
    verts = (Rb * v_posed.unsqueeze(-2)).sum(dim=-1) + tb
    joints = torch.cat([tG, verts[:, m["tip_ids"]]], dim=1)[:, m["joint_order"]]  # 6
    if center_idx is not None:                                                    # 7
        c = joints[:, center_idx: center_idx + 1]
        verts, joints = verts - c, joints - c
    return verts, joints, tG


class TorchManoLayer:
    """the restatement behind the layer contract (float32 on `device`): what tests hand SegmentRefineModel as the other side, and what
    tools/mano_bench.py times against the HIP layer"""

    def __init__(self, arrays, center_idx=0, device="cpu", dtype=torch.float32):
        self.m, self.center_idx, self.dtype, self.device = to_torch(arrays, dtype, device), center_idx, dtype, device
        self.th_faces = torch.as_tensor(arrays.faces).long().to(device)

    def __call__(self, pose_coeffs, betas):
        from types import SimpleNamespace

        v, j, _ = mano_forward(self.m, pose_coeffs.to(device=self.device, dtype=self.dtype), betas.to(device=self.device, dtype=self.dtype),
                               self.center_idx)
        return SimpleNamespace(verts=v, joints=j)
