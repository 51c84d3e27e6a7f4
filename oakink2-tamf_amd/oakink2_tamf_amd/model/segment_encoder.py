"""SegmentEncoder - the motion encoder of the FID score (reference model/segment_encoder.py:16-111), computed by the gfx950 HIP
library (tamf_encode, kind "E").

Same constructor signature and the same state-dict key set as the reference, so its checkpoints load with load_state_dict; the module
is a parameter container plus a dispatcher, with no PyTorch compute path and no CPU fallback.  forward(batch) is the reference's
forward on the batch it is handed (object means over every row of the zero-padded object axis); encode(batch, obj_num=...) takes each
clip's own object count, which is what the reference's FID script computes by calling the encoder one clip at a time
(script/compute_score/compute_score_fid.py:306-349).  Eval only: dropout is identity.  The library supports latent_dim 64 with 4 heads
(config/arch_encoder.yml); other shapes raise hip_backend.TamfError naming the limit.

No weight depends on `output_dim` (the output head is built with `input_dim`, reference :73); it is kept for the signature.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch
import torch.nn as nn

from .interaction_segment_mdm import HandsideProcess, PositionalEncoding, _Linear


class _OutputProcess(nn.Module):
    def __init__(self, output_feats, latent_dim):
        super().__init__()
        self.poseFinal = nn.Sequential(nn.Linear(latent_dim, latent_dim), nn.SiLU(), nn.Linear(latent_dim, latent_dim), nn.SiLU(),
                                       nn.Linear(latent_dim, output_feats))


class SegmentEncoder(nn.Module):
    def __init__(self, output_dim, input_dim=99, obj_input_dim=9, hand_shape_dim=10, obj_embed_dim=768, latent_dim=256, ff_size=1024,
                 num_layers=8, num_heads=4, dropout=0.1, activation="gelu"):
        super().__init__()
        if activation != "gelu":
            raise NotImplementedError("the HIP encoder computes the exact erf-GELU (activation='gelu') only")
        self.output_dim, self.latent_dim, self.ff_size = output_dim, latent_dim, ff_size
        self.num_layers, self.num_heads, self.dropout, self.activation = num_layers, num_heads, dropout, activation
        self.input_feats, self.obj_input_feats = input_dim, obj_input_dim
        self.hand_shape_feats, self.obj_embed_feats = hand_shape_dim, obj_embed_dim
        self.hand_side_process = HandsideProcess(latent_dim)
        self.hand_shape_process = _Linear("shape_embed", hand_shape_dim, latent_dim)
        self.obj_embed_process = _Linear("embedding", obj_embed_dim, latent_dim)
        self.register_buffer("classification_token", torch.zeros(1, 1, latent_dim))
        self.input_process = _Linear("poseEmbedding", input_dim, latent_dim)
        self.obj_input_process = _Linear("poseEmbedding", obj_input_dim, latent_dim)
        self.input_merge = nn.Sequential(nn.Linear(latent_dim * 2, latent_dim), nn.SiLU(), nn.Linear(latent_dim, latent_dim))
        self.sequence_pos_encoder = PositionalEncoding(latent_dim, dropout)
        layer = nn.TransformerEncoderLayer(d_model=latent_dim, nhead=num_heads, dim_feedforward=ff_size, dropout=dropout,
                                           activation=activation)
        self.seqTransEncoder = nn.TransformerEncoder(layer, num_layers=num_layers, enable_nested_tensor=False)
        self.output_process = _OutputProcess(input_dim, latent_dim)
        for p in self.parameters():
            p.requires_grad_(False)
        self.eval()
        self._arch = dict(input_dim=input_dim, obj_input_dim=obj_input_dim, hand_shape_dim=hand_shape_dim, obj_embed_dim=obj_embed_dim,
                          latent_dim=latent_dim, ff_size=ff_size, num_layers=num_layers, num_heads=num_heads)
        self._ctx = None
        self._ctx_dirty = True

    # weights changed -> re-upload lazily
    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        out = super().load_state_dict(state_dict, strict=strict, **kw)
        self._ctx_dirty = True
        return out

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._ctx_dirty = True
        return out

    def refresh_hip_weights(self):
        """Call after modifying parameters in place."""
        self._ctx_dirty = True

    def close(self):
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None

    def _context(self, B: int, T: int):
        from ..hip_backend import TamfContext, require_gpu

        dev = require_gpu(next(self.parameters()).device)
        if self._ctx is not None and not self._ctx_dirty and self._ctx.device == dev:
            if B > self._ctx.max_batch or T > self._ctx.max_frames:
                self._ctx.resize(max(B, self._ctx.max_batch), max(T, self._ctx.max_frames))
            return self._ctx
        self.close()
        ctx = TamfContext(self._arch, B, T, precision="f32", device=dev, kind="E")
        try:
            ctx.load_state_dict(self.state_dict())
        except Exception:
            ctx.close()
            raise
        self._ctx, self._ctx_dirty = ctx, False
        return ctx

    @torch.no_grad()
    def encode(self, batch: Dict, obj_num: Optional[Sequence[int]] = None, with_activation: bool = True) -> Dict:
        """batch: "pose_repr" (B, T, input_dim), "hand_side" (B x "rh"/"lh"), "shape" (B, T, 10), "obj_embedding" (B, nobj, 768),
        "obj_traj" (B, nobj, T, 9); obj_num: per-clip object counts or None (all nobj rows)
        -> {"encoding": (1, B, latent_dim), "activation": (B, input_dim) or None}"""
        pose = batch["pose_repr"]
        B, T = int(pose.shape[0]), int(pose.shape[1])
        ctx = self._context(B, T)
        enc, act = ctx.encode(pose, batch["shape"], batch["hand_side"], batch["obj_embedding"], batch["obj_traj"], obj_num=obj_num,
                              with_activation=with_activation)
        return {"encoding": enc.unsqueeze(0), "activation": act}

    def forward(self, batch: Dict) -> Dict:
        """the reference's forward (segment_encoder.py:77-111) on this batch: {"encoding": (1, B, d), "activation": (B, input_dim)}"""
        return self.encode(batch, obj_num=None)
