"""InterationSegmentMDMTrainStep - the training forward and backward of the denoiser G (InterationSegmentMDM) on the gfx950 HIP
library libtamf_mdmtrain.so (include/tamf_mdmtrain.h), and the diffusion training objective around it.

forward() returns the model output as a tensor that carries autograd: whatever loss the caller builds on it (the masked MSE of
training_losses, the hand-interaction terms through MANO and nearest neighbours), its .backward() reaches a torch.autograd.Function
whose backward runs the HIP backward and fills the .grad of every parameter, OVERWRITING it.  The kernels read the parameters where
torch keeps them, so any torch.optim optimiser (and the reference's clip_gradient) then works on the .grad tensors as they are.  There
is no PyTorch compute path and no fallback.  A forward serves one backward; a second forward before the backward of the first is
refused, like two backwards through one forward (the mechanism of segment_refine_train.py).

training_losses() is the reference's GaussianDiffusion.training_losses (gaussian_diffusion.py:1106-1188) for the configuration
create_gaussian_diffusion builds - MSE loss, x0 prediction, fixed variance - as a function of a diffusion object and any callable
model; uniform_timesteps() is the reference's uniform schedule sampler.  loss_and_grads() is the reference's whole step
(launch/train.py:518-529) on this package's kernels.

The module InterationSegmentMDM sets requires_grad False on its parameters and warns on train(True): it is the inference container.
The step enables requires_grad itself and never calls train().  After optimiser steps call model.refresh_hip_weights() before using
the inference path (InterationSegmentMDM.forward, fused_sample_loop): the inference context keeps its own composed copy of the weights.

cond_mask_prob is not built (the reference's launcher never sets it: mask_cond is the identity).

Dropout masks are Philox draws keyed by (seed, step, clip id, site, element): see the header for the sites.  dropout_mask() returns the
keep-mask the step uses at one site.
"""
from __future__ import annotations

import ctypes
from ctypes import c_char_p, c_float, c_int32, c_int64, c_uint32, c_uint64, c_void_p
from typing import Callable, Dict, Mapping, Optional, Sequence

import numpy as np
import torch

from .. import _lib
from ..hip_backend import _Arch, _dev_f32, _stream_ptr, hand_side_code, obj_num_vector
from . import _train_step
from ._train_step import TrainStep, clip_id_vector
from .segment_refine_train import PendingForward, _TrunkFunction

BUFFERS = ("hand_side_process.rh_embed", "hand_side_process.lh_embed", "sequence_pos_encoder.pe")
PREFIX = "tamf_mdmtrain_"
MAX_TIMESTEP = 4999  # the last row of sequence_pos_encoder.pe


def lib() -> ctypes.CDLL:
    return _train_step.typed_lib(_lib.load_mdmtrain, PREFIX, {
        "forward": [c_void_p, c_int32, c_int32, c_int32] + [c_void_p] * 9 + [c_float, c_uint64, c_uint32, c_void_p, c_void_p],
        "backward": [c_void_p, c_void_p, c_void_p], "set_profile": [c_void_p, c_int32], "get_profile": [c_void_p, c_char_p, c_int64]})


def dropout_mask(seed: int, step: int, clip_id: int, site: int, rows: int, cols: int, p: float, device=None) -> torch.Tensor:
    """the (rows, cols) bool keep-mask of one dropout site of one clip (tamf_mdmtrain_dropout_mask)"""
    return _train_step.dropout_mask(lib(), PREFIX, seed, step, clip_id, site, rows, cols, p, device)


def check_mdm_batch(x_t, timesteps, batch: Mapping, text_embedding, arch: Mapping[str, int], obj_num=None, clip_ids=None):
    """The Python-side refusals, device-free: -> (B, T, nobj, hand-side codes, int32 timesteps, int32 obj_num or None, int64 clip ids or
    None).  ValueError for shapes that do not agree with each other or with the architecture and for a timestep outside
    [0, MAX_TIMESTEP], TypeError for a tensor that is not floating point (timesteps: not integer)."""
    sh, oe, ot = batch["shape"], batch["obj_embedding"], batch["obj_traj"]
    for name, t in (("x_t", x_t), ("text_embedding", text_embedding), ("shape", sh), ("obj_embedding", oe), ("obj_traj", ot)):
        if not torch.is_tensor(t) or not t.dtype.is_floating_point:
            raise TypeError(f"{name}: expected a floating-point tensor, got {t.dtype if torch.is_tensor(t) else type(t).__name__}")
    if x_t.dim() != 4 or x_t.shape[1] != arch["input_dim"] or x_t.shape[2] != 1:
        raise ValueError(f"x_t: expected (B, {arch['input_dim']}, 1, T), got {tuple(x_t.shape)}")
    B, _, _, T = (int(s) for s in x_t.shape)
    if B < 1 or T < 1:
        raise ValueError(f"x_t: an empty batch {tuple(x_t.shape)}")
    if torch.is_tensor(timesteps) and (timesteps.dtype.is_floating_point or timesteps.dtype == torch.bool):
        raise TypeError(f"timesteps: expected an integer tensor, got {timesteps.dtype}")
    t_np = np.ascontiguousarray(timesteps.detach().cpu().numpy() if torch.is_tensor(timesteps) else timesteps)
    if t_np.dtype.kind not in "iu":
        raise TypeError(f"timesteps: expected integers, got {t_np.dtype}")
    if t_np.shape != (B,):
        raise ValueError(f"timesteps: expected ({B},), got {t_np.shape}")
    if t_np.min() < 0 or t_np.max() > MAX_TIMESTEP:
        raise ValueError(f"timesteps must be in [0, {MAX_TIMESTEP}], got [{int(t_np.min())}, {int(t_np.max())}]")
    if tuple(text_embedding.shape) != (B, arch["clip_dim"]):
        raise ValueError(f"text_embedding: expected {(B, arch['clip_dim'])}, got {tuple(text_embedding.shape)}")
    if tuple(sh.shape) != (B, T, arch["hand_shape_dim"]):
        raise ValueError(f"shape: expected {(B, T, arch['hand_shape_dim'])}, got {tuple(sh.shape)}")
    if oe.dim() != 3 or oe.shape[0] != B or oe.shape[1] < 1 or oe.shape[2] != arch["obj_embed_dim"]:
        raise ValueError(f"obj_embedding: expected ({B}, nobj, {arch['obj_embed_dim']}), got {tuple(oe.shape)}")
    nobj = int(oe.shape[1])
    if tuple(ot.shape) != (B, nobj, T, arch["obj_input_dim"]):
        raise ValueError(f"obj_traj: expected {(B, nobj, T, arch['obj_input_dim'])}, got {tuple(ot.shape)}")
    side = [hand_side_code(hs) for hs in batch["hand_side"]]
    if len(side) != B:
        raise ValueError(f"hand_side: expected {B} entries, got {len(side)}")
    num_np = obj_num_vector(obj_num, B)
    if num_np is not None and (num_np.min() < 1 or num_np.max() > nobj):
        raise ValueError(f"obj_num must be in [1, nobj = {nobj}], got [{int(num_np.min())}, {int(num_np.max())}]")
    return B, T, nobj, side, t_np.astype(np.int32), num_np, clip_id_vector(clip_ids, B)


# ---- the diffusion training objective ----
def uniform_timesteps(diffusion, batch_size: int, device=None, rng: Optional[np.random.Generator] = None):
    """The reference's UniformSampler.sample (model/diffusion/resample.py:42-67): -> (t (batch_size,) int64 uniform over the diffusion's
    timesteps, weights (batch_size,) float32, all 1).  rng: a numpy Generator (default: numpy's global state, as the reference)."""
    n = int(diffusion.num_timesteps)
    idx = rng.integers(0, n, size=(batch_size,)) if rng is not None else np.random.choice(n, size=(batch_size,))
    return torch.from_numpy(np.asarray(idx, np.int64)).to(device), torch.ones(batch_size, dtype=torch.float32, device=device)


def masked_l2(a: torch.Tensor, b: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
    """reference gaussian_diffusion.py:163-175: a, b (B, J, F, T), mask (B, 1, 1, T) -> per clip, the squared error summed over the
    unmasked frames over (their count * J * F)"""
    loss = ((a - b) ** 2 * mask.float()).flatten(1).sum(dim=1)
    return loss / (mask.flatten(1).sum(dim=1) * (a.shape[1] * a.shape[2]))


def training_losses(diffusion, model: Callable, x_start: torch.Tensor, t: torch.Tensor, model_kwargs: Optional[Mapping] = None,
                    noise: Optional[torch.Tensor] = None, loss_callback: Optional[Callable] = None):
    """The reference's GaussianDiffusion.training_losses for MSE loss, x0 prediction and fixed variance: x_t = q_sample(x_start, t,
    noise), model_output = model(x_t, t, **model_kwargs), terms["mse"] = masked_l2(x_start, model_output, batch["mask"] as (B, 1, 1, T)),
    terms["loss"] = terms["mse"], then loss_callback(model_output, batch).  x_start (B, F, 1, T); model_kwargs carries "batch".
    -> (terms, (extra_loss, extra_loss_dict)), the pair None without a callback.  `model` is any callable."""
    if model_kwargs is None or "batch" not in model_kwargs:
        raise KeyError("model_kwargs['batch'] (with its 'mask') is needed")
    B, _, _, T = x_start.shape
    batch = model_kwargs["batch"]
    mask = batch["mask"].reshape(B, 1, 1, T)
    if noise is None:
        noise = torch.randn_like(x_start)
    x_t = diffusion.q_sample(x_start, t, noise=noise)
    if hasattr(diffusion, "_wrap_model"):  # (a respaced process hands the model its base timesteps, respace.py:85-88; else the identity)
        model = diffusion._wrap_model(model)
    model_output = model(x_t, diffusion._scale_timesteps(t), **model_kwargs)
    if model_output.shape != x_start.shape:
        raise ValueError(f"the model returned {tuple(model_output.shape)} for x_start {tuple(x_start.shape)}")
    terms = {"mse": masked_l2(x_start, model_output, mask)}
    terms["loss"] = terms["mse"]
    extra = loss_callback(model_output, batch) if loss_callback is not None else (None, None)
    return terms, (extra[0], extra[1])


class InterationSegmentMDMTrainStep(TrainStep):
    """forward(x_t, timesteps, batch) / loss_and_grads(diffusion, batch, loss) around an InterationSegmentMDM on a GPU.  Enables
    requires_grad on the parameters (the hand-side embeddings and the PE table are buffers; a CLIP tower is left frozen and unbound)
    and allocates their .grad.  dropout=None takes the model's."""

    LIB, PREFIX, BUFFERS = staticmethod(lib), PREFIX, BUFFERS

    def __init__(self, model, max_batch: int, max_frames: int, dropout: Optional[float] = None, seed: int = 0):
        dropout = float(model.dropout if dropout is None else dropout)
        if not 0.0 <= dropout < 1.0:
            raise ValueError(f"dropout must be in [0, 1), got {dropout}")
        if getattr(model, "cond_mask_prob", 0.0):
            raise NotImplementedError("cond_mask_prob > 0 is not built (the reference's launcher never sets it)")
        self.arch = dict(model._arch)
        a = self.arch
        arch = _Arch(a["input_dim"], a["obj_input_dim"], a["hand_shape_dim"], a["obj_embed_dim"], a["latent_dim"], a["ff_size"], a["num_layers"],
                     a["num_heads"], a["clip_dim"], 0, 0)
        self._pending = None
        self._keep = None
        self.module = model  # (self.model, what TrainStep binds, is its view without the CLIP tower)
        super().__init__(_WithoutClip(model), arch, max_batch, max_frames, dropout, seed)

    def dropout_mask(self, step: int, clip_id: int, site: int, rows: int, cols: int) -> torch.Tensor:
        """the keep-mask this step object uses (its seed and dropout) at one site of one clip"""
        return dropout_mask(self.seed, step, clip_id, site, rows, cols, self.dropout, self.device)

    def _text_embedding(self, batch: Mapping) -> torch.Tensor:
        if batch.get("text_embedding") is not None:
            return batch["text_embedding"]
        if "text" not in batch:
            raise KeyError("batch['text_embedding'] (B, clip_dim) is needed - or batch['text'] with a model built with load_clip=True")
        return self.module._text_embedding(batch)

    def forward(self, x_t: torch.Tensor, timesteps, batch: Mapping, obj_num: Optional[Sequence[int]] = None,
                clip_ids: Optional[Sequence[int]] = None, step: int = 0) -> torch.Tensor:
        """x_t (B, input_dim, 1, T); timesteps (B,) integers in [0, 4999]; batch: "text_embedding" (B, clip_dim) (or "text" when the
        model was built with load_clip=True), "hand_side" (B x "rh"/"lh"), "shape" (B, T, 10), "obj_embedding" (B, nobj, od),
        "obj_traj" (B, nobj, T, 9).  obj_num: per-clip object counts (None: the mean over all nobj padded rows, the reference's
        forward); clip_ids: the keys of the dropout masks (None: the position in the batch).  -> model_output (B, input_dim, 1, T),
        carrying autograd to every parameter's .grad; x_t is data and gets no gradient."""
        self._require_open()
        if self._pending is not None and self._pending.open:
            raise RuntimeError("InterationSegmentMDMTrainStep: the previous forward has had no backward yet and a second forward would "
                               "replace its activations; run its backward first, or drop it with discard_forward()")
        text = self._text_embedding(batch)
        B, T, nobj, side, t_np, num_np, clip_np = check_mdm_batch(x_t, timesteps, batch, text, self.arch, obj_num, clip_ids)
        dev = self.device
        self._rebind_moved()
        x = _dev_f32(x_t, dev)[:, :, 0, :].permute(0, 2, 1).contiguous()  # (B, T, F)
        te, sh = _dev_f32(text, dev), _dev_f32(batch["shape"], dev)
        oe, ot = _dev_f32(batch["obj_embedding"], dev), _dev_f32(batch["obj_traj"], dev)
        side_d = torch.tensor(side, dtype=torch.uint8, device=dev)
        out = torch.empty(B, T, self.arch["input_dim"], dtype=torch.float32, device=dev)
        null = c_void_p(0)
        with torch.cuda.device(dev):
            self._call(
                "forward", self._h, B, T, nobj, num_np.ctypes.data_as(c_void_p) if num_np is not None else null, t_np.ctypes.data_as(c_void_p),
                c_void_p(x.data_ptr()), c_void_p(te.data_ptr()), c_void_p(sh.data_ptr()), c_void_p(side_d.data_ptr()), c_void_p(oe.data_ptr()),
                c_void_p(ot.data_ptr()), clip_np.ctypes.data_as(c_void_p) if clip_np is not None else null, self.dropout, self.seed, int(step),
                c_void_p(out.data_ptr()), c_void_p(_stream_ptr(dev)))
        self._keep = [x, te, sh, oe, ot, side_d]  # (the backward reads x_t and the text features again)
        self._pending = PendingForward()
        anchor = next(self.model.parameters())
        out = _TrunkFunction.apply(self, self._pending, out, anchor)
        return out.permute(0, 2, 1).unsqueeze(2)  # (B, F, 1, T)

    def profile(self, on: bool) -> None:
        """measurement only: bracket every kernel launch of the following calls with events (tamf_mdmtrain_set_profile)"""
        self._call("set_profile", self._h, int(bool(on)))

    def read_profile(self) -> Dict[str, tuple]:
        """{kind of kernel: (launches, milliseconds)} since the last read (tamf_mdmtrain_get_profile); waits for the device"""
        buf = ctypes.create_string_buffer(1 << 16)
        self._call("get_profile", self._h, buf, len(buf))
        rows = [ln.split("\t") for ln in buf.value.decode().splitlines()]
        return {r[0]: (int(r[1]), float(r[2])) for r in rows}

    def discard_forward(self) -> None:
        """give up the pending forward (a forward whose loss is not going to be differentiated)"""
        if self._pending is not None:
            self._pending.open = False

    def run_backward(self, grad: torch.Tensor) -> None:
        """tamf_mdmtrain_backward: the .grad of every parameter from d loss / d model_output as (B, T, F) (called by autograd)"""
        self._require_open()
        g = _dev_f32(grad, self.device)
        self._rebind_moved()
        with torch.cuda.device(self.device):
            self._call("backward", self._h, c_void_p(g.data_ptr()), c_void_p(_stream_ptr(self.device)))
        self._keep = (self._keep or []) + [g]

    def loss_and_grads(self, diffusion, batch: Mapping, loss: Optional[Callable] = None, t: Optional[torch.Tensor] = None,
                       noise: Optional[torch.Tensor] = None, weights: Optional[torch.Tensor] = None, obj_num: Optional[Sequence[int]] = None,
                       clip_ids: Optional[Sequence[int]] = None, step: int = 0) -> Dict:
        """The reference's step launch/train.py:518-529: x_start from batch["pose_repr"] (B, T, input_dim) as (B, input_dim, 1, T),
        training_losses with this step's forward as the model and `loss` (a HandInteractionLoss, or None) as the callback,
        (terms["loss"] * weights).mean() + the extra loss, .backward().  t / weights default to uniform_timesteps, noise to randn.
        batch as forward() plus "pose_repr" and "mask" (B, T), and what `loss` reads ("obj_points", "obj_num", "sdf_grid_id").  Afterwards every
        p.grad holds the gradient of the reference's loss.  -> the loss dict: the terms, "diffusion_loss", "loss" (the total) and,
        with a callback, "extra" (its dict)."""
        dev = self.device
        on_dev = {k: (v if not torch.is_tensor(v) else _dev_f32(v, dev) if v.dtype.is_floating_point else v.to(dev)) for k, v in batch.items()}
        x_start = on_dev["pose_repr"].unsqueeze(3).permute(0, 2, 3, 1)
        B = x_start.shape[0]
        if t is None:
            t, w = uniform_timesteps(diffusion, B, dev)
            weights = w if weights is None else weights
        t = torch.as_tensor(t).to(dev)
        weights = torch.ones(B, dtype=torch.float32, device=dev) if weights is None else _dev_f32(torch.as_tensor(weights), dev)
        if noise is not None:
            noise = _dev_f32(noise, dev)
        try:
            terms, (extra, extra_dict) = training_losses(
                diffusion, lambda x, ts, batch: self.forward(x, ts, batch, obj_num=obj_num, clip_ids=clip_ids, step=step), x_start, t,
                model_kwargs={"batch": on_dev}, noise=noise, loss_callback=loss)
            diffusion_loss = (terms["loss"] * weights).mean()
            total = diffusion_loss if extra is None else diffusion_loss + extra
            total.backward()
        finally:
            self.discard_forward()
        out = {k: v.detach() for k, v in terms.items()}
        out["diffusion_loss"], out["loss"] = diffusion_loss.detach(), total.detach()
        if extra_dict is not None:
            out["extra"] = {k: (v.detach() if torch.is_tensor(v) else v) for k, v in extra_dict.items()}
        return out


class _WithoutClip:
    """the view of a model that TrainStep binds: its parameters and buffers without a frozen CLIP tower"""

    def __init__(self, model):
        self._m = model

    def parameters(self):
        return (p for _, p in self.named_parameters())

    def named_parameters(self):
        return ((k, p) for k, p in self._m.named_parameters() if not k.startswith("clip_model."))

    def named_buffers(self):
        return ((k, b) for k, b in self._m.named_buffers() if not k.startswith("clip_model."))
