"""Native text embeddings: `HipClipTextEncoder` runs the text tower of CLIP (ViT-B/32's text side by default) on the HIP kernels of
libtamf_textenc.so (include/tamf_textenc.h, csrc/tamf_textenc.h): tokenised prompts -> the 512-vector `text_embedding` that the
denoiser, the refiner and the FID encoder condition on.  Float32 activations, inference only.

The weights are not part of this package: `load_checkpoint` takes OpenAI's `ViT-B-32.pt` archive (a TorchScript file; it is read
with torch.jit.load, the `clip` package is not needed) or a torch.save'd state dict with the archive's key names.  The reference
(model/interaction_segment_mdm.py:84-132) loads the tower with `clip.load(..., jit=False)`, converts the Linear / attention
parameters and `text_projection` to fp16 and runs fp16 activations; here those tensors are rounded to fp16 at load (`round_fp16`,
a no-op for the archive, which stores them as fp16) and the activations stay float32.  Parity with the model definition is pinned on
seeded weights (tests/test_textenc_gpu.py against tests/textenc_restatement.py); agreement with the reference's fp16 activations on
the real checkpoint is not verified."""
from __future__ import annotations

import ctypes
from ctypes import c_int32, c_int64, c_void_p
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np

from ..hip_backend import TamfError
from ._native import NativeLibrary, NativeModel

# ViT-B/32's text side
DEFAULT_CFG = dict(vocab_size=49408, context_length=77, width=512, num_heads=8, num_layers=12, embed_dim=512)
CFG_FIELDS = ("vocab_size", "context_length", "width", "num_heads", "num_layers", "embed_dim")
CKPT_PREFIX = "clip_model."  # how the reference's module names the tower
MAX_PROMPTS_PER_CALL = 256  # bounds the workspace (4.5 MB per 22-token prompt at full size); no output bit depends on it


class _Config(ctypes.Structure):
    _fields_ = [(k, c_int32) for k in CFG_FIELDS]


class TextEncoderError(TamfError):
    pass


def make_cfg(cfg: Optional[Mapping] = None) -> Dict[str, int]:
    """DEFAULT_CFG overridden by `cfg` (unknown fields are an error)"""
    out = dict(DEFAULT_CFG)
    for k, v in dict(cfg or {}).items():
        if k not in out:
            raise KeyError(f"text encoder cfg: unknown field {k!r} (known: {sorted(out)})")
        out[k] = int(v)
    return out


def expected_shapes(cfg: Mapping[str, int]) -> Dict[str, Tuple[int, ...]]:
    """state-dict name -> shape, the text side of OpenAI's archive"""
    V, C, W, E = int(cfg["vocab_size"]), int(cfg["context_length"]), int(cfg["width"]), int(cfg["embed_dim"])
    s: Dict[str, Tuple[int, ...]] = {"token_embedding.weight": (V, W), "positional_embedding": (C, W)}
    for l in range(int(cfg["num_layers"])):
        p = f"transformer.resblocks.{l}."
        s[p + "ln_1.weight"], s[p + "ln_1.bias"] = (W,), (W,)
        s[p + "attn.in_proj_weight"], s[p + "attn.in_proj_bias"] = (3 * W, W), (3 * W,)
        s[p + "attn.out_proj.weight"], s[p + "attn.out_proj.bias"] = (W, W), (W,)
        s[p + "ln_2.weight"], s[p + "ln_2.bias"] = (W,), (W,)
        s[p + "mlp.c_fc.weight"], s[p + "mlp.c_fc.bias"] = (4 * W, W), (4 * W,)
        s[p + "mlp.c_proj.weight"], s[p + "mlp.c_proj.bias"] = (W, 4 * W), (W,)
    s["ln_final.weight"], s["ln_final.bias"] = (W,), (W,)
    s["text_projection"] = (W, E)
    return s


def is_fp16_key(key: str) -> bool:
    """the tensors the reference's convert_weights turns into fp16 (and `round_fp16` rounds): the Linear and attention parameters,
    weights and biases, and text_projection - not the embeddings, not the LayerNorm parameters"""
    return key == "text_projection" or ".attn." in key or ".mlp." in key


def map_state_dict(state_dict: Mapping, cfg: Mapping[str, int]):
    """The text tower's tensors out of a state dict: an optional `clip_model.` prefix removed, `visual.*` and the archive's scalars
    dropped.  -> (tensors, missing, ignored)"""
    want = expected_shapes(cfg)
    got = {(k[len(CKPT_PREFIX):] if k.startswith(CKPT_PREFIX) else k): v for k, v in state_dict.items()}
    missing = [k for k in want if k not in got]
    ignored = [k for k in got if k not in want]
    return {k: got[k] for k in want if k in got}, missing, ignored


def _argtypes(lib) -> None:
    lib.tamf_textenc_finalize.argtypes = [c_void_p, c_int32]
    lib.tamf_textenc_workspace_bytes.argtypes = [c_void_p, c_int32, c_int64]
    lib.tamf_textenc_encode.argtypes = [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int64, c_void_p]


_NATIVE = NativeLibrary("textenc", TextEncoderError, _argtypes)
_bind, _check = _NATIVE.bind, _NATIVE.check


def eot_positions(ids: np.ndarray) -> np.ndarray:
    """the first index of every row's largest id: where the output is read"""
    return np.argmax(np.asarray(ids), axis=1)


class HipClipTextEncoder(NativeModel):
    """The text tower on the GPU.  `cfg`: the fields of DEFAULT_CFG (missing ones take their defaults).  A missing kernel library or
    a device that is no GPU is an error; there is no torch fall-back."""

    _native = _NATIVE

    def __init__(self, cfg: Optional[Mapping] = None, device="cuda:0", round_fp16: bool = True):
        import torch

        from ..hip_backend import require_gpu

        self.cfg = make_cfg(cfg)
        self.round_fp16 = bool(round_fp16)
        self.device = require_gpu(torch.device(device))
        self._lib = _bind()
        self._model = c_void_p()
        self._loaded = False
        c = _Config(**{k: self.cfg[k] for k in CFG_FIELDS})
        _check(self._lib.tamf_textenc_model_create(ctypes.byref(c), ctypes.byref(self._model)))

    @property
    def out_dim(self) -> int:
        return self.cfg["embed_dim"]

    # ---- weights ----
    def load_state_dict(self, state_dict: Mapping) -> List[str]:
        """archive names (an optional `clip_model.` prefix is removed) -> tensors / arrays of any float type.  A missing name, a wrong
        shape or a non-finite value raises TextEncoderError; names the tower does not have (`visual.*`, `logit_scale`, ...) are
        ignored and returned."""
        import logging

        if self._loaded:
            raise TextEncoderError("the weights are loaded already")
        sd, missing, ignored = map_state_dict(state_dict, self.cfg)
        if missing:
            raise TextEncoderError(f"text encoder: missing keys {missing}")
        if ignored:
            logging.getLogger(__name__).info("text encoder: %d keys ignored (%s ...)", len(ignored), ", ".join(ignored[:4]))
        self._load_weights(sd, int(self.round_fp16))
        self._loaded = True
        return ignored

    def load_checkpoint(self, path) -> List[str]:
        """OpenAI's archive (TorchScript: torch.jit.load(...).state_dict()), or a torch.save'd dict - the state dict itself or under
        'state_dict'.  -> the ignored names."""
        import torch

        try:
            sd = torch.jit.load(path, map_location="cpu").state_dict()
        except (RuntimeError, ValueError):  # no TorchScript archive
            ckpt = torch.load(path, map_location="cpu", weights_only=True)
            if not isinstance(ckpt, Mapping):
                raise TextEncoderError(f"{path}: neither a TorchScript archive nor a state dict")
            sd = ckpt["state_dict"] if isinstance(ckpt.get("state_dict"), Mapping) else ckpt
        return self.load_state_dict(sd)

    # ---- encoding ----
    def encode_tokens(self, ids) -> "torch.Tensor":  # noqa: F821
        """(B, context_length) integer ids -> (B, embed_dim) float32 on the device; the output row of a prompt is read at the first
        index of its largest id"""
        import torch

        from ..hip_backend import _stream_ptr

        if not self._loaded:
            raise TextEncoderError("no weights loaded")
        a = ids.detach().cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)
        if a.ndim != 2 or a.shape[1] != self.cfg["context_length"] or a.shape[0] < 1 or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"ids: expected integers of shape (B, {self.cfg['context_length']}), got {a.dtype} {a.shape}")
        if a.min() < -2 ** 31 or a.max() >= 2 ** 31:
            raise TextEncoderError("ids: values outside the int32 range")
        a = np.ascontiguousarray(a, dtype=np.int32)  # (the library rejects ids outside [0, vocab_size), naming the entry)
        B = a.shape[0]
        out = torch.empty((B, self.out_dim), dtype=torch.float32, device=self.device)
        rows = eot_positions(a) + 1
        with torch.cuda.device(self.device):
            for b0 in range(0, B, MAX_PROMPTS_PER_CALL):
                n = min(MAX_PROMPTS_PER_CALL, B - b0)
                nbytes = int(self._lib.tamf_textenc_workspace_bytes(self._model, n, int(rows[b0: b0 + n].sum())))
                ws = torch.empty(nbytes // 4, dtype=torch.float32, device=self.device)  # (freed stream-ordered by torch's allocator)
                _check(self._lib.tamf_textenc_encode(self._model, a[b0:].ctypes.data, n, out[b0:].data_ptr(), ws.data_ptr(), nbytes,
                                                               _stream_ptr(self.device)))
        return out

    def encode_text(self, texts: Sequence[str], tokenizer, max_text_len: int = 20):
        """the reference's call (interaction_segment_mdm.py:118-132): tokenize at max_text_len + 2 with truncation, zero-pad the ids
        to the model's context, encode"""
        if isinstance(texts, str):
            texts = [texts]
        ctx = self.cfg["context_length"]
        n = min(int(max_text_len) + 2, ctx)
        ids = np.zeros((len(texts), ctx), dtype=np.int32)
        ids[:, :n] = tokenizer.tokenize(list(texts), context_length=n, truncate=True)
        return self.encode_tokens(ids)


__all__ = ["HipClipTextEncoder", "TextEncoderError", "DEFAULT_CFG", "CKPT_PREFIX", "make_cfg", "expected_shapes", "map_state_dict", "is_fp16_key",
           "eot_positions"]
