"""What the wrappers of the native model libraries share (libtamf_pointenc.so, libtamf_textenc.so): a library bound once by its
symbol prefix, its status codes raised as the wrapper's own error class, a state-dict entry handed to `load_weight`, and the end of a
model's life.  The entry points only one library has keep their argtypes with that library's wrapper."""
from ctypes import POINTER, c_char_p, c_int32, c_int64, c_void_p

import numpy as np


class NativeLibrary:
    """tamf_<prefix>_* of _lib.load_<prefix>(), bound on first use: `error` is what a non-zero status raises, `argtypes(lib)` sets the
    argtypes of the entry points beyond last_error / model_create / load_weight / destroy (and workspace_bytes' int64 result)."""

    def __init__(self, prefix, error, argtypes):
        self.prefix, self.error, self._argtypes, self._lib = prefix, error, argtypes, None

    def fn(self, name: str):
        return getattr(self.bind(), f"tamf_{self.prefix}_{name}")

    def bind(self):
        if self._lib is None:
            from .. import _lib

            self._lib = getattr(_lib, f"load_{self.prefix}")()
            self.fn("last_error").restype = c_char_p
            self.fn("model_create").argtypes = [c_void_p, POINTER(c_void_p)]  # (a pointer to the wrapper's _Config)
            self.fn("load_weight").argtypes = [c_void_p, c_char_p, c_void_p, c_int32, POINTER(c_int64)]
            self.fn("destroy").argtypes = [c_void_p]
            self.fn("workspace_bytes").restype = c_int64
            self._argtypes(self._lib)
        return self._lib

    def check(self, rc: int) -> None:
        if rc != 0:
            raise self.error(f"libtamf_{self.prefix}: {self.fn('last_error')().decode()} (status {rc})")

    def load_weight(self, model, key: str, value) -> None:
        """a tensor or array of any float type, as contiguous float32"""
        import torch

        a = value.detach().float().cpu().numpy() if isinstance(value, torch.Tensor) else np.asarray(value)
        a = np.ascontiguousarray(a, dtype=np.float32)
        self.check(self.fn("load_weight")(model, key.encode(), a.ctypes.data, a.ndim, (c_int64 * max(a.ndim, 1))(*a.shape)))


class NativeModel:
    """a model handle `_model` of `_native` (the subclass's NativeLibrary) on `device`"""

    def _load_weights(self, tensors, *finalize_args) -> None:
        import torch

        for k, v in tensors.items():
            self._native.load_weight(self._model, k, v)
        with torch.cuda.device(self.device):
            self._native.check(self._native.fn("finalize")(self._model, *finalize_args))

    def close(self) -> None:
        if getattr(self, "_model", None) is not None and self._model.value:
            import torch

            torch.cuda.synchronize(self.device)
            self._native.fn("destroy")(self._model)
            self._model = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
