"""Capture the SegmentEncoder and FID fixtures (tests/golden/segment_encoder_*.npz, tests/golden/fid_*.npz) from the reference.

Run where a checkout of the reference is available (CPU only):  python tools/capture_encoder_golden.py REFERENCE_ROOT

The reference's model/segment_encoder.py and script/compute_score/compute_score_fid.py are imported as they are; the modules they import
but that the FID computation does not use (CLIP, MANO, trimesh, the config registry, the upkeep / transform helpers, ...) are stubbed
in sys.modules when they are not installed.  Weights and inputs are seeded (tests/encoder_restatement.py); the fixtures hold them and
the reference's outputs - data only.  The sin/cos PE table is not stored whole (1.3 MB): its first rows are, and the tests rebuild it.
"""
from __future__ import annotations

import contextlib
import importlib
import importlib.abc
import importlib.machinery
import io
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oakink2-tamf_amd"))
from encoder_restatement import ARCH_ENCODER, seeded_inputs, seeded_state_dict  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
PE_ROWS = 256
STUBBED = ("clip", "trimesh", "manotorch", "config_reg", "dev_fn", "tqdm", "oakink2_toolkit", "pytorch3d", "chamfer_distance")


class _Anything(types.ModuleType):
    """a stand-in module: every attribute is another stand-in (callable, subscriptable), enough for import-time use"""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        sub = _Anything(f"{self.__name__}.{name}")
        setattr(self, name, sub)
        return sub

    def __call__(self, *a, **k):
        return _Anything(self.__name__ + "()")

    def __getitem__(self, k):
        return _Anything(self.__name__ + "[]")


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path=None, target=None):
        if name.split(".")[0] not in STUBBED:
            return None
        try:  # an installed module wins
            if name.split(".")[0] == name and importlib.machinery.PathFinder.find_spec(name) is not None:
                return None
        except (ImportError, ValueError):
            pass
        return importlib.machinery.ModuleSpec(name, self, is_package=True)

    def create_module(self, spec):
        m = _Anything(spec.name)
        m.__path__ = []
        return m

    def exec_module(self, module):
        pass


def import_reference(ref_root: str):
    sys.meta_path.insert(0, _StubFinder())
    sys.path.insert(0, os.path.join(ref_root, "src"))
    sys.path.insert(0, os.path.join(ref_root, "script", "compute_score"))
    from oakink2_tamf.model.segment_encoder import SegmentEncoder

    fid_mod = importlib.import_module("compute_score_fid")
    return SegmentEncoder, fid_mod


def run_encoder(SegmentEncoder, sd, inputs, obj_num=None):
    model = SegmentEncoder(17, **{k: ARCH_ENCODER[k] for k in ARCH_ENCODER}).eval()
    missing, unexpected = model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    assert not missing and not unexpected
    batch = {"pose_repr": torch.from_numpy(inputs["pose_repr"]), "shape": torch.from_numpy(inputs["shape"]),
             "hand_side": list(inputs["hand_side"]), "obj_embedding": torch.from_numpy(inputs["obj_embedding"]),
             "obj_traj": torch.from_numpy(inputs["obj_traj"])}
    with torch.no_grad():
        if obj_num is None:
            out = model(batch)
            return out["encoding"][0].numpy(), out["activation"].numpy(), sorted(model.state_dict().keys())
        encs, acts = [], []
        for b, n in enumerate(obj_num):  # one clip at a time, its own objects only (compute_score_fid.py:306-349)
            one = {k: (v[b:b + 1, :n] if k in ("obj_embedding", "obj_traj") else [v[b]] if k == "hand_side" else v[b:b + 1])
                   for k, v in batch.items()}
            out = model(one)
            encs.append(out["encoding"][0, 0].numpy())
            acts.append(out["activation"][0].numpy())
        return np.stack(encs), np.stack(acts), sorted(model.state_dict().keys())


def save_encoder_case(name, sd, inputs, outputs, keys, obj_num=None):
    data = {f"sd/{k}": v for k, v in sd.items() if k != "sequence_pos_encoder.pe"}
    data["pe_head"] = sd["sequence_pos_encoder.pe"][:PE_ROWS, 0]
    for k in ("pose_repr", "shape", "obj_embedding", "obj_traj"):
        data[f"in/{k}"] = inputs[k]
    data["in/hand_side"] = np.array(inputs["hand_side"])
    if obj_num is not None:
        data["in/obj_num"] = np.asarray(obj_num, np.int32)
    data.update(outputs)
    data["arch"] = np.array([ARCH_ENCODER[k] for k in ("input_dim", "obj_input_dim", "hand_shape_dim", "obj_embed_dim", "latent_dim",
                                                       "ff_size", "num_layers", "num_heads")], np.int32)
    data["state_dict_keys"] = np.array(keys)
    path = os.path.join(GOLDEN, name)
    np.savez_compressed(path, **data)
    print(f"{name}: {os.path.getsize(path)} bytes")


def main(ref_root: str):
    SegmentEncoder, fid_mod = import_reference(ref_root)
    torch.manual_seed(0)
    # (a) + (b): B = 4, T = 160, objects padded to 3, clips of 1, 2, 3 (and 3) objects, hands mixed
    sd = seeded_state_dict(ARCH_ENCODER, seed=11)
    obj_num = [1, 2, 3, 3]
    inp = seeded_inputs(4, 160, 3, seed=12, obj_num=obj_num)
    inp["hand_side"] = ["rh", "lh", "rh", "lh"]
    enc, act, keys = run_encoder(SegmentEncoder, sd, inp)
    enc1, act1, _ = run_encoder(SegmentEncoder, sd, inp, obj_num=obj_num)
    save_encoder_case("segment_encoder_b4_t160.npz", sd, inp, {"out/encoding": enc, "out/activation": act,
                                                                "out/encoding_single": enc1, "out/activation_single": act1}, keys, obj_num)
    # (c) T = 7
    sd = seeded_state_dict(ARCH_ENCODER, seed=21)
    inp = seeded_inputs(3, 7, 2, seed=22)
    enc, act, keys = run_encoder(SegmentEncoder, sd, inp)
    save_encoder_case("segment_encoder_t7.npz", sd, inp, {"out/encoding": enc, "out/activation": act}, keys)
    # (d) non-finite object inputs: NaN in an object embedding and in object trajectories (the prefix / frame rows take nan_to_num)
    sd = seeded_state_dict(ARCH_ENCODER, seed=31)
    inp = seeded_inputs(3, 24, 2, seed=32)
    inp["obj_embedding"][0, 1, 5] = np.nan
    inp["obj_traj"][1, 0, 3:9, 2] = np.nan
    inp["obj_traj"][2, 1, :, 0] = np.nan
    enc, act, keys = run_encoder(SegmentEncoder, sd, inp)
    assert np.isfinite(enc).all() and np.isfinite(act).all()
    save_encoder_case("segment_encoder_nonfinite.npz", sd, inp, {"out/encoding": enc, "out/activation": act}, keys)

    # FID: two feature sets N = 512, d = 64; and a near-singular pair - fewer samples than features, so both covariances are singular
    # (scipy 1.15's sqrtm returns a finite root for it: eps_path records whether the reference took its eps retry)
    rng = np.random.default_rng(41)
    mix = rng.normal(size=(64, 64)) / 8.0
    a = rng.normal(size=(512, 64)) @ mix
    b = rng.normal(0.1, 1.1, size=(512, 64)) @ mix + 0.05
    cases = {"fid_n512_d64.npz": (a, b)}
    c = rng.normal(size=(48, 64)) @ mix
    e = rng.normal(0.2, 0.9, size=(48, 64)) @ mix
    cases["fid_near_singular.npz"] = (c, e)
    for name, (x, y) in cases.items():
        s1, s2 = fid_mod.calculate_activation_statistics(x), fid_mod.calculate_activation_statistics(y)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            fid = fid_mod.calculate_fid(s1, s2)
        eps_path = "adding" in buf.getvalue()
        path = os.path.join(GOLDEN, name)
        np.savez_compressed(path, act1=x, act2=y, fid=np.float64(fid), eps_path=np.bool_(eps_path))
        print(f"{name}: fid {fid!r} eps_path {eps_path} {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        raise SystemExit("usage: python tools/capture_encoder_golden.py REFERENCE_ROOT")
    main(sys.argv[1])
