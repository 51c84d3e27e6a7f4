"""What the CR and PSKL-J score launchers share (reference script/compute_score/compute_score_cr.py, compute_score_psklj.py):
the `--data.*` / `--debug.*` / `--mano.*` arguments of the two scripts, the clip pairs, and the ground-truth MANO pass.

compute_score_fid.py keeps its own (older) copies of the argument and pair code: its cache option is spelled `--debug.cache_dict_filepath`
in the reference, and its generated item is a pose, not a save dict."""
from __future__ import annotations

import argparse
import os
from typing import Dict, List, Tuple

import numpy as np

from . import formats
from .sample import DEFAULT_CACHE_DICT, _abspath, _str_list, decode_file_macro
from .sample_refine import load_mano

DEFAULTS = {  # reference compute_score_cr.py:53-110 = compute_score_psklj.py:55-112 (paths relative to the working directory)
    "data.data_prefix": "data",
    "data.process_range": None,
    "data.obj_embedding_prefix": os.path.join("common", "retrieve_obj_embedding", "main", "embedding"),
    "data.obj_pointcloud_prefix": os.path.join("common", "retrieve_obj_pointcloud", "main", "pointcloud"),
    "data.cache_dict_filepath": DEFAULT_CACHE_DICT,
    "debug.sample_refine_filepath": os.path.join("common", "sample_refine", "main", "sample", "test", "arch_mdm_l__0399"),
    "mano.mano_path": os.path.join("asset", "mano_v1_2"),
    "mano.factory": None,
}
PATH_KEYS = ("data.data_prefix", "data.obj_embedding_prefix", "data.obj_pointcloud_prefix", "data.cache_dict_filepath",
             "debug.sample_refine_filepath", "mano.mano_path")


def make_parser(module: str) -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="oakink2_tamf_amd.launch." + module, allow_abbrev=False)
    for key in DEFAULTS:
        ap.add_argument("--" + key, dest=key.replace(".", "__"), default=None)
    ap.add_argument("--batch_size", type=int, default=64, help="clips per MANO pass / kernel launch")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--out_json", default=None, help="also write the printed figures to this JSON file")
    ap.add_argument("--dry_run", action="store_true", help="list the clip pairs found and exit (no GPU, no MANO)")
    return ap


def build_config(a) -> Dict:
    cfg: Dict = {"data": {}, "debug": {}, "mano": {}}
    for key, default in DEFAULTS.items():
        sect, name = key.split(".")
        val = getattr(a, key.replace(".", "__"))
        if val is None:
            val = default
        if key == "data.process_range" and val is not None:
            val = _str_list(val) if isinstance(val, str) else decode_file_macro(list(val))
        if key in PATH_KEYS and val is not None:
            val = _abspath(val)
        cfg[sect][name] = val
    cfg["runtime"] = {"batch_size": max(1, a.batch_size), "device": a.device, "out_json": a.out_json, "dry_run": a.dry_run}
    return cfg


def load_pairs(cfg, obj_model_loader=None) -> List[Tuple[Dict, str]]:
    """(ground-truth item, path of its save_dict.pkl) of every clip with a save dict, in dataset order, duplicates of `info` skipped
    (reference compute_score_cr.py:213-231).  obj_model_loader(obj_id) -> (verts, faces), when given, is handed to the dataset, whose
    items then carry obj_verts / obj_faces (the SIV score); without it they do not, as before."""
    from ..dataset.interaction_segment import InteractionSegmentData, load_cache_dict

    d = cfg["data"]
    if not os.path.exists(d["cache_dict_filepath"]):
        raise SystemExit(f"segment cache {d['cache_dict_filepath']} not found; pass --data.cache_dict_filepath <pkl>")
    dataset = InteractionSegmentData(process_range_list=d.get("process_range"), data_prefix=d.get("data_prefix"),
                                     obj_embedding_prefix=d["obj_embedding_prefix"], enable_obj_model=True,
                                     obj_pointcloud_prefix=d["obj_pointcloud_prefix"], append_reverse_segment=False,
                                     cache_dict=load_cache_dict(d["cache_dict_filepath"]), obj_model_loader=obj_model_loader)
    root = cfg["debug"]["sample_refine_filepath"]
    seen, pairs = set(), []
    for i in range(len(dataset)):
        item = dataset[i]
        info = item["info"]
        key = tuple(info) if isinstance(info, (list, tuple)) else info
        if key in seen:
            continue
        seen.add(key)
        path = formats.refine_sample_path_in(root, info)
        if not os.path.exists(path):
            continue
        pairs.append((item, path))
    return pairs


def pair_listing(pairs) -> List[Dict]:
    """what --dry_run prints per pair"""
    return [{"info": list(it["info"]) if isinstance(it["info"], (list, tuple)) else it["info"], "len": int(it["len"]),
             "hand_side": it["hand_side"], "save_dict": path} for it, path in pairs]


def ground_truth_mano(items: List[Dict], mano, device, batch_size: int = 64):
    """Ground-truth hand joints and vertices of the items, in order (reference compute_score_cr.py:247-266,
    compute_score_psklj.py:249-268): pose_repr -> (tsl, quaternions) by the HIP pose decode -> the MANO layer of the clip's hand_side ->
    `joints + tsl`, `verts + tsl`.  Clips of one hand side go through the layer batch_size at a time, frames concatenated (the layer
    works per frame).  -> (list of (T, 21, 3), list of (T, 778, 3)) float32 numpy"""
    import torch

    from ..geometry import pose_repr_to_quat

    layer_rh, layer_lh = mano[0], mano[1]
    joints: List = [None] * len(items)
    verts: List = [None] * len(items)
    for side, layer in (("rh", layer_rh), ("lh", layer_lh)):
        idx = [i for i, it in enumerate(items) if it["hand_side"] == side]
        for s in range(0, len(idx), batch_size):
            part = idx[s: s + batch_size]
            frames = [int(np.asarray(items[i]["pose_repr"]).shape[0]) for i in part]
            pose = torch.from_numpy(np.concatenate([np.asarray(items[i]["pose_repr"], dtype=np.float32) for i in part], axis=0)).to(device)
            shape = torch.from_numpy(np.concatenate([np.asarray(items[i]["shape"], dtype=np.float32) for i in part], axis=0)).to(device)
            with torch.no_grad():
                tsl, quat = pose_repr_to_quat(pose)
                mo = layer(pose_coeffs=quat, betas=shape)
                j = (mo.joints + tsl.unsqueeze(1)).detach().cpu().numpy()
                v = (mo.verts + tsl.unsqueeze(1)).detach().cpu().numpy()
            o = 0
            for i, n in zip(part, frames):
                joints[i], verts[i] = j[o: o + n], v[o: o + n]
                o += n
    for it, j in zip(items, joints):
        if j is None:
            raise ValueError(f"unexpected hand_side: {it['hand_side']}")
    return joints, verts


def write_json(path: str, payload: Dict) -> None:
    import json

    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(payload, f, indent=1)


__all__ = ["DEFAULTS", "make_parser", "build_config", "load_pairs", "pair_listing", "ground_truth_mano", "load_mano", "write_json"]
