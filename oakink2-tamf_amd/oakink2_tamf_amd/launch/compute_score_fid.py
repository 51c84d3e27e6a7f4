"""FID of generated motions on MI355X (reference script/compute_score/compute_score_fid.py:208-361).

    python -m oakink2_tamf_amd.launch.compute_score_fid --cfg config/arch_encoder.yml \
        --data.process_range "?(file:./asset/split/test.txt)" --debug.cache_dict_filepath common/save_cache_dict/main/cache/test.pkl \
        --debug.sample_refine_filepath common/sample_refine/main/sample/test/arch_mdm_l__0399 \
        --debug.encoder_checkpoint_filepath ENCODER_CKPT [--batch_size 64] [--device cuda:0] [--out_json fid.json]

The reference's argument names and defaults (`--data.*`, `--debug.*`, the `model:` keys of the yml), plus `--batch_size`, `--device`,
`--out_json`, `--output_dim` and `--dry_run` of this build.  The clips come from the segment cache through
dataset.interaction_segment.InteractionSegmentData; a clip whose `info` was seen before is skipped, and so is a clip without a
`save_dict.pkl` under --debug.sample_refine_filepath (the tree launch.sample_refine writes, launch/formats.py).  The generated clip is the
ground-truth item with `pose_repr` replaced by the save dict's `refine_pose_repr`, frames from `len` on set to zero (reference :319-321).

Both sets go through the SegmentEncoder (model/segment_encoder.py, HIP) in batches of clips of equal length, each clip averaging over
its own objects - the same numbers as the reference's batches of one clip (:306-349).  The FID of the two sets of `encoding`s
(metrics/fid.py) is printed with its four terms.  The reference's ActionRecognitionAdapter only supplies `output_dim` to the encoder,
on which no weight depends; `--output_dim` sets it (default 0).
"""
from __future__ import annotations

import argparse
import json
import logging
import os
import sys
from typing import Dict, List, Tuple

import numpy as np

from . import formats
from .sample import DEFAULT_CACHE_DICT, _abspath, _merge, _str_list, decode_file_macro

_logger = logging.getLogger("oakink2_tamf_amd.launch.compute_score_fid")
PROG = "compute_score_fid"

MODEL_DEFAULTS = dict(input_dim=99, obj_input_dim=9, hand_shape_dim=10, obj_embed_dim=768, latent_dim=256, ff_size=1024,
                      num_layers=8, num_heads=4, dropout=0.1, activation="gelu")  # SegmentEncoder's own defaults
DEFAULTS = {  # reference :54-127 (paths relative to the working directory)
    "data.data_prefix": "data",
    "data.process_range": None,
    "data.obj_embedding_prefix": os.path.join("common", "retrieve_obj_embedding", "main", "embedding"),
    "data.obj_pointcloud_prefix": os.path.join("common", "retrieve_obj_pointcloud", "main", "pointcloud"),
    "debug.cache_dict_filepath": DEFAULT_CACHE_DICT,
    "debug.sample_refine_filepath": os.path.join("common", "sample_refine", "main", "sample", "test", "arch_mdm_l__0399"),
    "debug.encoder_checkpoint_filepath": None,
}
PATH_KEYS = ("data.data_prefix", "data.obj_embedding_prefix", "data.obj_pointcloud_prefix", "debug.cache_dict_filepath",
             "debug.sample_refine_filepath", "debug.encoder_checkpoint_filepath")


def parse_args(argv: List[str]) -> Dict:
    ap = argparse.ArgumentParser(prog="oakink2_tamf_amd.launch.compute_score_fid", allow_abbrev=False)
    ap.add_argument("--cfg", action="append", default=[], help="yml preset(s) with a `model:` section (config/arch_encoder.yml)")
    for key in DEFAULTS:
        ap.add_argument("--" + key, dest=key.replace(".", "__"), default=None)
    for key, v in MODEL_DEFAULTS.items():
        ap.add_argument("--model." + key, dest="model__" + key, type=type(v), default=None)
    ap.add_argument("--batch_size", type=int, default=64, help="clips per encoder launch (clips of equal length are batched)")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--output_dim", type=int, default=0, help="SegmentEncoder's output_dim (no weight depends on it)")
    ap.add_argument("--out_json", default=None, help="also write the score, its terms and n_clips to this JSON file")
    ap.add_argument("--dry_run", action="store_true", help="list the clip pairs found and exit (no GPU, no checkpoint read)")
    a = ap.parse_args(argv)
    import yaml

    cfg: Dict = {"model": dict(MODEL_DEFAULTS), "data": {}, "debug": {}}
    for path in a.cfg:
        with open(path) as f:
            _merge(cfg, yaml.safe_load(f) or {})
    for key, default in DEFAULTS.items():
        sect, name = key.split(".")
        val = getattr(a, key.replace(".", "__"))
        if val is None:
            val = cfg[sect].get(name, default)
        if key == "data.process_range" and val is not None:
            val = _str_list(val) if isinstance(val, str) else decode_file_macro(list(val))
        if key in PATH_KEYS and val is not None:
            val = _abspath(val)
        cfg[sect][name] = val
    for key in MODEL_DEFAULTS:
        val = getattr(a, "model__" + key)
        if val is not None:
            cfg["model"][key] = val
    if not cfg["debug"]["encoder_checkpoint_filepath"] and not a.dry_run:
        ap.error("--debug.encoder_checkpoint_filepath is required")
    cfg["runtime"] = {"batch_size": max(1, a.batch_size), "device": a.device, "output_dim": a.output_dim, "out_json": a.out_json,
                      "dry_run": a.dry_run}
    return cfg


def load_pairs(cfg) -> List[Tuple[Dict, Dict]]:
    """(ground-truth item, generated item) of every clip with a save dict, in dataset order, duplicates of `info` skipped"""
    from ..dataset.interaction_segment import InteractionSegmentData, load_cache_dict

    d, g = cfg["data"], cfg["debug"]
    if not os.path.exists(g["cache_dict_filepath"]):
        raise SystemExit(f"segment cache {g['cache_dict_filepath']} not found; pass --debug.cache_dict_filepath <pkl>")
    dataset = InteractionSegmentData(process_range_list=d.get("process_range"), data_prefix=d.get("data_prefix"),
                                     obj_embedding_prefix=d["obj_embedding_prefix"], obj_pointcloud_prefix=d["obj_pointcloud_prefix"],
                                     append_reverse_segment=False, cache_dict=load_cache_dict(g["cache_dict_filepath"]))
    root = g["sample_refine_filepath"]
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
        gen = dict(item)
        pose = np.array(formats.read_refine_sample(path)["refine_pose_repr"], dtype=np.float32, copy=True)
        pose[int(item["len"]):] = 0.0
        gen["pose_repr"] = pose
        pairs.append((item, gen))
    return pairs


ENCODER_FIELDS = ("pose_repr", "shape", "hand_side", "obj_embedding", "obj_traj", "obj_num")


def encode_items(model, items: List[Dict], batch_size: int, device) -> np.ndarray:
    """(N, d) float64 encodings of the items, in order: clips of equal length in batches of up to batch_size, per-clip object means"""
    import torch

    from ..dataset.batching import interaction_segment_collate

    out = [None] * len(items)
    by_T: Dict[int, List[int]] = {}
    for i, it in enumerate(items):
        by_T.setdefault(int(np.asarray(it["pose_repr"]).shape[0]), []).append(i)
    for T in sorted(by_T):
        idx = by_T[T]
        for s in range(0, len(idx), batch_size):
            part = idx[s: s + batch_size]
            batch = interaction_segment_collate([{k: items[i][k] for k in ENCODER_FIELDS} for i in part])
            for k in ("pose_repr", "shape", "obj_embedding", "obj_traj"):
                batch[k] = batch[k].to(device=device, dtype=torch.float32)
            enc = model.encode(batch, obj_num=batch["obj_num"].cpu().numpy(), with_activation=False)["encoding"][0]
            enc = enc.cpu().numpy().astype(np.float64)
            for j, i in enumerate(part):
                out[i] = enc[j]
    return np.stack(out, axis=0) if out else np.zeros((0, 0))


def main(argv=None) -> int:
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    cfg = parse_args(sys.argv[1:] if argv is None else argv)
    rt = cfg["runtime"]
    pairs = load_pairs(cfg)
    _logger.info("clips with a generated sample: %d", len(pairs))
    if rt["dry_run"]:
        print(json.dumps({"n_clips": len(pairs), "model": cfg["model"], "sample_refine_filepath": cfg["debug"]["sample_refine_filepath"]}))
        return 0
    if len(pairs) < 2:
        raise SystemExit(f"FID needs at least two clips with a generated sample, found {len(pairs)} under "
                         f"{cfg['debug']['sample_refine_filepath']}")
    import torch

    from ..metrics.fid import calculate_activation_statistics, frechet_distance_terms
    from ..model.segment_encoder import SegmentEncoder

    device = torch.device(rt["device"])
    mc = cfg["model"]
    model = SegmentEncoder(rt["output_dim"], **{k: mc[k] for k in MODEL_DEFAULTS}).to(device)
    state = torch.load(cfg["debug"]["encoder_checkpoint_filepath"], map_location="cpu")
    missing, unexpected = model.load_state_dict(state, strict=False)
    _logger.info("missing_keys: %s", [k for k in missing if not k.startswith("clip_model")])
    _logger.info("unexpected_keys: %s", unexpected)
    bs = rt["batch_size"]
    gt = encode_items(model, [p[0] for p in pairs], bs, device)
    gen = encode_items(model, [p[1] for p in pairs], bs, device)
    model.close()
    terms = frechet_distance_terms(*calculate_activation_statistics(gt), *calculate_activation_statistics(gen))
    print(f"n_clips {len(pairs)}")
    print(f"mean_sq_diff {terms['mean_sq_diff']!r}")
    print(f"trace_sigma1 {terms['trace_sigma1']!r}")
    print(f"trace_sigma2 {terms['trace_sigma2']!r}")
    print(f"trace_covmean {terms['trace_covmean']!r}")
    print(f"fid {terms['fid']!r}")
    if rt["out_json"]:
        os.makedirs(os.path.dirname(os.path.abspath(rt["out_json"])), exist_ok=True)
        with open(rt["out_json"], "w") as f:
            json.dump({"n_clips": len(pairs), **terms}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
