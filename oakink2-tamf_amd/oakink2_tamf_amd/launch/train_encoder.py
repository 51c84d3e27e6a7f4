"""Train the FID score's SegmentEncoder on MI355X (reference launch/train_encoder.py): an action classifier over the segment cache
whose checkpoints `script/compute_score_fid.sh` reads as they are.

    python -m oakink2_tamf_amd.launch.train_encoder --cfg config/arch_encoder.yml --train.cache_dict_filepath TRAIN.pkl \
        --train.data.pose_repr_sample_dir_list common/sample/main/sample/train/arch_mdm_l__0099 --train.num_epoch 400 \
        --train.scheduler_milestone 80,160,240,320 --val.val_freq 20 --test.test_freq 20 --exp_id "encoder__?(ts)" --commit

The reference's argument names (`--train.*`, `--val.*`, `--test.*`, `--data.*`, `--runtime.seed`, `--exp_id`, `--commit`, the `model:`
keys of the yml) plus `--dry_run` of this build, which lists dataset sizes, steps per epoch and the schedule without touching the GPU.

As the reference: the training set is the concatenation identity + generated samples + Gaussian perturbation of the train cache
(dataset/pose_repr_sample.py) under ActionRecognitionAdapter, `pose_repr` replaced by `sample_pose_repr`; shuffled batches with
drop_last; AdamW(lr 1e-4, weight_decay 0); per-parameter clip_grad_norm_(param, 0.1, 2.0); MultiStepLR stepped per epoch; with
--commit, `save/model_%04d.pt` (a flat state dict) and `save/optimizer_%04d.pt` under common/train_encoder/<exp_id>/ after epoch 0,
every record_freq-th epoch and the last.  Forward, loss and gradients of a batch are the HIP training step
(model/segment_encoder_train.py); the optimiser, the clipping and the schedule are PyTorch on the device.  Validation and test
accuracy go through the inference kernel (SegmentEncoder.forward).

One device: the reference's 4-GPU DDP run with a world batch of 256 is one batch of 256 on one GPU here."""
from __future__ import annotations

import argparse
import json
import logging
import os
import sys
import time
from typing import Dict, List, Optional

import numpy as np

from .compute_score_fid import MODEL_DEFAULTS
from .sample import _abspath, _int_list, _merge, _str_list

_logger = logging.getLogger("oakink2_tamf_amd.launch.train_encoder")
PROG = "train_encoder"

DEFAULTS = {  # reference launch/train_encoder.py:61-275 (paths relative to the working directory)
    "data.data_prefix": "data",
    "data.obj_embedding_prefix": None,
    "data.obj_pointcloud_prefix": None,
    "train.process_range": None, "val.process_range": None, "test.process_range": None,
    "train.cache_dict_filepath": None, "val.cache_dict_filepath": None, "test.cache_dict_filepath": None,
    "train.batch_size": 256,
    "train.num_epoch": 400,
    "train.record_freq": 20,
    "train.scheduler_milestone": [150, 250],
    "train.scheduler_gamma": 0.5,
    "train.reload_ckpt_model_filepath": None,
    "train.reload_ckpt_optimizer_filepath": None,
    "train.data.pose_repr_sample_dir_list": [],
    "train.data.gaussian_perturb_range": [0.02, 0.1],
    "val.val_freq": 20,
    "test.test_freq": 20,
    "runtime.seed": 0,
    "runtime.num_worker": 0,
    "runtime.device_id": [0],
}
PATH_KEYS = ("data.data_prefix", "data.obj_embedding_prefix", "data.obj_pointcloud_prefix", "train.cache_dict_filepath", "val.cache_dict_filepath",
             "test.cache_dict_filepath", "train.reload_ckpt_model_filepath", "train.reload_ckpt_optimizer_filepath")
CONVERT = {"train.batch_size": int, "train.num_epoch": int, "train.record_freq": int, "train.scheduler_milestone": _int_list,
           "train.scheduler_gamma": float, "val.val_freq": int, "test.test_freq": int, "runtime.seed": int, "runtime.num_worker": int,
           "runtime.device_id": _int_list, "train.process_range": _str_list, "val.process_range": _str_list, "test.process_range": _str_list,
           "train.data.pose_repr_sample_dir_list": lambda v: [p for p in str(v).replace(",", ":").split(":") if p],
           "train.data.gaussian_perturb_range": lambda v: [float(x) for x in str(v).split(",")]}
ENCODER_FIELDS = ("pose_repr", "shape", "hand_side", "obj_embedding", "obj_traj")


def _get(cfg: Dict, dotted: str, default=None):
    node = cfg
    for part in dotted.split("."):
        if not isinstance(node, dict) or part not in node:
            return default
        node = node[part]
    return node


def _set(cfg: Dict, dotted: str, value) -> None:
    parts = dotted.split(".")
    for part in parts[:-1]:
        cfg = cfg.setdefault(part, {})
    cfg[parts[-1]] = value


def parse_args(argv: List[str]) -> Dict:
    ap = argparse.ArgumentParser(prog="oakink2_tamf_amd.launch.train_encoder", allow_abbrev=False)
    ap.add_argument("--cfg", action="append", default=[], help="yml preset(s): arch_encoder.yml, cache_dict.yml, bs_256.yml, ...")
    for key in DEFAULTS:
        ap.add_argument("--" + key, dest=key.replace(".", "__"), default=None)
    for key, v in MODEL_DEFAULTS.items():
        ap.add_argument("--model." + key, dest="model__" + key, type=type(v), default=None)
    ap.add_argument("--data.enable_obj_model", dest="enable_obj_model", action="store_true")
    ap.add_argument("--exp_id", default="encoder__?(ts)")
    ap.add_argument("--commit", action="store_true", help="write log, options and checkpoints under common/train_encoder/<exp_id>/")
    ap.add_argument("--dry_run", action="store_true", help="list dataset sizes, steps per epoch and the schedule; no GPU")
    a = ap.parse_args(argv)
    import yaml

    cfg: Dict = {"model": dict(MODEL_DEFAULTS)}
    for path in a.cfg:
        with open(path) as f:
            _merge(cfg, yaml.safe_load(f) or {})
    for key, default in DEFAULTS.items():
        val = getattr(a, key.replace(".", "__"))
        if val is not None:
            val = CONVERT.get(key, str)(val)
        else:
            val = _get(cfg, key, default)
        if key in PATH_KEYS and val is not None:
            val = _abspath(val)
        if key == "train.data.pose_repr_sample_dir_list":
            val = [_abspath(p) for p in (val or [])]
        _set(cfg, key, val)
    for key in MODEL_DEFAULTS:
        val = getattr(a, "model__" + key)
        if val is not None:
            cfg["model"][key] = val
    cfg["data"]["enable_obj_model"] = bool(a.enable_obj_model)
    exp_id = a.exp_id.replace("?(ts)", time.strftime("%Y_%m%d_%H%M_%S"))
    cfg["ckpt"] = {"exp_id": exp_id, "commit": bool(a.commit), "ckpt_path": os.path.join(os.getcwd(), "common", PROG, exp_id)}
    cfg["dry_run"] = bool(a.dry_run)
    return cfg


class _Concat:
    """items of several datasets, one after the other (torch.utils.data.ConcatDataset's indexing)"""

    def __init__(self, parts):
        self.parts = list(parts)
        self.ends = np.cumsum([len(p) for p in self.parts])

    def __len__(self) -> int:
        return int(self.ends[-1]) if len(self.ends) else 0

    def __getitem__(self, index: int) -> Dict:
        if index < 0 or index >= len(self):
            raise IndexError(index)
        k = int(np.searchsorted(self.ends, index, side="right"))
        return self.parts[k][index - (int(self.ends[k - 1]) if k else 0)]


def _base_dataset(cfg: Dict, split: str):
    from ..dataset.interaction_segment import InteractionSegmentData, load_cache_dict

    path = cfg[split]["cache_dict_filepath"]
    if path is None:
        return None
    if not os.path.exists(path):
        raise SystemExit(f"segment cache {path} not found; pass --{split}.cache_dict_filepath <pkl>")
    d = cfg["data"]
    return InteractionSegmentData(process_range_list=cfg[split].get("process_range"), data_prefix=d.get("data_prefix"),
                                  obj_embedding_prefix=d["obj_embedding_prefix"], obj_pointcloud_prefix=d["obj_pointcloud_prefix"],
                                  cache_dict=load_cache_dict(path))


def build_datasets(cfg: Dict) -> Dict:
    """{"train": ActionRecognitionAdapter(identity + generated + perturbed), "val", "test" (or None), "parts": the three lengths}"""
    from ..dataset.action_adapter import ActionRecognitionAdapter
    from ..dataset.pose_repr_sample import GeneratedPoseReprSampleAdaptor, GuassianPerturbSampleAdaptor, IdentitySampleAdaptor

    base = _base_dataset(cfg, "train")
    if base is None:
        raise SystemExit("--train.cache_dict_filepath is required")
    td = cfg["train"]["data"]
    parts = [IdentitySampleAdaptor(base), GeneratedPoseReprSampleAdaptor(base, td["pose_repr_sample_dir_list"]),
             GuassianPerturbSampleAdaptor(base, td["gaussian_perturb_range"])]
    out = {"train": ActionRecognitionAdapter(_Concat(parts)), "parts": [len(p) for p in parts], "base": base, "generated": parts[1]}
    for split in ("val", "test"):
        ds = _base_dataset(cfg, split)
        out[split] = ActionRecognitionAdapter(ds) if ds is not None else None
    return out


def record_epochs(num_epoch: int, freq: Optional[int]) -> List[int]:
    """the epochs after which the reference records / validates / tests: 0, every freq-th and the last (:569-570, :582, :626)"""
    if freq is None or freq == -1:
        return []
    return [e for e in range(num_epoch) if e == 0 or e % freq == freq - 1 or e == num_epoch - 1]


def plan(cfg: Dict, sets: Dict) -> Dict:
    t = cfg["train"]
    n, bs = len(sets["train"]), int(t["batch_size"])
    lrs, lr = [], 1e-4
    for e in range(int(t["num_epoch"])):
        lrs.append(lr)
        if e + 1 in t["scheduler_milestone"]:
            lr *= float(t["scheduler_gamma"])
    return {"train_identity": sets["parts"][0], "train_generated": sets["parts"][1], "train_gaussian_perturb": sets["parts"][2], "train_total": n,
            "val": len(sets["val"]) if sets["val"] is not None else None, "test": len(sets["test"]) if sets["test"] is not None else None,
            "batch_size": bs, "steps_per_epoch": n // bs, "num_epoch": int(t["num_epoch"]), "scheduler_milestone": list(t["scheduler_milestone"]),
            "scheduler_gamma": float(t["scheduler_gamma"]), "lr_first": lrs[0] if lrs else None, "lr_last": lrs[-1] if lrs else None,
            "record_epochs": record_epochs(int(t["num_epoch"]), t["record_freq"]), "model": cfg["model"]}


def collate(items: List[Dict], device):
    """-> (batch of the encoder's fields on `device`, with pose_repr = sample_pose_repr where the item has one; labels int64 numpy)"""
    import torch

    from ..dataset.batching import interaction_segment_collate

    rows = []
    for it in items:
        row = {k: it[k] for k in ENCODER_FIELDS}
        if "sample_pose_repr" in it:
            row["pose_repr"] = it["sample_pose_repr"]
        rows.append(row)
    batch = interaction_segment_collate(rows)
    for k in ("pose_repr", "shape", "obj_embedding", "obj_traj"):
        batch[k] = batch[k].to(device=device, dtype=torch.float32)
    return batch, np.asarray([int(it["action_label_id"]) for it in items], np.int64)


def evaluate(model, dataset, batch_size: int, device) -> Dict:
    """cross-entropy and accuracy of the inference kernel's activation over a dataset, in order"""
    import torch

    ce, hit, n = 0.0, 0, len(dataset)
    for s in range(0, n, batch_size):
        batch, labels = collate([dataset[i] for i in range(s, min(n, s + batch_size))], device)
        act = model(batch)["activation"]
        lab = torch.from_numpy(labels).to(device)
        ce += float(torch.nn.functional.cross_entropy(act, lab, reduction="sum"))
        hit += int((act.argmax(1) == lab).sum())
    return {"ce": ce / max(n, 1), "acc": hit / max(n, 1)}


def main(argv=None) -> int:
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    argv = sys.argv[1:] if argv is None else argv
    cfg = parse_args(argv)
    np.random.seed(int(cfg["runtime"]["seed"]))  # (the Gaussian perturbation draws from np.random, as the reference)
    sets = build_datasets(cfg)
    info = plan(cfg, sets)
    if cfg["dry_run"]:
        print(json.dumps(info))
        return 0
    if info["steps_per_epoch"] < 1:
        raise SystemExit(f"{info['train_total']} training items do not fill one batch of {info['batch_size']} (drop_last)")
    import torch

    from . import upkeep
    from ..model.segment_encoder import SegmentEncoder
    from ..model.segment_encoder_train import SegmentEncoderTrainStep

    ck, t = cfg["ckpt"], cfg["train"]
    upkeep.ckpt_setup(ck, argv=argv)
    upkeep.ckpt_opt({**ck, "run": {k: v for k, v in cfg.items() if k != "ckpt"}})
    if len(cfg["runtime"]["device_id"]) > 1:
        _logger.info("one device only: using cuda:%d of --runtime.device_id %s", cfg["runtime"]["device_id"][0], cfg["runtime"]["device_id"])
    device = torch.device(f"cuda:{cfg['runtime']['device_id'][0]}")
    seed = int(cfg["runtime"]["seed"])
    torch.manual_seed(seed)
    train = sets["train"]
    mc = cfg["model"]
    model = SegmentEncoder(train.max_action, **{k: mc[k] for k in MODEL_DEFAULTS})
    if t["reload_ckpt_model_filepath"]:
        missing, unexpected = model.load_state_dict(torch.load(t["reload_ckpt_model_filepath"], map_location="cpu"), strict=False)
        _logger.info("missing_keys: %s unexpected_keys: %s", missing, unexpected)
    model = model.to(device)
    bs = info["batch_size"]
    # the longest clip of the training set: the cache's padded poses and the generated samples (the perturbed copies have the cache's
    # lengths; read from the base dataset, so that no np.random draw is spent here)
    max_frames = max([int(np.asarray(sets["base"][i]["pose_repr"]).shape[0]) for i in range(len(sets["base"]))] +
                     [int(np.asarray(v).shape[0]) for v in sets["generated"].pose_repr_map.values()])
    step_fn = SegmentEncoderTrainStep(model, bs, max_frames, seed=seed)
    optimizer = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=0.0)
    if t["reload_ckpt_optimizer_filepath"]:
        optimizer.load_state_dict(torch.load(t["reload_ckpt_optimizer_filepath"], map_location="cpu"))
    scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=list(t["scheduler_milestone"]), gamma=float(t["scheduler_gamma"]))
    num_epoch, step = info["num_epoch"], 0
    evals = {"val": record_epochs(num_epoch, cfg["val"]["val_freq"]), "test": record_epochs(num_epoch, cfg["test"]["test_freq"])}
    for epoch in range(num_epoch):
        gen = torch.Generator().manual_seed(seed + epoch)
        order = torch.randperm(len(train), generator=gen).tolist()
        out = None
        for s in range(info["steps_per_epoch"]):
            idx = order[s * bs:(s + 1) * bs]
            batch, labels = collate([train[i] for i in idx], device)
            out = step_fn.loss_and_grads(batch, labels, clip_ids=idx, step=step)
            for group in optimizer.param_groups:  # (the reference's clip_gradient: each parameter on its own)
                for p in group["params"]:
                    torch.nn.utils.clip_grad_norm_(p, 0.1, 2.0)
            optimizer.step()
            step += 1
        scheduler.step()
        _logger.info("train epoch %04d conclude | loss: %f acc: %f", epoch, float(out["loss"]), float(out["acc"]))
        _logger.info("train epoch %04d lr %s", epoch, [g["lr"] for g in optimizer.param_groups])
        if ck["commit"] and epoch in info["record_epochs"]:
            save = os.path.join(ck["ckpt_path"], "save")
            os.makedirs(save, exist_ok=True)
            torch.save({k: v.detach().cpu() for k, v in model.state_dict().items()}, os.path.join(save, f"model_{epoch:0>4}.pt"))
            torch.save(optimizer.state_dict(), os.path.join(save, f"optimizer_{epoch:0>4}.pt"))
        for split in ("val", "test"):
            if sets[split] is not None and epoch in evals[split]:
                model.refresh_hip_weights()
                res = evaluate(model, sets[split], bs, device)
                _logger.info("%s epoch %04d | ce: %f acc: %f", split, epoch, res["ce"], res["acc"])
    model.refresh_hip_weights()
    step_fn.close()
    model.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
