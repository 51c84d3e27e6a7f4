"""What launch/train.py (the denoiser G) and launch/train_refine.py (the refiner R) share: the reference's argument names
(launch/train.py:60-271, launch/train_refine.py), the training loop, the optimiser and the checkpoints.  A launcher supplies its
model, its native training step, its dataset and the function that runs one batch.

Behaviour (that of launch/train_encoder.py on this port): one device; shuffled batches with drop_last, the epoch's order from
torch.randperm under seed + epoch; `clip_ids` are the dataset indices and `step` the global step, so dropout masks are reproducible;
per-parameter clipping at (0.1, 2.0), AdamW(lr 1e-4, weight_decay 0), MultiStepLR per epoch; with --commit, `save/model_%04d.pt` (a flat
state dict without clip_model.*, what script/sample.sh / sample_refine.sh load) and `save/optimizer_%04d.pt` under
common/<prog>/<exp_id>/ after epoch 0, every record_freq-th epoch and the last.

The optimiser is optim.HipAdamW (`--train.optimizer hip`, two launches per step) or the reference's own sequence
(`--train.optimizer torch`: one clip_grad_norm_ per parameter, then torch.optim.AdamW.step()); their optimizer_%04d.pt files interchange.

Every random draw of an epoch (the order, the Gaussian perturbation, the diffusion timesteps and noise) is seeded by seed + epoch,
and `--train.start_epoch E` (this build's) continues at epoch E: a run resumed from model_%04d.pt + optimizer_%04d.pt of epoch E - 1
repeats the uninterrupted run bit for bit.  Without it a reloaded run starts again at epoch 0, as the reference's does.

--val.* / --test.* are accepted and logged as not run; one device only."""
from __future__ import annotations

import argparse
import importlib
import json
import logging
import os
import sys
import time
from typing import Callable, Dict, List, Optional, Sequence

import numpy as np

from .sample import _abspath, _int_list, _merge, _str_list
from .train_encoder import _Concat, _get, _set, record_epochs

BASE_LR, CLIP_MAX_NORM, CLIP_NORM_TYPE = 1e-4, 0.1, 2.0  # reference launch/train.py: AdamW(lr=1e-4), clip_gradient(optimizer, 0.1, 2.0)


def _path_list(v) -> List[str]:
    return [p for p in str(v).replace(",", ":").split(":") if p]


def _float_list(v) -> List[float]:
    return [float(x) for x in str(v).split(",")]


DEFAULTS = {  # reference launch/train.py:60-271 (paths relative to the working directory); the last block is this build's own
    "data.data_prefix": "data",
    "data.obj_embedding_prefix": None,
    "data.obj_pointcloud_prefix": None,
    "train.process_range": None, "val.process_range": None, "test.process_range": None,
    "train.cache_dict_filepath": None, "val.cache_dict_filepath": None, "test.cache_dict_filepath": None,
    "train.batch_size": 64, "val.batch_size": 64, "test.batch_size": 64,
    "train.num_epoch": 400,
    "train.record_freq": 20,
    "train.scheduler_milestone": [150, 250],
    "train.scheduler_gamma": 0.5,
    "train.reload_ckpt_model_filepath": None,
    "train.reload_ckpt_optimizer_filepath": None,
    "train.loss.vpe_path": None,
    "train.loss.c_weight_path": None,
    "val.val_freq": 20,
    "test.test_freq": 20,
    "runtime.seed": 0,
    "runtime.num_worker": 0,
    "runtime.device_id": [0],
    "mano.mano_path": None,
    "mano.factory": None,
    "train.optimizer": "hip",
    "train.start_epoch": 0,
    "data.obj_sdf_prefix": None,
}
PATH_KEYS = ("data.data_prefix", "data.obj_embedding_prefix", "data.obj_pointcloud_prefix", "train.cache_dict_filepath", "val.cache_dict_filepath",
             "test.cache_dict_filepath", "train.reload_ckpt_model_filepath", "train.reload_ckpt_optimizer_filepath", "train.loss.vpe_path",
             "train.loss.c_weight_path", "mano.mano_path", "data.text_embedding_filepath", "data.obj_sdf_prefix")
PATH_LIST_KEYS = ("train.data.pose_repr_sample_dir_list", "val.data.pose_repr_sample_dir_list", "test.data.pose_repr_sample_dir_list")
CONVERT = {"train.batch_size": int, "val.batch_size": int, "test.batch_size": int, "train.num_epoch": int, "train.record_freq": int,
           "train.scheduler_milestone": _int_list, "train.scheduler_gamma": float, "val.val_freq": int, "test.test_freq": int,
           "runtime.seed": int, "runtime.num_worker": int, "runtime.device_id": _int_list, "train.process_range": _str_list,
           "val.process_range": _str_list, "test.process_range": _str_list, "train.start_epoch": int,
           "train.data.pose_repr_sample_dir_list": _path_list, "val.data.pose_repr_sample_dir_list": _path_list,
           "test.data.pose_repr_sample_dir_list": _path_list, "train.data.gaussian_perturb_range": _float_list}


def parse_args(argv: List[str], prog: str, model_defaults: Dict, loss_coefs: Sequence[str], extra_defaults: Dict, exp_default: str,
               own_coefs: Sequence[str] = ()) -> Dict:
    """-> the resolved options: yml presets merged in order, then the command line over them; `loss_coefs` are the launcher's
    --train.loss.coef_* names (default 0.0, launch/param/loss.py / loss_refine.py), `extra_defaults` its own dotted options;
    `own_coefs` are --train.loss.coef_* of this build's own terms: 0.0 when absent like the others, but listed under train.loss only
    when a preset or the command line gives them, so that a run without them resolves to the options it always had"""
    own = {f"train.loss.{c}" for c in own_coefs}
    defaults = {**DEFAULTS, **{f"train.loss.{c}": 0.0 for c in tuple(loss_coefs) + tuple(own_coefs)}, **extra_defaults}
    convert = {**CONVERT, **{f"train.loss.{c}": float for c in tuple(loss_coefs) + tuple(own_coefs)}}
    ap = argparse.ArgumentParser(prog=f"oakink2_tamf_amd.launch.{prog}", allow_abbrev=False)
    ap.add_argument("--cfg", action="append", default=[], help="yml preset(s), merged in order: arch_mdm_l.yml, loss_param.yml, bs_64.yml, ...")
    for key in defaults:
        ap.add_argument("--" + key, dest=key.replace(".", "__"), default=None)
    for key, v in model_defaults.items():
        ap.add_argument("--model." + key, dest="model__" + key, type=type(v), default=None)
    ap.add_argument("--data.enable_obj_model", dest="enable_obj_model", action="store_true")
    ap.add_argument("--data.append_reverse_segment", dest="append_reverse_segment", action="store_true")
    ap.add_argument("--exp_id", default=exp_default)
    ap.add_argument("--commit", action="store_true", help=f"write log, options and checkpoints under common/{prog}/<exp_id>/")
    ap.add_argument("--dry_run", action="store_true", help="list dataset sizes, steps per epoch and the schedule; no GPU")
    a = ap.parse_args(argv)
    import yaml

    cfg: Dict = {"model": dict(model_defaults)}
    for path in a.cfg:
        with open(path) as f:
            _merge(cfg, yaml.safe_load(f) or {})
    for key, default in defaults.items():
        val = getattr(a, key.replace(".", "__"))
        if key in own and val is None and _get(cfg, key, None) is None:
            continue
        val = convert.get(key, str)(val) if val is not None else _get(cfg, key, default)
        if key in PATH_KEYS and val is not None:
            val = _abspath(val)
        if key in PATH_LIST_KEYS:
            val = [_abspath(p) for p in (val or [])]
        _set(cfg, key, val)
    for key in model_defaults:
        val = getattr(a, "model__" + key)
        if val is not None:
            cfg["model"][key] = val
    cfg["data"]["enable_obj_model"] = bool(a.enable_obj_model or _get(cfg, "data.enable_obj_model", False))
    cfg["data"]["append_reverse_segment"] = bool(a.append_reverse_segment or _get(cfg, "data.append_reverse_segment", False))
    if cfg["train"]["optimizer"] not in ("hip", "torch"):
        ap.error(f"--train.optimizer must be hip or torch, got {cfg['train']['optimizer']!r}")
    if not 0 <= cfg["train"]["start_epoch"] <= cfg["train"]["num_epoch"]:
        ap.error("--train.start_epoch must lie in [0, --train.num_epoch]")
    exp_id = a.exp_id.replace("?(ts)", time.strftime("%Y_%m%d_%H%M_%S"))
    cfg["ckpt"] = {"exp_id": exp_id, "commit": bool(a.commit), "ckpt_path": os.path.join(os.getcwd(), "common", prog, exp_id)}
    cfg["dry_run"] = bool(a.dry_run)
    return cfg


def base_dataset(cfg: Dict, reverse: bool = False):
    """InteractionSegmentData on the train cache; its frame count is the cache's own padded length"""
    from ..dataset.interaction_segment import InteractionSegmentData, load_cache_dict

    path = cfg["train"]["cache_dict_filepath"]
    if path is None:
        raise SystemExit("--train.cache_dict_filepath is required")
    if not os.path.exists(path):
        raise SystemExit(f"segment cache {path} not found; pass --train.cache_dict_filepath <pkl>")
    d = cfg["data"]
    if not d["obj_embedding_prefix"]:
        raise SystemExit("--data.obj_embedding_prefix (config/obj_embedding.yml) is required: the models read batch['obj_embedding']")
    cache = load_cache_dict(path)
    poses = cache["interaction_segment_pose_list"]
    frames = int(np.asarray(poses[0]).shape[0]) if len(poses) else 160
    return InteractionSegmentData(process_range_list=cfg["train"].get("process_range"), data_prefix=d.get("data_prefix"), slice_max_len=frames,
                                  obj_embedding_prefix=d["obj_embedding_prefix"], obj_pointcloud_prefix=d["obj_pointcloud_prefix"],
                                  cache_dict=cache, append_reverse_segment=reverse)


def lr_at(epoch: int, milestones: Sequence[int], gamma: float, base: float = BASE_LR) -> float:
    """the learning rate MultiStepLR has reached at the start of `epoch`: one multiplication by gamma per milestone passed"""
    lr = base
    for m in sorted(milestones):
        if m <= epoch:
            lr *= gamma
    return lr


def plan(cfg: Dict, n_train: int, extra: Dict) -> Dict:
    """what --dry_run prints: sizes, steps per epoch, the schedule"""
    t = cfg["train"]
    bs, ne = int(t["batch_size"]), int(t["num_epoch"])
    ms, gamma = list(t["scheduler_milestone"]), float(t["scheduler_gamma"])
    return {**extra, "train_total": n_train, "batch_size": bs, "steps_per_epoch": n_train // bs, "num_epoch": ne, "start_epoch": int(t["start_epoch"]),
            "scheduler_milestone": ms, "scheduler_gamma": gamma, "lr_first": lr_at(0, ms, gamma) if ne else None,
            "lr_last": lr_at(ne - 1, ms, gamma) if ne else None, "record_epochs": record_epochs(ne, t["record_freq"]),
            "optimizer": t["optimizer"], "loss": dict(t["loss"]), "val": "not run", "test": "not run", "model": cfg["model"]}


def positive_coefs(cfg: Dict) -> Dict[str, float]:
    return {k: float(v) for k, v in cfg["train"]["loss"].items() if k.startswith("coef_") and float(v or 0.0) > 0.0}


PEN_COEF = "coef_pen_loss"  # this build's own term (model/interaction_loss.py): the excess penetration depth from the objects' SDF lattices


def pen_on(cfg: Dict) -> bool:
    return float(cfg["train"]["loss"].get(PEN_COEF) or 0.0) > 0.0


def sdf_grid_set(cfg: Dict, base, device=None, upload: bool = True):
    """The lattices of the `pen` term: one per distinct object id of the train cache `base` that has a pickle under
    --data.obj_sdf_prefix.  -> (sdfgrid.SdfGridSet or None, the ids without a pickle); (None, []) when the term is off.  upload=False
    reads and checks the files and touches no GPU."""
    if not pen_on(cfg):
        return None, []
    prefix = cfg["data"].get("obj_sdf_prefix")
    if not prefix:
        raise SystemExit("--train.loss.coef_pen_loss > 0 needs the objects' signed distance files: pass --data.obj_sdf_prefix DIR "
                         "(script/process_object_sdf.sh writes DIR/<obj_id>.pkl)")
    if not os.path.isdir(prefix):
        raise SystemExit(f"--data.obj_sdf_prefix {prefix} is no directory (script/process_object_sdf.sh writes DIR/<obj_id>.pkl)")
    from ..sdfgrid import SdfGridSet

    try:
        grids, missing = SdfGridSet.from_prefix(prefix, sorted(set(base.interaction_object_list)), device=device, upload=upload)
    except ValueError as e:
        raise SystemExit(f"--data.obj_sdf_prefix: {e}")
    if grids is None:
        raise SystemExit(f"--data.obj_sdf_prefix {prefix} holds no <obj_id>.pkl of the train cache's objects (script/process_object_sdf.sh writes them)")
    return grids, missing


def load_loss(cfg: Dict, device, coefs: Sequence[str], sdf_grids=None):
    """HandInteractionLoss over the MANO layers of --mano.factory (which must be differentiable) with --train.loss.*; `sdf_grids`:
    sdf_grid_set's lattices when coef_pen_loss is positive"""
    from ..model.interaction_loss import HandInteractionLoss

    spec = cfg["mano"].get("factory")
    if not spec or ":" not in str(spec):
        raise SystemExit("the hand losses need differentiable MANO layers: pass --mano.factory oakink2_tamf_amd.mano:make_mano_differentiable "
                         "--mano.mano_path DIR (the MANO assets are licence-gated and not shipped)")
    mod, fn = str(spec).split(":", 1)
    layer_rh, layer_lh = getattr(importlib.import_module(mod), fn)(cfg["mano"], device)[:2]
    for layer in (layer_rh, layer_lh):
        if not getattr(layer, "differentiable", True):
            raise SystemExit(f"--mano.factory {spec} returned inference-only layers; training needs differentiable ones "
                             "(oakink2_tamf_amd.mano:make_mano_differentiable)")
    lc = cfg["train"]["loss"]
    if not lc.get("c_weight_path") or not os.path.exists(lc["c_weight_path"]):
        raise SystemExit(f"--train.loss.c_weight_path {lc.get('c_weight_path')} not found (config/loss_param.yml: asset/grabnet/rhand_weight.npy)")
    v_weights = np.load(lc["c_weight_path"])
    if float(lc.get("coef_edge_len_loss") or 0.0) > 0.0:
        if not lc.get("vpe_path") or not os.path.exists(lc["vpe_path"]):
            raise SystemExit(f"--train.loss.vpe_path {lc.get('vpe_path')} not found (config/loss_param.yml: asset/grabnet/verts_per_edge.npy)")
        vpe = np.load(lc["vpe_path"]).astype(np.int64)
    else:
        vpe = np.zeros((0, 2), np.int64)
    kw = {c: float(lc.get(c) or 0.0) for c in coefs}
    if kw.get(PEN_COEF, 0.0) > 0.0:
        kw["sdf_grids"] = sdf_grids
    return HandInteractionLoss(layer_rh, layer_lh, vpe, v_weights, **kw).to(device)


def pad_points(clouds: Sequence[np.ndarray]):
    """per-clip (nobj_i, P, 3) point clouds -> (B, max nobj, P, 3) float32, zero rows for the padded objects"""
    import torch

    nobj = max(int(c.shape[0]) for c in clouds)
    out = np.zeros((len(clouds), nobj) + tuple(clouds[0].shape[1:]), np.float32)
    for b, c in enumerate(clouds):
        out[b, :c.shape[0]] = c
    return torch.from_numpy(out)


def collate(items: List[Dict], device, fields: Sequence[str], want_points: bool, grid_index=None) -> Dict:
    """interaction_segment_collate, then the float fields in `fields` on the device as float32, hand_side, obj_num as a list of ints,
    when asked obj_points (B, nobj, P, 3) from the items' obj_pointcloud and, with `grid_index` ({obj_id: lattice} of the `pen` term's
    set), sdf_grid_id (B, nobj) int32 from the items' obj_list"""
    import torch

    from ..dataset.batching import interaction_segment_collate

    full = interaction_segment_collate(items)
    batch = {k: full[k].to(device=device, dtype=torch.float32) for k in fields}
    batch["hand_side"] = list(full["hand_side"])
    batch["obj_num"] = [int(n) for n in full["obj_num"]]
    if want_points:
        if "obj_pointcloud" not in full:
            raise SystemExit("the distance losses need the objects' point clouds: pass --data.obj_pointcloud_prefix (config/obj_pointcloud.yml)")
        batch["obj_points"] = pad_points(full["obj_pointcloud"]).to(device)
    if grid_index is not None:
        from ..sdfgrid import grid_ids

        batch["sdf_grid_id"] = grid_ids(full["obj_list"], grid_index).to(device)
    return batch


def make_optimizer(kind: str, params):
    import torch

    params = list(params)
    if kind == "hip":
        from ..optim import HipAdamW

        return HipAdamW(params, lr=BASE_LR, weight_decay=0.0, clip_max_norm=CLIP_MAX_NORM)
    return torch.optim.AdamW(params, lr=BASE_LR, weight_decay=0.0)


def optimizer_step(kind: str, optimizer) -> None:
    """the reference's clip_gradient(optimizer, 0.1, 2.0) + optimizer.step()"""
    if kind != "hip":
        import torch

        for group in optimizer.param_groups:
            for p in group["params"]:
                if p.grad is not None:
                    torch.nn.utils.clip_grad_norm_(p, CLIP_MAX_NORM, CLIP_NORM_TYPE)
    optimizer.step()


def train_loop(cfg: Dict, argv: List[str], info: Dict, prog: str, dataset, build: Callable, run_batch: Callable, logger: logging.Logger) -> int:
    """build(device) -> (model, step_fn, context); run_batch(step_fn, context, items, idx, step, gen, device) -> {name: loss term} with
    "loss"; the parameters' .grad hold the gradients afterwards"""
    if info["steps_per_epoch"] < 1:
        raise SystemExit(f"{info['train_total']} training items do not fill one batch of {info['batch_size']} (drop_last)")
    import torch

    from . import upkeep

    ck, t = cfg["ckpt"], cfg["train"]
    upkeep.ckpt_setup(ck, argv=argv)
    upkeep.ckpt_opt({**ck, "run": {k: v for k, v in cfg.items() if k != "ckpt"}})
    for split, freq in (("val", cfg["val"]["val_freq"]), ("test", cfg["test"]["test_freq"])):
        logger.info("%s: not run (accepted for the reference's command line: cache %s, every %s epochs)", split, cfg[split]["cache_dict_filepath"], freq)
    if len(cfg["runtime"]["device_id"]) > 1:
        logger.info("one device only: using cuda:%d of --runtime.device_id %s", cfg["runtime"]["device_id"][0], cfg["runtime"]["device_id"])
    device = torch.device(f"cuda:{cfg['runtime']['device_id'][0]}")
    seed = int(cfg["runtime"]["seed"])
    torch.manual_seed(seed)
    model, step_fn, context = build(device)
    params = [p for k, p in model.named_parameters() if not k.startswith("clip_model.")]
    kind = t["optimizer"]
    optimizer = make_optimizer(kind, params)
    if t["reload_ckpt_optimizer_filepath"]:
        logger.info("optimizer reload ckpt: %s", t["reload_ckpt_optimizer_filepath"])
        optimizer.load_state_dict(torch.load(t["reload_ckpt_optimizer_filepath"], map_location="cpu"))
    start, num_epoch = int(t["start_epoch"]), info["num_epoch"]
    ms, gamma = list(t["scheduler_milestone"]), float(t["scheduler_gamma"])
    for group in optimizer.param_groups:  # the schedule is a function of the epoch, whatever a reloaded optimizer file carries
        group["lr"] = lr_at(start, ms, gamma)
        group.pop("initial_lr", None)
    scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=[m - start for m in ms if m > start], gamma=gamma)
    bs, spe = info["batch_size"], info["steps_per_epoch"]
    logger.info("train_dataset: length %d | %d steps per epoch | optimizer %s", len(dataset), spe, kind)
    for epoch in range(start, num_epoch):
        np.random.seed(seed + epoch)  # (the Gaussian perturbation and the timestep sampler draw from np.random, as the reference)
        gen = torch.Generator().manual_seed(seed + epoch)
        order = torch.randperm(len(dataset), generator=gen).tolist()
        out = None
        for s in range(spe):
            idx = order[s * bs:(s + 1) * bs]
            out = run_batch(step_fn, context, [dataset[i] for i in idx], idx, epoch * spe + s, gen, device)
            optimizer_step(kind, optimizer)
        scheduler.step()
        logger.info("train epoch %04d conclude | loss: %f", epoch, float(out["loss"]))
        logger.info("train epoch %04d lr %s", epoch, [g["lr"] for g in optimizer.param_groups])
        logger.info("train epoch %04d detail loss:", epoch)
        for name, value in out.items():
            if name != "loss":
                logger.info("                     %s: %f", name.ljust(20), float(value))
        if ck["commit"] and epoch in info["record_epochs"]:
            save = os.path.join(ck["ckpt_path"], "save")
            os.makedirs(save, exist_ok=True)
            torch.save({k: v.detach().cpu() for k, v in model.state_dict().items() if not k.startswith("clip_model.")},
                       os.path.join(save, f"model_{epoch:0>4}.pt"))
            torch.save(optimizer.state_dict(), os.path.join(save, f"optimizer_{epoch:0>4}.pt"))
    torch.cuda.synchronize(device)
    model.refresh_hip_weights()  # (before anything inference-side reads the weights)
    if hasattr(optimizer, "close"):
        optimizer.close()
    step_fn.close()
    if hasattr(model, "close"):
        model.close()
    return 0


def main_common(argv, prog: str, parse: Callable, datasets: Callable, build_factory: Callable, run_batch: Callable, logger: logging.Logger) -> int:
    """parse(argv) -> cfg; datasets(cfg) -> (dataset, dry-run extras); build_factory(cfg, dataset) -> build(device)"""
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    argv = sys.argv[1:] if argv is None else list(argv)
    cfg = parse(argv)
    np.random.seed(int(cfg["runtime"]["seed"]))
    dataset, extra = datasets(cfg)
    info = plan(cfg, len(dataset), extra)
    if cfg["dry_run"]:
        print(json.dumps(info))
        return 0
    return train_loop(cfg, argv, info, prog, dataset, build_factory(cfg, dataset), run_batch, logger)


__all__ = ["parse_args", "base_dataset", "lr_at", "plan", "positive_coefs", "load_loss", "pen_on", "sdf_grid_set", "PEN_COEF", "pad_points", "collate", "make_optimizer", "optimizer_step",
           "train_loop", "main_common", "_Concat", "BASE_LR", "CLIP_MAX_NORM"]
