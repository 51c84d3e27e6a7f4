"""Train the refiner R (SegmentRefineModel) on MI355X (reference launch/train_refine.py, script/train_refine.sh): its checkpoints are
what `script/sample_refine.sh` loads as they are.

    python -m oakink2_tamf_amd.launch.train_refine --cfg config/obj_embedding.yml --cfg config/obj_pointcloud.yml --cfg config/arch_refine.yml \
        --train.cache_dict_filepath common/save_cache_dict/main/cache/train.pkl \
        --train.data.pose_repr_sample_dir_list common/sample/main/sample/train/arch_mdm_l__0099 --train.data.gaussian_perturb_range 0.02,0.1 \
        --train.loss.coef_rec_joint_loss 1.0 --train.loss.coef_rec_vert_loss 1.0 --train.loss.coef_dist_h_loss 0.1 \
        --mano.factory oakink2_tamf_amd.mano:make_mano_differentiable --mano.mano_path asset/mano_npz --exp_id "refine__?(ts)" --commit

The reference's argument names (`--train.*`, `--train.data.*`, `--train.loss.*` of launch/param/loss_refine.py, `--val.*`, `--test.*`,
`--data.*`, `--model.*`, `--runtime.*`, `--exp_id`, `--commit`) plus this build's `--mano.factory` / `--mano.mano_path` (as
launch/sample_refine.py; the layers must be differentiable), `--train.optimizer hip|torch`, `--train.start_epoch`, `--dry_run` and
this build's own loss term `--train.loss.coef_pen_loss C --data.obj_sdf_prefix DIR` (as launch/train.py).
The loop, the optimiser and the checkpoints: launch/_train_common.py.

The training set is the reference's (train_refine.py:367-373): GeneratedPoseReprSampleAdaptor (the G stage's samples of the train
cache) + GuassianPerturbSampleAdaptor, concatenated.  A batch is the reference's step train_refine.py:546-550 as
SegmentRefineTrainStep.loss_and_grads, with `obj_points` from the dataset's `obj_pointcloud`.  Validation and test are not run (the
reference's are logging only)."""
from __future__ import annotations

import logging
import sys
from typing import Dict, List

from . import _train_common as C
from .sample_refine import MODEL_DEFAULTS

_logger = logging.getLogger("oakink2_tamf_amd.launch.train_refine")
PROG = "train_refine"
LOSS_COEFS = ("coef_rec_joint_loss", "coef_rec_vert_loss", "coef_dist_h_loss")  # launch/param/loss_refine.py
OWN_COEFS = (C.PEN_COEF,)  # this build's own term
FIELDS = ("mask", "pose_repr", "shape", "obj_traj", "obj_embedding", "sample_pose_repr")  # the float part of the `select` of train_refine.py:536-541
EXTRA_DEFAULTS = {"train.data.pose_repr_sample_dir_list": [], "train.data.gaussian_perturb_range": [0.02, 0.1],
                  "val.data.pose_repr_sample_dir_list": [], "test.data.pose_repr_sample_dir_list": []}


def parse_args(argv: List[str]) -> Dict:
    return C.parse_args(argv, PROG, MODEL_DEFAULTS, LOSS_COEFS, EXTRA_DEFAULTS, "refine__?(ts)", OWN_COEFS)


def datasets(cfg: Dict):
    import os

    from ..dataset.pose_repr_sample import GeneratedPoseReprSampleAdaptor, GuassianPerturbSampleAdaptor

    if not cfg["data"]["obj_pointcloud_prefix"]:
        raise SystemExit("--data.obj_pointcloud_prefix (config/obj_pointcloud.yml) is required: the refiner's distance feature reads the point clouds")
    base = C.base_dataset(cfg)
    td = cfg["train"]["data"]
    missing = [p for p in td["pose_repr_sample_dir_list"] if not os.path.isdir(p)]
    if missing or not td["pose_repr_sample_dir_list"]:
        raise SystemExit(f"G-stage sample directory not found: {missing[0] if missing else '(none given)'}; pass --train.data.pose_repr_sample_dir_list "
                         "(run launch.sample over the train cache with --commit first)")
    parts = [GeneratedPoseReprSampleAdaptor(base, td["pose_repr_sample_dir_list"]), GuassianPerturbSampleAdaptor(base, td["gaussian_perturb_range"])]
    ds = C._Concat(parts)
    ds.frames = int(base.slice_max_len)
    ds.sdf_grids, no_sdf = C.sdf_grid_set(cfg, base, upload=False)  # (checked before anything touches the GPU; build() uploads the set)
    pen = {"n_objects_without_sdf": len(no_sdf)} if C.pen_on(cfg) else {}
    if no_sdf:
        _logger.info("pen: %d of the cache's objects have no file under --data.obj_sdf_prefix and contribute nothing", len(no_sdf))
    return ds, {**pen, "frames": ds.frames, "train_generated": len(parts[0]), "train_gaussian_perturb": len(parts[1])}


def build_factory(cfg: Dict, dataset):
    def build(device):
        import torch

        from ..model.segment_refine_model import SegmentRefineModel
        from ..model.segment_refine_train import SegmentRefineTrainStep

        t = cfg["train"]
        model = SegmentRefineModel(cfg["mano"].get("mano_path"), **{k: cfg["model"][k] for k in MODEL_DEFAULTS}, use_pc=True)
        if t["reload_ckpt_model_filepath"]:
            _logger.info("model reload ckpt: %s", t["reload_ckpt_model_filepath"])
            missing, unexpected = model.load_state_dict(torch.load(t["reload_ckpt_model_filepath"], map_location="cpu"), strict=False)
            _logger.info("model reload ckpt missing_key_list: %s unexpected_key_list: %s", missing, unexpected)
        model = model.to(device)
        step_fn = SegmentRefineTrainStep(model, int(t["batch_size"]), dataset.frames, seed=int(cfg["runtime"]["seed"]))
        grids = dataset.sdf_grids.upload(device) if dataset.sdf_grids is not None else None
        return model, step_fn, {"loss": C.load_loss(cfg, device, LOSS_COEFS + OWN_COEFS, grids), "grid_index": None if grids is None else grids.index_of}

    return build


def run_batch(step_fn, context, items, idx, step, gen, device) -> Dict:
    batch = C.collate(items, device, FIELDS, True, context["grid_index"])
    obj_points = batch.pop("obj_points")
    res = step_fn.loss_and_grads(batch, context["loss"], obj_points, obj_num=batch["obj_num"], clip_ids=idx, step=step)
    return {k: res[k] for k in ("loss", "rec_joint", "rec_vert", "dist_h", "pen") if k in res}


def main(argv=None) -> int:
    return C.main_common(argv, PROG, parse_args, datasets, build_factory, run_batch, _logger)


if __name__ == "__main__":
    sys.exit(main())
