"""Train the denoiser G (InterationSegmentMDM) on MI355X (reference launch/train.py, script/train.sh): its checkpoints are what
`script/sample.sh` loads as they are.

    python -m oakink2_tamf_amd.launch.train --cfg config/data_reverse_segment.yml --cfg config/obj_embedding.yml \
        --cfg config/obj_pointcloud.yml --cfg config/arch_mdm_l.yml --train.cache_dict_filepath common/save_cache_dict/main/cache/train.pkl \
        --data.text_embedding_filepath common/text_embedding/train.pkl --train.loss.coef_rec_joint_loss 1.0 ... \
        --mano.factory oakink2_tamf_amd.mano:make_mano_differentiable --mano.mano_path asset/mano_npz --exp_id "main__?(ts)" --commit

The reference's argument names (`--train.*`, `--train.loss.*` of launch/param/loss.py, `--val.*`, `--test.*`, `--data.*`, `--model.*`,
`--runtime.*`, `--exp_id`, `--commit`) plus this build's `--data.text_embedding_filepath` (the prompt table script/embed_text.sh writes:
the CLIP tower is not run inside the loop), `--mano.factory` / `--mano.mano_path` (as launch/sample_refine.py), `--train.optimizer
hip|torch`, `--train.start_epoch`, `--dry_run` and this build's own loss term `--train.loss.coef_pen_loss C --data.obj_sdf_prefix DIR`
(the excess penetration depth of model/interaction_loss.py, from the DIR/<obj_id>.pkl that script/process_object_sdf.sh writes; an object
without a file contributes nothing).  The loop, the optimiser and the checkpoints: launch/_train_common.py.

A batch: InteractionSegmentData items of the train cache collated by interaction_segment_collate, `text_embedding` looked up per item,
then the reference's step launch/train.py:518-529 as InterationSegmentMDMTrainStep.loss_and_grads - uniform timesteps, q_sample, HIP
forward, the masked MSE, HandInteractionLoss as the callback when any --train.loss.coef_* is positive (else none, and no MANO is
needed), HIP backward.  Validation and test are not run (the reference's validation samples 1000 steps and discards the result)."""
from __future__ import annotations

import logging
import sys
from typing import Dict, List

import numpy as np

from . import _train_common as C
from .sample import MODEL_DEFAULTS, load_text_embeddings

_logger = logging.getLogger("oakink2_tamf_amd.launch.train")
PROG = "train"
LOSS_COEFS = ("coef_rec_joint_loss", "coef_rec_vert_loss", "coef_edge_len_loss", "coef_dist_h_loss", "coef_dist_o_loss")  # launch/param/loss.py
OWN_COEFS = (C.PEN_COEF,)  # this build's own term
DIST_COEFS = ("coef_dist_h_loss", "coef_dist_o_loss")
FIELDS = ("mask", "pose_repr", "shape", "obj_traj", "obj_embedding")  # the float part of the `select` of launch/train.py:509-514
EXTRA_DEFAULTS = {"data.text_embedding_filepath": None}


def parse_args(argv: List[str]) -> Dict:
    return C.parse_args(argv, PROG, MODEL_DEFAULTS, LOSS_COEFS, EXTRA_DEFAULTS, "main__?(ts)", OWN_COEFS)


def datasets(cfg: Dict):
    ds = C.base_dataset(cfg, reverse=cfg["data"]["append_reverse_segment"])
    path = cfg["data"]["text_embedding_filepath"]
    if not path:
        raise SystemExit("--data.text_embedding_filepath is required: the table of prompt embeddings that script/embed_text.sh writes")
    table = load_text_embeddings(path)
    missing = sorted(set(ds.texts()) - set(table))
    if missing:
        raise SystemExit(f"--data.text_embedding_filepath lacks {len(missing)} of the cache's prompts, e.g. {missing[0]!r}")
    ds.text_table = table
    ds.sdf_grids, no_sdf = C.sdf_grid_set(cfg, ds, upload=False)  # (checked before anything touches the GPU; build() uploads the set)
    pen = {"n_objects_without_sdf": len(no_sdf)} if C.pen_on(cfg) else {}
    if no_sdf:
        _logger.info("pen: %d of the cache's objects have no file under --data.obj_sdf_prefix and contribute nothing", len(no_sdf))
    return ds, {**pen, "frames": int(ds.slice_max_len), "prompts": len(set(ds.texts())), "append_reverse_segment": bool(cfg["data"]["append_reverse_segment"]),
                "extra_loss": sorted(C.positive_coefs(cfg))}


def build_factory(cfg: Dict, dataset):
    def build(device):
        import torch

        from ..model.diffusion_util import create_gaussian_diffusion
        from ..model.interaction_segment_mdm import InterationSegmentMDM
        from ..model.interaction_segment_mdm_train import InterationSegmentMDMTrainStep

        t = cfg["train"]
        model = InterationSegmentMDM(**cfg["model"])
        if t["reload_ckpt_model_filepath"]:
            _logger.info("model reload ckpt: %s", t["reload_ckpt_model_filepath"])
            missing, unexpected = model.load_state_dict(torch.load(t["reload_ckpt_model_filepath"], map_location="cpu"), strict=False)
            _logger.info("model reload ckpt missing_key_list: %s unexpected_key_list: %s", [k for k in missing if not k.startswith("clip_model")], unexpected)
        model = model.to(device)
        step_fn = InterationSegmentMDMTrainStep(model, int(t["batch_size"]), int(dataset.slice_max_len), seed=int(cfg["runtime"]["seed"]))
        grids = dataset.sdf_grids.upload(device) if dataset.sdf_grids is not None else None
        crit = C.load_loss(cfg, device, LOSS_COEFS + OWN_COEFS, grids) if C.positive_coefs(cfg) else None
        context = {"diffusion": create_gaussian_diffusion(1000, "cosine"), "loss": crit, "table": dataset.text_table,
                   "points": any(c in C.positive_coefs(cfg) for c in DIST_COEFS), "grid_index": None if grids is None else grids.index_of}
        return model, step_fn, context

    return build


def run_batch(step_fn, context, items, idx, step, gen, device) -> Dict:
    import torch

    batch = C.collate(items, device, FIELDS, context["points"], context["grid_index"])
    batch["text_embedding"] = torch.from_numpy(np.stack([context["table"][it["text"]] for it in items])).to(device)
    B, T, F = batch["pose_repr"].shape
    noise = torch.randn(B, F, 1, T, generator=gen)
    res = step_fn.loss_and_grads(context["diffusion"], batch, context["loss"], noise=noise, obj_num=batch["obj_num"], clip_ids=idx, step=step)
    out = {"loss": res["loss"], "diffusion_loss": res["diffusion_loss"]}
    out.update({k: v for k, v in res.get("extra", {}).items() if k != "loss"})
    return out


def main(argv=None) -> int:
    return C.main_common(argv, PROG, parse_args, datasets, build_factory, run_batch, _logger)


if __name__ == "__main__":
    sys.exit(main())
