"""Contact Ratio of refined motions on MI355X (reference script/compute_score/compute_score_cr.py:152-289).

    python -m oakink2_tamf_amd.launch.compute_score_cr --data.process_range "?(file:./asset/split/test.txt)" \
        --data.cache_dict_filepath common/save_cache_dict/main/cache/test.pkl \
        --debug.sample_refine_filepath common/sample_refine/main/sample/test/arch_mdm_l__0399 --mano.factory pkg.mod:make_mano \
        [--batch_size 64] [--device cuda:0] [--out_json cr.json] [--save_dir DIR] [--dry_run]

The reference's argument names and defaults (`--data.*`, `--debug.sample_refine_filepath`, `--mano.mano_path`), plus `--mano.factory`
(the contract of launch/sample_refine.py), `--batch_size`, `--device`, `--out_json`, `--save_dir` and `--dry_run` of this build.  Clips
come from the segment cache; a clip whose `info` was seen before is skipped, and so is a clip without a `save_dict.pkl` under
--debug.sample_refine_filepath.  Ground-truth hand vertices: HIP pose decode -> MANO -> + tsl (launch/_score_common.py); refined hand
vertices: the save dict's `verts`.  Both against the clip's object point clouds moved along `obj_traj`, first `len` frames
(metrics/contact.py -> tamf_contact_min_dist); a frame is in contact below 5 mm.  `--save_dir DIR` writes gt_contact_dist.npy and
refined_contact_dist.npy there (the reference always writes them under ./tmp/compute_score/contact_ratio)."""
from __future__ import annotations

import json
import logging
import os
import sys

import numpy as np

from . import _score_common as C
from . import formats

_logger = logging.getLogger("oakink2_tamf_amd.launch.compute_score_cr")
PROG = "compute_score_cr"


def parse_args(argv):
    ap = C.make_parser(PROG)
    ap.add_argument("--save_dir", default=None, help="write gt_contact_dist.npy / refined_contact_dist.npy here")
    a = ap.parse_args(argv)
    cfg = C.build_config(a)
    cfg["runtime"]["save_dir"] = a.save_dir
    return cfg


def main(argv=None) -> int:
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    cfg = parse_args(sys.argv[1:] if argv is None else argv)
    rt = cfg["runtime"]
    pairs = C.load_pairs(cfg)
    _logger.info("clips with a refined sample: %d", len(pairs))
    if rt["dry_run"]:
        print(json.dumps({"n_clips": len(pairs), "pairs": C.pair_listing(pairs),
                          "sample_refine_filepath": cfg["debug"]["sample_refine_filepath"]}))
        return 0
    import torch

    device = torch.device(rt["device"])
    mano = C.load_mano(cfg, device)
    if not pairs:
        raise SystemExit(f"no clip with a refined sample under {cfg['debug']['sample_refine_filepath']}")
    torch.cuda.set_device(device)
    from ..metrics.contact import THRESHOLD, contact_distances, contact_ratio_of

    items = [p[0] for p in pairs]
    _, gt_verts = C.ground_truth_mano(items, mano, device, rt["batch_size"])
    refined_verts = [np.asarray(formats.read_refine_sample(p[1])["verts"], dtype=np.float32) for p in pairs]
    gt_dist = contact_distances(items, gt_verts, rt["batch_size"], device)
    refined_dist = contact_distances(items, refined_verts, rt["batch_size"], device)
    res = {"n_clips": len(pairs), "n_frames": int(gt_dist.shape[0]), "threshold": THRESHOLD,
           "gt_contact_ratio": contact_ratio_of(gt_dist), "refined_contact_ratio": contact_ratio_of(refined_dist)}
    print(f"n_frames {res['n_frames']}")
    print(f"gt_contact_ratio {res['gt_contact_ratio']!r}")
    print(f"refined_contact_ratio {res['refined_contact_ratio']!r}")
    if rt["save_dir"]:
        os.makedirs(rt["save_dir"], exist_ok=True)
        np.save(os.path.join(rt["save_dir"], "gt_contact_dist.npy"), gt_dist)
        np.save(os.path.join(rt["save_dir"], "refined_contact_dist.npy"), refined_dist)
    if rt["out_json"]:
        C.write_json(rt["out_json"], res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
