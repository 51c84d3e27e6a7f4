"""PSKL-J of refined motions on MI355X (reference script/compute_score/compute_score_psklj.py:154-317).

    python -m oakink2_tamf_amd.launch.compute_score_psklj --data.process_range "?(file:./asset/split/test.txt)" \
        --data.cache_dict_filepath common/save_cache_dict/main/cache/test.pkl \
        --debug.sample_refine_filepath common/sample_refine/main/sample/test/arch_mdm_l__0399 --mano.factory pkg.mod:make_mano \
        [--batch_size 64] [--device cuda:0] [--out_json psklj.json] [--dry_run]

The reference's argument names and defaults, plus `--mano.factory` (the contract of launch/sample_refine.py), `--batch_size`, `--device`,
`--out_json` and `--dry_run` of this build.  Clip selection as in compute_score_cr.  Ground-truth joints: HIP pose decode -> MANO ->
+ tsl; model joints: the save dict's `joints`; both with the frames from `len` on held at frame len - 1 (:270-271, done inside the
kernel).  The summed power spectra of the joint accelerations come from tamf_power_spectrum_sum (metrics/psklj.py), the two KL sums
from pskl_terms on the (T - 2, 21, 3) arrays - the reference divides by its `shape[1]`, the 21 joints.  Prints n_clips, pskl_gt_model
and pskl_model_gt (the reference's pskl_1, pskl_2)."""
from __future__ import annotations

import json
import logging
import sys

import numpy as np

from . import _score_common as C
from . import formats

_logger = logging.getLogger("oakink2_tamf_amd.launch.compute_score_psklj")
PROG = "compute_score_psklj"


def parse_args(argv):
    return C.build_config(C.make_parser(PROG).parse_args(argv))


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
    from ..metrics.psklj import power_spectrum_sum, pskl_terms

    items = [p[0] for p in pairs]
    lens = [int(it["len"]) for it in items]
    gt_joints, _ = C.ground_truth_mano(items, mano, device, rt["batch_size"])
    model_joints = [np.asarray(formats.read_refine_sample(p[1])["joints"], dtype=np.float32) for p in pairs]
    spectra = []
    for clips in (gt_joints, model_joints):
        s = power_spectrum_sum([torch.from_numpy(np.ascontiguousarray(c)) for c in clips], lens).cpu().numpy()
        spectra.append(s.reshape((s.shape[0],) + tuple(clips[0].shape[1:])))  # (T - 2, 21, 3), as the reference's np.sum(psd, axis=0)
    terms = pskl_terms(spectra[0], spectra[1])
    res = {"n_clips": len(pairs), **terms}
    print(f"n_clips {res['n_clips']}")
    print(f"pskl_gt_model {res['pskl_gt_model']!r}")
    print(f"pskl_model_gt {res['pskl_model_gt']!r}")
    if rt["out_json"]:
        C.write_json(rt["out_json"], res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
