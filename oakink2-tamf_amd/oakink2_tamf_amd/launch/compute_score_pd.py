"""Penetration depth of refined motions on MI355X: how deep the hand goes into the objects, beside compute_score_siv's how much volume.
The reference has no such script; the definition is metrics/pd.py's.

    python -m oakink2_tamf_amd.launch.compute_score_pd --data.process_range "?(file:./asset/split/test.txt)" \
        --data.cache_dict_filepath common/save_cache_dict/main/cache/test.pkl \
        --debug.sample_refine_filepath common/sample_refine/main/sample/test/arch_mdm_l__0399 --mano.factory pkg.mod:make_mano \
        --data.obj_model_loader pkg.mod:load_obj [--stride 20] [--batch_size 64] [--device cuda:0] [--out_json pd.json] [--save_dir DIR]
        [--sign parity|winding] [--dry_run]   (or --data.obj_mesh_prefix DIR in place of --data.obj_model_loader)

The argument names of compute_score_siv.py, and `--stride` (every stride-th frame of the first `len` frames of a clip is scored: 20, the
frames SIV scores).  Clips and hands as in compute_score_cr.py.  Every hand vertex of a scored frame, ground truth and refined, is taken
into each object's frame and measured against the object's mesh with the exact point-to-mesh distance (include/tamf_meshdist.h); a
frame's depth is the largest distance among the vertices inside an object (the inside test of SIV), 0 when none is.  One kernel launch
per clip.  Printed and written with --out_json:
    n_clips, n_frames, n_objects, n_objects_skipped          an object without a mesh is left out and counted, as SIV does
    gt_pd, refined_pd                                        mean depth over the frames, cm
    gt_pd_max, refined_pd_max                                the deepest frame, cm
    gt_pen_frame_ratio, refined_pen_frame_ratio              the share of frames with any vertex inside an object
    n_objects_open (with --data.obj_mesh_prefix)             objects whose mesh is not closed: the default inside test presumes a closed mesh
    sign                                                     the inside test used
`--sign winding` takes `inside` from the generalized winding number (|w| > 0.5, include/tamf_winding.h) on the same vertices and
transforms: it needs no closed mesh and equals the default on a clean closed one.  The distance is the same either way.
`--save_dir DIR` writes the per-frame depths gt.npy / refined.npy there."""
from __future__ import annotations

import json
import logging
import os
import sys

import numpy as np

from . import _score_common as C
from . import formats
from .compute_score_siv import add_mesh_prefix_argument, mesh_loader, set_mesh_prefix

_logger = logging.getLogger("oakink2_tamf_amd.launch.compute_score_pd")
PROG = "compute_score_pd"
NO_MESH_SOURCE = ("the PD score needs the objects' meshes: pass --data.obj_model_loader module:function returning (verts, faces) per object id, "
                  "or --data.obj_mesh_prefix DIR of mesh files")


def parse_args(argv):
    ap = C.make_parser(PROG)
    ap.add_argument("--data.obj_model_loader", dest="data__obj_model_loader", default=None, help="module:function, function(obj_id) -> (verts, faces)")
    add_mesh_prefix_argument(ap)
    ap.add_argument("--stride", type=int, default=20, help="every stride-th frame is scored (20: the frames SIV scores)")
    ap.add_argument("--save_dir", default=None, help="write gt.npy / refined.npy here")
    ap.add_argument("--sign", choices=("parity", "winding"), default=None,
                    help="which vertices count as inside an object: the reference's ray parity (the default; presumes a closed mesh) or the generalized "
                         "winding number")
    a = ap.parse_args(argv)
    if a.stride < 1:
        ap.error("--stride must be at least 1")
    cfg = C.build_config(a)
    cfg["data"]["obj_model_loader"] = a.data__obj_model_loader
    set_mesh_prefix(ap, a, cfg)
    if cfg["data"]["obj_model_loader"] is None and cfg["data"].get("obj_mesh_prefix") is None:
        ap.error(NO_MESH_SOURCE)
    cfg["runtime"]["save_dir"] = a.save_dir
    cfg["runtime"]["stride"] = a.stride
    if a.sign is not None:  # (present only when the flag is given, so a run without it is configured exactly as before)
        cfg["runtime"]["sign"] = a.sign
    return cfg


def main(argv=None) -> int:
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    cfg = parse_args(sys.argv[1:] if argv is None else argv)
    rt = cfg["runtime"]
    sign = rt.get("sign", "parity")
    loader = mesh_loader(cfg)
    mesh_prefix = cfg["data"].get("obj_mesh_prefix")
    pairs = C.load_pairs(cfg, obj_model_loader=loader)
    _logger.info("clips with a refined sample: %d", len(pairs))
    if rt["dry_run"]:
        print(json.dumps({"n_clips": len(pairs), "pairs": C.pair_listing(pairs), "sample_refine_filepath": cfg["debug"]["sample_refine_filepath"],
                          "obj_model_loader": cfg["data"]["obj_model_loader"], "stride": rt["stride"], "sign": sign,
                          **({"obj_mesh_prefix": mesh_prefix} if mesh_prefix else {})}))
        return 0
    import torch

    device = torch.device(rt["device"])
    mano = C.load_mano(cfg, device)
    if not pairs:
        raise SystemExit(f"no clip with a refined sample under {cfg['debug']['sample_refine_filepath']}")
    torch.cuda.set_device(device)
    from ..meshdist import MeshDistError, MeshSet
    from ..metrics.pd import clip_pd, summary

    items = [p[0] for p in pairs]
    _, gt_verts = C.ground_truth_mano(items, mano, device, rt["batch_size"])
    # every object once: its mesh in the set, or None (no mesh, or one the host half refuses: left out and counted)
    mesh_of, meshes, skipped, open_objects = {}, [], [], []
    for item in items:
        if len(set(item["obj_list"])) != len(item["obj_list"]):
            raise ValueError(f"clip {item['info']}: an object id occurs twice in obj_list")
        for k, obj_id in enumerate(item["obj_list"]):
            if obj_id in mesh_of:
                continue
            mesh_of[obj_id] = None
            if "obj_verts" in item:
                try:
                    MeshSet([(item["obj_verts"][k], item["obj_faces"][k])], upload=False)  # (the host checks alone)
                    mesh_of[obj_id] = len(meshes)
                    meshes.append((item["obj_verts"][k], item["obj_faces"][k]))
                except (ValueError, IndexError, MeshDistError) as e:
                    _logger.info("object %s: no mesh to measure against (%s)", obj_id, e)
            if mesh_of[obj_id] is None:
                skipped.append(obj_id)
            elif mesh_prefix:
                from ..mesh_io import mesh_report

                rep = mesh_report(item["obj_verts"][k], item["obj_faces"][k])
                if not rep["closed"]:
                    open_objects.append(obj_id)
                    _logger.info("object %s: the mesh is not closed (%d boundary edges, %d non-manifold edges): which vertices count as inside "
                                 + ("is decided by the winding number (|w| > 0.5)" if sign == "winding" else "rests on a test that presumes a closed mesh"),
                                 obj_id, rep["n_boundary_edges"], rep["n_nonmanifold_edges"])
    mesh_set = MeshSet(meshes, device=device) if meshes else None
    winding_set = None
    if sign == "winding" and meshes:
        from ..winding import WindingSet

        winding_set = WindingSet(meshes, device=device)  # (MeshSet accepted every mesh: the same validity predicate)
    gt_pd, refined_pd, gt_pen, refined_pen = [], [], [], []
    for (item, path), gt_hv in zip(pairs, gt_verts):
        refined_hv = np.asarray(formats.read_refine_sample(path)["verts"], dtype=np.float32)
        ids = [mesh_of[o] for o in item["obj_list"]] if mesh_set is not None else [None] * len(item["obj_list"])
        depth, pen = clip_pd(gt_hv, refined_hv, item["obj_traj"], mesh_set, ids, int(item["len"]), stride=rt["stride"], sign=sign,
                             winding_set=winding_set)
        gt_pd.extend(depth[0].tolist())
        refined_pd.extend(depth[1].tolist())
        gt_pen.extend(pen[0].tolist())
        refined_pen.extend(pen[1].tolist())
    if not gt_pd:
        raise SystemExit("no frame to score: every clip with a refined sample has len 0")
    res = {"n_clips": len(pairs), "n_frames": len(gt_pd), "n_objects": len(mesh_of), "n_objects_skipped": len(skipped), "objects_skipped": skipped,
           "stride": rt["stride"], "sign": sign, **summary(gt_pd, refined_pd, gt_pen, refined_pen)}
    if mesh_prefix:
        res.update(n_objects_open=len(open_objects), objects_open=open_objects)
    for key in ("n_clips", "n_frames", "n_objects", "n_objects_skipped"):
        print(f"{key} {res[key]}")
    for key in ("gt_pd", "refined_pd", "gt_pd_max", "refined_pd_max", "gt_pen_frame_ratio", "refined_pen_frame_ratio"):
        print(f"{key} {res[key]!r}")
    if mesh_prefix:
        print(f"n_objects_open {res['n_objects_open']}")
    print(f"sign {res['sign']}")
    if rt["save_dir"]:
        os.makedirs(rt["save_dir"], exist_ok=True)
        np.save(os.path.join(rt["save_dir"], "gt.npy"), gt_pd)
        np.save(os.path.join(rt["save_dir"], "refined.npy"), refined_pd)
    if rt["out_json"]:
        C.write_json(rt["out_json"], res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
