"""Solid Intersection Volume of refined motions on MI355X (reference script/compute_score/compute_score_siv.py:158-306).

    python -m oakink2_tamf_amd.launch.compute_score_siv --data.process_range "?(file:./asset/split/test.txt)" \
        --data.cache_dict_filepath common/save_cache_dict/main/cache/test.pkl \
        --debug.sample_refine_filepath common/sample_refine/main/sample/test/arch_mdm_l__0399 --mano.factory pkg.mod:make_mano \
        --data.obj_model_loader pkg.mod:load_obj [--data.obj_sdf_prefix DIR] [--batch_size 64] [--device cuda:0] [--out_json siv.json]
        [--save_dir DIR] [--dry_run]   (or --data.obj_mesh_prefix DIR in place of --data.obj_model_loader)

The reference's argument names and defaults, plus those of compute_score_cr.py of this build and three of its own:
  --data.obj_model_loader module:function   function(obj_id) -> (verts, faces) of the object's closed mesh (the OakInk2 toolkit that the
                                            reference's dataset loads meshes with does not ship); required unless every object of the
                                            clips has a pickle under --data.obj_sdf_prefix
  --data.obj_mesh_prefix DIR                the built-in loader in its place: mesh_io.directory_loader(DIR), DIR/<obj_id>.{obj,ply,stl} or the
                                            single mesh file in DIR/<obj_id>/ (giving both flags is refused).  The result then also holds
                                            `n_objects_open`: the objects whose mesh_report is not closed - the inside test presumes a
                                            closed mesh, so their SIV rests on a presumption that does not hold
  --data.obj_sdf_prefix DIR                 DIR/<obj_id>.pkl, a voxel set written by the reference (sdf_util.load_sdf_data's format),
                                            takes the place of the native lattice of that object
Clips and hands as in compute_score_cr.py; the closed hand faces are the 3rd / 4th element of the --mano.factory tuple.  Every object is
voxelised once (metrics/siv.py: a 100^3 lattice, the reference's check_mesh_contains as the inside test - pysdf, whose sign the reference
uses, does not ship; the two agree away from the surface).  Every 20th frame of the first `len` frames of a clip is scored, ground truth
and refined, in one kernel launch per clip.  An object without mesh and pickle is left out, as the reference's
`if obj_id not in obj_sdf_map: continue` does, and counted in `n_objects_skipped`.  `--save_dir DIR` writes gt.npy / refined.npy there
(the reference always writes them under ./tmp/compute_score/solid_intersection_volume)."""
from __future__ import annotations

import importlib
import json
import logging
import os
import pickle
import sys

import numpy as np

from . import _score_common as C
from . import formats

_logger = logging.getLogger("oakink2_tamf_amd.launch.compute_score_siv")
PROG = "compute_score_siv"


def parse_args(argv):
    ap = C.make_parser(PROG)
    ap.add_argument("--data.obj_model_loader", dest="data__obj_model_loader", default=None,
                    help="module:function, function(obj_id) -> (verts, faces)")
    add_mesh_prefix_argument(ap)
    ap.add_argument("--data.obj_sdf_prefix", dest="data__obj_sdf_prefix", default=None, help="DIR/<obj_id>.pkl overrides the native lattice")
    ap.add_argument("--save_dir", default=None, help="write gt.npy / refined.npy here")
    ap.add_argument("--data.obj_sign", dest="data__obj_sign", choices=("parity", "winding"), default=None,
                    help="the inside test of the OBJECTS' voxel sets: the reference's ray parity (the default; presumes a closed mesh) or the generalized "
                         "winding number; the hand's containment test is the reference's either way")
    a = ap.parse_args(argv)
    cfg = C.build_config(a)
    if a.data__obj_sign is not None:  # (present only when the flag is given, so a run without it is configured exactly as before)
        cfg["data"]["obj_sign"] = a.data__obj_sign
    cfg["data"]["obj_model_loader"] = a.data__obj_model_loader
    set_mesh_prefix(ap, a, cfg)
    cfg["data"]["obj_sdf_prefix"] = os.path.abspath(a.data__obj_sdf_prefix) if a.data__obj_sdf_prefix else None
    cfg["runtime"]["save_dir"] = a.save_dir
    return cfg


def resolve_loader(spec):
    if not spec:
        return None
    if ":" not in str(spec):
        raise SystemExit("--data.obj_model_loader takes module:function, function(obj_id) -> (verts, faces)")
    mod, fn = str(spec).split(":", 1)
    return getattr(importlib.import_module(mod), fn)


def add_mesh_prefix_argument(ap) -> None:
    ap.add_argument("--data.obj_mesh_prefix", dest="data__obj_mesh_prefix", default=None,
                    help="DIR/<obj_id>.{obj,ply,stl} or DIR/<obj_id>/<one mesh file>: the built-in mesh loader (not with --data.obj_model_loader)")


def set_mesh_prefix(ap, a, cfg) -> None:
    """cfg["data"]["obj_mesh_prefix"]: present only when the flag is given, so a run without it is configured exactly as before"""
    if a.data__obj_mesh_prefix is None:
        return
    if a.data__obj_model_loader is not None:
        ap.error("--data.obj_mesh_prefix and --data.obj_model_loader both name the source of the object meshes: give one")
    cfg["data"]["obj_mesh_prefix"] = os.path.abspath(a.data__obj_mesh_prefix)


def mesh_loader(cfg):
    """the obj_model_loader of a run: --data.obj_model_loader's function, or mesh_io.directory_loader of --data.obj_mesh_prefix"""
    prefix = cfg["data"].get("obj_mesh_prefix")
    if prefix is None:
        return resolve_loader(cfg["data"]["obj_model_loader"])
    from ..mesh_io import directory_loader

    if not os.path.isdir(prefix):
        raise SystemExit(f"--data.obj_mesh_prefix: {prefix} is no directory")
    load = directory_loader(prefix)

    def checked(obj_id):
        try:
            return load(obj_id)
        except ValueError as e:  # no file, several candidates, or a file that is no mesh: named, not a traceback
            raise SystemExit(f"--data.obj_mesh_prefix: {e}")

    return checked


def sdf_pickle_path(cfg, obj_id):
    prefix = cfg["data"].get("obj_sdf_prefix")
    path = os.path.join(prefix, f"{obj_id}.pkl") if prefix else None
    return path if path and os.path.exists(path) else None


def main(argv=None) -> int:
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    cfg = parse_args(sys.argv[1:] if argv is None else argv)
    rt = cfg["runtime"]
    loader = mesh_loader(cfg)
    mesh_prefix = cfg["data"].get("obj_mesh_prefix")
    pairs = C.load_pairs(cfg, obj_model_loader=loader)
    _logger.info("clips with a refined sample: %d", len(pairs))
    if rt["dry_run"]:
        print(json.dumps({"n_clips": len(pairs), "pairs": C.pair_listing(pairs),
                          "sample_refine_filepath": cfg["debug"]["sample_refine_filepath"],
                          "obj_model_loader": cfg["data"]["obj_model_loader"], "obj_sdf_prefix": cfg["data"]["obj_sdf_prefix"],
                          "obj_sign": cfg["data"].get("obj_sign", "parity"), **({"obj_mesh_prefix": mesh_prefix} if mesh_prefix else {})}))
        return 0
    import torch

    device = torch.device(rt["device"])
    mano = C.load_mano(cfg, device)
    if not pairs:
        raise SystemExit(f"no clip with a refined sample under {cfg['debug']['sample_refine_filepath']}")
    items = [p[0] for p in pairs]
    obj_ids = list(dict.fromkeys(o for it in items for o in it["obj_list"]))
    if loader is None and any(sdf_pickle_path(cfg, o) is None for o in obj_ids):
        raise SystemExit("the SIV score needs the objects' meshes: pass --data.obj_model_loader module:function returning (verts, faces) "
                         "per object id (or --data.obj_mesh_prefix DIR of mesh files), or a pickle per object under --data.obj_sdf_prefix")
    torch.cuda.set_device(device)
    from ..metrics.siv import clip_siv, load_sdf_pickle, object_lattice
    from ..winding import WindingError

    obj_sign = cfg["data"].get("obj_sign", "parity")

    faces_closed = {"rh": np.asarray(mano[2]), "lh": np.asarray(mano[3])}
    _, gt_verts = C.ground_truth_mano(items, mano, device, rt["batch_size"])
    lattice_map, skipped, open_objects = {}, [], []
    gt_siv, refined_siv = [], []
    for (item, path), gt_hv in zip(pairs, gt_verts):
        if len(set(item["obj_list"])) != len(item["obj_list"]):  # (the dataset's obj_list is the sorted key set of the clip's trajectories)
            raise ValueError(f"clip {item['info']}: an object id occurs twice in obj_list")
        refined_hv = np.asarray(formats.read_refine_sample(path)["verts"], dtype=np.float32)
        for k, obj_id in enumerate(item["obj_list"]):
            if obj_id in lattice_map:
                continue
            pkl = sdf_pickle_path(cfg, obj_id)
            try:
                if pkl is not None:
                    lattice_map[obj_id] = load_sdf_pickle(pkl)
                elif "obj_verts" in item:
                    lattice_map[obj_id] = object_lattice(item["obj_verts"][k], item["obj_faces"][k], device=device, sign=obj_sign)
                else:
                    lattice_map[obj_id] = None
            except (ValueError, IndexError, AssertionError, KeyError, pickle.UnpicklingError, WindingError) as e:
                # what a bad mesh or pickle raises in the host half (wrong shapes, face indices outside the vertices, no faces, missing
                # fields): the object is left out.  Library, build and HIP errors (TamfError, TamfBuildError) are not caught.
                _logger.info("object %s: no lattice (%s)", obj_id, e)
                lattice_map[obj_id] = None
            if lattice_map[obj_id] is None:
                skipped.append(obj_id)
            elif mesh_prefix and pkl is None:
                from ..mesh_io import mesh_report

                rep = mesh_report(item["obj_verts"][k], item["obj_faces"][k])
                if not rep["closed"]:
                    open_objects.append(obj_id)
                    _logger.info("object %s: the mesh is not closed (%d boundary edges, %d non-manifold edges): its SIV rests on "
                                 + ("the winding number's inside test (|w| > 0.5)" if obj_sign == "winding" else "an inside test that presumes a closed mesh"),
                                 obj_id, rep["n_boundary_edges"], rep["n_nonmanifold_edges"])
        g, r = clip_siv(gt_hv, refined_hv, faces_closed[item["hand_side"]], item["obj_traj"], [lattice_map[o] for o in item["obj_list"]],
                        int(item["len"]), device=device)
        gt_siv.extend(g)
        refined_siv.extend(r)
    if not gt_siv:
        raise SystemExit("no frame to score: every clip with a refined sample has len 0")
    res = {"n_clips": len(pairs), "n_frames": len(gt_siv), "n_objects": len(lattice_map), "n_objects_skipped": len(skipped),
           "objects_skipped": skipped, "gt_siv": float(np.mean(gt_siv)), "refined_siv": float(np.mean(refined_siv)), "obj_sign": obj_sign}
    if mesh_prefix:
        res.update(n_objects_open=len(open_objects), objects_open=open_objects)
    print(f"n_frames {res['n_frames']}")
    print(f"n_objects_skipped {res['n_objects_skipped']}")
    print(f"gt_siv {res['gt_siv']!r}")
    print(f"refined_siv {res['refined_siv']!r}")
    print(f"obj_sign {res['obj_sign']}")
    if rt["save_dir"]:
        os.makedirs(rt["save_dir"], exist_ok=True)
        np.save(os.path.join(rt["save_dir"], "gt.npy"), gt_siv)
        np.save(os.path.join(rt["save_dir"], "refined.npy"), refined_siv)
    if rt["out_json"]:
        C.write_json(rt["out_json"], res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
