"""Pictures of refined motions on MI355X: every clip with a refined sample rendered frame by frame, hand and objects, to PNG files.
Stands where the reference's viewers (script/viz_seg.py, script/debug/debug_refine_sample.py, script/debug/debug_train_sample.py) open
an Open3D window and dev_fn/util/vis_pyrender_util.py renders through OpenGL; a headless node has neither.

    python -m oakink2_tamf_amd.launch.render_samples --data.process_range "?(file:./asset/split/test.txt)" \
        --data.cache_dict_filepath common/save_cache_dict/main/cache/test.pkl \
        --debug.sample_refine_filepath common/sample_refine/main/sample/test/arch_mdm_l__0399 --out_dir render/test/arch_mdm_l__0399 \
        [--data.obj_model_loader pkg.mod:load_obj] [--with_gt --mano.factory pkg.mod:make_mano] [--render.width 512] [--render.height 512]
        [--render.every 1] [--render.sheet_cols 8] [--render.point_size 3] [--max_clips N] [--device cuda:0] [--out_json index.json] [--dry_run]
        [--render.contact_map [--render.contact_far_mm 30]] [--render.obj_alpha 1.0] [--render.layers K] [--render.ssaa 1]
        [--render.apng [--render.apng_fps 10]] [--render.penetration_map [--render.penetration_far_mm 10] [--render.penetration_sign parity|winding]]

The `--data.*`, `--debug.sample_refine_filepath` and `--mano.*` names of compute_score_cr.py (launch/_score_common.py), and:
  --data.obj_model_loader module:function   function(obj_id) -> (verts, faces), as compute_score_siv.py takes it: the objects are drawn
                                            as meshes; without it as the splats of their `obj_pointcloud`
  --data.obj_mesh_prefix DIR                the built-in loader in its place: mesh_io.directory_loader(DIR), DIR/<obj_id>.{obj,ply,stl} or the
                                            single mesh file in DIR/<obj_id>/ (giving both flags is refused)
  --with_gt                                 a second panel beside the refined one: the ground-truth hand (pose decode -> MANO) in a second
                                            colour with the same objects and camera; needs --mano.factory and is refused without it
  --render.contact_map                      every hand panel's vertices are coloured by their distance to the clip's objects
                                            (contact.merged_h2o_dist against `obj_pointcloud` moved along `obj_traj`): the contact colour at
                                            5 mm (the CR score's threshold) and nearer, the hand's own colour from --render.contact_far_mm
                                            (a display default) on; refused when the item carries no point cloud.  On the hand only.
  --render.penetration_map                  every hand panel's vertices that lie INSIDE an object are coloured by how deep they are: the
                                            hand's own colour at depth 0 to the penetration colour at --render.penetration_far_mm (a
                                            display default, not a measurement) and deeper; depth = the exact distance to the object's
                                            mesh (meshdist.py), inside = the test of the SIV and PD scores.  Needs the objects' meshes
                                            (refused without --data.obj_model_loader / --data.obj_mesh_prefix) and is refused together
                                            with --render.contact_map.  One MeshSet.distance call per clip.
  --render.obj_alpha A                      the objects are drawn see-through with alpha A in (0, 1]: the fingers behind them show
  --render.layers K                         depth layers peeled per pixel, 1 .. 8 (default 1, and 4 when obj_alpha < 1)
  --render.ssaa S                           S x S sub-samples a pixel, 1 .. 4 (default 1)
  --render.apng                             also clip.apng beside sheet.png: the drawn frames as one animated PNG at --render.apng_fps
                                            (default 10, the dataset's target_fps)
Per clip: the refined hand is the save dict's `verts` over its `faces` (the --mano.factory tuple's closed faces when the save dict
holds none), every object of `obj_list` moves along the item's `obj_traj`, frames 0, every, 2 every, ... of the first `len` frames are
drawn from ONE camera fitted to everything in them (render.look_at_camera).  Output under
<out_dir>/<process_key with '/' -> '++'>/<info[1]>/<info[2]>/: frame_%04d.png per drawn frame (numbered by clip frame) and sheet.png,
every sheet_cols-th drawn frame tiled sheet_cols to a row.  The image is this package's rasterisation and Lambert shading, not
pyrender's (render.py)."""
from __future__ import annotations

import json
import logging
import os
import sys

import numpy as np

from . import _score_common as C
from . import formats
from .compute_score_siv import add_mesh_prefix_argument, mesh_loader, resolve_loader, set_mesh_prefix  # noqa: F401

_logger = logging.getLogger("oakink2_tamf_amd.launch.render_samples")
PROG = "render_samples"
HAND_COLOR, GT_HAND_COLOR = (0.91, 0.72, 0.60), (0.45, 0.65, 0.90)
OBJ_COLORS = ((0.55, 0.80, 0.45), (0.90, 0.55, 0.35), (0.70, 0.55, 0.85), (0.85, 0.80, 0.40))
RENDER_DEFAULTS = {"width": 512, "height": 512, "every": 1, "sheet_cols": 8, "point_size": 3}
CONTACT_COLOR = (1.0, 0.1, 0.05)
CONTACT_NEAR = 0.005  # metres: the contact threshold of the CR score
# what draws the picture differently; kept apart from cfg["render"], which stays the five sizes above
PENETRATION_COLOR = (0.55, 0.10, 0.85)
PENETRATION_FAR_MM = 10.0  # a display default, not a measurement
DISPLAY_DEFAULTS = {"contact_map": False, "contact_far_mm": 30.0, "obj_alpha": 1.0, "layers": 1, "ssaa": 1, "apng": False, "apng_fps": 10}


def parse_args(argv):
    ap = C.make_parser(PROG)
    ap.add_argument("--data.obj_model_loader", dest="data__obj_model_loader", default=None,
                    help="module:function, function(obj_id) -> (verts, faces): draw the objects as meshes")
    add_mesh_prefix_argument(ap)
    for key, default in RENDER_DEFAULTS.items():
        ap.add_argument("--render." + key, dest="render__" + key, type=int, default=default)
    ap.add_argument("--render.contact_map", dest="display__contact_map", action="store_true", help="colour the hand by its distance to the objects")
    ap.add_argument("--render.contact_far_mm", dest="display__contact_far_mm", type=float, default=DISPLAY_DEFAULTS["contact_far_mm"])
    ap.add_argument("--render.obj_alpha", dest="display__obj_alpha", type=float, default=DISPLAY_DEFAULTS["obj_alpha"])
    ap.add_argument("--render.layers", dest="display__layers", type=int, default=None, help="peeled depth layers (default 1; 4 when obj_alpha < 1)")
    ap.add_argument("--render.ssaa", dest="display__ssaa", type=int, default=DISPLAY_DEFAULTS["ssaa"])
    ap.add_argument("--render.apng", dest="display__apng", action="store_true", help="also write clip.apng")
    ap.add_argument("--render.apng_fps", dest="display__apng_fps", type=int, default=DISPLAY_DEFAULTS["apng_fps"])
    ap.add_argument("--render.penetration_map", dest="penetration__map", action="store_true", help="colour the hand vertices inside an object by their depth")
    ap.add_argument("--render.penetration_far_mm", dest="penetration__far_mm", type=float, default=None)
    ap.add_argument("--render.penetration_sign", dest="penetration__sign", choices=("parity", "winding"), default=None,
                    help="which vertices count as inside an object: the reference's ray parity (the default; presumes a closed mesh) or the "
                         "generalized winding number")
    ap.add_argument("--out_dir", default=os.path.join("common", "render_samples", "main"))
    ap.add_argument("--max_clips", type=int, default=None, help="render the first N clips only")
    ap.add_argument("--with_gt", action="store_true", help="second panel: the ground-truth hand (needs --mano.factory)")
    a = ap.parse_args(argv)
    cfg = C.build_config(a)
    cfg["data"]["obj_model_loader"] = a.data__obj_model_loader
    set_mesh_prefix(ap, a, cfg)
    r = {key: getattr(a, "render__" + key) for key in RENDER_DEFAULTS}
    if not (1 <= r["width"] <= 4096 and 1 <= r["height"] <= 4096):
        ap.error("--render.width and --render.height must lie in [1, 4096]")
    if r["every"] < 1 or r["sheet_cols"] < 1:
        ap.error("--render.every and --render.sheet_cols must be at least 1")
    if r["point_size"] % 2 != 1 or not 1 <= r["point_size"] <= 15:
        ap.error("--render.point_size must be odd and lie in [1, 15]")
    if a.max_clips is not None and a.max_clips < 1:
        ap.error("--max_clips must be at least 1")
    if a.with_gt and not cfg["mano"]["factory"]:
        ap.error("--with_gt draws the ground-truth hand through MANO: pass --mano.factory module:function")
    d = {key: getattr(a, "display__" + key) for key in DISPLAY_DEFAULTS}
    if not 0.0 < d["obj_alpha"] <= 1.0:
        ap.error("--render.obj_alpha must lie in (0, 1]")
    if d["layers"] is None:
        d["layers"] = 4 if d["obj_alpha"] < 1.0 else 1
    if not 1 <= d["layers"] <= 8:
        ap.error("--render.layers must lie in [1, 8]")
    if not 1 <= d["ssaa"] <= 4 or d["ssaa"] * max(r["width"], r["height"]) > 4096:
        ap.error("--render.ssaa must lie in [1, 4], with ssaa * width and ssaa * height at most 4096")
    if d["ssaa"] * r["point_size"] + (1 - d["ssaa"] * r["point_size"] % 2) > 15:
        ap.error("--render.ssaa * --render.point_size (made odd) must not exceed 15")
    if not d["contact_far_mm"] > 1e3 * CONTACT_NEAR:  # (false for NaN)
        ap.error("--render.contact_far_mm must exceed the contact threshold of %g mm" % (1e3 * CONTACT_NEAR))
    if not 1 <= d["apng_fps"] <= 1000:
        ap.error("--render.apng_fps must lie in [1, 1000]")
    if a.penetration__far_mm is not None and not a.penetration__map:
        ap.error("--render.penetration_far_mm belongs to --render.penetration_map")
    if a.penetration__sign is not None and not a.penetration__map:
        ap.error("--render.penetration_sign belongs to --render.penetration_map")
    if a.penetration__map:  # cfg["penetration"]: present only when the flag is given, so a run without it is configured exactly as before
        if d["contact_map"]:
            ap.error("--render.penetration_map and --render.contact_map both colour the hand: give one")
        if a.data__obj_model_loader is None and a.data__obj_mesh_prefix is None:
            ap.error("--render.penetration_map measures the hand against the objects' meshes: pass --data.obj_model_loader module:function "
                     "or --data.obj_mesh_prefix DIR")
        far = PENETRATION_FAR_MM if a.penetration__far_mm is None else a.penetration__far_mm
        if not (far > 0.0 and np.isfinite(far)):
            ap.error("--render.penetration_far_mm must be a positive number")
        cfg["penetration"] = {"far_mm": float(far)}
        if a.penetration__sign is not None:  # (present only when given: a run without the flag is configured, and reported, exactly as before)
            cfg["penetration"]["sign"] = a.penetration__sign
    cfg["render"] = r
    cfg["display"] = d
    cfg["runtime"].update(out_dir=os.path.abspath(a.out_dir), max_clips=a.max_clips, with_gt=a.with_gt)
    return cfg


def clip_dir(out_dir: str, info) -> str:
    return os.path.join(out_dir, str(info[0]).replace("/", "++"), str(info[1]), str(info[2]))


def drawn_frames(length: int, every: int):
    return list(range(0, int(length), every))


def render_clip(item, hands, faces, cfg, device):
    """hands: [(verts (T, 778, 3), colour)], one panel each -> (frames, images (n, H, panels * W, 3) uint8 numpy)"""
    from .. import render as R

    r, d = cfg["render"], cfg["display"]
    frames = drawn_frames(item["len"], r["every"])
    if not frames:
        return frames, None
    if d["contact_map"] and "obj_pointcloud" not in item:
        raise SystemExit(f"--render.contact_map: clip {tuple(item['info'])} carries no obj_pointcloud to measure the hand against "
                         "(pass --data.obj_pointcloud_prefix)")
    poses = [R.tslrot6d_to_matrix(np.asarray(item["obj_traj"])[k]) for k in range(len(item["obj_list"]))]
    meshes = "obj_verts" in item
    shapes = [np.asarray(item["obj_verts"][k] if meshes else item["obj_pointcloud"][k], np.float64) for k in range(len(item["obj_list"]))]
    seen = [np.asarray(h, np.float64)[frames].reshape(-1, 3) for h, _ in hands]
    for m, s in zip(poses, shapes):
        seen.append((np.einsum("fij,pj->fpi", m[frames][:, :, :3], s) + m[frames][:, None, :, 3]).reshape(-1, 3))
    cam = R.look_at_camera(np.concatenate(seen), r["width"], r["height"])
    panels = []
    pen = penetration_maps(item, hands, frames, cfg["penetration"]["far_mm"], device, cfg["penetration"].get("sign", "parity")) if "penetration" in cfg else None
    for n_panel, (verts, colour) in enumerate(hands):
        rd = R.HipRenderer(r["width"], r["height"], device)
        hand = np.asarray(verts, np.float32)[frames]
        vcol = contact_map(item, hand, frames, colour, d, device) if d["contact_map"] else pen[n_panel] if pen is not None else None
        rd.add_mesh(hand, faces, color=colour, smooth=True, name="hand", vertex_colors=vcol)
        for k, (m, s) in enumerate(zip(poses, shapes)):
            colour_k = OBJ_COLORS[k % len(OBJ_COLORS)]
            if meshes:
                rd.add_mesh(s, item["obj_faces"][k], color=colour_k, pose=m[frames], name=str(item["obj_list"][k]), alpha=d["obj_alpha"])
            else:
                rd.add_points(s, color=colour_k, pose=m[frames], point_size=r["point_size"], name=str(item["obj_list"][k]), alpha=d["obj_alpha"])
        panels.append(rd.render(cam, layers=d["layers"], ssaa=d["ssaa"])[0].cpu().numpy())
    return frames, np.concatenate(panels, axis=2)


def contact_map(item, hand, frames, colour, d, device):
    """the heat map of one hand panel: hand (n, V, 3) at the drawn frames -> colours (n, V, 3) on the device, from the distance of every
    vertex to the nearest point of any of the clip's objects (contact.merged_h2o_dist, the refiner's feature)"""
    import torch

    from .. import render as R
    from ..contact import merged_h2o_dist

    nobj = len(item["obj_list"])
    traj = np.stack([np.asarray(item["obj_traj"])[k][frames] for k in range(nobj)]).astype(np.float32)  # (nobj, n, 9)
    clouds = np.stack([np.asarray(item["obj_pointcloud"][k], np.float32) for k in range(nobj)])  # (nobj, P, 3)
    with torch.no_grad():
        dist = merged_h2o_dist(torch.from_numpy(np.ascontiguousarray(hand))[None].to(device), torch.from_numpy(traj)[None].to(device),
                               torch.from_numpy(clouds)[None].to(device))[0]
    return R.contact_colors(dist, colour, hot=CONTACT_COLOR, near=CONTACT_NEAR, far=1e-3 * d["contact_far_mm"])


def penetration_depths(item, hands, frames, device, sign="parity"):
    """Per panel the depth of every hand vertex at the drawn frames: hands [(verts (T, V, 3), colour)] -> depth (panels, n, V) float64
    metres and inside (panels, n, V) bool, on the device.  A vertex's depth is its largest distance to the mesh of an object it lies
    inside (0 outside all of them); poses and their inverses as the PD score takes them (metrics/pd.py).  All frames, panels and
    objects of the clip go through ONE MeshSet.distance call; with sign="winding" `inside` comes from one WindingSet.points call on
    the same jobs (the generalized winding number, for object meshes that are not closed)."""
    import torch

    from ..meshdist import MeshSet
    from ..metrics.pd import inverse_transf
    from ..metrics.siv import tslrot6d_to_transf

    if "obj_verts" not in item:
        raise SystemExit(f"--render.penetration_map: clip {tuple(item['info'])} carries no object meshes to measure the hand against")
    nobj, n, P = len(item["obj_list"]), len(frames), len(hands)
    pts = np.ascontiguousarray(np.stack([np.asarray(v, np.float32)[frames] for v, _ in hands]))  # (P, n, V, 3)
    V = pts.shape[2]
    ms = MeshSet([(item["obj_verts"][k], item["obj_faces"][k]) for k in range(nobj)], device=device)
    inv = inverse_transf(tslrot6d_to_transf(np.asarray(item["obj_traj"])))[:, frames].astype(np.float64)  # (nobj, n, 3, 4)
    slot = np.arange(P * n, dtype=np.int64).repeat(nobj)  # (panel, frame)-major, the objects innermost
    obj = np.tile(np.arange(nobj, dtype=np.int64), P * n)
    dist, _, inside = ms.distance(pts.reshape(-1, 3), obj.astype(np.int32), inv[obj, slot % n], slot * V, np.full(slot.shape, V, np.int64),
                                  inside=sign == "parity")
    if sign == "winding":
        from ..winding import WindingSet

        ws = WindingSet([(item["obj_verts"][k], item["obj_faces"][k]) for k in range(nobj)], device=device)
        _, inside = ws.points(pts.reshape(-1, 3), obj.astype(np.int32), inv[obj, slot % n], slot * V, np.full(slot.shape, V, np.int64))
    dist, inside = dist.reshape(P, n, nobj, V), inside.reshape(P, n, nobj, V)
    return torch.where(inside, dist, torch.zeros_like(dist)).amax(dim=2), inside.any(dim=2)


def penetration_maps(item, hands, frames, far_mm, device, sign="parity"):
    """the heat maps of a clip's hand panels: [colours (n, V, 3) float32 on the device, one per panel]"""
    from .. import render as R

    depth, inside = penetration_depths(item, hands, frames, device, sign)
    return [R.penetration_colors(depth[p], inside[p], colour, hot=PENETRATION_COLOR, far=1e-3 * far_mm) for p, (_, colour) in enumerate(hands)]


def main(argv=None) -> int:
    logging.basicConfig(level=logging.INFO, format="%(message)s")
    cfg = parse_args(sys.argv[1:] if argv is None else argv)
    rt = cfg["runtime"]
    loader = mesh_loader(cfg)
    pairs = C.load_pairs(cfg, obj_model_loader=loader)
    if rt["max_clips"] is not None:
        pairs = pairs[: rt["max_clips"]]
    _logger.info("clips with a refined sample: %d", len(pairs))
    if rt["dry_run"]:
        print(json.dumps({"n_clips": len(pairs), "pairs": C.pair_listing(pairs), "sample_refine_filepath": cfg["debug"]["sample_refine_filepath"],
                          "obj_model_loader": cfg["data"]["obj_model_loader"], "out_dir": rt["out_dir"], "render": cfg["render"],
                          "display": cfg["display"], "with_gt": rt["with_gt"], **({"penetration": cfg["penetration"]} if "penetration" in cfg else {}),
                          **({"obj_mesh_prefix": cfg["data"]["obj_mesh_prefix"]} if cfg["data"].get("obj_mesh_prefix") else {})}))
        return 0
    import torch

    from .. import render as R

    device = torch.device(rt["device"])
    mano = C.load_mano(cfg, device) if cfg["mano"]["factory"] else None
    if not pairs:
        raise SystemExit(f"no clip with a refined sample under {cfg['debug']['sample_refine_filepath']}")
    torch.cuda.set_device(device)
    items = [p[0] for p in pairs]
    gt_verts = C.ground_truth_mano(items, mano, device, rt["batch_size"])[1] if rt["with_gt"] else [None] * len(items)
    index = []
    for (item, path), gt in zip(pairs, gt_verts):
        save = formats.read_refine_sample(path)
        faces = save.get("faces")
        if faces is None:
            if mano is None:
                raise SystemExit(f"{path} holds no hand faces: pass --mano.factory module:function (its closed faces are used)")
            faces = mano[2] if item["hand_side"] == "rh" else mano[3]
        hands = [(np.asarray(save["verts"], np.float32), HAND_COLOR)] + ([(gt, GT_HAND_COLOR)] if gt is not None else [])
        frames, images = render_clip(item, hands, np.asarray(faces), cfg, device)
        out = clip_dir(rt["out_dir"], item["info"])
        entry = {"info": list(item["info"]), "dir": out, "frames": frames, "files": [], "sheet": None,
                 "objects": "mesh" if "obj_verts" in item else "points"}
        if frames:
            os.makedirs(out, exist_ok=True)
            for k, fr in enumerate(frames):
                name = "frame_%04d.png" % fr
                R.write_png(os.path.join(out, name), images[k])
                entry["files"].append(name)
            R.write_png(os.path.join(out, "sheet.png"), R.contact_sheet(images[:: cfg["render"]["sheet_cols"]], cfg["render"]["sheet_cols"]))
            entry["sheet"] = "sheet.png"
            if cfg["display"]["apng"]:
                R.write_apng(os.path.join(out, "clip.apng"), images, cfg["display"]["apng_fps"])
                entry["apng"] = "clip.apng"
        index.append(entry)
        print(f"{out} {len(frames)} frames")
    res = {"n_clips": len(index), "n_frames": sum(len(e["frames"]) for e in index), "out_dir": rt["out_dir"], "render": cfg["render"],
           "with_gt": rt["with_gt"], "clips": index}
    if cfg["display"] != DISPLAY_DEFAULTS:
        res["display"] = cfg["display"]
    if "penetration" in cfg:
        res["penetration"] = cfg["penetration"]
    print(f"n_frames {res['n_frames']}")
    if rt["out_json"]:
        C.write_json(rt["out_json"], res)
    return 0


if __name__ == "__main__":
    sys.exit(main())
