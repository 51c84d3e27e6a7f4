"""Object point clouds from mesh files: `<mesh prefix>/<obj_id>.{obj,ply,stl}` (or the single mesh file inside `<mesh prefix>/<obj_id>/`)
-> `<out_dir>/<obj_id>.npz`, the file `<obj_pointcloud_prefix>/<obj_id>.npz["point"]` that the refiner's distance feature, the contact
losses, the CR score, the contact heat map and embed_objects read.  The published OakInk2 clouds come from a `retrieve_obj_pointcloud`
step the reference does not ship, and how they were sampled is not known: these clouds are this package's own.

    python -m oakink2_tamf_amd.launch.sample_object_points <mesh prefix> [--out_dir common/retrieve_obj_pointcloud/main/pointcloud]
        [--obj_ids a,b | ?(file:ids.txt)] [--n_points 8192] [--oversample 4] [--seed 0] [--scale 1.0] [--with_normals] [--from_points]
        [--overwrite] [--dry_run] [--out_json FILE] [--device cuda:0]

A cloud is n_points * oversample area-uniform surface samples (surface.sample_surface: the bit-defined HIP sampler of
include/tamf_surface.h, Philox key = FNV-1a 64 of the object id, seed = --seed) thinned to n_points by farthest-point sampling from
sample 0, in FPS order: the same mesh, id and seed give the same file on every machine.  The file holds
    point         float32 (n_points, 3), or (n_points, 6) = xyz | unit normal with --with_normals
    face_index    int64 (n_points,): the face every point was drawn from (--from_points: point_index, the row of the scan)
    seed          uint64, n_candidates int64: what it was made with
(readers use ["point"] only).  --scale multiplies the vertices first (0.001 for an asset in millimetres).  --from_points treats the inputs
as scans (.ply / .obj vertices, .npy, .npz["point"]) and thins them with surface.resample_points.  An existing file is kept unless
--overwrite is given.  --dry_run lists every object's mesh_report and touches no GPU."""
from __future__ import annotations

import argparse
import io
import json
import os
import sys
import zipfile
from typing import Dict, List, Optional

import numpy as np

from .. import mesh_io
from .embed_objects import DEFAULT_POINTCLOUD_PREFIX
from .sample import _abspath, _str_list

PROG = "sample_object_points"
POINT_EXTENSIONS = (".ply", ".obj", ".npy", ".npz")


def make_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="oakink2_tamf_amd.launch.sample_object_points", allow_abbrev=False)
    ap.add_argument("prefix", help="directory of mesh files: <obj_id>.{obj,ply,stl} or <obj_id>/<one mesh file>")
    ap.add_argument("--out_dir", default=DEFAULT_POINTCLOUD_PREFIX)
    ap.add_argument("--obj_ids", default=None, help="comma-separated ids or ?(file:list.txt); default: every mesh under the prefix, sorted")
    ap.add_argument("--n_points", type=int, default=8192)
    ap.add_argument("--oversample", type=int, default=4, help="surface samples drawn per kept point (n_points * oversample <= 32768)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies the vertices (0.001: millimetres -> metres)")
    ap.add_argument("--with_normals", action="store_true", help="point (n_points, 6) = xyz | unit normal of the face")
    ap.add_argument("--from_points", action="store_true", help="the inputs are scans (point files): thin them, no surface sampling")
    ap.add_argument("--overwrite", action="store_true")
    ap.add_argument("--dry_run", action="store_true", help="list every object's mesh report and exit (no GPU)")
    ap.add_argument("--out_json", default=None, help="write the index (counts, area, closed per object) here")
    ap.add_argument("--device", default="cuda:0")
    return ap


def list_work(prefix: str, obj_ids: Optional[List[str]], out_dir: str, from_points: bool) -> List[Dict]:
    ext = POINT_EXTENSIONS if from_points else mesh_io.MESH_EXTENSIONS
    if not os.path.isdir(prefix):
        raise SystemExit(f"{PROG}: {prefix} is no directory")
    if obj_ids is None:
        obj_ids = mesh_io.list_object_ids(prefix, ext)
    work = []
    for oid in obj_ids:
        try:
            src = mesh_io.resolve_object_file(prefix, oid, ext)
        except ValueError as e:
            raise SystemExit(f"{PROG}: {e}")
        work.append({"obj_id": oid, "source": src, "pointcloud": os.path.join(out_dir, f"{oid}.npz")})
    return work


def scaled(verts: np.ndarray, scale: float) -> np.ndarray:
    """the vertices times `scale`: the product in float64, rounded once to float32 (scale 1 changes no bit)"""
    return verts if scale == 1.0 else (verts.astype(np.float64) * float(scale)).astype(np.float32)


def write_npz(path: str, arrays: Dict[str, np.ndarray]) -> None:
    """An uncompressed .npz whose bytes depend on the arrays alone (np.savez stamps every member with the time of day), written
    beside `path` and moved into place"""
    tmp = path + ".tmp"
    with zipfile.ZipFile(tmp, "w", zipfile.ZIP_STORED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(a), allow_pickle=False)  # (a scalar stays 0-dimensional)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())
    os.replace(tmp, path)


def object_cloud(verts, faces, obj_id: str, n_points: int, oversample: int, seed: int, with_normals: bool, device) -> Dict[str, np.ndarray]:
    """the arrays of one object's file, from its (already scaled) mesh"""
    from .. import surface as S

    got = S.sample_point_cloud(verts, faces, n_points=n_points, oversample=oversample, seed=seed, key=S.object_key(obj_id), normals=with_normals,
                               faces_out=True, device=device)
    point = np.concatenate([t.cpu().numpy() for t in got[:-1]], axis=1).astype(np.float32)
    return {"point": point, "face_index": got[-1].cpu().numpy().astype(np.int64), "seed": np.uint64(seed), "n_candidates": np.int64(n_points * oversample)}


def main(argv=None) -> int:
    a = make_parser().parse_args(sys.argv[1:] if argv is None else argv)
    prefix, out_dir = _abspath(a.prefix), _abspath(a.out_dir)
    if a.n_points < 1 or a.oversample < 1:
        raise SystemExit(f"{PROG}: --n_points and --oversample must be at least 1")
    from ..surface import FPS_MAX_POINTS

    if (a.n_points if a.from_points else a.n_points * a.oversample) > FPS_MAX_POINTS:
        raise SystemExit(f"{PROG}: --n_points * --oversample = {a.n_points * a.oversample} candidates, the FPS kernel takes at most {FPS_MAX_POINTS}")
    if not 0 <= a.seed < 2 ** 64:
        raise SystemExit(f"{PROG}: --seed must lie in [0, 2^64)")
    if not (a.scale > 0 and np.isfinite(a.scale)):
        raise SystemExit(f"{PROG}: --scale must be a positive number")
    if a.from_points and a.with_normals:
        raise SystemExit(f"{PROG}: --with_normals needs a mesh (a scan has no faces to take normals from)")
    work = list_work(prefix, _str_list(a.obj_ids) if a.obj_ids is not None else None, out_dir, a.from_points)
    if not work:
        raise SystemExit(f"{PROG}: no {'point' if a.from_points else 'mesh'} file under {prefix}")
    index = []
    for w in work:
        try:
            if a.from_points:
                pts = scaled(mesh_io.read_points(w["source"]), a.scale)
                w["points"], rep = pts, {"n_points_in": int(pts.shape[0])}
            else:
                v, f = mesh_io.read_mesh(w["source"])
                w["mesh"] = (scaled(v, a.scale), f)
                rep = mesh_io.mesh_report(*w["mesh"])
        except ValueError as e:
            raise SystemExit(f"{PROG}: {e}")
        index.append({"obj_id": w["obj_id"], "source": w["source"], "pointcloud": w["pointcloud"], **rep})
    if a.dry_run:
        print(json.dumps({"n_points": a.n_points, "oversample": a.oversample, "seed": a.seed, "scale": a.scale, "with_normals": a.with_normals,
                          "from_points": a.from_points, "objects": index}, indent=1))
        return 0
    from .. import surface as S

    os.makedirs(out_dir, exist_ok=True)
    for w, entry in zip(work, index):
        if os.path.exists(w["pointcloud"]) and not a.overwrite:
            entry["status"] = "kept"
            print(f"{w['obj_id']}: {w['pointcloud']} exists, kept (--overwrite replaces it)")
            continue
        try:
            if a.from_points:
                pts, rows = S.resample_points(w["points"], a.n_points, seed=a.seed, key=S.object_key(w["obj_id"]), device=a.device, indices_out=True)
                arrays = {"point": pts.cpu().numpy(), "point_index": rows.cpu().numpy().astype(np.int64), "seed": np.uint64(a.seed),
                          "n_candidates": np.int64(min(w["points"].shape[0], FPS_MAX_POINTS))}
            else:
                arrays = object_cloud(*w["mesh"], w["obj_id"], a.n_points, a.oversample, a.seed, a.with_normals, a.device)
        except (ValueError, S.SurfaceError) as e:
            raise SystemExit(f"{PROG}: {w['source']}: {e}")
        write_npz(w["pointcloud"], arrays)
        entry.update(status="written", n_points=int(arrays["point"].shape[0]), n_candidates=int(arrays["n_candidates"]))
        print(f"{w['obj_id']}: {w['pointcloud']}")
    if a.out_json:
        with open(a.out_json, "w") as f:
            json.dump({"seed": a.seed, "scale": a.scale, "objects": index}, f, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
