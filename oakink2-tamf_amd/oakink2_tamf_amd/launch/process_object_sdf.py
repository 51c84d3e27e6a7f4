"""Signed distance files of objects from mesh files: `<mesh prefix>/<obj_id>.{obj,ply,stl}` (or the single mesh file inside
`<mesh prefix>/<obj_id>/`) -> `<out_dir>/<obj_id>.pkl`, the pickled dict of the twelve SDFData fields that the reference's
sdf_util.load_sdf_data reads (dev_fn/util/sdf_util.py:40-56,133-137).  `compute_score_siv --data.obj_sdf_prefix <out_dir>` takes the
files as they are.

    python -m oakink2_tamf_amd.launch.process_object_sdf <mesh prefix> [--out_dir common/retrieve_obj_sdf/main/sdf] [--obj_ids a,b | ?(file:ids.txt)]
        [--resolution 100] [--bbox_expand_ratio 1.2] [--sign parity|winding] [--overwrite] [--dry_run] [--out_json FILE] [--device cuda:0]

This is no speed cache: voxelising an object takes milliseconds.  It is the reference's file format made without
pysdf, with a real distance in it: `sdf` = +distance inside, -distance outside (the reference's "negative outside"), float64, the
distance exact to the definition of include/tamf_meshdist.h.  The SIGN is that of the reference's check_mesh_contains
(geometry.voxelize_lattice), which presumes a closed mesh - not pysdf's; the two agree away from the surface.  An interior lattice point
whose distance is exactly 0 has sdf = 0 and so is not in `sdf > 0`: each file's count of them is listed as n_surface_points.
--sign winding takes the sign from the generalized winding number instead (|w| > 0.5, include/tamf_winding.h): it needs no closed mesh
and equals the default on a clean closed one.  The file keeps the same twelve fields; the sign used is listed per object.
An existing file is kept unless --overwrite is given.  --dry_run lists every object's mesh_report and touches no GPU."""
from __future__ import annotations

import argparse
import json
import os
import pickle
import sys
from typing import Dict, List, Optional

from .. import mesh_io
from .sample import _abspath, _str_list

PROG = "process_object_sdf"
DEFAULT_SDF_PREFIX = os.path.join("common", "retrieve_obj_sdf", "main", "sdf")


def make_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="oakink2_tamf_amd.launch.process_object_sdf", allow_abbrev=False)
    ap.add_argument("prefix", help="directory of mesh files: <obj_id>.{obj,ply,stl} or <obj_id>/<one mesh file>")
    ap.add_argument("--out_dir", default=DEFAULT_SDF_PREFIX)
    ap.add_argument("--obj_ids", default=None, help="comma-separated ids or ?(file:list.txt); default: every mesh under the prefix, sorted")
    ap.add_argument("--resolution", type=int, default=100, help="lattice points per axis (2 .. 512)")
    ap.add_argument("--bbox_expand_ratio", type=float, default=1.2)
    ap.add_argument("--sign", choices=("parity", "winding"), default="parity",
                    help="the inside test behind the sign: the reference's ray parity (presumes a closed mesh) or the generalized winding number")
    ap.add_argument("--overwrite", action="store_true")
    ap.add_argument("--dry_run", action="store_true", help="list every object's mesh report and exit (no GPU)")
    ap.add_argument("--out_json", default=None, help="write the index (counts per object) here")
    ap.add_argument("--device", default="cuda:0")
    return ap


def list_work(prefix: str, obj_ids: Optional[List[str]], out_dir: str) -> List[Dict]:
    if not os.path.isdir(prefix):
        raise SystemExit(f"{PROG}: {prefix} is no directory")
    if obj_ids is None:
        obj_ids = mesh_io.list_object_ids(prefix)
    work = []
    for oid in obj_ids:
        try:
            src = mesh_io.resolve_object_file(prefix, oid)
        except ValueError as e:
            raise SystemExit(f"{PROG}: {e}")
        work.append({"obj_id": oid, "source": src, "sdf": os.path.join(out_dir, f"{oid}.pkl")})
    return work


def write_pickle(path: str, fields: Dict) -> None:
    """written beside `path` and moved into place"""
    tmp = path + ".tmp"
    with open(tmp, "wb") as f:
        pickle.dump(dict(fields), f, protocol=4)
    os.replace(tmp, path)


def main(argv=None) -> int:
    a = make_parser().parse_args(sys.argv[1:] if argv is None else argv)
    prefix, out_dir = _abspath(a.prefix), _abspath(a.out_dir)
    if not 2 <= a.resolution <= 512:
        raise SystemExit(f"{PROG}: --resolution must lie in [2, 512]")
    if not a.bbox_expand_ratio > 0:
        raise SystemExit(f"{PROG}: --bbox_expand_ratio must be positive")
    work = list_work(prefix, _str_list(a.obj_ids) if a.obj_ids is not None else None, out_dir)
    if not work:
        raise SystemExit(f"{PROG}: no mesh file under {prefix}")
    index = []
    for w in work:
        try:
            w["mesh"] = mesh_io.read_mesh(w["source"])
            rep = mesh_io.mesh_report(*w["mesh"])
        except ValueError as e:
            raise SystemExit(f"{PROG}: {e}")
        index.append({"obj_id": w["obj_id"], "source": w["source"], "sdf": w["sdf"], **rep})
    if a.dry_run:
        print(json.dumps({"resolution": a.resolution, "bbox_expand_ratio": a.bbox_expand_ratio, "sign": a.sign, "objects": index}, indent=1))
        return 0
    from .. import meshdist as MD
    from ..winding import WindingError

    os.makedirs(out_dir, exist_ok=True)
    for w, entry in zip(work, index):
        if os.path.exists(w["sdf"]) and not a.overwrite:
            entry["status"] = "kept"
            print(f"{w['obj_id']}: {w['sdf']} exists, kept (--overwrite replaces it)")
            continue
        if not entry["closed"] and a.sign == "winding":
            print(f"{w['obj_id']}: the mesh is not closed ({entry['n_boundary_edges']} boundary edges, {entry['n_nonmanifold_edges']} non-manifold "
                  "edges): the sign is the winding number's (|w| > 0.5)", file=sys.stderr)
        elif not entry["closed"]:
            print(f"{w['obj_id']}: the mesh is not closed ({entry['n_boundary_edges']} boundary edges, {entry['n_nonmanifold_edges']} non-manifold "
                  "edges): the sign rests on an inside test that presumes a closed mesh", file=sys.stderr)
        try:
            fields, info = MD.process_sdf(*w["mesh"], bbox_expand_ratio=a.bbox_expand_ratio, resolution=a.resolution, device=a.device, info=True,
                                          sign=a.sign)
        except (ValueError, MD.MeshDistError, WindingError) as e:
            raise SystemExit(f"{PROG}: {w['source']}: {e}")
        write_pickle(w["sdf"], fields)
        entry.update(status="written", sign=a.sign, **info)
        print(f"{w['obj_id']}: {w['sdf']} (n_inside {info['n_inside']}, n_surface_points {info['n_surface_points']}, sign {a.sign})")
    if a.out_json:
        with open(a.out_json, "w") as f:
            json.dump({"resolution": a.resolution, "bbox_expand_ratio": a.bbox_expand_ratio, "sign": a.sign, "objects": index}, f, indent=1)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
