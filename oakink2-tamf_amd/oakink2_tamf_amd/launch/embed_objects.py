"""Object embeddings from point clouds: `<obj_pointcloud_prefix>/<obj_id>.npz["point"]` (P, 3) or (P, 6) ->
`<out_dir>/<obj_id>.pt`, a float32 tensor of shape (2 * trans_dim,) = (768,) - the file `InteractionSegmentData.load_object_embedding`
reads.  The encoder is model/point_encoder.py (PointBERT, native HIP); its weights are not shipped: `--point_encoder.ckpt` is a
checkpoint holding them under `module.point_encoder.`.

The reference has no such script and does not say how the published embeddings were made, so the preprocessing is explicit here:
  --color r,g,b   fills the colour channels of xyz-only clouds when the encoder takes 6 channels (required then)
  --pc_norm       centres the xyz on their centroid and scales by the largest norm (off by default)
  --seed          draws the FPS start indices from a CPU generator (default: index 0 everywhere)
  --data.obj_mesh_prefix DIR   takes the clouds from mesh files instead of .npz files: DIR/<obj_id>.{obj,ply,stl} (or the single mesh file
                  in DIR/<obj_id>/) is sampled in memory exactly as launch/sample_object_points.py writes it (`npoints` points,
                  --sample.oversample 4, --sample.seed 0, --sample.scale 1.0, --sample.with_normals; key = FNV-1a 64 of the id), so the
                  embedding equals, bit for bit, the one made from that launcher's file; --data.obj_pointcloud_prefix is not read then
A cloud with more than `npoints` points is FPS-resampled to `npoints` (from the same start index); one with fewer is rejected."""
from __future__ import annotations

import argparse
import glob
import os
from typing import Dict, List, Optional

import numpy as np

from .sample import _abspath, _str_list

DEFAULT_POINTCLOUD_PREFIX = os.path.join("common", "retrieve_obj_pointcloud", "main", "pointcloud")
DEFAULT_OUT_DIR = os.path.join("common", "retrieve_obj_embedding", "main", "embedding")


def make_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="oakink2_tamf_amd.launch.embed_objects", allow_abbrev=False)
    ap.add_argument("--point_encoder.ckpt", dest="ckpt", default=None, help="checkpoint with the encoder under module.point_encoder.")
    ap.add_argument("--point_encoder.cfg", dest="cfg", default=None,
                    help="yaml with the encoder's fields (the reference's PointTransformer_8192point_2layer.yaml layout, or the fields "
                         "at top level); default: trans_dim 384, depth 12, 6 heads, 512 groups of 32, encoder_dims 256, point_dims 6, 8192 points")
    ap.add_argument("--data.obj_pointcloud_prefix", dest="prefix", default=DEFAULT_POINTCLOUD_PREFIX)
    ap.add_argument("--data.obj_mesh_prefix", dest="mesh_prefix", default=None,
                    help="sample the clouds from the mesh files of this directory (as sample_object_points does) instead of reading .npz files")
    ap.add_argument("--sample.oversample", dest="sample_oversample", type=int, default=4)
    ap.add_argument("--sample.seed", dest="sample_seed", type=int, default=0)
    ap.add_argument("--sample.scale", dest="sample_scale", type=float, default=1.0)
    ap.add_argument("--sample.with_normals", dest="sample_with_normals", action="store_true")
    ap.add_argument("--obj_ids", default=None, help="comma-separated ids or ?(file:list.txt); default: every .npz (or mesh) under the prefix")
    ap.add_argument("--out_dir", default=DEFAULT_OUT_DIR)
    ap.add_argument("--color", default=None, help="r,g,b for xyz-only clouds")
    ap.add_argument("--pc_norm", action="store_true")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--batch_size", type=int, default=4, help="clouds per encoder call (no output bit depends on it)")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--dry_run", action="store_true", help="list the work and exit (no GPU, no checkpoint)")
    return ap


def load_cfg(path: Optional[str]) -> Dict[str, int]:
    from ..model.point_encoder import make_cfg

    if path is None:
        return make_cfg()
    import yaml

    with open(path) as f:
        y = yaml.safe_load(f) or {}
    fields = dict(y.get("model", {k: v for k, v in y.items() if k != "npoints"}))
    if "npoints" in y:
        fields["npoints"] = y["npoints"]
    return make_cfg(fields)


def list_mesh_work(prefix: str, obj_ids: Optional[List[str]], out_dir: str) -> List[Dict]:
    """list_work over a directory of mesh files: `pointcloud` names the mesh the cloud is sampled from"""
    from .sample_object_points import list_work as list_meshes

    return [{"obj_id": w["obj_id"], "pointcloud": w["source"], "embedding": os.path.join(out_dir, f"{w['obj_id']}.pt")}
            for w in list_meshes(prefix, obj_ids, out_dir, False)]


def load_cloud(w: Dict, a, npoints: int) -> np.ndarray:
    """the raw cloud of one work item: the .npz's "point", or - with --data.obj_mesh_prefix - the mesh sampled as sample_object_points does"""
    if a.mesh_prefix is None:
        with np.load(w["pointcloud"]) as z:
            return z["point"]
    from .. import mesh_io
    from .sample_object_points import object_cloud, scaled

    try:
        v, f = mesh_io.read_mesh(w["pointcloud"])
        return object_cloud(scaled(v, a.sample_scale), f, w["obj_id"], npoints, a.sample_oversample, a.sample_seed, a.sample_with_normals, a.device)["point"]
    except ValueError as e:
        raise SystemExit(f"embed_objects: {w['pointcloud']}: {e}")


def list_work(prefix: str, obj_ids: Optional[List[str]], out_dir: str) -> List[Dict]:
    if obj_ids is None:
        obj_ids = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(prefix, "*.npz")))
    work = []
    for oid in obj_ids:
        src = os.path.join(prefix, f"{oid}.npz")
        if not os.path.exists(src):
            raise SystemExit(f"embed_objects: {src} not found")
        work.append({"obj_id": oid, "pointcloud": src, "embedding": os.path.join(out_dir, f"{oid}.pt")})
    return work


def prepare_cloud(point: np.ndarray, point_dims: int, color, pc_norm: bool) -> np.ndarray:
    """(P, 3) or (P, 6) -> (P, point_dims) float32, before any resampling"""
    p = np.asarray(point, dtype=np.float32)
    if p.ndim != 2 or p.shape[1] not in (3, 6):
        raise ValueError(f"expected a (P, 3) or (P, 6) array, got {p.shape}")
    if not np.isfinite(p).all():
        raise ValueError("the cloud holds a non-finite value")
    xyz, rest = p[:, :3], p[:, 3:]
    if pc_norm:
        xyz = xyz - xyz.mean(0, keepdims=True)
        xyz = xyz / np.sqrt((xyz ** 2).sum(1)).max()
    if point_dims == 3:
        return np.ascontiguousarray(xyz, dtype=np.float32)
    if rest.shape[1] == 0:
        if color is None:
            raise ValueError("an xyz-only cloud and a 6-channel encoder: give --color r,g,b")
        rest = np.broadcast_to(np.asarray(color, dtype=np.float32), (p.shape[0], 3))
    return np.ascontiguousarray(np.concatenate([xyz, rest], 1), dtype=np.float32)


def save_embedding(path: str, emb) -> None:
    """one embedding as InteractionSegmentData.load_object_embedding reads it: a float32 CPU tensor of shape (2 * trans_dim,)"""
    import torch

    e = torch.as_tensor(emb).detach().to(device="cpu", dtype=torch.float32).reshape(-1).clone()
    if not bool(torch.isfinite(e).all()):
        raise ValueError(f"{path}: the embedding holds a non-finite value")
    torch.save(e, path)


def main(argv=None) -> int:
    a = make_parser().parse_args(argv)
    cfg = load_cfg(a.cfg)
    prefix, out_dir = _abspath(a.prefix), _abspath(a.out_dir)
    color = None
    if a.color is not None:
        color = [float(x) for x in a.color.split(",")]
        if len(color) != 3:
            raise SystemExit("embed_objects: --color takes r,g,b")
    ids = _str_list(a.obj_ids) if a.obj_ids is not None else None
    work = list_work(prefix, ids, out_dir) if a.mesh_prefix is None else list_mesh_work(_abspath(a.mesh_prefix), ids, out_dir)
    if a.dry_run:
        import json

        print(json.dumps({"cfg": cfg, "pc_norm": a.pc_norm, "color": color, "seed": a.seed, "work": work}, indent=1))
        return 0
    if a.ckpt is None:
        raise SystemExit("embed_objects: --point_encoder.ckpt is required (the encoder's weights are not shipped)")
    import torch

    from ..model.point_encoder import HipPointEncoder

    enc = HipPointEncoder(cfg, device=a.device)
    enc.load_checkpoint(_abspath(a.ckpt))
    npoints = cfg["npoints"]
    gen = torch.Generator().manual_seed(a.seed) if a.seed is not None else None
    os.makedirs(out_dir, exist_ok=True)
    for s in range(0, len(work), max(1, a.batch_size)):
        part = work[s: s + max(1, a.batch_size)]
        clouds, starts = [], []
        for w in part:
            try:
                p = prepare_cloud(load_cloud(w, a, npoints), cfg["point_dims"], color, a.pc_norm)
            except ValueError as e:
                raise SystemExit(f"embed_objects: {w['pointcloud']}: {e}")
            if p.shape[0] < npoints:
                raise SystemExit(f"embed_objects: {w['pointcloud']}: {p.shape[0]} points, the encoder takes {npoints}")
            start = int(torch.randint(0, npoints, (1,), generator=gen)) if gen is not None else 0
            if p.shape[0] > npoints:  # farthest-point resampling from the same start
                keep = enc.fps(p[None], num=npoints, start_index=start)[0].cpu().numpy()
                p, start = p[keep], 0  # (the start point is row 0 of the resampled cloud)
            clouds.append(p)
            starts.append(start)
        emb = enc.encode(np.stack(clouds), start_index=torch.tensor(starts)).cpu()
        for w, e in zip(part, emb):
            save_embedding(w["embedding"], e)
            print(f"{w['obj_id']}: {w['embedding']}")
    enc.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
