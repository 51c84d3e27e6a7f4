"""A user-written `--data.obj_model_loader` hook and the mesh files that say the same: oracle.fixtures' synthetic object meshes as
float32 / int32, from a function (`load_obj`) and written under a prefix in both directory layouts and three formats (`write_prefix`).
tests/test_object_points_launch_gpu.py runs the launchers once with each and expects the same bytes."""
import os

import numpy as np


def load_obj(obj_id):
    from oracle.fixtures import synthetic_object_mesh

    v, f = synthetic_object_mesh(str(obj_id))
    return np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int32)


def write_prefix(prefix, obj_ids, open_ids=()):
    """object k of the sorted ids as <id>.obj, <id>/model.ply (binary) or <id>.ply (ascii), by k mod 3; the meshes of `open_ids` lose
    their first face.  -> {obj_id: (verts, faces)} as written"""
    from oakink2_tamf_amd import mesh_io

    os.makedirs(prefix, exist_ok=True)
    out = {}
    for k, oid in enumerate(sorted(obj_ids)):
        v, f = load_obj(oid)
        if oid in open_ids:
            f = f[1:]
        if k % 3 == 0:
            mesh_io.write_obj(os.path.join(prefix, f"{oid}.obj"), v, f)
        elif k % 3 == 1:
            os.makedirs(os.path.join(prefix, oid), exist_ok=True)
            mesh_io.write_ply(os.path.join(prefix, oid, "model.ply"), v, f)
        else:
            mesh_io.write_ply(os.path.join(prefix, f"{oid}.ply"), v, f, binary=False)
        out[oid] = (v, f)
    return out
