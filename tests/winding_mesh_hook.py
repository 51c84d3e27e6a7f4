"""A `--data.obj_model_loader` hook for the winding-number launcher tests: oracle.fixtures' closed synthetic meshes, except that the
object OPEN_ID is a cube turned out of the axes with one whole side (two triangles) removed - a mesh with a hole, of the kind a scan
gives.  `turned_cube(open=...)` is that cube by itself."""
import numpy as np

OPEN_ID = "S11005"
HALF = 0.04


def turned_cube(open=False):
    """(verts float32 (8, 3), faces int32 (12 or 10, 3)): the cube of half edge HALF under a rotation far from the identity; open: without
    its two top triangles"""
    import meshdist_cases as C
    import winding_restatement as WR

    v, f = WR.open_cube(HALF) if open else WR.cube(HALF)
    rot = C.rigid(3)[:, :3]
    return np.ascontiguousarray((v @ rot.T).astype(np.float32)), np.ascontiguousarray(f, dtype=np.int32)


def load_obj(obj_id):
    if str(obj_id) == OPEN_ID:
        return turned_cube(open=True)
    from oracle.fixtures import synthetic_object_mesh

    v, f = synthetic_object_mesh(str(obj_id))
    return np.ascontiguousarray(v, dtype=np.float32), np.ascontiguousarray(f, dtype=np.int32)
