"""A `--data.obj_model_loader` hook for the penetration depth tests: tests/object_mesh_hook.py's meshes, except that object S11005 comes
with faces that are all degenerate (a repeated index, three collinear vertices) - a mesh nothing can be measured against, which the
launcher leaves out and counts."""
import numpy as np

NO_MESH = "S11005"


def load_obj(obj_id):
    import object_mesh_hook

    v, f = object_mesh_hook.load_obj(obj_id)
    if str(obj_id) == NO_MESH:
        v = np.concatenate([v, [[1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [3.0, 3.0, 3.0]]]).astype(np.float32)
        f = np.asarray([[0, 0, 1], [len(v) - 3, len(v) - 2, len(v) - 1]], dtype=np.int32)
    return v, f
