"""Lattices and scenes for the SDF-lattice tests: SDFData-shaped field dicts built from a function of the object-frame point, the way
process_sdf lays them out (ticks = linspace(-extent_expanded / 2, extent_expanded / 2, R), point = tick + mesh_center, flat index
(i R + j) R + k), and hand / trajectory arrays that put vertices inside, on the faces of, just outside and far from them."""
import numpy as np


def fields_from(fn, center, extent_expanded, res, ratio=1.2):
    """the twelve SDFData fields (the boxes as process_sdf derives them) with sdf = fn(point), float64"""
    center, ext = np.asarray(center, np.float64), np.asarray(extent_expanded, np.float64)
    ticks = np.linspace(-ext / 2.0, ext / 2.0, res)
    x, y, z = np.meshgrid(ticks[:, 0], ticks[:, 1], ticks[:, 2], indexing="ij")
    query = np.vstack((x.flatten(), y.flatten(), z.flatten())).T
    point = query + center
    lo, hi = -ext / ratio / 2.0, ext / ratio / 2.0
    corners = np.array([[(lo, hi)[(c >> k) & 1][k] for k in range(3)] for c in range(8)])
    return {"mesh_center": center, "bbox": corners + center, "bbox_centered": corners, "bbox_centered_expanded": corners * ratio,
            "bbox_expanded": corners * ratio + center, "bbox_expand_ratio": ratio, "resolution": int(res), "extent": ext / ratio,
            "extent_expanded": ext, "tick_unit": ext / res, "point": point, "sdf": np.asarray(fn(point), np.float64)}


def sphere_fn(radius, centre=(0.0, 0.0, 0.0)):
    c = np.asarray(centre, np.float64)
    return lambda p: radius - np.linalg.norm(p - c, axis=-1)


def affine_fn(a, b):
    a = np.asarray(a, np.float64)
    return lambda p: p @ a + b


# dyadic lattices: every tick, every value of an affine function with dyadic coefficients and every product below is exact in float32
DYADIC_CENTER, DYADIC_STEP = np.array([0.5, -1.0, 0.25]), np.array([0.25, 0.5, 0.125])
AFFINE_A, AFFINE_B = np.array([1.5, -0.75, 2.0]), 3.0  # positive over the dyadic lattice of R = 5: at least 3 - 0.75 - 0.75 - 0.5


def dyadic_fields(res=5, fn=None):
    return fields_from(affine_fn(AFFINE_A, AFFINE_B) if fn is None else fn, DYADIC_CENTER, DYADIC_STEP * (res - 1), res)


def grid_set_fields():
    """G = 3 for the GPU shapes: R = 2 (one cell), R = 5 with three different extents and steps, R = 100 (a sphere of radius 0.3)"""
    one_cell = fields_from(lambda p: 0.2 + 0.5 * p[:, 0] - 0.25 * p[:, 1] * p[:, 2], [0.1, 0.0, -0.1], [0.5, 0.75, 1.0], 2)
    five = fields_from(lambda p: 0.15 - np.abs(p - np.array([0.05, -0.02, 0.03])).sum(-1) * 0.4 + 0.1 * np.sin(9.0 * p[:, 0]), [0.0, 0.05, 0.0],
                       [0.8, 0.5, 1.1], 5)
    sphere = fields_from(sphere_fn(0.3, (0.02, -0.01, 0.0)), [0.02, -0.01, 0.0], [0.9, 0.84, 0.96], 100)
    return [one_cell, five, sphere]


def random_traj(rng, shape, spread=0.05):
    """obj_traj rows tsl | rot6d (..., 9) float32: small translations, generic (unnormalised, non-orthogonal) rot6d"""
    tr = np.concatenate([rng.normal(0.0, spread, size=shape + (3,)), rng.normal(0.0, 1.0, size=shape + (6,))], -1)
    return tr.astype(np.float32)


def world_points(traj_row, p_obj):
    """object-frame points (N, 3) float64 -> world points float32 under one obj_traj row: y = R p + t, R's rows the Gram-Schmidt of the
    row (float64, then rounded: the points land NEAR p_obj in the object frame, which is all the scenes need)"""
    import sdfgrid_restatement as RS

    R, t = RS.pose(traj_row)
    return (p_obj @ R.T + t).astype(np.float32)
