#!/usr/bin/env python
"""Capture the SIV fixtures of tests/golden/ from the reference's own arithmetic.  CPU, numpy only.

    python tools/capture_siv_golden.py REFERENCE_ROOT [--out tests/golden]      (after oracle/build_ref.sh)

What runs for real, read from REFERENCE_ROOT when the tool runs (nothing of its text is written anywhere):
  * process_sdf (src/dev_fn/util/sdf_util.py), imported as it is;
  * solid_intersection_volume of script/compute_score/compute_score_siv.py, cut from the script by content (from its `def` line to
    its `return siv`) and executed on the scope this tool supplies;
  * check_mesh_contains (src/dev_fn/external/libmesh/inside_mesh.py with the TriangleHash that oracle/build_ref.sh compiled into
    oracle/_ref/) and tslrot6d_to_transf_np / transf_point_array_np (src/dev_fn/transform/transform_np.py).
Stand-ins, for the imports that are absent here only:
  * `trimesh.Trimesh`: a minimal mesh with `vertices`, `faces`, `bounding_box.vertices` (the 8 corners, x slowest) and
    `bounding_box.extents`;
  * `pysdf.SDF`: its sign is the reference's check_mesh_contains (+1 inside, -1 outside);
  * `skimage` (imported by sdf_util.py, not used by process_sdf): empty modules.
So the fixtures pin the numpy-line arithmetic of process_sdf / solid_intersection_volume and the containment semantics.  THEY DO NOT
PIN PYSDF: how far pysdf's sign differs from check_mesh_contains next to the surface is not measured by anything here.

At capture time the tool asserts that oracle.geometry_oracle.mesh_contains reproduces every captured mask exactly, and every captured
count when the query points are formed in float64 as ((R00 x + R01 y) + R02 z) + t0 instead of by the reference's matmul (whose
summation order is the BLAS's).  A seed for which a count differs would have to be replaced, and said so here; none had to be: seeds
20270 (sphere), 20271 (rotations), 20272 and 20273 (clips) passed at the first attempt.

Fixtures (data only): siv_lattice_<mesh>.npz - the mesh, R, the SDFData fields the score uses, the packed mask; siv_clip_<name>.npz -
hand meshes, object trajectories, the names of the lattice fixtures that are its objects, counts and volumes."""
import argparse
import importlib
import importlib.util
import os
import sys
import textwrap
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import fixtures as FX  # noqa: E402
from oracle import geometry_oracle as G  # noqa: E402

ASKED = []  # the query points of every call of the SDF stand-in
START, END = "def solid_intersection_volume(hand_verts, hand_faces, obj_transf_map):", "return siv"


class _Box:
    def __init__(self, v):
        self._lo, self._hi = v.min(axis=0), v.max(axis=0)

    @property
    def vertices(self):
        b = (self._lo, self._hi)
        return np.array([[b[i][0], b[j][1], b[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=np.float64)

    @property
    def extents(self):
        return self._hi - self._lo


class MiniMesh:
    """the part of trimesh.Trimesh that process_sdf and solid_intersection_volume touch"""

    def __init__(self, vertices, faces, **_):
        self.vertices = np.array(vertices, copy=True)
        self.faces = np.asarray(faces)

    @property
    def bounding_box(self):
        return _Box(np.asarray(self.vertices))


def load_reference(reference_root):
    """-> (process_sdf, solid_intersection_volume, its module-level obj_sdf_map, check_mesh_contains, transform_np module)"""
    src = os.path.join(reference_root, "src")
    sys.path.insert(0, src)
    ref_pkg = os.path.join(src, "dev_fn", "external", "libmesh")
    built = os.path.join(ROOT, "oracle", "_ref", "libmesh")
    if not os.path.isdir(built) or not any(n.startswith("triangle_hash") for n in os.listdir(built)):
        raise SystemExit("run oracle/build_ref.sh first (the reference's TriangleHash)")
    pkg = types.ModuleType("tamf_ref_libmesh")
    pkg.__path__ = [built, ref_pkg]
    sys.modules["tamf_ref_libmesh"] = pkg
    spec = importlib.util.spec_from_file_location("tamf_ref_libmesh.inside_mesh", os.path.join(ref_pkg, "inside_mesh.py"))
    inside_mesh = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = inside_mesh
    spec.loader.exec_module(inside_mesh)
    check = inside_mesh.check_mesh_contains

    class SDF:
        def __init__(self, verts, faces, robust=True):
            self.mesh = MiniMesh(verts, faces)

        def __call__(self, points):
            ASKED.append(np.array(points, copy=True))  # (the lattice as process_sdf made it, before the centre is added back)
            return np.where(check(self.mesh, np.asarray(points)), 1.0, -1.0)

    tm = types.ModuleType("trimesh")
    tm.Trimesh = MiniMesh
    ps = types.ModuleType("pysdf")
    ps.SDF = SDF
    sk, skm = types.ModuleType("skimage"), types.ModuleType("skimage.measure")
    sk.measure = skm
    for name, mod in (("trimesh", tm), ("pysdf", ps), ("skimage", sk), ("skimage.measure", skm)):
        sys.modules.setdefault(name, mod)
    sdf_util = importlib.import_module("dev_fn.util.sdf_util")
    tnp = importlib.import_module("dev_fn.transform.transform_np")
    path = os.path.join(reference_root, "script", "compute_score", "compute_score_siv.py")
    with open(path) as f:
        lines = f.read().splitlines()
    first = [i for i, l in enumerate(lines) if l.strip() == START]
    if len(first) != 1:
        raise SystemExit(f"{path}: `{START}` was not found exactly once")
    last = next((i for i in range(first[0], len(lines)) if lines[i].strip() == END), None)
    if last is None:
        raise SystemExit(f"{path}: no `{END}` behind the function's first line")
    scope = {"np": np, "trimesh": tm, "obj_sdf_map": {}, "transf_point_array_np": tnp.transf_point_array_np, "check_mesh_contains": check}
    exec(compile(textwrap.dedent("\n".join(lines[first[0]: last + 1])), "<reference solid_intersection_volume>", "exec"), scope)
    return sdf_util.process_sdf, scope["solid_intersection_volume"], scope["obj_sdf_map"], check, tnp


def rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def box_mesh(half):
    v = np.array([[sx * half[0], sy * half[1], sz * half[2]] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float64)
    f = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7],
                  [1, 7, 3]], dtype=np.int64)
    return v, f


def meshes():
    """(name, verts, faces, R).  Generic position (a random rotation, an irrational offset) keeps lattice columns off the triangle
    edges; `aabox` is axis-aligned on purpose: vertical faces, adet == 0."""
    out = []
    rng = np.random.default_rng(20271)
    v, f = box_mesh((0.031, 0.022, 0.043))
    out.append(("rotbox", v @ rotation(rng).T + np.array([0.0113, -0.0071, 0.0029]), f, 37))
    v, f = FX.icosphere(4)  # 5 120 faces
    srng = np.random.default_rng(20270)
    radial = 1.0 + 0.2 * np.sin(4.0 * v[:, 0] + 1.0) * np.cos(3.0 * v[:, 1]) + 0.1 * np.sin(6.0 * v[:, 2]) + 0.01 * srng.normal(size=len(v))
    out.append(("sphere", (v * radial[:, None] * np.array([0.04, 0.05, 0.03])) @ rotation(rng).T + np.array([0.0021, 0.0037, -0.0013]), f, 48))
    v, f = FX.torus()  # 2 304 faces
    out.append(("torus", (v * 0.045) @ rotation(rng).T + np.array([-0.0017, 0.0023, 0.0031]), f, 100))
    va, fa = box_mesh((0.02, 0.015, 0.012))
    vb, fb = FX.icosphere(2)
    vb = vb * 0.014 + np.array([0.047, 0.011, -0.006])
    out.append(("twoparts", np.concatenate([va @ rotation(rng).T, vb]), np.concatenate([fa, fb + len(va)]), 37))
    v, f = box_mesh((0.03, 0.02, 0.025))
    out.append(("aabox", v + np.array([0.1, -0.05, 0.2]), f, 37))
    return out


def capture_lattice(process_sdf, name, v, f, R):
    sdf = process_sdf(MiniMesh(v, f), resolution=R)
    mask = np.asarray(sdf.sdf) > 0
    query = ASKED[-1]
    assert np.array_equal(query + sdf.mesh_center, sdf.point)
    mine = G.mesh_contains(v - sdf.mesh_center, f, query)
    assert np.array_equal(mine, mask), f"{name}: the oracle differs from the reference's mask at {int((mine != mask).sum())} points"
    print(f"siv_lattice_{name}: {len(f)} faces, R = {R}, inside {int(mask.sum())} of {mask.size}; oracle mask identical")
    return sdf, {"verts": v, "faces": f.astype(np.int32), "R": np.int32(R), "bbox_expand_ratio": np.float64(sdf.bbox_expand_ratio),
                 "mesh_center": sdf.mesh_center, "extent": sdf.extent, "extent_expanded": sdf.extent_expanded, "tick_unit": sdf.tick_unit,
                 "point_first": sdf.point[0], "point_last": sdf.point[-1], "mask_packed": np.packbits(mask), "n_inside": np.int64(mask.sum()),
                 "numpy_version": np.asarray(np.__version__)}


def hand_sequence(rng, T):
    """closed float32 blobs about the size of a hand, drifting and deforming over T frames"""
    v, f = FX.icosphere(2)
    out = []
    for t in range(T):
        radial = 1.0 + 0.2 * np.sin(3.0 * v[:, 0] + 0.05 * t) * np.cos(2.0 * v[:, 1]) + 0.1 * np.sin(5.0 * v[:, 2] - 0.03 * t)
        out.append(v * radial[:, None] * np.array([0.05, 0.07, 0.03]) + np.array([0.004, -0.003, 0.002]) * np.sin(0.1 * t))
    return np.asarray(out).astype(np.float32), f


def capture_clip(ref, name, sdfs, obj_names, T, avai_len, seed):
    process_sdf, siv_fn, sdf_map, check, tnp = ref
    rng = np.random.default_rng(seed)
    gt, faces = hand_sequence(rng, T)
    refined = (gt.astype(np.float64) * 1.04 + rng.normal(scale=5e-4, size=gt.shape)).astype(np.float32)
    traj = np.zeros((len(obj_names), T, 9), np.float32)
    for o in range(len(obj_names)):
        traj[o, :, 0:3] = rng.normal(scale=0.015, size=(T, 3))
        traj[o, :, 3:9] = rng.normal(size=(T, 6))
    transf = tnp.tslrot6d_to_transf_np(traj[:, :avai_len])
    sdf_map.clear()
    for o in obj_names:
        if o in sdfs:  # (an object missing from the map is skipped by the reference)
            sdf_map[o] = sdfs[o]
    frames = list(range(0, avai_len, 20))
    vols = {"gt": [], "refined": []}
    counts = np.zeros((len(frames), 2, len(obj_names)), np.int64)
    for fi, fr in enumerate(frames):
        tmap = {o: transf[k, fr] for k, o in enumerate(obj_names)}
        for h, (key, hv) in enumerate((("gt", gt), ("refined", refined))):
            vols[key].append(siv_fn(hv[fr], faces, tmap))
            for k, o in enumerate(obj_names):
                if o not in sdfs:
                    continue
                s = sdfs[o]
                pin = s.point[s.sdf > 0] + s.mesh_center
                counts[fi, h, k] = int(check(MiniMesh(hv[fr], faces), tnp.transf_point_array_np(tmap[o], pin)).sum())
                M = tmap[o].astype(np.float64)
                q = np.stack([((M[r, 0] * pin[:, 0] + M[r, 1] * pin[:, 1]) + M[r, 2] * pin[:, 2]) + M[r, 3] for r in range(3)], axis=1)
                mine = int(G.mesh_contains(hv[fr].astype(np.float64), faces, q).sum())
                assert mine == counts[fi, h, k], f"{name}: frame {fr} hand {key} object {o}: oracle {mine}, reference {counts[fi, h, k]}: pick another seed"
    el = np.array([np.prod(sdfs[o].tick_unit) if o in sdfs else 0.0 for o in obj_names])
    for h, key in enumerate(("gt", "refined")):  # the captured volumes are the counts' (sanity of the capture itself)
        assert np.array_equal(np.asarray(vols[key]), [sum(counts[fi, h, k] * el[k] * (10 ** 6) for k in range(len(obj_names)) if obj_names[k] in sdfs) + 0.0
                                                      for fi in range(len(frames))])
    print(f"siv_clip_{name}: frames {frames}, counts gt {counts[:, 0].tolist()} refined {counts[:, 1].tolist()}; oracle counts identical")
    return {"hand_verts_gt": gt, "hand_verts_refined": refined, "faces": faces.astype(np.int32), "obj_traj": traj,
            "obj_names": np.asarray(obj_names), "obj_has_lattice": np.asarray([o in sdfs for o in obj_names]), "avai_len": np.int32(avai_len),
            "frames": np.asarray(frames, np.int64), "transf": transf, "counts": counts, "gt_siv": np.asarray(vols["gt"], np.float64),
            "refined_siv": np.asarray(vols["refined"], np.float64), "numpy_version": np.asarray(np.__version__)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference_root")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    ref = load_reference(a.reference_root)
    os.makedirs(a.out, exist_ok=True)
    sdfs = {}
    for name, v, f, R in meshes():
        sdfs[name], arrays = capture_lattice(ref[0], name, v, f, R)
        np.savez_compressed(os.path.join(a.out, f"siv_lattice_{name}.npz"), **arrays)
    clips = {"two_objects": capture_clip(ref, "two_objects", sdfs, ["rotbox", "twoparts"], 48, 45, 20272),
             "skipped_object": capture_clip(ref, "skipped_object", sdfs, ["aabox", "no_such_object", "sphere"], 24, 21, 20273)}
    for name, arrays in clips.items():
        np.savez_compressed(os.path.join(a.out, f"siv_clip_{name}.npz"), **arrays)
    for n in sorted(os.listdir(a.out)):
        if n.startswith("siv_"):
            print(n, os.path.getsize(os.path.join(a.out, n)), "bytes")


if __name__ == "__main__":
    main()
