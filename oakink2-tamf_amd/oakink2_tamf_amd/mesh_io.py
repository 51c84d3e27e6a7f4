"""Triangle meshes and point sets from files, with numpy alone: Wavefront OBJ, PLY (ascii and both binary byte orders) and STL
(binary and ascii), written from the formats' definitions.  What the object chain of this package starts from: the surface sampler
(surface.py, launch/sample_object_points.py) and the launchers that take `--data.obj_mesh_prefix` read meshes through `read_mesh` /
`directory_loader`; scans go through `read_points`.

    read_mesh(path)   -> (verts float32 (V, 3), faces int32 (F, 3)); polygons are fanned from their first vertex
    read_points(path) -> float32 (N, 3): the vertices of a PLY or OBJ (faces, if any, ignored), a .npy (N, 3), or .npz["point"]
    write_obj / write_ply: the round trip (and the tests' fixtures)
    mesh_report(verts, faces) -> counts, area, bounding box and whether the mesh is closed
    directory_loader(prefix) -> load(obj_id) -> (verts, faces), cached per id

Every refusal is a ValueError that names the file."""
from __future__ import annotations

import os
import struct
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

MESH_EXTENSIONS = (".obj", ".ply", ".stl")

_PLY_TYPES = {
    "char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2", "ushort": "u2", "uint16": "u2",
    "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4", "float": "f4", "float32": "f4", "double": "f8", "float64": "f8",
}
_PLY_INDEX_NAMES = ("vertex_indices", "vertex_index")


def _fan(polygons: List[List[int]]) -> np.ndarray:
    """polygons of >= 3 indices -> (F, 3): (p0, p[i], p[i+1]), in file order"""
    tris = [(p[0], p[i], p[i + 1]) for p in polygons for i in range(1, len(p) - 1)]
    return np.asarray(tris, dtype=np.int64).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------------------------------------------
# OBJ
# ---------------------------------------------------------------------------------------------------------------------------------
def _parse_obj(path: str) -> Tuple[np.ndarray, np.ndarray]:
    verts: List[Tuple[float, float, float]] = []
    polygons: List[List[int]] = []
    with open(path, "r", errors="replace") as f:
        for ln, line in enumerate(f, 1):
            tok = line.split("#", 1)[0].split()
            if not tok:
                continue
            if tok[0] == "v":
                if len(tok) < 4:
                    raise ValueError(f"{path}:{ln}: a vertex needs three coordinates")
                try:
                    verts.append((float(tok[1]), float(tok[2]), float(tok[3])))
                except ValueError:
                    raise ValueError(f"{path}:{ln}: cannot read the vertex {' '.join(tok[1:4])!r}") from None
            elif tok[0] == "f":
                poly = []
                for t in tok[1:]:
                    try:
                        i = int(t.split("/", 1)[0])
                    except ValueError:
                        raise ValueError(f"{path}:{ln}: cannot read the face index {t!r}") from None
                    if i == 0:
                        raise ValueError(f"{path}:{ln}: face index 0 (OBJ indices start at 1)")
                    # a negative index counts back from the vertices read so far; one out of range stays so and is named below
                    poly.append(i - 1 if i > 0 else len(verts) + i if len(verts) + i >= 0 else -1)
                if len(poly) < 3:
                    raise ValueError(f"{path}:{ln}: a face needs at least three vertices")
                polygons.append(poly)
    return np.asarray(verts, dtype=np.float64).reshape(-1, 3), _fan(polygons)


# ---------------------------------------------------------------------------------------------------------------------------------
# PLY
# ---------------------------------------------------------------------------------------------------------------------------------
def _ply_header(path: str, f):
    """-> (format, [(element name, count, [property])]), property = (name, dtype code) or (name, count code, item code)"""
    if f.readline().strip() != b"ply":
        raise ValueError(f"{path}: not a PLY file (no 'ply' line)")
    fmt, elements = None, []
    while True:
        raw = f.readline()
        if not raw:
            raise ValueError(f"{path}: the PLY header has no end_header")
        tok = raw.decode("ascii", "replace").split()
        if not tok or tok[0] in ("comment", "obj_info"):
            continue
        if tok[0] == "end_header":
            break
        try:
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                elements.append((tok[1], int(tok[2]), []))
            elif tok[0] == "property":
                if not elements:
                    raise ValueError(f"{path}: a PLY property before any element")
                if tok[1] == "list":
                    elements[-1][2].append((tok[4], _PLY_TYPES[tok[2]], _PLY_TYPES[tok[3]]))
                else:
                    elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]]))
        except (IndexError, KeyError):
            raise ValueError(f"{path}: cannot read the PLY header line {raw.decode('ascii', 'replace').strip()!r}") from None
    if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
        raise ValueError(f"{path}: PLY format {fmt!r} (known: ascii, binary_little_endian, binary_big_endian)")
    return fmt, elements


def _parse_ply(path: str, want_faces: bool) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    with open(path, "rb") as f:
        fmt, elements = _ply_header(path, f)
        body = f.read()
    verts, polygons, tris = None, None, None
    order = {"binary_little_endian": "<", "binary_big_endian": ">"}.get(fmt)
    tokens, pos = (body.split(), 0) if order is None else (None, 0)
    for name, count, props in elements:
        scalar = all(len(p) == 2 for p in props)
        if order is not None and scalar:  # a fixed-size record: one structured read
            dt = np.dtype([(f"{i}:{p[0]}", order + p[1]) for i, p in enumerate(props)])
            if pos + count * dt.itemsize > len(body):
                raise ValueError(f"{path}: the file ends inside element {name!r}")
            rec = np.frombuffer(body, dtype=dt, count=count, offset=pos)
            pos += count * dt.itemsize
            cols = {p[0]: rec[f"{i}:{p[0]}"] for i, p in enumerate(props)}
            lists = {}
        else:
            cols = {p[0]: [] for p in props if len(p) == 2}
            lists = {p[0]: [] for p in props if len(p) == 3}
            wanted = name == "vertex" or (name == "face" and want_faces)
            if order is not None and name == "face" and len(props) == 1 and count > 0:
                # the usual face element, one list and nothing else: when every list has the first one's length, one strided read
                _, ct, it = props[0]
                cdt, idt = np.dtype(order + ct), np.dtype(order + it)
                if pos + cdt.itemsize > len(body):
                    raise ValueError(f"{path}: the file ends inside element {name!r}")
                n0 = int(np.frombuffer(body, dtype=cdt, count=1, offset=pos)[0])
                dt = np.dtype([("n", cdt), ("i", idt, (n0,))]) if n0 > 0 else None
                if dt is not None and pos + count * dt.itemsize <= len(body):
                    rec = np.frombuffer(body, dtype=dt, count=count, offset=pos)
                    if bool((rec["n"] == n0).all()) and n0 >= 3:
                        pos += count * dt.itemsize
                        idx = rec["i"].astype(np.int64)
                        if wanted:
                            tris = np.stack([np.stack([idx[:, 0], idx[:, i], idx[:, i + 1]], 1) for i in range(1, n0 - 1)], 1).reshape(-1, 3)
                        continue
            for _ in range(count):
                for p in props:
                    if len(p) == 2:
                        if order is None:
                            if pos >= len(tokens):
                                raise ValueError(f"{path}: the file ends inside element {name!r}")
                            v = float(tokens[pos]) if p[1][0] == "f" else int(float(tokens[pos]))
                            pos += 1
                        else:
                            dt = np.dtype(order + p[1])
                            if pos + dt.itemsize > len(body):
                                raise ValueError(f"{path}: the file ends inside element {name!r}")
                            v = np.frombuffer(body, dtype=dt, count=1, offset=pos)[0]
                            pos += dt.itemsize
                        if wanted:
                            cols[p[0]].append(v)
                    else:
                        if order is None:
                            if pos >= len(tokens):
                                raise ValueError(f"{path}: the file ends inside element {name!r}")
                            n = int(float(tokens[pos]))
                            if n < 0 or pos + 1 + n > len(tokens):
                                raise ValueError(f"{path}: the file ends inside element {name!r}")
                            item = [int(float(t)) for t in tokens[pos + 1: pos + 1 + n]]
                            pos += 1 + n
                        else:
                            cdt, idt = np.dtype(order + p[1]), np.dtype(order + p[2])
                            if pos + cdt.itemsize > len(body):
                                raise ValueError(f"{path}: the file ends inside element {name!r}")
                            n = int(np.frombuffer(body, dtype=cdt, count=1, offset=pos)[0])
                            pos += cdt.itemsize
                            if n < 0 or pos + n * idt.itemsize > len(body):
                                raise ValueError(f"{path}: the file ends inside element {name!r}")
                            item = np.frombuffer(body, dtype=idt, count=n, offset=pos).astype(np.int64).tolist()
                            pos += n * idt.itemsize
                        if wanted:
                            lists[p[0]].append(item)
        if name == "vertex":
            if not all(k in cols for k in "xyz"):
                raise ValueError(f"{path}: the PLY vertex element has no x, y, z")
            verts = np.stack([np.asarray(cols[k], dtype=np.float64) for k in "xyz"], 1).reshape(-1, 3)
        elif name == "face" and want_faces:
            key = next((k for k in _PLY_INDEX_NAMES if k in lists), None)
            if key is not None:
                for n, poly in enumerate(lists[key]):
                    if len(poly) < 3:
                        raise ValueError(f"{path}: face {n} has {len(poly)} vertices")
                polygons = lists[key]
    if verts is None:
        raise ValueError(f"{path}: the PLY file has no vertex element")
    if tris is None and polygons is not None:
        tris = _fan(polygons)
    return verts, tris


# ---------------------------------------------------------------------------------------------------------------------------------
# STL
# ---------------------------------------------------------------------------------------------------------------------------------
_STL_RECORD = np.dtype([("n", "<f4", (3,)), ("v", "<f4", (3, 3)), ("attr", "<u2")])


def _merge_by_bits(corners: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """corners (3F, 3) float32 -> (verts, faces): corners with equal coordinate BITS become one vertex, numbered by first occurrence
    (so -0.0 and 0.0 stay apart, and a NaN, refused later, equals itself)"""
    bits = np.ascontiguousarray(corners, dtype=np.float32).view(np.uint32).reshape(-1, 3)
    if bits.shape[0] == 0:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int64)
    _, first, inverse = np.unique(bits, axis=0, return_index=True, return_inverse=True)
    rank = np.empty(first.shape[0], dtype=np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(first.shape[0])
    verts = bits[np.sort(first)].view(np.float32)
    return verts, rank[np.asarray(inverse).reshape(-1)].reshape(-1, 3)


def _parse_stl(path: str) -> Tuple[np.ndarray, np.ndarray]:
    size = os.path.getsize(path)
    with open(path, "rb") as f:
        data = f.read()
    if size >= 84:
        n = struct.unpack_from("<I", data, 80)[0]
        if 84 + 50 * n == size:  # binary, whatever the header's first word
            rec = np.frombuffer(data, dtype=_STL_RECORD, count=n, offset=84)
            return _merge_by_bits(rec["v"].reshape(-1, 3))
    tok = data.decode("ascii", "replace").split()
    if not tok or tok[0] != "solid":
        raise ValueError(f"{path}: neither a binary STL (80 + 4 + 50 n bytes) nor an ascii one (no 'solid')")
    corners = []
    for i, t in enumerate(tok):
        if t == "vertex":
            try:
                corners.append([np.float32(tok[i + 1]), np.float32(tok[i + 2]), np.float32(tok[i + 3])])
            except (IndexError, ValueError):
                raise ValueError(f"{path}: cannot read vertex {len(corners)} of the ascii STL") from None
    if len(corners) % 3:
        raise ValueError(f"{path}: {len(corners)} vertices in the ascii STL, no multiple of 3")
    return _merge_by_bits(np.asarray(corners, dtype=np.float32).reshape(-1, 3))


# ---------------------------------------------------------------------------------------------------------------------------------
# the public readers
# ---------------------------------------------------------------------------------------------------------------------------------
def _checked_verts(path: str, verts) -> np.ndarray:
    with np.errstate(over="ignore"):
        v = np.ascontiguousarray(np.asarray(verts).reshape(-1, 3), dtype=np.float32)
    bad = np.flatnonzero(~np.isfinite(v).all(1))
    if bad.size:
        raise ValueError(f"{path}: vertex {int(bad[0])} is not finite ({v[bad[0]].tolist()})")
    return v


def read_mesh(path) -> Tuple[np.ndarray, np.ndarray]:
    """(verts float32 (V, 3), faces int32 (F, 3)) of an .obj, .ply or .stl file"""
    path = os.fspath(path)
    ext = os.path.splitext(path)[1].lower()
    if ext == ".obj":
        verts, faces = _parse_obj(path)
    elif ext == ".ply":
        verts, faces = _parse_ply(path, want_faces=True)
    elif ext == ".stl":
        verts, faces = _parse_stl(path)
    else:
        raise ValueError(f"{path}: unknown mesh format {ext!r} (known: {', '.join(MESH_EXTENSIONS)})")
    verts = _checked_verts(path, verts)
    if faces is None or len(faces) == 0:
        raise ValueError(f"{path}: the file has no faces ({verts.shape[0]} vertices): read a point set with read_points")
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    bad = np.flatnonzero(((faces < 0) | (faces >= verts.shape[0])).any(1))
    if bad.size:
        raise ValueError(f"{path}: face {int(bad[0])} = {faces[bad[0]].tolist()} has an index outside [0, {verts.shape[0]})")
    return verts, np.ascontiguousarray(faces, dtype=np.int32)


def read_points(path) -> np.ndarray:
    """float32 (N, 3): the vertices of a .ply or .obj (with or without faces), a .npy (N, 3), or the "point" entry of an .npz (its
    first three columns: an (N, 6) cloud carries normals or colours behind them)"""
    path = os.fspath(path)
    ext = os.path.splitext(path)[1].lower()
    if ext == ".obj":
        pts = _parse_obj(path)[0]
    elif ext == ".ply":
        pts = _parse_ply(path, want_faces=False)[0]
    elif ext == ".npy":
        pts = np.load(path, allow_pickle=False)
    elif ext == ".npz":
        with np.load(path, allow_pickle=False) as z:
            if "point" not in z.files:
                raise ValueError(f"{path}: no 'point' entry (has: {z.files})")
            pts = z["point"]
    else:
        raise ValueError(f"{path}: unknown point format {ext!r} (known: .ply, .obj, .npy, .npz)")
    pts = np.asarray(pts)
    if ext in (".npy", ".npz"):
        if pts.ndim != 2 or pts.shape[1] not in (3, 6) or (ext == ".npy" and pts.shape[1] != 3):
            raise ValueError(f"{path}: expected an (N, 3) array, got {pts.shape}")
        pts = pts[:, :3]
    pts = _checked_verts(path, pts)
    if pts.shape[0] == 0:
        raise ValueError(f"{path}: the file has no points")
    return pts


# ---------------------------------------------------------------------------------------------------------------------------------
# writers
# ---------------------------------------------------------------------------------------------------------------------------------
def _mesh_arrays(verts, faces):
    v = np.ascontiguousarray(np.asarray(verts, dtype=np.float32).reshape(-1, 3))
    f = np.zeros((0, 3), np.int32) if faces is None else np.ascontiguousarray(np.asarray(faces, dtype=np.int32).reshape(-1, 3))
    return v, f


def write_obj(path, verts, faces=None) -> None:
    """`v` and `f` lines; every float32 coordinate is written with 9 significant digits, which reads back to the same bits"""
    v, f = _mesh_arrays(verts, faces)
    with open(os.fspath(path), "w") as out:
        out.write("".join("v %.9g %.9g %.9g\n" % tuple(float(c) for c in row) for row in v))
        out.write("".join("f %d %d %d\n" % tuple(int(i) + 1 for i in row) for row in f))


def write_ply(path, verts, faces=None, binary: bool = True, big_endian: bool = False) -> None:
    """float x y z and `list uchar int vertex_indices`; binary little-endian by default"""
    v, f = _mesh_arrays(verts, faces)
    fmt = "ascii" if not binary else "binary_big_endian" if big_endian else "binary_little_endian"
    head = f"ply\nformat {fmt} 1.0\nelement vertex {v.shape[0]}\nproperty float x\nproperty float y\nproperty float z\n"
    if f.shape[0]:
        head += f"element face {f.shape[0]}\nproperty list uchar int vertex_indices\n"
    head += "end_header\n"
    with open(os.fspath(path), "wb") as out:
        out.write(head.encode("ascii"))
        if not binary:
            out.write("".join("%.9g %.9g %.9g\n" % tuple(float(c) for c in row) for row in v).encode("ascii"))
            out.write("".join("3 %d %d %d\n" % tuple(int(i) for i in row) for row in f).encode("ascii"))
            return
        o = ">" if big_endian else "<"
        out.write(v.astype(o + "f4").tobytes())
        rec = np.empty(f.shape[0], dtype=np.dtype([("n", "u1"), ("i", o + "i4", (3,))]))
        rec["n"], rec["i"] = 3, f
        out.write(rec.tobytes())


def write_stl(path, verts, faces, binary: bool = True, header: bytes = b"") -> None:
    """one facet per face with its unit normal (zero for a degenerate face); `header`: the first of the 80 header bytes"""
    v, f = _mesh_arrays(verts, faces)
    tri = v[f]  # (F, 3, 3)
    c = np.cross(tri[:, 1].astype(np.float64) - tri[:, 0], tri[:, 2].astype(np.float64) - tri[:, 0])
    norm = np.sqrt((c * c).sum(1, keepdims=True))
    normal = np.divide(c, norm, out=np.zeros_like(c), where=norm > 0).astype(np.float32)
    if binary:
        rec = np.zeros(f.shape[0], dtype=_STL_RECORD)
        rec["n"], rec["v"] = normal, tri
        with open(os.fspath(path), "wb") as out:
            out.write(bytes(header[:80]).ljust(80, b"\0") + struct.pack("<I", f.shape[0]) + rec.tobytes())
        return
    with open(os.fspath(path), "w") as out:
        out.write("solid mesh\n")
        for n, t in zip(normal, tri):
            out.write("facet normal %.9g %.9g %.9g\n outer loop\n" % tuple(float(x) for x in n))
            out.write("".join("  vertex %.9g %.9g %.9g\n" % tuple(float(x) for x in p) for p in t))
            out.write(" endloop\nendfacet\n")
        out.write("endsolid mesh\n")


# ---------------------------------------------------------------------------------------------------------------------------------
# report
# ---------------------------------------------------------------------------------------------------------------------------------
def face_areas(verts, faces) -> np.ndarray:
    """float64 (F,): 0.5 |(v1 - v0) x (v2 - v0)|"""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    c = np.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]])
    return 0.5 * np.sqrt((c * c).sum(1))


def mesh_report(verts, faces) -> Dict:
    """What a mesh is, before anything is sampled from it or voxelised: n_verts, n_faces, n_degenerate_faces (a repeated index or zero
    area), n_unreferenced_verts, n_boundary_edges (used once), n_nonmanifold_edges (used more than twice), closed (every edge of every
    face is used exactly twice), area (float64, the sum over the faces) and bbox ([[min x, y, z], [max x, y, z]], float64)"""
    v = np.asarray(verts, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError(f"mesh_report: a face index lies outside [0, {v.shape[0]})")
    area = face_areas(v, f)
    repeated = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])
    edges = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    edges = edges[edges[:, 0] != edges[:, 1]]  # (the collapsed edge of a repeated index is no edge)
    uses = np.unique(edges, axis=0, return_counts=True)[1] if edges.shape[0] else np.zeros(0, np.int64)
    referenced = np.zeros(v.shape[0], dtype=bool)
    referenced[f.reshape(-1)] = True
    return {
        "n_verts": int(v.shape[0]), "n_faces": int(f.shape[0]), "n_degenerate_faces": int((repeated | ~(area > 0)).sum()),
        "n_unreferenced_verts": int((~referenced).sum()), "n_boundary_edges": int((uses == 1).sum()),
        "n_nonmanifold_edges": int((uses > 2).sum()), "closed": bool(f.shape[0] > 0 and uses.size > 0 and (uses == 2).all()),
        "area": float(area.sum()), "bbox": [v.min(0).tolist(), v.max(0).tolist()] if v.shape[0] else None,
    }


# ---------------------------------------------------------------------------------------------------------------------------------
# a directory of objects
# ---------------------------------------------------------------------------------------------------------------------------------
def resolve_object_file(prefix, obj_id: str, extensions=MESH_EXTENSIONS) -> str:
    """<prefix>/<obj_id>.<ext>, else the single file with one of `extensions` inside <prefix>/<obj_id>/ (OakInk2's object directory
    keeps one directory per object).  Several candidates, or none, is a ValueError that lists them."""
    prefix = os.fspath(prefix)
    flat = [p for p in (os.path.join(prefix, obj_id + e) for e in extensions) if os.path.isfile(p)]
    sub = os.path.join(prefix, obj_id)
    inner = sorted(os.path.join(sub, n) for n in os.listdir(sub)
                   if os.path.splitext(n)[1].lower() in extensions and os.path.isfile(os.path.join(sub, n))) if os.path.isdir(sub) else []
    found = flat + inner
    if len(found) == 1:
        return found[0]
    if not found:
        raise ValueError(f"object {obj_id!r}: no file under {prefix} (looked for {obj_id}{{{','.join(extensions)}}} and a single such file in {obj_id}/)")
    raise ValueError(f"object {obj_id!r}: {len(found)} candidates under {prefix}, keep one: {found}")


def list_object_ids(prefix, extensions=MESH_EXTENSIONS) -> List[str]:
    """the ids `resolve_object_file` would look up under `prefix`, sorted: files by their stem, directories that hold such a file"""
    prefix = os.fspath(prefix)
    ids = set()
    for n in os.listdir(prefix):
        p = os.path.join(prefix, n)
        if os.path.isfile(p) and os.path.splitext(n)[1].lower() in extensions:
            ids.add(os.path.splitext(n)[0])
        elif os.path.isdir(p) and any(os.path.splitext(m)[1].lower() in extensions for m in os.listdir(p)):
            ids.add(n)
    return sorted(ids)


def directory_loader(prefix) -> Callable[[str], Tuple[np.ndarray, np.ndarray]]:
    """load(obj_id) -> (verts, faces) of the object's mesh file under `prefix` (resolve_object_file), read once per id.  What
    `--data.obj_mesh_prefix` hands to the dataset as its obj_model_loader."""
    prefix = os.path.abspath(os.fspath(prefix))
    cache: Dict[str, Tuple[np.ndarray, np.ndarray]] = {}

    def load(obj_id):
        key = str(obj_id)
        if key not in cache:
            cache[key] = read_mesh(resolve_object_file(prefix, key))
        return cache[key]

    load.prefix = prefix
    load.cache = cache
    return load


__all__ = ["MESH_EXTENSIONS", "read_mesh", "read_points", "write_obj", "write_ply", "write_stl", "face_areas", "mesh_report",
           "resolve_object_file", "list_object_ids", "directory_loader"]
