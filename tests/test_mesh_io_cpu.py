"""oakink2_tamf_amd/mesh_io.py: the mesh and point readers against files the tests write themselves (write_obj / write_ply / write_stl
and hand-written text), every refusal, mesh_report and directory_loader.  CPU only, numpy only."""
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oakink2-tamf_amd")]

from oakink2_tamf_amd import mesh_io as M  # noqa: E402

# coordinates that need all 24 bits of a float32 mantissa, so a text round trip that loses a digit shows
TETRA_V = np.array([[0.1, 0.2, 0.3], [1.0 / 3.0, -0.7, 0.25], [-0.123456789, 0.987654321, 1e-3], [2.5e-7, 3.0, -1.0 / 7.0]], dtype=np.float32)
TETRA_F = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], dtype=np.int32)
CUBE_V = (np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], dtype=np.float32) * np.float32(0.1) + np.float32(1.0 / 3.0)).astype(np.float32)
# vertex index = 4x + 2y + z; two triangles per side, outward
CUBE_F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]],
                  dtype=np.int32)
MESHES = {"tetra": (TETRA_V, TETRA_F), "cube": (CUBE_V, CUBE_F)}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _write(fmt, path, v, f):
    if fmt == "obj":
        M.write_obj(path, v, f)
    elif fmt == "ply_ascii":
        M.write_ply(path, v, f, binary=False)
    elif fmt == "ply_le":
        M.write_ply(path, v, f)
    elif fmt == "ply_be":
        M.write_ply(path, v, f, big_endian=True)
    elif fmt == "stl_bin":
        M.write_stl(path, v, f)
    else:
        M.write_stl(path, v, f, binary=False)


EXT = {"obj": ".obj", "ply_ascii": ".ply", "ply_le": ".ply", "ply_be": ".ply", "stl_bin": ".stl", "stl_ascii": ".stl"}


@pytest.mark.parametrize("mesh", sorted(MESHES))
@pytest.mark.parametrize("fmt", sorted(EXT))
def test_round_trip(tmp_path, fmt, mesh):
    v, f = MESHES[mesh]
    path = str(tmp_path / ("m" + EXT[fmt]))
    _write(fmt, path, v, f)
    rv, rf = M.read_mesh(path)
    assert rv.dtype == np.float32 and rf.dtype == np.int32 and rv.shape == (len(v), 3) and rf.shape == (len(f), 3)
    if fmt.startswith("stl"):
        # an STL holds corners: vertices come back merged by their bits, numbered by first occurrence over the faces
        order = list(dict.fromkeys(f.reshape(-1).tolist()))
        assert np.array_equal(_bits(rv), _bits(v[order]))
        assert np.array_equal(np.asarray(order)[rf], f)
    else:
        assert np.array_equal(_bits(rv), _bits(v))  # (9 significant digits carry a float32 through text, so the ascii forms too)
        assert np.array_equal(rf, f)


def test_obj_quads_slash_forms_and_negative_indices(tmp_path):
    p = tmp_path / "q.obj"
    p.write_text("# a comment\nmtllib x.mtl\no thing\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0 0\nvn 0 0 1\ng grp\nusemtl m\ns off\n"
                 "f 1/1/1 2/1/1 3/1/1 4/1/1\n"     # a quad -> (0,1,2) (0,2,3)
                 "v 0.5 0.5 1\n"
                 "f -1 -5 -4\n"                    # relative to the 5 vertices read so far -> (4, 0, 1)
                 "f 2//1 3//1 5//1\n"
                 "f 1/1 2/1 3/1 4/1 5/1\n"         # a pentagon -> three triangles from vertex 0
                 "l 1 2\n")
    v, f = M.read_mesh(str(p))
    assert v.shape == (5, 3) and v[4].tolist() == [0.5, 0.5, 1.0]
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [4, 0, 1], [1, 2, 4], [0, 1, 2], [0, 2, 3], [0, 3, 4]]


@pytest.mark.parametrize("order", ["ascii", "<", ">"])
def test_ply_with_extra_properties_and_other_list_types(tmp_path, order):
    """vertex: double x, a uchar colour between the coordinates, short z; face: an int count with uchar items, named vertex_index,
    behind a float property of the face; a third element after them"""
    v = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [2.0, 2.0, 3.0], [0.0, 2.0, -3.0]])
    polys = [[0, 1, 2, 3], [0, 2, 3]]
    fmt = {"ascii": "ascii", "<": "binary_little_endian", ">": "binary_big_endian"}[order]
    head = (f"ply\nformat {fmt} 1.0\ncomment made by hand\nelement vertex 4\nproperty double x\nproperty uchar red\nproperty float y\n"
            "property short z\nelement face 2\nproperty float quality\nproperty list int uchar vertex_index\nelement edge 1\nproperty int a\nend_header\n")
    body = b""
    if order == "ascii":
        body += "".join(f"{x} 200 {y} {int(z)}\n" for x, y, z in v).encode()
        body += "".join(f"0.5 {len(p)} " + " ".join(map(str, p)) + "\n" for p in polys).encode()
        body += b"7\n"
    else:
        for x, y, z in v:
            body += struct.pack(order + "dBfh", x, 200, y, int(z))
        for p in polys:
            body += struct.pack(order + "fi", 0.5, len(p)) + bytes(p)
        body += struct.pack(order + "i", 7)
    path = tmp_path / "e.ply"
    path.write_bytes(head.encode() + body)
    rv, rf = M.read_mesh(str(path))
    assert np.array_equal(rv, v.astype(np.float32))
    assert rf.tolist() == [[0, 1, 2], [0, 2, 3], [0, 2, 3]]
    assert np.array_equal(M.read_points(str(path)), v.astype(np.float32))


def test_binary_stl_whose_header_begins_with_solid(tmp_path):
    path = str(tmp_path / "s.stl")
    M.write_stl(path, TETRA_V, TETRA_F, header=b"solid made by a program that does not mind")
    with open(path, "rb") as f:
        assert f.read(5) == b"solid"
    v, f = M.read_mesh(path)
    assert v.shape == (4, 3) and f.shape == (4, 3)
    assert np.array_equal(_bits(v[f]), _bits(TETRA_V[TETRA_F]))


def test_stl_merges_by_bits_not_by_value(tmp_path):
    v = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [-0.0, 0, 0], [0, 1, 0], [1, 0, 0]], dtype=np.float32)
    path = str(tmp_path / "z.stl")
    M.write_stl(path, v, [[0, 1, 2], [3, 4, 5]])
    rv, rf = M.read_mesh(path)
    assert rv.shape == (4, 3) and rf.tolist() == [[0, 1, 2], [3, 2, 1]]  # -0.0 is a vertex of its own; the others are shared
    assert np.signbit(rv[3, 0]) and not np.signbit(rv[0, 0])


def test_refusals(tmp_path):
    def obj(name, text):
        p = tmp_path / name
        p.write_text(text)
        return str(p)

    with pytest.raises(ValueError, match=r"nan\.obj: vertex 1 is not finite"):
        M.read_mesh(obj("nan.obj", "v 0 0 0\nv nan 0 0\nv 0 1 0\nf 1 2 3\n"))
    with pytest.raises(ValueError, match=r"inf\.obj: vertex 2 is not finite"):
        M.read_mesh(obj("inf.obj", "v 0 0 0\nv 1 0 0\nv 0 1e60 0\nf 1 2 3\n"))  # (finite as text, not as a float32)
    with pytest.raises(ValueError, match=r"big\.obj: face 1 = \[0, 1, 3\] has an index outside \[0, 3\)"):
        M.read_mesh(obj("big.obj", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\nf 1 2 4\n"))
    with pytest.raises(ValueError, match=r"neg\.obj: face 0 .* outside \[0, 3\)"):
        M.read_mesh(obj("neg.obj", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf -1 -2 -4\n"))
    with pytest.raises(ValueError, match=r"zero\.obj:4: face index 0"):
        M.read_mesh(obj("zero.obj", "v 0 0 0\nv 1 0 0\nv 0 1 0\nf 0 1 2\n"))
    with pytest.raises(ValueError, match=r"pts\.obj: the file has no faces \(3 vertices\).*read_points"):
        M.read_mesh(obj("pts.obj", "v 0 0 0\nv 1 0 0\nv 0 1 0\n"))
    ply = str(tmp_path / "pts.ply")
    M.write_ply(ply, TETRA_V)
    with pytest.raises(ValueError, match=r"pts\.ply: the file has no faces.*read_points"):
        M.read_mesh(ply)
    bad = str(tmp_path / "bad.ply")
    M.write_ply(bad, TETRA_V, [[0, 1, 4]])
    with pytest.raises(ValueError, match=r"bad\.ply: face 0 = \[0, 1, 4\]"):
        M.read_mesh(bad)
    short = tmp_path / "short.ply"
    with open(ply, "rb") as f:
        short.write_bytes(f.read()[:-5])
    with pytest.raises(ValueError, match=r"short\.ply: the file ends inside element 'vertex'"):
        M.read_points(str(short))
    junk = tmp_path / "junk.stl"
    junk.write_bytes(b"\1" * 100)
    with pytest.raises(ValueError, match=r"junk\.stl: neither a binary STL"):
        M.read_mesh(str(junk))
    with pytest.raises(ValueError, match="unknown mesh format"):
        M.read_mesh(str(tmp_path / "x.off"))


def test_read_points(tmp_path):
    M.write_ply(str(tmp_path / "a.ply"), TETRA_V)
    M.write_obj(str(tmp_path / "a.obj"), TETRA_V)
    M.write_ply(str(tmp_path / "withfaces.ply"), CUBE_V, CUBE_F, binary=False)
    np.save(str(tmp_path / "a.npy"), TETRA_V.astype(np.float64))
    np.savez(str(tmp_path / "a.npz"), point=TETRA_V)
    np.savez(str(tmp_path / "six.npz"), point=np.concatenate([TETRA_V, TETRA_V], 1))
    for name in ("a.ply", "a.obj", "a.npy", "a.npz", "six.npz"):
        p = M.read_points(str(tmp_path / name))
        assert p.dtype == np.float32 and np.array_equal(_bits(p), _bits(TETRA_V)), name
    assert np.array_equal(M.read_points(str(tmp_path / "withfaces.ply")), CUBE_V)
    np.save(str(tmp_path / "flat.npy"), np.zeros(9))
    with pytest.raises(ValueError, match=r"flat\.npy: expected an \(N, 3\) array"):
        M.read_points(str(tmp_path / "flat.npy"))
    np.savez(str(tmp_path / "other.npz"), cloud=TETRA_V)
    with pytest.raises(ValueError, match=r"other\.npz: no 'point' entry"):
        M.read_points(str(tmp_path / "other.npz"))
    with pytest.raises(ValueError, match="unknown point format"):
        M.read_points(str(tmp_path / "a.stl"))


def test_mesh_report():
    r = M.mesh_report(CUBE_V, CUBE_F)
    assert (r["n_verts"], r["n_faces"], r["n_degenerate_faces"], r["n_unreferenced_verts"], r["n_boundary_edges"], r["n_nonmanifold_edges"]) == (8, 12, 0, 0, 0, 0)
    assert r["closed"] is True
    side = float(CUBE_V[7, 0]) - float(CUBE_V[0, 0])
    assert abs(r["area"] - 6 * side * side) < 1e-12 and isinstance(r["area"], float)
    assert np.array_equal(np.asarray(r["bbox"]), np.stack([CUBE_V.min(0), CUBE_V.max(0)]).astype(np.float64))
    # the x = 0 side removed: its four outer edges are used once, its diagonal not at all
    r = M.mesh_report(CUBE_V, CUBE_F[2:])
    assert (r["n_faces"], r["n_boundary_edges"], r["n_nonmanifold_edges"], r["closed"]) == (10, 4, 0, False)
    # a repeated-index face, a zero-area face of distinct indices (three points on a line), an unreferenced vertex, a fin
    v = np.concatenate([CUBE_V, [[9, 9, 9]], [(CUBE_V[0] + CUBE_V[1]) / 2]]).astype(np.float32)
    f = np.concatenate([CUBE_F, [[0, 0, 1]], [[0, 9, 1]], [[0, 1, 7]]])
    r = M.mesh_report(v, f)
    assert (r["n_verts"], r["n_faces"], r["n_degenerate_faces"], r["n_unreferenced_verts"]) == (10, 15, 2, 1)
    assert r["n_nonmanifold_edges"] >= 1 and r["closed"] is False
    with pytest.raises(ValueError, match="outside"):
        M.mesh_report(CUBE_V, [[0, 1, 8]])


def test_directory_loader_on_both_layouts(tmp_path):
    M.write_obj(str(tmp_path / "O01.obj"), TETRA_V, TETRA_F)
    (tmp_path / "O02").mkdir()
    M.write_ply(str(tmp_path / "O02" / "scan_model.ply"), CUBE_V, CUBE_F)
    (tmp_path / "O02" / "texture.png").write_bytes(b"x")
    (tmp_path / "O03").mkdir()
    M.write_stl(str(tmp_path / "O03" / "a.stl"), TETRA_V, TETRA_F)
    M.write_obj(str(tmp_path / "O03" / "b.obj"), TETRA_V, TETRA_F)
    M.write_obj(str(tmp_path / "O04.obj"), TETRA_V, TETRA_F)
    M.write_ply(str(tmp_path / "O04.ply"), TETRA_V, TETRA_F)
    (tmp_path / "notes.txt").write_text("x")
    assert M.list_object_ids(str(tmp_path)) == ["O01", "O02", "O03", "O04"]
    load = M.directory_loader(str(tmp_path))
    v, f = load("O01")
    assert np.array_equal(v, TETRA_V) and np.array_equal(f, TETRA_F)
    v, f = load("O02")
    assert np.array_equal(v, CUBE_V) and np.array_equal(f, CUBE_F)
    assert load("O02")[0] is v  # cached per id
    os.remove(str(tmp_path / "O01.obj"))
    assert load("O01")[1] is load("O01")[1]  # (still served from the cache)
    with pytest.raises(ValueError, match=r"'O03': 2 candidates .*a\.stl.*b\.obj"):
        load("O03")
    with pytest.raises(ValueError, match=r"'O04': 2 candidates .*O04\.obj.*O04\.ply"):
        load("O04")
    with pytest.raises(ValueError, match=r"'O05': no file under"):
        load("O05")
