"""CPU: the layered restatement (tests/render_layers_restatement.py) against its own invariants and against the single-layer restatement,
the near-tie share that tests/test_render_layers_gpu.py may exclude (asserted here for every scene it peels), composite and resolve on
cases worked by hand, render.contact_colors at its breakpoints, the animated PNG writer, and the launcher's new flags in a dry run."""
import json
import os
import re
import struct
import sys
import zlib

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_layers_restatement as LR  # noqa: E402
import render_restatement as R  # noqa: E402
import render_scenes as S  # noqa: E402


# ---- peeling ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LR.NAMES)
def test_layers_are_the_sorted_candidates_and_near_ties_stay_under_the_cap(name):
    """layer 0 is the single-layer restatement; (depth, id) strictly increases over the layers; layer k is covered exactly where the pixel
    has more than k candidates; pixels with a near tie among their first K + 1 candidates are at most 0.5 % of the covered ones"""
    ref = LR.reference(name)
    sc, lay = ref["scene"], ref["layers"]
    buf = S.draw(sc, [(p, xy) for p, xy, _ in ref["proj"]])
    assert np.array_equal(lay.prim_id[0], buf.prim_id) and np.array_equal(lay.depth[0], buf.depth)
    assert np.array_equal(lay.count, buf.cover)
    for k in range(LR.K):
        covered = lay.prim_id[k] >= 0
        assert np.array_equal(covered, lay.count > k) and np.isinf(lay.depth[k][~covered]).all()
        if k:
            both = covered
            d0, d1, i0, i1 = lay.depth[k - 1][both], lay.depth[k][both], lay.prim_id[k - 1][both], lay.prim_id[k][both]
            assert ((d1 > d0) | ((d1 == d0) & (i1 > i0))).all()
            assert (lay.prim_id[k - 1][covered] >= 0).all()  # no layer without the one before it
    covered = int((lay.count > 0).sum())
    share = lay.near_tie_share()
    print(f"RENDER layers scene {name}: covered {covered}, per layer {[int((lay.prim_id[k] >= 0).sum()) for k in range(LR.K)]}, "
          f"near ties {int(lay.near_tie.sum())} share {share:.5f}")
    assert covered > 100 and (lay.prim_id[LR.K - 1] >= 0).sum() > 0 and share <= 0.005


def test_shells_hold_four_fragments_from_different_calls():
    ref = LR.reference("shells")
    sc, lay = ref["scene"], ref["layers"]
    ends = np.cumsum(S.counts(sc))
    item = np.where(lay.prim_id >= 0, np.searchsorted(ends, lay.prim_id, side="right"), -1)  # (K,F,H,W)
    deep = lay.count >= 4
    three = np.array([len(set(item[:, f, j, i])) == 3 for f, j, i in zip(*np.nonzero(deep))])
    alternating = (item[0] != item[1]) & (item[1] != item[2]) & deep
    print(f"RENDER shells: {int(deep.sum())} pixels with >= 4 fragments, {int(three.sum())} of them from all three calls, most {int(lay.count.max())}")
    assert deep.sum() > 200 and three.sum() > 100 and alternating.sum() > 100 and lay.count.max() >= 8


def test_points_mesh_mixes_splats_and_triangles_in_one_pixel():
    ref = LR.reference("points_mesh")
    sc, lay = ref["scene"], ref["layers"]
    b = S.bases(sc)
    is_mesh = (lay.prim_id >= b[1]) & (lay.prim_id < b[2])
    is_point = (lay.prim_id >= 0) & ~is_mesh
    assert (is_mesh.any(axis=0) & is_point.any(axis=0)).sum() > 50
    assert (is_point[0] & is_mesh[1]).sum() > 5 and (is_mesh[0] & is_point[1]).sum() > 5  # in front of the sphere, and inside or behind it


def test_exact_ties_resolve_to_the_lower_id_then_the_higher():
    cam = R.camera(32, 32)
    tri = np.array([[-1.0, -1.0, 3.0], [1.0, -1.0, 3.0], [0.0, 1.2, 3.3]])
    sc = dict(W=32, H=32, F=1, cam=cam, items=[dict(kind="mesh", verts=tri, faces=np.array([[0, 1, 2]], np.int32), model=None),
                                               dict(kind="mesh", verts=tri, faces=np.array([[0, 2, 1]], np.int32), model=None)])
    proj = S.project_items(sc)
    lay = LR.Layers(LR.collect(sc, [(p, xy) for p, xy, _ in proj]), 3)
    m = lay.prim_id[0] >= 0
    assert m.sum() > 50 and (lay.prim_id[0][m] == 0).all() and (lay.prim_id[1][m] == 1).all() and (lay.prim_id[2] == -1).all()
    assert np.array_equal(lay.depth[0], lay.depth[1]) and np.array_equal(lay.prim_id[1] >= 0, m)
    assert lay.near_tie[m].all()  # an exact tie is a near tie


# ---- composite and resolve ----------------------------------------------------------------------------------------------------------
def test_composite_by_hand():
    ids = np.array([[0, 0, 5, -1, 7], [5, -1, 0, -1, -1]], np.int64).reshape(2, 1, 1, 5)
    rgb = np.zeros((2, 1, 1, 5, 3), np.uint8)
    rgb[0, ..., :] = [[200, 100, 0]] * 5
    rgb[1, ..., :] = [[0, 50, 250]] * 5
    out, C = LR.composite(rgb, ids, [0, 5], [5, 3], [0.25, 1.0], (0.2, 0.4, 0.6))
    bg = np.array([0.2, 0.4, 0.6])
    front, back = np.array([200, 100, 0]) / 255.0, np.array([0, 50, 250]) / 255.0
    want = [0.25 * front + 0.75 * back,  # see-through item 0 over opaque item 1
            0.25 * front + 0.75 * bg,  # over the background
            back * 0 + front * 0 + np.array([200, 100, 0]) / 255.0,  # an alpha-1 item hides what lies behind it
            bg, front]
    assert np.allclose(C[0, 0], want, atol=1e-15)
    assert np.array_equal(out[0, 0], R.to_byte(np.array(want)))
    one, _ = LR.composite(rgb[:1], ids[:1], [0, 5], [5, 3], [1.0, 1.0], (0.2, 0.4, 0.6))
    assert np.array_equal(one[0, 0, [0, 1, 2, 4]], rgb[0, 0, 0, [0, 1, 2, 4]]) and np.array_equal(one[0, 0, 3], R.to_byte(bg))


def test_resolve_by_hand():
    for s in (2, 3, 4):
        const = np.full((2, 3 * s, 5 * s, 3), 137, np.uint8)
        assert (LR.resolve(const, s) == 137).all()
        img = np.zeros((1, s, s, 3), np.uint8)
        img[0, 0, 0] = [255, 1, 0]
        n = s * s
        assert np.array_equal(LR.resolve(img, s)[0, 0, 0], [(255 + n // 2) // n, (1 + n // 2) // n, 0])
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, size=(2, 6, 9, 3), dtype=np.uint8)
    got = LR.resolve(img, 3)
    assert got.shape == (2, 2, 3, 3)
    assert got[1, 1, 2, 0] == (int(img[1, 3:6, 6:9, 0].astype(np.int64).sum()) + 4) // 9


def test_colour_blend_of_equal_colours_is_that_colour():
    q = R.quad_scene()
    cam = q["cam"]
    pos, xy, _ = R.project(q["verts"] + [0, 0, 0.0], None, cam["view"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["near"])
    buf = R.Buffers(1, q["H"], q["W"])
    R.raster(buf, xy, pos, q["faces"])
    lights = np.array([[0.0, 0.0, 1.0, 0.5]])
    a = np.zeros((1, q["H"], q["W"], 3), np.uint8)
    b = np.zeros_like(a)
    R.shade_mesh(a, buf.prim_id, xy, pos, None, q["faces"], 0, (0.9, 0.6, 0.3), 0.2, lights)
    LR.shade_mesh_colors(b, buf.prim_id, xy, pos, None, q["faces"], 0, np.tile([[0.9, 0.6, 0.3]], (4, 1)), 0.2, lights)
    assert np.array_equal(a, b) and a.any()
    cols = np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0], [1.0, 1.0, 1.0]])
    LR.shade_mesh_colors(b, buf.prim_id, xy, pos, None, q["faces"], 0, cols, 1.0, np.zeros((0, 4)))
    assert len(np.unique(b[0][q["expect"]], axis=0)) > 50  # the colours do vary over the quad


# ---- host helpers -------------------------------------------------------------------------------------------------------------------
def test_contact_colors_at_the_breakpoints():
    import torch

    from oakink2_tamf_amd import render

    base, hot = (0.91, 0.72, 0.60), (1.0, 0.1, 0.05)
    d = np.array([[-0.001, 0.0, 0.005], [0.0175, 0.03, 0.5]], np.float32)
    for dist in (d, torch.from_numpy(d)):
        c = render.contact_colors(dist, base, hot)
        c = c.numpy() if hasattr(c, "numpy") else c
        assert c.shape == (2, 3, 3) and c.dtype == np.float32
        # inside near = 5 mm the contact colour and beyond far = 30 mm the base colour, exactly; AT a breakpoint w is a quotient of
        # rounded float32 differences, within a few ulp of 1 or 0
        assert np.array_equal(c[0, :2], np.tile(np.float32(hot), (2, 1))) and np.array_equal(c[1, 2], np.float32(base))
        assert np.allclose(c[0, 2], np.float32(hot), atol=1e-6) and np.allclose(c[1, 1], np.float32(base), atol=1e-6)
        assert np.allclose(c[1, 0], 0.5 * (np.float32(base) + np.float32(hot)), atol=1e-6)  # half way
    c = render.contact_colors(np.float32([0.01, 0.02]), base, hot, near=0.01, far=0.02)
    assert np.allclose(c, np.float32([hot, base]), atol=1e-6)
    mono = render.contact_colors(np.linspace(0.0, 0.04, 41, dtype=np.float32), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))[:, 0]
    assert (np.diff(mono) <= 0).all() and mono[0] == 1.0 and mono[-1] == 0.0
    for near, far in ((0.03, 0.03), (0.03, 0.01), (0.0, float("nan"))):
        with pytest.raises(ValueError):
            render.contact_colors(d, base, hot, near=near, far=far)


def _chunks(data):
    out, pos = [], 8
    while pos < len(data):
        n, tag = struct.unpack(">I", data[pos: pos + 4])[0], data[pos + 4: pos + 8]
        assert struct.unpack(">I", data[pos + 8 + n: pos + 12 + n])[0] == zlib.crc32(data[pos + 4: pos + 8 + n]) & 0xFFFFFFFF, tag
        out.append((tag, data[pos + 8: pos + 8 + n]))
        pos += 12 + n
    return out


def test_apng_round_trip_chunk_order_and_first_frame(tmp_path):
    from oakink2_tamf_amd import render

    rng = np.random.default_rng(4)
    for n, h, w, fps in ((1, 1, 1, 10), (4, 7, 13, 10), (3, 40, 48, 25)):
        frames = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
        path = str(tmp_path / f"a_{n}.apng")
        render.write_apng(path, frames, fps)
        data = open(path, "rb").read()
        assert data[:8] == b"\x89PNG\r\n\x1a\n"
        chunks = _chunks(data)  # (every CRC is checked there, independently of read_apng)
        assert [t for t, _ in chunks] == [b"IHDR", b"acTL", b"fcTL", b"IDAT"] + [b"fcTL", b"fdAT"] * (n - 1) + [b"IEND"]
        assert struct.unpack(">II", chunks[1][1]) == (n, 0)  # n frames, played for ever
        seq = [struct.unpack(">I", body[:4])[0] for t, body in chunks if t in (b"fcTL", b"fdAT")]
        assert seq == list(range(2 * n - 1))
        for t, body in chunks:
            if t == b"fcTL":
                assert len(body) == 26 and struct.unpack(">IIIIHHBB", body[4:]) == (w, h, 0, 0, 1, fps, 0, 0)  # delay 1 / fps s, full frame
        got, got_fps = render.read_apng(path)
        assert np.array_equal(got, frames) and got_fps == fps
        assert np.array_equal(render.read_png(path), frames[0])  # a plain PNG reader sees the first frame
        for k, (t, body) in enumerate(c for c in chunks if c[0] == b"fdAT"):  # an independent decode of the later frames
            rows = np.frombuffer(zlib.decompress(body[4:]), np.uint8).reshape(h, 1 + 3 * w)
            assert not rows[:, 0].any() and np.array_equal(rows[:, 1:].reshape(h, w, 3), frames[k + 1])
        try:
            from PIL import Image
        except ImportError:
            Image = None
        if Image is not None:
            im = Image.open(path)
            assert getattr(im, "n_frames", 1) == n
            im.seek(n - 1)
            assert np.array_equal(np.asarray(im.convert("RGB")), frames[n - 1])
    for bad in (np.zeros((2, 4, 4), np.uint8), np.zeros((0, 4, 4, 3), np.uint8), np.zeros((2, 4, 4, 3), np.float32)):
        with pytest.raises(ValueError):
            render.write_apng(str(tmp_path / "b.apng"), bad, 10)
    with pytest.raises(ValueError):
        render.write_apng(str(tmp_path / "b.apng"), np.zeros((2, 4, 4, 3), np.uint8), 0)
    data = bytearray(open(path, "rb").read())
    data[-40] ^= 1  # inside the last fdAT
    open(str(tmp_path / "c.apng"), "wb").write(bytes(data))
    with pytest.raises(ValueError, match="CRC"):
        render.read_apng(str(tmp_path / "c.apng"))


# ---- launcher -----------------------------------------------------------------------------------------------------------------------
def test_dry_run_prints_the_new_settings_and_bad_values_are_refused(tmp_path):
    import test_score_cpu as SC

    from oakink2_tamf_amd.launch import render_samples

    paths, cache, tree = SC._synthetic_tree(str(tmp_path))
    base = SC._data_args(paths, tree) + ["--dry_run", "--max_clips", "1", "--render.width", "64", "--render.height", "64"]
    r = SC._launch("render_samples", base, str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["display"] == {"contact_map": False, "contact_far_mm": 30.0, "obj_alpha": 1.0, "layers": 1, "ssaa": 1, "apng": False, "apng_fps": 10}
    assert out["display"] == render_samples.DISPLAY_DEFAULTS
    assert out["render"] == {"width": 64, "height": 64, "every": 1, "sheet_cols": 8, "point_size": 3}
    r = SC._launch("render_samples", base + ["--render.contact_map", "--render.contact_far_mm", "20", "--render.obj_alpha", "0.4", "--render.ssaa", "2",
                                             "--render.apng", "--render.apng_fps", "5"], str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["display"] == {"contact_map": True, "contact_far_mm": 20.0, "obj_alpha": 0.4, "layers": 4, "ssaa": 2, "apng": True, "apng_fps": 5}
    args = SC._data_args(paths, tree) + ["--dry_run"]
    assert render_samples.parse_args(args + ["--render.obj_alpha", "0.4", "--render.layers", "2"])["display"]["layers"] == 2  # the flag beats the default of 4
    assert render_samples.parse_args(args + ["--render.layers", "8"])["display"]["layers"] == 8
    for bad in (["--render.obj_alpha", "0"], ["--render.obj_alpha", "1.5"], ["--render.obj_alpha", "nan"], ["--render.layers", "0"], ["--render.layers", "9"],
                ["--render.ssaa", "0"], ["--render.ssaa", "5"], ["--render.ssaa", "2", "--render.width", "2049"], ["--render.ssaa", "4", "--render.point_size", "5"],
                ["--render.contact_far_mm", "5"], ["--render.contact_far_mm", "nan"], ["--render.apng_fps", "0"]):
        with pytest.raises(SystemExit) as e:
            render_samples.parse_args(args + bad)
        assert e.value.code == 2, bad


def test_header_names_fourteen_functions_and_its_limits_are_the_wrappers():
    from oakink2_tamf_amd import _lib, render

    with open(os.path.join(_lib.INCLUDE, "tamf_render.h")) as f:
        head = f.read()
    text = re.sub(r"/\*.*?\*/", "", head, flags=re.S)
    names = sorted(set(re.findall(r"\b(tamf_render_\w+)\s*\(", text)))
    assert names == sorted(_lib.RENDER_EXPORTS) and len(names) == 14 and "14 functions" in head
    for new in ("raster_behind", "points_behind", "shade_mesh_colors", "shade_points_colors", "composite", "resolve"):
        assert "tamf_render_" + new in names
    for name, val in (("MAX_LAYERS", render.MAX_LAYERS), ("MAX_ITEMS", render.MAX_ITEMS)):
        assert int(re.search(rf"#define\s+TAMF_RENDER_{name}\s+(\d+)", head).group(1)) == val
    assert render.MAX_LAYERS == 8 and render.MAX_ITEMS == 64
