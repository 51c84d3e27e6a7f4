"""CPU: the renderer's definition (tests/render_restatement.py) against analytic cases, the host helpers of render.py (PNG writer,
camera fit, lights, contact sheet), the launcher's dry run and shell entry point on a synthetic tree, and the description and exports of
libtamf_render.so.  The near-tie share that the GPU tests rely on is asserted here for every scene they use."""
import json
import os
import re
import shlex
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_restatement as R  # noqa: E402
import render_scenes as S  # noqa: E402


def _raster_scene(sc, dtype=np.float64):
    cam = sc["cam"]
    pos, xy, _ = R.project(sc["verts"], None, cam["view"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["near"], dtype=dtype)
    buf = R.Buffers(1, sc["H"], sc["W"], dtype)
    R.raster(buf, xy, pos, sc["faces"])
    return buf, pos, xy


# ---- the raster restatement against analytic cases ---------------------------------------------------------------------------------
def test_quad_covers_exactly_the_expected_pixels_once():
    sc = R.quad_scene()
    buf, pos, xy = _raster_scene(sc)
    assert np.array_equal(xy[0], [[1408, 896], [5248, 896], [5248, 3200], [1408, 3200]])  # the corners lie ON pixel centres
    assert np.array_equal(buf.prim_id[0] >= 0, sc["expect"])
    assert int(buf.cover.max()) == 1 and np.array_equal(buf.cover[0] == 1, sc["expect"])  # the shared diagonal is counted once
    on_diagonal = [(j, i) for j in range(4, 13) for i in range(5, 20) if (i - 5) * 9 == (j - 3) * 15]
    assert len(on_diagonal) == 2  # the diagonal does pass through interior centres: (10.5, 6.5) and (15.5, 9.5)
    assert set(np.unique(buf.prim_id[0][sc["expect"]])) == {0, 1}
    assert np.allclose(buf.depth[0][sc["expect"]], 2.0, rtol=1e-12) and np.isinf(buf.depth[0][~sc["expect"]]).all()
    # the other winding draws the same pixels
    sc2 = dict(sc, faces=sc["faces"][:, ::-1])
    assert np.array_equal(_raster_scene(sc2)[0].prim_id >= 0, buf.prim_id >= 0)


def test_closed_sphere_covers_every_pixel_an_even_number_of_times():
    v, f = R.uv_sphere(9, 14, 0.8, (0.1, -0.05, 3.0))
    sc = dict(W=64, H=48, cam=R.camera(64, 48), verts=v, faces=f)
    buf, _, _ = _raster_scene(sc)
    covered = buf.cover[0] > 0
    assert covered.sum() > 300
    assert (buf.cover[0][covered] % 2 == 0).all()  # a closed surface: every ray leaves as often as it enters


def test_nearer_triangle_wins_and_coincident_pair_resolves_to_the_lower_id():
    cam = R.camera(32, 32)
    tri = np.array([[-1.0, -1.0, 0.0], [1.0, -1.0, 0.0], [0.0, 1.2, 0.0]])
    verts = np.concatenate([tri + [0, 0, 4.0], tri + [0.1, 0.0, 3.0], tri + [0.1, 0.0, 3.0]])
    for faces, want in (([[0, 1, 2], [3, 4, 5]], 1), ([[3, 4, 5], [0, 1, 2]], 0), ([[0, 1, 2], [3, 4, 5], [6, 8, 7]], 1), ([[6, 8, 7], [0, 1, 2], [3, 4, 5]], 0)):
        sc = dict(W=32, H=32, cam=cam, verts=verts, faces=np.array(faces, np.int32))
        buf, _, _ = _raster_scene(sc)
        assert buf.prim_id[0, 16, 16] == want and abs(buf.depth[0, 16, 16] - 3.0) < 1e-9, faces
    # across calls the earlier call wins an exact tie
    sc = dict(W=32, H=32, cam=cam, verts=verts, faces=np.array([[3, 4, 5]], np.int32))
    buf, pos, xy = _raster_scene(sc)
    R.raster(buf, xy, pos, np.array([[6, 7, 8]], np.int32), prim_base=100)
    assert buf.prim_id[0, 16, 16] == 0 and (buf.prim_id < 100).all()


def test_invalid_vertices_and_point_splats():
    cam = R.camera(16, 16, near=0.5)
    verts = np.array([[0, 0, 0.4], [np.nan, 0, 2], [0, 0, 2.0], [1e9, 0, 1.0], [0.3, -0.2, 2.0]])
    pos, xy, _ = R.project(verts, None, cam["view"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["near"])
    assert (xy[0, [0, 1, 3]] == R.INVALID).all() and (xy[0, [2, 4]] != R.INVALID).all()
    buf = R.Buffers(1, 16, 16)
    R.points(buf, xy, pos, 3)
    qx, qy = int(xy[0, 4, 0]) // 256, int(xy[0, 4, 1]) // 256
    want = np.zeros((16, 16), bool)
    want[7:10, 7:10] = True
    want[qy - 1: qy + 2, qx - 1: qx + 2] = True
    assert np.array_equal(buf.prim_id[0] >= 0, want) and buf.prim_id[0, 8, 8] == 2 and buf.prim_id[0, qy, qx] == 4


@pytest.mark.parametrize("name", S.NAMES)
def test_near_tie_share_of_the_gpu_scenes(name):
    """what tests/test_render_gpu.py may exclude: pixels whose two nearest candidates lie within 1e-5 relative depth are at most
    0.5 % of the covered pixels, in every scene"""
    ref = S.reference(name)
    covered = int((ref["buf"].prim_id >= 0).sum())
    share = ref["buf"].near_tie_share()
    print(f"RENDER scene {name}: covered {covered} near ties {int(ref['buf'].near_tie().sum())} share {share:.5f}")
    assert covered > 0 and share <= 0.005


# ---- host helpers -------------------------------------------------------------------------------------------------------------------
def test_write_png_round_trips(tmp_path):
    from oakink2_tamf_amd import render

    rng = np.random.default_rng(0)
    for h, w in ((1, 1), (7, 13), (40, 48)):
        img = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        path = str(tmp_path / f"a_{h}x{w}.png")
        render.write_png(path, img)
        data = open(path, "rb").read()
        assert data[:8] == b"\x89PNG\r\n\x1a\n" and struct.unpack(">II", data[16:24]) == (w, h)
        # an independent decode: the chunks by hand, zlib, filter byte 0 per row
        pos, idat = 8, b""
        while pos < len(data):
            n, tag = struct.unpack(">I", data[pos: pos + 4])[0], data[pos + 4: pos + 8]
            assert struct.unpack(">I", data[pos + 8 + n: pos + 12 + n])[0] == zlib.crc32(data[pos + 4: pos + 8 + n]) & 0xFFFFFFFF
            idat += data[pos + 8: pos + 8 + n] if tag == b"IDAT" else b""
            pos += 12 + n
        rows = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 3 * w)
        assert not rows[:, 0].any() and np.array_equal(rows[:, 1:].reshape(h, w, 3), img)
        assert np.array_equal(render.read_png(path), img)
        try:
            from PIL import Image
        except ImportError:
            Image = None
        if Image is not None:
            assert np.array_equal(np.asarray(Image.open(path).convert("RGB")), img)
    with pytest.raises(ValueError):
        render.write_png(str(tmp_path / "b.png"), np.zeros((4, 4), np.uint8))


def test_look_at_camera_keeps_every_point_in_view():
    from oakink2_tamf_amd import render

    rng = np.random.default_rng(1)
    for W, H, fov, fwd in ((64, 64, 45.0, (0, 0, 1)), (96, 40, 30.0, (1, 0.5, 0.2)), (33, 80, 70.0, (0, -1, 0.3))):
        pts = rng.normal(size=(500, 3)) * [0.3, 0.1, 0.2] + [1.0, -2.0, 0.5]
        up = (0, -1, 0) if abs(fwd[1]) < 0.9 else (0, 0, 1)
        cam = render.look_at_camera(pts, W, H, fov_deg=fov, forward=fwd, up=up)
        R3 = cam.view[:, :3]
        assert np.allclose(R3 @ R3.T, np.eye(3), atol=1e-12) and np.linalg.det(R3) > 0
        pos, xy, uv = R.project(pts, None, cam.view, cam.fx, cam.fy, cam.cx, cam.cy, cam.near)
        assert (xy != R.INVALID).all() and (pos[..., 2] > cam.near).all()
        assert (uv[..., 0] > 0).all() and (uv[..., 0] < 256 * W).all() and (uv[..., 1] > 0).all() and (uv[..., 1] < 256 * H).all()
    with pytest.raises(ValueError):
        render.look_at_camera(np.full((3, 3), np.nan), 8, 8)


def test_default_lights_and_contact_sheet():
    from oakink2_tamf_amd import render

    L = render.default_lights()
    assert L.shape == (3, 4) and np.allclose(np.linalg.norm(L[:, :3], axis=1), 1.0)
    assert np.allclose(L[:, 2], np.cos(np.pi / 6))  # 30 degrees off the optical axis, shining away from the viewer
    assert np.allclose([L[a, :3] @ L[b, :3] for a, b in ((0, 1), (1, 2), (0, 2))], L[0, :3] @ L[1, :3])  # 120 degrees apart
    assert np.allclose(L[:, :2].sum(axis=0), 0.0, atol=1e-12) and render.AMBIENT == 0.2
    assert render.AMBIENT + L[:, 3].sum() * np.cos(np.pi / 6) < 1.05
    frames = np.arange(5 * 2 * 3 * 3, dtype=np.uint8).reshape(5, 2, 3, 3)
    sheet = render.contact_sheet(frames, 3, background=255)
    assert sheet.shape == (4, 9, 3) and np.array_equal(sheet[2:4, 3:6], frames[4]) and (sheet[2:4, 6:9] == 255).all()
    assert render.contact_sheet(frames[:2], 8).shape == (2, 6, 3)


def test_pose_rows_are_the_score_codes_transform():
    from oakink2_tamf_amd import render
    from oakink2_tamf_amd.dataset.interaction_segment import transf_to_tslrot6d
    from oracle.fixtures import _det_rotations

    T4 = np.zeros((5, 4, 4), np.float32)
    T4[:, :3, :3], T4[:, :3, 3], T4[:, 3, 3] = _det_rotations("render/pose", (5,)), np.arange(15).reshape(5, 3) * 0.1, 1.0
    back = render.tslrot6d_to_matrix(transf_to_tslrot6d(T4))
    assert back.shape == (5, 3, 4) and np.allclose(back, T4[:, :3], atol=1e-6)


# ---- launcher -----------------------------------------------------------------------------------------------------------------------
def test_dry_run_lists_the_pairs_and_with_gt_needs_a_factory(tmp_path):
    import test_score_cpu as SC

    paths, cache, tree = SC._synthetic_tree(str(tmp_path))
    r = SC._launch("render_samples", SC._data_args(paths, tree) + ["--dry_run", "--max_clips", "2", "--render.width", "64"], str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    infos = cache["interaction_segment_info_list"]
    assert out["n_clips"] == 2 and [tuple(p["info"]) for p in out["pairs"]] == [tuple(infos[i]) for i in (0, 1)]
    assert out["render"] == {"width": 64, "height": 512, "every": 1, "sheet_cols": 8, "point_size": 3} and not out["with_gt"]
    from oakink2_tamf_amd.launch import render_samples

    for bad in (["--with_gt"], ["--render.point_size", "4"], ["--render.width", "0"], ["--render.every", "0"], ["--max_clips", "0"], ["--no_such_flag", "1"]):
        with pytest.raises(SystemExit) as e:  # (argparse: usage + message on stderr, status 2)
            render_samples.parse_args(SC._data_args(paths, tree) + ["--dry_run"] + bad)
        assert e.value.code == 2, bad
    assert render_samples.parse_args(SC._data_args(paths, tree) + ["--with_gt", "--mano.factory", "fake_mano:make"])["runtime"]["with_gt"]


def test_shell_entry_point():
    from oakink2_tamf_amd.launch import render_samples

    path = os.path.join(ROOT, "script", "render_samples.sh")
    assert os.access(path, os.X_OK)
    r = subprocess.run(["bash", path, "-n", "val", "arch_mdm_l__0399", "--render.every", "4", "--with_gt", "--mano.factory", "my.mano:make"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "split:" in r.stdout and "model_name:" in r.stdout
    toks = shlex.split([l for l in r.stdout.splitlines() if l.startswith("python -m ")][-1])
    assert toks[:3] == ["python", "-m", "oakink2_tamf_amd.launch.render_samples"]
    assert toks[3:] == ["--data.process_range", "?(file:./asset/split/val.txt)", "--data.cache_dict_filepath",
                        "common/save_cache_dict/main/cache/val.pkl", "--debug.sample_refine_filepath",
                        "common/sample_refine/main/sample/val/arch_mdm_l__0399", "--out_dir", "common/render_samples/main/val/arch_mdm_l__0399",
                        "--render.every", "4", "--with_gt", "--mano.factory", "my.mano:make"]
    args = list(toks[3:])
    args[1] = "scene_a:scene_b"  # (the ?(file:...) macro needs the split file; the parser takes the rest as it is)
    cfg = render_samples.parse_args(args)
    assert cfg["render"]["every"] == 4 and cfg["runtime"]["with_gt"] and cfg["mano"]["factory"] == "my.mano:make"
    assert cfg["runtime"]["out_dir"].endswith("common/render_samples/main/val/arch_mdm_l__0399")
    r = subprocess.run(["bash", path, "val"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "usage" in r.stderr
    r = subprocess.run(["bash", path, "-h"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "split" in r.stdout


# ---- the library's description --------------------------------------------------------------------------------------------------------
def test_lib_description_and_exports():
    import shutil

    from oakink2_tamf_amd import _lib

    with open(os.path.join(_lib.INCLUDE, "tamf_render.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(tamf_render_\w+)\s*\(", text))) == sorted(_lib.RENDER_EXPORTS)
    lib = _lib.RENDER
    assert _lib.RENDERING == (lib,) and lib.root == "tamf_render.hip" and lib.headers == ("tamf_render.h", "tamf_hip.h")
    assert [o.file for o in lib.outputs] == ["libtamf_render.so"] and lib.outputs[0].exports == _lib.RENDER_EXPORTS
    assert _lib.RENDER_LIB_PATH == lib.paths[0] and lib.sources == ["tamf_raster.h", "tamf_render.hip"] and not lib.counted_waits
    import inspect

    assert "RENDERING" in inspect.getsource(_lib.build) and callable(_lib.load_render)
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    res = subprocess.run([nm, "-D", "--defined-only", lib.build()], capture_output=True, text=True, check=True)
    syms = sorted(ln.split()[-1] for ln in res.stdout.splitlines() if ln.split() and ln.split()[-1].startswith("tamf_"))
    assert syms == sorted(_lib.RENDER_EXPORTS)
    # the header's limits are the wrapper's and the kernels'
    from oakink2_tamf_amd import render

    with open(os.path.join(_lib.INCLUDE, "tamf_render.h")) as f:
        head = f.read()
    for name, val in (("MAX_LIGHTS", render.MAX_LIGHTS), ("MAX_SIDE", render.MAX_SIDE), ("MAX_POINT_SIZE", render.MAX_POINT_SIZE)):
        assert int(re.search(rf"#define\s+TAMF_RENDER_{name}\s+(\d+)", head).group(1)) == val
    assert ctypes_size_of_camera() == 17 * 4


def ctypes_size_of_camera():
    import ctypes

    from oakink2_tamf_amd import render

    return ctypes.sizeof(render.CameraStruct)
