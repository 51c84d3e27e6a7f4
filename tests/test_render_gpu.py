"""GPU: libtamf_render.so through its C interface against the numpy restatement (tests/render_restatement.py) on the scenes of
tests/render_scenes.py: projection, primitive ids and depths of the rasteriser and the point splats, shading, determinism, frame
independence, guard bands around the outputs, and the rejected arguments."""
import ctypes
import os
import sys
from ctypes import c_void_p

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_restatement as R  # noqa: E402
import render_scenes as S  # noqa: E402

pytestmark = pytest.mark.gpu
INVALID_ARG = -1  # TAMF_ERR_INVALID
BASE, AMBIENT, BG = (0.9, 0.6, 0.3), 0.2, (0.1, 0.2, 0.3)
SENTINEL = 0x5A
_cache = {}


def _lib():
    from oakink2_tamf_amd import render

    return render._bind()


def P(t):
    return None if t is None else c_void_p(t.data_ptr())


def H(a):
    return a.ctypes.data_as(c_void_p)


def _cam(c):
    from oakink2_tamf_amd import render

    return render.camera_struct(render.Camera(c["view"], c["fx"], c["fy"], c["cx"], c["cy"], c["near"]))


def _lights():
    from oakink2_tamf_amd import render

    return np.ascontiguousarray(render.default_lights(), np.float32)


def ok(rc):
    assert rc == 0, _lib().tamf_render_last_error().decode()


def project(sc, it, frames=None):
    """tamf_render_project of one item -> (pos (F,V,3), xy (F,V,2)) device tensors; frames: a subset of the scene's frames"""
    import torch

    L = _lib()
    sel = list(range(sc["F"])) if frames is None else list(frames)
    v = np.asarray(it["verts"], np.float32)
    per_frame = v.ndim == 3
    v = torch.from_numpy(np.ascontiguousarray(v[sel] if per_frame else v)).cuda()
    m = None if it["model"] is None else torch.from_numpy(np.ascontiguousarray(it["model"][sel], np.float32)).cuda()
    F, V = len(sel), int(v.shape[-2])
    pos = torch.empty((F, V, 3), dtype=torch.float32, device="cuda")
    xy = torch.empty((F, V, 2), dtype=torch.int32, device="cuda")
    cam = _cam(sc["cam"])
    ok(L.tamf_render_project(P(v), P(m), ctypes.addressof(cam), F, V, int(per_frame), P(pos), P(xy), None))
    return pos, xy


def run(sc, frames=None, normals=None, out=None):
    """the whole pipeline on the scene (flat shading unless normals = {item index: (F,V,3) camera-space tensor}) ->
    dict(proj [(pos, xy)], depth, prim, rgb) device tensors; out: (depth, prim, rgb) to draw into instead of fresh buffers"""
    import torch

    L = _lib()
    F, Hh, W = (sc["F"] if frames is None else len(frames)), sc["H"], sc["W"]
    if out is None:
        out = (torch.empty((F, Hh, W), dtype=torch.float32, device="cuda"), torch.empty((F, Hh, W), dtype=torch.int32, device="cuda"),
               torch.full((F, Hh, W, 3), SENTINEL, dtype=torch.uint8, device="cuda"))
    depth, prim, rgb = out
    ok(L.tamf_render_clear(P(depth), P(prim), F, Hh, W, None))
    proj, faces = [], []
    for it, base in zip(sc["items"], S.bases(sc)):
        pos, xy = project(sc, it, frames)
        V = int(pos.shape[1])
        if it["kind"] == "mesh":
            f = torch.from_numpy(np.ascontiguousarray(it["faces"], np.int32)).cuda()
            ok(L.tamf_render_raster(P(xy), P(pos), P(f), F, V, int(f.shape[0]), Hh, W, base, P(depth), P(prim), None))
        else:
            f = None
            ok(L.tamf_render_points(P(xy), P(pos), F, V, Hh, W, it["point_size"], base, P(depth), P(prim), None))
        proj.append((pos, xy))
        faces.append(f)
    base_rgb, lights, bg = np.asarray(BASE, np.float32), _lights(), np.asarray(BG, np.float32)
    for k, (it, base, (pos, xy), f) in enumerate(zip(sc["items"], S.bases(sc), proj, faces)):
        if it["kind"] == "mesh":
            n = None if normals is None else normals.get(k)
            ok(L.tamf_render_shade_mesh(P(prim), P(xy), P(pos), P(n), P(f), F, int(pos.shape[1]), int(f.shape[0]), Hh, W, base, H(base_rgb), AMBIENT,
                                        H(lights), 3, P(rgb), None))
        else:
            ok(L.tamf_render_shade_points(P(prim), F, Hh, W, base, int(pos.shape[1]), H(base_rgb), P(rgb), None))
    ok(L.tamf_render_fill(P(prim), F, Hh, W, H(bg), P(rgb), None))
    torch.cuda.synchronize()
    return dict(proj=proj, depth=depth, prim=prim, rgb=rgb)


def case(name):
    """the scene on the GPU, and the restatement (float64 and float32) fed the library's own xy and pos_cam: computed once"""
    if name not in _cache:
        sc = S.scene(name)
        got = run(sc)
        proj = [(p.cpu().numpy(), xy.cpu().numpy().astype(np.int64)) for p, xy in got["proj"]]
        _cache[name] = dict(scene=sc, got=got, proj=proj, r64=S.draw(sc, proj), r32=S.draw(sc, proj, np.float32))
    return _cache[name]


# ---- projection -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.NAMES)
def test_project(name):
    c = case(name)
    sc = c["scene"]
    r64, r32 = S.project_items(sc), S.project_items(sc, np.float32)
    for k, ((pos, xy), (p64, xy64, uv64), (p32, _, _)) in enumerate(zip(c["proj"], r64, r32)):
        assert np.array_equal(xy[..., 0] == R.INVALID, xy64[..., 0] == R.INVALID) and np.array_equal(xy[..., 0] == R.INVALID, xy[..., 1] == R.INVALID)
        valid = (xy[..., 0] != R.INVALID) & (np.abs(uv64) <= 4096 * 256).all(axis=-1)
        err = np.abs(xy[valid] - uv64[valid]).max()
        # 0.5 of the rounding + the fp32 projection: spacing 1/8 unit at 4096 px, about six roundings
        print(f"RENDER project {name}[{k}]: max |xy - float64| = {err:.3f} units over {int(valid.sum())} vertices")
        assert valid.sum() > 0 and err <= 1.0
        scale = np.abs(p64).max()
        hip_dev, ref_dev = np.abs(pos.astype(np.float64) - p64).max() / scale, np.abs(p32.astype(np.float64) - p64).max() / scale
        print(f"RENDER pos_cam {name}[{k}]: hip {hip_dev:.3e}  float32 restatement {ref_dev:.3e}  gate {4 * ref_dev:.3e}")
        assert hip_dev <= 4 * ref_dev and (ref_dev > 0 or name == "quad")  # (the quad's coordinates are exact in fp32: both are 0)


def test_invalid_vertices_carry_the_marker():
    sc = dict(F=1, cam=R.camera(64, 64, near=0.5))
    verts = np.array([[0.1, 0.1, 2.0], [0, 0, 0.4999], [0, 0, -3.0], [np.nan, 0, 2], [0, np.inf, 2], [0, 0, np.nan], [3e6, 0, 1.0], [0, -3e6, 1.0],
                      [0.0, 0.0, 0.5], [1e30, 1e30, 1e30]], np.float32)
    pos, xy = project(sc, dict(verts=verts, model=None))
    xy = xy.cpu().numpy()[0]
    bad = [1, 2, 3, 4, 5, 6, 7]  # behind near, NaN / inf, |snapped| > 2^28
    assert (xy[bad] == R.INVALID).all() and (xy[[0, 8, 9]] != R.INVALID).all()
    assert np.array_equal(xy[8], [32 * 256, 32 * 256])  # z == near is valid
    _, want, _ = R.project(verts, None, sc["cam"]["view"], sc["cam"]["fx"], sc["cam"]["fy"], sc["cam"]["cx"], sc["cam"]["cy"], 0.5)
    assert np.array_equal(xy == R.INVALID, want[0] == R.INVALID)
    assert np.array_equal(pos.cpu().numpy()[0, [0, 8]], verts[[0, 8]])  # identity view: pos_cam is written for every vertex


# ---- raster and points ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.NAMES)
def test_ids_and_depth_equal_the_restatement(name):
    c = case(name)
    r64, r32 = c["r64"], c["r32"]
    prim, depth = c["got"]["prim"].cpu().numpy().astype(np.int64), c["got"]["depth"].cpu().numpy()
    tie = r64.near_tie()
    covered = r64.prim_id >= 0
    share = tie.sum() / covered.sum()
    print(f"RENDER {name}: covered {int(covered.sum())} near ties {int(tie.sum())} (share {share:.5f}) id mismatches outside them "
          f"{int(((prim != r64.prim_id) & ~tie).sum())}")
    assert covered.sum() > 100 and share <= 0.005
    assert np.array_equal(prim[~tie], r64.prim_id[~tie])
    assert np.array_equal(prim >= 0, covered)  # coverage is integer arithmetic: exact, ties or not
    assert np.isinf(depth[~covered]).all() and (depth[~covered] > 0).all() and (prim[~covered] == -1).all()
    same = covered & (prim == r64.prim_id) & (r32.prim_id == r64.prim_id)
    scale = r64.depth[same].max()
    hip_dev, ref_dev = np.abs(depth[same] - r64.depth[same]).max() / scale, np.abs(r32.depth[same].astype(np.float64) - r64.depth[same]).max() / scale
    print(f"RENDER depth {name}: hip {hip_dev:.3e}  float32 restatement {ref_dev:.3e}  gate {4 * ref_dev:.3e}")
    if name.startswith("points") or name == "quad":  # a splat's depth is the point's z, the quad's a constant: no arithmetic to gate
        assert hip_dev <= 4 * max(ref_dev, 2.0 ** -24)
    else:
        assert ref_dev > 0 and hip_dev <= 4 * ref_dev
    if name == "quad":
        assert np.array_equal(prim[0] >= 0, R.quad_scene()["expect"])


def test_coincident_triangles_lower_id_within_a_call_earlier_call_across_calls():
    import torch

    L = _lib()
    W = Hh = 32
    sc = dict(F=1, cam=R.camera(W, Hh))
    tri = np.array([[-1.0, -1.0, 3.0], [1.0, -1.0, 3.0], [0.0, 1.2, 3.3]])
    pos, xy = project(sc, dict(verts=np.concatenate([tri, tri]), model=None))
    depth = torch.empty((1, Hh, W), dtype=torch.float32, device="cuda")
    prim = torch.empty((1, Hh, W), dtype=torch.int32, device="cuda")
    for faces, want in (([[0, 1, 2], [3, 5, 4]], 0), ([[3, 5, 4], [0, 1, 2]], 0), ([[0, 2, 1], [3, 4, 5], [0, 1, 2]], 0)):
        f = torch.tensor(faces, dtype=torch.int32, device="cuda")
        ok(L.tamf_render_clear(P(depth), P(prim), 1, Hh, W, None))
        ok(L.tamf_render_raster(P(xy), P(pos), P(f), 1, 6, len(faces), Hh, W, 0, P(depth), P(prim), None))
        ids = prim.cpu().numpy()
        assert (ids >= 0).sum() > 50 and set(np.unique(ids)) == {-1, want}, faces
    first = depth.clone()
    f = torch.tensor([[3, 4, 5]], dtype=torch.int32, device="cuda")
    ok(L.tamf_render_raster(P(xy), P(pos), P(f), 1, 6, 1, Hh, W, 1000, P(depth), P(prim), None))  # a second call: the earlier one keeps its pixels
    assert set(np.unique(prim.cpu().numpy())) == {-1, 0} and torch.equal(depth, first)


# ---- shading ------------------------------------------------------------------------------------------------------------------------
def _shade_reference(c, normals):
    sc = c["scene"]
    prim = c["r64"].prim_id
    rgb = np.full(prim.shape + (3,), SENTINEL, np.uint8)
    facing = np.full(prim.shape, np.nan)
    for k, (it, base, (pos, xy)) in enumerate(zip(sc["items"], S.bases(sc), c["proj"])):
        if it["kind"] == "mesh":
            fk = R.shade_mesh(rgb, prim, xy, pos, None if normals is None else normals.get(k), it["faces"], base, BASE, AMBIENT, _lights().astype(np.float64))
            facing = np.where(np.isnan(fk), facing, fk)
        else:
            R.shade_points(rgb, prim, base, pos.shape[1], np.asarray(BASE, np.float32))
    R.fill(rgb, prim, np.asarray(BG, np.float32))
    return rgb, facing


@pytest.mark.parametrize("name,smooth", [("soup", False), ("hand_spheres", False), ("hand_spheres", True), ("points5", False)])
def test_shade_within_one_level_of_the_restatement(name, smooth):
    import torch

    c = case(name)
    sc = c["scene"]
    normals_np = normals_dev = None
    got = c["got"]
    if smooth:
        normals_np, normals_dev = {}, {}
        for k, (it, (pos, _)) in enumerate(zip(sc["items"], c["proj"])):
            n = S.vertex_normals(pos.astype(np.float64), it["faces"]).astype(np.float32)  # of the camera-space vertices: already in the camera frame
            normals_np[k], normals_dev[k] = n, torch.from_numpy(n).cuda()
        got = run(sc, normals=normals_dev)
        assert torch.equal(got["prim"], c["got"]["prim"])
    want, facing = _shade_reference(c, normals_np)
    rgb, prim = got["rgb"].cpu().numpy(), got["prim"].cpu().numpy()
    same = prim == c["r64"].prim_id
    diff = np.abs(rgb.astype(np.int64) - want.astype(np.int64))[same]
    lit = same & (prim >= 0)
    print(f"RENDER shade {name} smooth={smooth}: max channel difference {int(diff.max())} over {int(same.sum())} pixels; "
          f"distinct levels {len(np.unique(rgb[lit]))}; least |n . view| {np.nanmin(facing) if np.isfinite(facing).any() else float('nan'):.2e}")
    assert diff.max() <= 1
    assert (rgb[prim == -1] == R.to_byte(np.asarray(BG, np.float32))).all() and (prim == -1).any()
    assert (rgb != SENTINEL).any(axis=-1)[prim >= 0].all()  # every covered pixel was written by its item's pass
    if name != "points5":
        assert len(np.unique(rgb[lit])) > 10  # the lights do vary over the surface


def test_shade_touches_its_own_id_range_only():
    import torch

    L = _lib()
    c = case("hand_spheres")
    sc, got = c["scene"], c["got"]
    F, Hh, W = sc["F"], sc["H"], sc["W"]
    base, count = S.bases(sc)[1], S.counts(sc)[1]
    pos, xy = got["proj"][1]
    f = torch.from_numpy(np.ascontiguousarray(sc["items"][1]["faces"], np.int32)).cuda()
    rgb = torch.full((F, Hh, W, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    ok(L.tamf_render_shade_mesh(P(got["prim"]), P(xy), P(pos), None, P(f), F, int(pos.shape[1]), count, Hh, W, base, H(np.asarray(BASE, np.float32)),
                                AMBIENT, H(_lights()), 3, P(rgb), None))
    torch.cuda.synchronize()
    mine = (got["prim"] >= base) & (got["prim"] < base + count)
    assert bool(mine.any()) and bool((~mine).any())
    assert bool((rgb[~mine] == SENTINEL).all()) and torch.equal(rgb[mine], got["rgb"][mine])
    rgb2 = torch.full((F, Hh, W, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    ok(L.tamf_render_fill(P(got["prim"]), F, Hh, W, H(np.asarray(BG, np.float32)), P(rgb2), None))
    ok(L.tamf_render_shade_points(P(got["prim"]), F, Hh, W, base, count, H(np.asarray([1.0, 0.0, 0.5], np.float32)), P(rgb2), None))
    torch.cuda.synchronize()
    none = got["prim"] == -1
    assert bool((rgb2[~none & ~mine] == SENTINEL).all()) and bool((rgb2[mine] == torch.tensor([255, 0, 128], dtype=torch.uint8, device="cuda")).all())
    assert bool((rgb2[none] == torch.from_numpy(R.to_byte(np.asarray(BG, np.float32))).cuda()).all())


# ---- determinism, frames, off-screen ---------------------------------------------------------------------------------------------------
def test_same_call_twice_gives_the_same_bits_and_a_frame_is_independent_of_the_others():
    import torch

    c = case("hand_spheres")
    sc, a = c["scene"], c["got"]
    b = run(sc)
    for key in ("depth", "prim", "rgb"):
        assert torch.equal(a[key], b[key]), key
    for (pa, xa), (pb, xb) in zip(a["proj"], b["proj"]):
        assert torch.equal(pa, pb) and torch.equal(xa, xb)
    alone = run(sc, frames=[1])
    for key in ("depth", "prim", "rgb"):
        assert torch.equal(alone[key][0], a[key][1]), key
    assert not torch.equal(a["prim"][0], a["prim"][1])  # the frames do differ


def test_off_screen_and_behind_the_camera_write_nothing():
    import torch

    L = _lib()
    W, Hh = 48, 40
    sc = dict(F=1, cam=R.camera(W, Hh))
    v, f = R.uv_sphere(6, 8, 0.5)
    f_dev = torch.from_numpy(f).cuda()
    depth = torch.full((1, Hh, W), 7.0, dtype=torch.float32, device="cuda")
    prim = torch.full((1, Hh, W), 42, dtype=torch.int32, device="cuda")
    for shift in ([30.0, 0.0, 3.0], [0.0, -30.0, 3.0], [0.0, 0.0, -3.0], [0.0, 0.0, 0.2]):  # right of, above, behind, straddling the near plane
        pos, xy = project(sc, dict(verts=v + shift, model=None))
        ok(L.tamf_render_raster(P(xy), P(pos), P(f_dev), 1, v.shape[0], f.shape[0], Hh, W, 0, P(depth), P(prim), None))
        ok(L.tamf_render_points(P(xy), P(pos), 1, v.shape[0], Hh, W, 5, 0, P(depth), P(prim), None))
        torch.cuda.synchronize()
        if shift[2] == 0.2:  # the near plane cuts the sphere: triangles with a vertex behind it are dropped, the far cap is drawn - and is nearer than 7
            assert bool((prim != 42).any()) and bool((depth[prim != 42] >= sc["cam"]["near"]).all())
        else:
            assert bool((depth == 7.0).all()) and bool((prim == 42).all()), shift


# ---- guard bands and rejected arguments ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,Hh", [(48, 40), (1, 1)])
def test_canaries_around_the_outputs(W, Hh):
    import torch

    G = 4096
    base = S.scene("soup")
    sc = dict(base, W=W, H=Hh, cam=R.camera(W, Hh) if W > 1 else dict(R.camera(1, 1), fx=0.2, fy=0.2))
    pts = S.scene("points5")["items"][0]
    sc["items"] = base["items"] + [dict(pts)]
    n = Hh * W
    raw = [torch.full((2 * G + n * size,), 0xC3, dtype=torch.uint8, device="cuda") for size in (4, 4, 3)]
    depth = raw[0][G: G + 4 * n].view(torch.float32).view(1, Hh, W)
    prim = raw[1][G: G + 4 * n].view(torch.int32).view(1, Hh, W)
    rgb = raw[2][G: G + 3 * n].view(1, Hh, W, 3)
    got = run(sc, out=(depth, prim, rgb))
    for r, size in zip(raw, (4, 4, 3)):
        assert bool((r[:G] == 0xC3).all()) and bool((r[G + n * size:] == 0xC3).all())
    assert bool((got["prim"] >= 0).any())
    proj = [(p.cpu().numpy(), xy.cpu().numpy().astype(np.int64)) for p, xy in got["proj"]]
    ref = S.draw(sc, proj)
    tie = ref.near_tie()
    print(f"RENDER canaries {W} x {Hh}: covered {int((ref.prim_id >= 0).sum())} near ties {int(tie.sum())}")
    assert np.array_equal(got["prim"].cpu().numpy()[~tie], ref.prim_id[~tie])


def test_rejected_arguments_launch_nothing():
    import torch

    L = _lib()
    c = case("soup")
    sc = c["scene"]
    W, Hh = sc["W"], sc["H"]
    pos, xy = c["got"]["proj"][0]
    V = int(pos.shape[1])
    f = torch.from_numpy(np.ascontiguousarray(sc["items"][0]["faces"], np.int32)).cuda()
    Nf = int(f.shape[0])
    depth = torch.full((1, Hh, W), 7.0, dtype=torch.float32, device="cuda")
    prim = torch.full((1, Hh, W), 3, dtype=torch.int32, device="cuda")  # an id inside every range below: a launched pass would write
    rgb = torch.full((1, Hh, W, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    pos_o, xy_o = torch.full_like(pos, 5.0), torch.full_like(xy, 5)
    verts = torch.zeros((V, 3), dtype=torch.float32, device="cuda")
    cam = _cam(sc["cam"])
    col, lights = np.asarray(BASE, np.float32), np.ascontiguousarray(np.tile(_lights()[:1], (9, 1)))
    N = None

    def raster(xy_=P(xy), pos_=P(pos), f_=P(f), F=1, h=Hh, w=W, base=0, d=P(depth), p=P(prim)):
        return L.tamf_render_raster(xy_, pos_, f_, F, V, Nf, h, w, base, d, p, N)

    def points(xy_=P(xy), pos_=P(pos), h=Hh, w=W, size=3, d=P(depth), p=P(prim)):
        return L.tamf_render_points(xy_, pos_, 1, V, h, w, size, 0, d, p, N)

    def shade(p=P(prim), xy_=P(xy), pos_=P(pos), f_=P(f), h=Hh, w=W, c_=H(col), li=H(lights), n=3, o=P(rgb)):
        return L.tamf_render_shade_mesh(p, xy_, pos_, N, f_, 1, V, Nf, h, w, 0, c_, AMBIENT, li, n, o, N)

    calls = [lambda: raster(w=0), lambda: raster(h=4097), lambda: raster(xy_=N), lambda: raster(pos_=N), lambda: raster(f_=N), lambda: raster(d=N),
             lambda: raster(p=N), lambda: raster(F=0), lambda: raster(base=-1),
             lambda: points(w=0), lambda: points(h=4097), lambda: points(size=2), lambda: points(size=0), lambda: points(size=17), lambda: points(xy_=N),
             lambda: points(pos_=N), lambda: points(d=N), lambda: points(p=N),
             lambda: shade(w=0), lambda: shade(h=4097), lambda: shade(n=9), lambda: shade(n=-1), lambda: shade(p=N), lambda: shade(xy_=N),
             lambda: shade(pos_=N), lambda: shade(f_=N), lambda: shade(c_=N), lambda: shade(li=N), lambda: shade(o=N),
             lambda: L.tamf_render_clear(P(depth), P(prim), 1, Hh, 0, N), lambda: L.tamf_render_clear(P(depth), P(prim), 1, 4097, W, N),
             lambda: L.tamf_render_clear(N, P(prim), 1, Hh, W, N), lambda: L.tamf_render_clear(P(depth), N, 1, Hh, W, N),
             lambda: L.tamf_render_fill(P(prim), 1, Hh, 0, H(col), P(rgb), N), lambda: L.tamf_render_fill(N, 1, Hh, W, H(col), P(rgb), N),
             lambda: L.tamf_render_fill(P(prim), 1, Hh, W, N, P(rgb), N), lambda: L.tamf_render_fill(P(prim), 1, Hh, W, H(col), N, N),
             lambda: L.tamf_render_shade_points(P(prim), 1, Hh, 0, 0, V, H(col), P(rgb), N), lambda: L.tamf_render_shade_points(N, 1, Hh, W, 0, V, H(col), P(rgb), N),
             lambda: L.tamf_render_shade_points(P(prim), 1, Hh, W, 0, V, H(col), N, N),
             lambda: L.tamf_render_project(N, N, ctypes.addressof(cam), 1, V, 0, P(pos_o), P(xy_o), N),
             lambda: L.tamf_render_project(P(verts), N, N, 1, V, 0, P(pos_o), P(xy_o), N),
             lambda: L.tamf_render_project(P(verts), N, ctypes.addressof(cam), 1, V, 0, N, P(xy_o), N),
             lambda: L.tamf_render_project(P(verts), N, ctypes.addressof(cam), 1, V, 0, P(pos_o), N, N),
             lambda: L.tamf_render_project(P(verts), N, ctypes.addressof(cam), 0, V, 0, P(pos_o), P(xy_o), N),
             lambda: L.tamf_render_project(P(verts), N, ctypes.addressof(cam), 1, 0, 0, P(pos_o), P(xy_o), N)]
    for k, call in enumerate(calls):
        assert call() == INVALID_ARG, k
        assert L.tamf_render_last_error(), k
    bad_cam = _cam(dict(sc["cam"], near=0.0))
    assert L.tamf_render_project(P(verts), N, ctypes.addressof(bad_cam), 1, V, 0, P(pos_o), P(xy_o), N) == INVALID_ARG
    torch.cuda.synchronize()
    assert bool((depth == 7.0).all()) and bool((prim == 3).all()) and bool((rgb == SENTINEL).all())
    assert bool((pos_o == 5.0).all()) and bool((xy_o == 5).all())
    assert raster() == 0 and shade() == 0  # the same arguments, valid: accepted
    torch.cuda.synchronize()
    assert bool((prim != 3).any()) and bool((rgb != SENTINEL).any())
