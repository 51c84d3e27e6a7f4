"""GPU: the renderer's second step through the C interface of libtamf_render.so and through render.HipRenderer, against the numpy
restatement of tests/render_layers_restatement.py fed the library's own projections: depth peeling (ids, coverage, depths, the tie rule
across calls), per-vertex and per-point colours, composite, resolve, determinism and frame independence, guard bands around every new
output, the refused arguments, and launch/render_samples.py end to end with the new flags."""
import json
import os
import pickle
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import render_layers_restatement as LR  # noqa: E402
import render_restatement as R  # noqa: E402
import render_scenes as S  # noqa: E402
import test_render_gpu as G  # noqa: E402  (its helpers: the library, pointers, project, run, the constants)

pytestmark = pytest.mark.gpu
P, H, ok = G.P, G.H, G.ok
SENTINEL, INVALID_ARG = G.SENTINEL, G.INVALID_ARG
ALPHAS = (0.4, 1.0, 0.6)  # per item, cycled
_cache = {}


def _faces(it):
    import torch

    return None if it["kind"] != "mesh" else torch.from_numpy(np.ascontiguousarray(it["faces"], np.int32)).cuda()


def peel(sc, K=LR.K, frames=None, out=None):
    """layer 0 by the plain calls, layers 1 .. K - 1 by the _behind calls over all items in ascending prim_base ->
    dict(proj [(pos, xy)], faces, depth (K,F,H,W), prim (K,F,H,W)) device tensors; out: (depth, prim) to draw into"""
    import torch

    L = G._lib()
    F, Hh, W = (sc["F"] if frames is None else len(frames)), sc["H"], sc["W"]
    depth, prim = out or (torch.empty((K, F, Hh, W), dtype=torch.float32, device="cuda"), torch.empty((K, F, Hh, W), dtype=torch.int32, device="cuda"))
    proj = [G.project(sc, it, frames) for it in sc["items"]]
    faces = [_faces(it) for it in sc["items"]]
    for k in range(K):
        ok(L.tamf_render_clear(P(depth[k]), P(prim[k]), F, Hh, W, None))
        for it, base, (pos, xy), f in zip(sc["items"], S.bases(sc), proj, faces):
            V = int(pos.shape[1])
            floor = () if k == 0 else (P(depth[k - 1]), P(prim[k - 1]))
            if it["kind"] == "mesh":
                fn = L.tamf_render_raster if k == 0 else L.tamf_render_raster_behind
                ok(fn(P(xy), P(pos), P(f), F, V, int(f.shape[0]), Hh, W, base, *floor, P(depth[k]), P(prim[k]), None))
            else:
                fn = L.tamf_render_points if k == 0 else L.tamf_render_points_behind
                ok(fn(P(xy), P(pos), F, V, Hh, W, it["point_size"], base, *floor, P(depth[k]), P(prim[k]), None))
    torch.cuda.synchronize()
    return dict(proj=proj, faces=faces, depth=depth, prim=prim)


def shade(sc, got, colors=None, rgb=None):
    """every layer of `got` shaded: item k by the _colors pass when colors = {k: device tensor (V,3) | (F,V,3)} names it, by the plain
    pass with G.BASE otherwise, then the background -> rgb (K,F,H,W,3)"""
    import torch

    L = G._lib()
    K, F, Hh, W = got["prim"].shape
    if rgb is None:
        rgb = torch.full((K, F, Hh, W, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    base_rgb, lights, bg = np.asarray(G.BASE, np.float32), G._lights(), np.asarray(G.BG, np.float32)
    for k in range(K):
        for i, (it, base, (pos, xy), f) in enumerate(zip(sc["items"], S.bases(sc), got["proj"], got["faces"])):
            c = None if colors is None else colors.get(i)
            V = int(pos.shape[1])
            if it["kind"] == "mesh" and c is None:
                ok(L.tamf_render_shade_mesh(P(got["prim"][k]), P(xy), P(pos), None, P(f), F, V, int(f.shape[0]), Hh, W, base, H(base_rgb), G.AMBIENT, H(lights),
                                            3, P(rgb[k]), None))
            elif it["kind"] == "mesh":
                ok(L.tamf_render_shade_mesh_colors(P(got["prim"][k]), P(xy), P(pos), None, P(f), F, V, int(f.shape[0]), Hh, W, base, P(c), int(c.dim() == 3),
                                                   G.AMBIENT, H(lights), 3, P(rgb[k]), None))
            elif c is None:
                ok(L.tamf_render_shade_points(P(got["prim"][k]), F, Hh, W, base, V, H(base_rgb), P(rgb[k]), None))
            else:
                ok(L.tamf_render_shade_points_colors(P(got["prim"][k]), F, Hh, W, base, V, P(c), int(c.dim() == 3), P(rgb[k]), None))
        ok(L.tamf_render_fill(P(got["prim"][k]), F, Hh, W, H(bg), P(rgb[k]), None))
    torch.cuda.synchronize()
    return rgb


def composite(sc, rgb, prim, alphas, out=None, bg=G.BG):
    import torch

    L = G._lib()
    K, F, Hh, W = prim.shape
    if out is None:
        out = torch.full((F, Hh, W, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    b, n, a = np.asarray(S.bases(sc), np.int32), np.asarray(S.counts(sc), np.int32), np.asarray(alphas, np.float32)
    ok(L.tamf_render_composite(P(rgb), P(prim), K, F, Hh, W, H(b), H(n), H(a), len(b), H(np.asarray(bg, np.float32)), P(out), None))
    torch.cuda.synchronize()
    return out


def case(name):
    """the scene peeled on the GPU, and the restatement (float64 and float32) fed the library's own xy and pos_cam: computed once"""
    if name not in _cache:
        sc = LR.scene(name)
        got = peel(sc)
        proj = [(p.cpu().numpy(), xy.cpu().numpy().astype(np.int64)) for p, xy in got["proj"]]
        _cache[name] = dict(scene=sc, got=got, proj=proj, r64=LR.Layers(LR.collect(sc, proj), LR.K), r32=LR.Layers(LR.collect(sc, proj, np.float32), LR.K))
    return _cache[name]


def _alphas(sc):
    return [ALPHAS[i % len(ALPHAS)] for i in range(len(sc["items"]))]


def _canaried(shape, dtype, G_=4096):
    """a tensor of `shape` inside a buffer with 4 KiB of 0xC3 on either side -> (the view, the raw buffer, its payload size in bytes)"""
    import torch

    size = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    raw = torch.full((2 * G_ + size,), 0xC3, dtype=torch.uint8, device="cuda")
    return raw[G_: G_ + size].view(dtype).view(shape), raw, size


def _intact(raw, size, G_=4096):
    return bool((raw[:G_] == 0xC3).all()) and bool((raw[G_ + size:] == 0xC3).all())


# ---- 1. peeling ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LR.NAMES)
def test_layers_equal_the_restatement(name):
    import torch

    c = case(name)
    sc, r64, r32 = c["scene"], c["r64"], c["r32"]
    prim, depth = c["got"]["prim"].cpu().numpy().astype(np.int64), c["got"]["depth"].cpu().numpy()
    tie = r64.near_tie
    covered = r64.count > 0
    share = tie.sum() / covered.sum()
    print(f"RENDER layers {name}: covered {int(covered.sum())} near ties {int(tie.sum())} (share {share:.5f}); per layer covered "
          f"{[int((prim[k] >= 0).sum()) for k in range(LR.K)]}, id mismatches outside ties {[int(((prim[k] != r64.prim_id[k]) & ~tie).sum()) for k in range(LR.K)]}")
    assert covered.sum() > 100 and share <= 0.005
    for k in range(LR.K):
        assert np.array_equal(prim[k][~tie], r64.prim_id[k][~tie]), k
        assert np.array_equal(prim[k] >= 0, r64.prim_id[k] >= 0), k  # coverage is integer arithmetic: exact, ties or not
        empty = prim[k] < 0
        assert np.isinf(depth[k][empty]).all() and (depth[k][empty] > 0).all() and (prim[k][empty] == -1).all()
    # depths: the existing gate, 4 x the float32 restatement's own error - over all layers, and per layer where the layer has enough
    # pixels for the maximum of the restatement's error to be an estimate (a maximum over a handful of pixels is not one)
    same = (prim >= 0) & (prim == r64.prim_id) & (r32.prim_id == r64.prim_id)
    scale = r64.depth[same].max()
    for k in [None] + list(range(LR.K)):
        m = same if k is None else same & (np.arange(LR.K) == k)[:, None, None, None]
        if k is not None and m.sum() < 300:
            continue
        hip_dev, ref_dev = np.abs(depth[m] - r64.depth[m]).max() / scale, np.abs(r32.depth[m].astype(np.float64) - r64.depth[m]).max() / scale
        print(f"RENDER layers depth {name} layer {k}: hip {hip_dev:.3e}  float32 restatement {ref_dev:.3e}  gate {4 * ref_dev:.3e}  pixels {int(m.sum())}")
        assert ref_dev > 0 and hip_dev <= 4 * ref_dev, k
    # layer 0 is the plain pipeline's output, bit for bit
    plain = G.run(sc)
    assert torch.equal(c["got"]["depth"][0], plain["depth"]) and torch.equal(c["got"]["prim"][0], plain["prim"])
    # on the GPU's own output: (depth, id) strictly increases over the layers at every pixel - so no (pixel, id) appears twice - and
    # no layer is covered where the one before it is not
    for k in range(1, LR.K):
        m = prim[k] >= 0
        assert (prim[k - 1][m] >= 0).all()
        d0, d1, i0, i1 = depth[k - 1][m], depth[k][m], prim[k - 1][m], prim[k][m]
        assert ((d1 > d0) | ((d1 == d0) & (i1 > i0))).all(), k
    stack = np.where(prim >= 0, prim, -np.arange(1, LR.K + 1)[:, None, None, None])  # (empty layers made distinct)
    srt = np.sort(stack, axis=0)
    assert (srt[1:] != srt[:-1]).all()


def test_a_tie_across_calls_goes_to_the_lower_id_then_the_higher():
    import torch

    L = G._lib()
    W = Hh = 32
    sc = dict(F=1, cam=R.camera(W, Hh))
    tri = np.array([[-1.0, -1.0, 3.0], [1.0, -1.0, 3.0], [0.0, 1.2, 3.3]])
    pos, xy = G.project(sc, dict(verts=np.concatenate([tri, tri]), model=None))
    depth = torch.empty((3, 1, Hh, W), dtype=torch.float32, device="cuda")
    prim = torch.empty((3, 1, Hh, W), dtype=torch.int32, device="cuda")
    calls = [(torch.tensor([[0, 1, 2]], dtype=torch.int32, device="cuda"), 7), (torch.tensor([[3, 5, 4]], dtype=torch.int32, device="cuda"), 1000)]
    for k in range(3):
        ok(L.tamf_render_clear(P(depth[k]), P(prim[k]), 1, Hh, W, None))
        for f, base in calls:  # ascending prim_base
            if k == 0:
                ok(L.tamf_render_raster(P(xy), P(pos), P(f), 1, 6, 1, Hh, W, base, P(depth[k]), P(prim[k]), None))
            else:
                ok(L.tamf_render_raster_behind(P(xy), P(pos), P(f), 1, 6, 1, Hh, W, base, P(depth[k - 1]), P(prim[k - 1]), P(depth[k]), P(prim[k]), None))
    torch.cuda.synchronize()
    m = prim[0] >= 0
    assert int(m.sum()) > 50
    assert bool((prim[0][m] == 7).all()) and bool((prim[1][m] == 1000).all()) and bool((prim[1][~m] == -1).all()) and bool((prim[2] == -1).all())
    assert torch.equal(depth[0], depth[1]) and bool(torch.isinf(depth[2]).all())
    # within one call: the lower index first, then the higher
    both = torch.tensor([[0, 1, 2], [3, 5, 4]], dtype=torch.int32, device="cuda")
    for k in range(3):
        ok(L.tamf_render_clear(P(depth[k]), P(prim[k]), 1, Hh, W, None))
        if k == 0:
            ok(L.tamf_render_raster(P(xy), P(pos), P(both), 1, 6, 2, Hh, W, 0, P(depth[k]), P(prim[k]), None))
        else:
            ok(L.tamf_render_raster_behind(P(xy), P(pos), P(both), 1, 6, 2, Hh, W, 0, P(depth[k - 1]), P(prim[k - 1]), P(depth[k]), P(prim[k]), None))
    torch.cuda.synchronize()
    assert bool((prim[0][m] == 0).all()) and bool((prim[1][m] == 1).all()) and bool((prim[2] == -1).all()) and torch.equal(depth[0], depth[1])


# ---- 3. colours -----------------------------------------------------------------------------------------------------------------------
def _palettes(sc, per_frame_item=None):
    out = {}
    for i, it in enumerate(sc["items"]):
        out[i] = LR.vertex_palette(int(np.asarray(it["verts"]).shape[-2]), 100 + i, sc["F"] if i == per_frame_item else None)
    return out


@pytest.mark.parametrize("name,per_frame_item", [("soup", None), ("points_mesh", None), ("hand_spheres", 0)])
def test_colours_within_one_level_of_the_restatement(name, per_frame_item):
    """layer 0 and layer 1 of the peeled scene, every item through its _colors pass (hand_spheres: the hand's colours per frame, F = 3)"""
    import torch

    c = case(name)
    sc = c["scene"]
    pal = _palettes(sc, per_frame_item)
    got = dict(c["got"], prim=c["got"]["prim"][:2].contiguous())
    rgb = shade(sc, got, {i: torch.from_numpy(p).cuda() for i, p in pal.items()}).cpu().numpy()
    prim = got["prim"].cpu().numpy().astype(np.int64)
    lights = G._lights().astype(np.float64)
    worst = 0
    for k in range(2):
        want = np.full(prim[k].shape + (3,), SENTINEL, np.uint8)
        for i, (it, base, (pos, xy)) in enumerate(zip(sc["items"], S.bases(sc), c["proj"])):
            if it["kind"] == "mesh":
                LR.shade_mesh_colors(want, prim[k], xy, pos, None, it["faces"], base, pal[i], G.AMBIENT, lights)
            else:
                LR.shade_points_colors(want, prim[k], base, pal[i])
        R.fill(want, prim[k], np.asarray(G.BG, np.float32))
        diff = np.abs(rgb[k].astype(np.int64) - want.astype(np.int64))
        worst = max(worst, int(diff.max()))
        assert diff.max() <= 1, k  # (the restatement shades the GPU's own ids: they agree everywhere)
        assert (rgb[k] != SENTINEL).any(axis=-1)[prim[k] >= 0].all()
        assert len(np.unique(rgb[k][prim[k] >= 0], axis=0)) > 50  # the colours do vary
    print(f"RENDER colours {name}: max channel difference {worst}")
    if per_frame_item is not None:  # the frames were given different colours and show them
        n = S.counts(sc)[per_frame_item]
        m = (prim[0][0] == prim[0][1]) & (prim[0][0] >= 0) & (prim[0][0] < n)
        assert (rgb[0][0][m] != rgb[0][1][m]).any()


@pytest.mark.parametrize("name", ["soup", "hand_spheres"])
def test_equal_vertex_colours_give_the_bytes_of_the_constant_colour_pass(name):
    import torch

    c = case(name)
    sc = c["scene"]
    got = dict(c["got"], prim=c["got"]["prim"][:2].contiguous())
    cols = {i: torch.from_numpy(np.tile(np.asarray(G.BASE, np.float32), (int(np.asarray(it["verts"]).shape[-2]), 1))).cuda()
            for i, it in enumerate(sc["items"]) if it["kind"] == "mesh"}
    a, b = shade(sc, got), shade(sc, got, cols)
    assert torch.equal(a, b) and bool((a != SENTINEL).any())
    per_frame = {i: t[None].expand(sc["F"], -1, -1).contiguous() for i, t in cols.items()}
    assert torch.equal(a, shade(sc, got, per_frame))


def test_a_colour_pass_writes_inside_its_own_id_range_only():
    import torch

    L = G._lib()
    c = case("points_mesh")
    sc, got = c["scene"], c["got"]
    F, Hh, W = sc["F"], sc["H"], sc["W"]
    prim = got["prim"][0]
    for i, it in enumerate(sc["items"]):
        base, count = S.bases(sc)[i], S.counts(sc)[i]
        pos, xy = got["proj"][i]
        col = torch.from_numpy(LR.vertex_palette(int(pos.shape[1]), 7) * 0.5 + 0.5).cuda()  # (no channel rounds to the sentinel's neighbourhood by design: >= 0.5)
        rgb = torch.full((F, Hh, W, 3), 0, dtype=torch.uint8, device="cuda")
        if it["kind"] == "mesh":
            ok(L.tamf_render_shade_mesh_colors(P(prim), P(xy), P(pos), None, P(got["faces"][i]), F, int(pos.shape[1]), count, Hh, W, base, P(col), 0, 1.0, None, 0,
                                               P(rgb), None))
        else:
            ok(L.tamf_render_shade_points_colors(P(prim), F, Hh, W, base, count, P(col), 0, P(rgb), None))
        torch.cuda.synchronize()
        mine = (prim >= base) & (prim < base + count)
        assert bool(mine.any()) and bool((~mine).any()), i
        assert bool((rgb[~mine] == 0).all()) and bool((rgb[mine] >= 127).all()), i  # ambient 1, no lights: the colour itself, >= 0.5


# ---- 4. composite ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["shells", "points_mesh", "hand_spheres"])
def test_composite_within_one_level_of_the_restatement(name):
    c = case(name)
    sc, got = c["scene"], c["got"]
    rgb = shade(sc, got)
    alphas = _alphas(sc)
    out = composite(sc, rgb, got["prim"], alphas).cpu().numpy()
    want, exact = LR.composite(rgb.cpu().numpy(), got["prim"].cpu().numpy().astype(np.int64), S.bases(sc), S.counts(sc), alphas, G.BG)
    diff = np.abs(out.astype(np.int64) - want.astype(np.int64))
    print(f"RENDER composite {name}: max channel difference {int(diff.max())}, pixels that differ {int((diff > 0).any(axis=-1).sum())} of {diff[..., 0].size}")
    assert diff.max() <= 1
    assert np.abs(out / 255.0 - exact).max() <= 0.5 / 255 + 1e-5  # the byte is the rounding of (nearly) the float64 colour
    # an alpha-1 item hides what lies behind it: with the bytes of every layer behind an opaque fragment replaced, the image is the same
    import torch

    prim = got["prim"]
    opaque = torch.zeros_like(prim, dtype=torch.bool)
    for b, n, a in zip(S.bases(sc), S.counts(sc), alphas):
        if a == 1.0:
            opaque |= (prim >= b) & (prim < b + n)
    behind = (torch.cumsum(opaque.to(torch.int32), dim=0) - opaque.to(torch.int32)) > 0  # layers strictly behind an opaque fragment
    assert int((behind & (prim >= 0)).sum()) > 20
    scrambled = torch.where(behind[..., None], torch.full_like(rgb, 255) - rgb, rgb)
    assert not torch.equal(scrambled, rgb) and np.array_equal(composite(sc, scrambled, prim, alphas).cpu().numpy(), out)
    first = (prim[0] >= 0) & opaque[0]
    assert np.array_equal(out[first.cpu().numpy()], rgb[0].cpu().numpy()[first.cpu().numpy()])  # and in front it is drawn as it is
    # a see-through one does not hide: where one is the nearest fragment and something lies behind it, the layers behind show
    seen = ((prim[0] >= 0) & ~opaque[0] & (prim[1] >= 0)).cpu().numpy()
    assert (out[seen] != rgb[0].cpu().numpy()[seen]).any(axis=-1).sum() > 20


@pytest.mark.parametrize("name", ["soup", "hand_spheres", "points_mesh"])
def test_composite_of_one_opaque_layer_is_the_plain_render(name):
    import torch

    sc = LR.scene(name)
    plain = G.run(sc)
    one = composite(sc, plain["rgb"][None].contiguous(), plain["prim"][None].contiguous(), [1.0] * len(sc["items"]))
    assert torch.equal(one, plain["rgb"])
    # and the deeper layers of an all-opaque scene change nothing
    c = case(name)
    rgb = shade(sc, c["got"])
    assert torch.equal(composite(sc, rgb, c["got"]["prim"], [1.0] * len(sc["items"])), plain["rgb"])


# ---- 5. resolve -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("s", [2, 3, 4])
def test_resolve_is_the_integer_mean(s):
    import torch

    from oakink2_tamf_amd import render

    L = G._lib()
    sc = LR.scene("hand_spheres")
    W, Hh, F = 25, 19, sc["F"]  # (neither a multiple of anything in sight)
    cam = sc["cam"]
    k = s * W / sc["W"]
    rd = render.HipRenderer(s * W, s * Hh, "cuda:0", background=G.BG, ambient=G.AMBIENT)
    for it in sc["items"]:
        rd.add_mesh(it["verts"], it["faces"], color=G.BASE, pose=it["model"])
    big = rd.render(render.Camera(cam["view"], cam["fx"] * k, cam["fy"] * k, cam["cx"] * k, cam["cy"] * k, cam["near"]))[0]
    assert len(torch.unique(big)) > 50
    out, raw, size = _canaried((F, Hh, W, 3), torch.uint8)
    ok(L.tamf_render_resolve(P(big), F, Hh, W, s, P(out), None))
    torch.cuda.synchronize()
    assert _intact(raw, size)
    assert np.array_equal(out.cpu().numpy(), LR.resolve(big.cpu().numpy(), s))
    const = torch.full((2, s * 5, s * 7, 3), 201, dtype=torch.uint8, device="cuda")
    flat = torch.zeros((2, 5, 7, 3), dtype=torch.uint8, device="cuda")
    ok(L.tamf_render_resolve(P(const), 2, 5, 7, s, P(flat), None))
    torch.cuda.synchronize()
    assert bool((flat == 201).all())
    noise = torch.from_numpy(np.random.default_rng(s).integers(0, 256, size=(2, s * 5, s * 7, 3), dtype=np.uint8)).cuda()
    ok(L.tamf_render_resolve(P(noise), 2, 5, 7, s, P(flat), None))
    torch.cuda.synchronize()
    assert np.array_equal(flat.cpu().numpy(), LR.resolve(noise.cpu().numpy(), s))


# ---- 6. HipRenderer -------------------------------------------------------------------------------------------------------------------
HAND_RGB, OBJ_RGB = (0.9, 0.6, 0.3), (0.2, 0.5, 0.9)  # no pair of light levels makes a shade of one a shade of the other in all channels


def _renderer(sc, width=None, height=None, obj_alpha=1.0, point_scale=1, hand_colors=None):
    from oakink2_tamf_amd import render

    rd = render.HipRenderer(width or sc["W"], height or sc["H"], "cuda:0", background=G.BG, ambient=G.AMBIENT)
    for i, it in enumerate(sc["items"]):
        first = i == 0
        if it["kind"] == "mesh":
            rd.add_mesh(it["verts"], it["faces"], color=HAND_RGB if first else OBJ_RGB, pose=it["model"], alpha=1.0 if first else obj_alpha,
                        vertex_colors=hand_colors if first else None)
        else:
            rd.add_points(it["verts"], color=HAND_RGB if first else OBJ_RGB, pose=it["model"], point_size=it["point_size"] * point_scale + (point_scale > 1),
                          alpha=1.0 if first else obj_alpha)
    return rd


def _camera(sc, k=1):
    from oakink2_tamf_amd import render

    c = sc["cam"]
    return render.Camera(c["view"], c["fx"] * k, c["fy"] * k, c["cx"] * k, c["cy"] * k, c["near"])


def test_renderer_defaults_are_the_plain_path_and_see_through_objects_show_the_hand_behind():
    import torch

    c = case("hand_spheres")
    sc, r64 = c["scene"], c["r64"]
    cam = _camera(sc)
    rd = _renderer(sc)
    a, b = rd.render(cam), rd.render(cam, layers=1, ssaa=1)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    plain = G.case("hand_spheres")["got"]  # the raw calls of the existing tests: ids and depths do not depend on the colours
    assert torch.equal(a[1], plain["depth"]) and torch.equal(a[2], plain["prim"])
    assert rd.frames_per_chunk() == rd.frames_per_chunk(1, 1) and rd.frames_per_chunk(4, 2) <= rd.frames_per_chunk()
    opaque4 = rd.render(cam, layers=4)  # every alpha 1: deeper layers are hidden
    assert torch.equal(opaque4[0], a[0]) and torch.equal(opaque4[1], a[1]) and torch.equal(opaque4[2], a[2])
    see = _renderer(sc, obj_alpha=0.4).render(cam, layers=4)
    assert torch.equal(see[1], a[1]) and torch.equal(see[2], a[2])  # depth and prim_id are layer 0's, whatever the alphas
    n_hand = S.counts(sc)[0]
    obj0, hand1 = r64.prim_id[0] >= n_hand, (r64.prim_id[1] >= 0) & (r64.prim_id[1] < n_hand)
    behind = obj0 & hand1 & ~r64.near_tie  # the restatement: a hand fragment right behind an object's nearest fragment
    deeper = obj0 & ((r64.prim_id[1:] >= 0) & (r64.prim_id[1:] < n_hand)).any(axis=0) & ~r64.near_tie
    differs = (see[0] != a[0]).any(dim=-1).cpu().numpy()
    print(f"RENDER see-through: {int(behind.sum())} pixels with the hand right behind an object, {int(deeper.sum())} with it in layers 1 .. 3; "
          f"{int(differs[deeper].sum())} of those differ from the opaque render")
    assert behind.sum() > 50 and differs[behind].all()
    hand0 = (r64.prim_id[0] >= 0) & (r64.prim_id[0] < n_hand)
    assert not differs[hand0 & ~r64.near_tie].any() and not differs[r64.count == 0].any()  # the opaque hand in front, and the background, stay


@pytest.mark.parametrize("name", ["hand_spheres", "points_mesh"])
def test_renderer_ssaa_is_the_resolve_of_the_doubled_render(name):
    import torch

    L = G._lib()
    sc = LR.scene(name)
    F, Hh, W = sc["F"], sc["H"], sc["W"]
    small = _renderer(sc, obj_alpha=0.4).render(_camera(sc), layers=3, ssaa=2)
    big = _renderer(sc, 2 * W, 2 * Hh, obj_alpha=0.4, point_scale=2).render(_camera(sc, 2), layers=3)  # splats of 2 * 3 + 1 = 7 pixels
    want = torch.empty((F, Hh, W, 3), dtype=torch.uint8, device="cuda")
    ok(L.tamf_render_resolve(P(big[0]), F, Hh, W, 2, P(want), None))
    torch.cuda.synchronize()
    assert torch.equal(small[0], want)
    assert torch.equal(small[1], big[1][:, ::2, ::2]) and torch.equal(small[2], big[2][:, ::2, ::2])  # the top-left sub-sample


def test_renderer_same_call_twice_frames_alone_and_chunks(monkeypatch):
    import torch

    from oakink2_tamf_amd import render

    sc = LR.scene("hand_spheres")
    pal = LR.vertex_palette(778, 3, sc["F"])
    rd = _renderer(sc, obj_alpha=0.4, hand_colors=pal)
    cam = _camera(sc)
    a, b = rd.render(cam, layers=4, ssaa=2), rd.render(cam, layers=4, ssaa=2)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    alone = rd.render(cam, frames=[1], layers=4, ssaa=2)
    for x, y in zip(alone, a):
        assert torch.equal(x[0], y[1])
    assert not torch.equal(a[0][0], a[0][1])
    monkeypatch.setattr(render, "PROJECTION_BYTES", 1)  # one frame per chunk
    assert rd.frames_per_chunk(4, 2) == 1
    for x, y in zip(rd.render(cam, layers=4, ssaa=2), a):
        assert torch.equal(x, y)
    flat = _renderer(sc, obj_alpha=0.4).render(cam, layers=4, ssaa=2)
    assert not torch.equal(flat[0], a[0]) and torch.equal(flat[2], a[2])  # the hand's colours are drawn


def test_renderer_refuses_before_any_device_call():
    from oakink2_tamf_amd import render

    sc = LR.scene("soup")
    it = sc["items"][0]
    V = it["verts"].shape[0]
    rd = render.HipRenderer(sc["W"], sc["H"], "cuda:0")
    bad_colours = [np.zeros((V, 4), np.float32), np.zeros((V + 1, 3), np.float32), np.zeros((2, V + 1, 3), np.float32), np.zeros((V * 3,), np.float32),
                   np.zeros((V, 3), np.int64), np.full((V, 3), np.nan, np.float32), np.full((V, 3), np.inf, np.float32)]
    for c in bad_colours:
        with pytest.raises(ValueError):
            rd.add_mesh(it["verts"], it["faces"], vertex_colors=c)
        with pytest.raises(ValueError):
            rd.add_points(it["verts"], point_colors=c)
    for alpha in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="alpha"):
            rd.add_mesh(it["verts"], it["faces"], alpha=alpha)
        with pytest.raises(ValueError, match="alpha"):
            rd.add_points(it["verts"], alpha=alpha)
    assert rd.items == []
    rd.add_mesh(it["verts"], it["faces"], vertex_colors=np.zeros((V, 3), np.float32), alpha=0.5)
    cam = _camera(sc)
    for kw in (dict(layers=0), dict(layers=9), dict(ssaa=0), dict(ssaa=5)):
        with pytest.raises(ValueError):
            rd.render(cam, **kw)
    wide = render.HipRenderer(2049, 8, "cuda:0")
    wide.add_mesh(it["verts"], it["faces"])
    with pytest.raises(ValueError, match="4096"):
        wide.render(cam, ssaa=2)
    rd.add_points(it["verts"], point_size=5)
    with pytest.raises(ValueError, match="point_size"):
        rd.render(cam, ssaa=4)  # a splat of 21 pixels
    with pytest.raises(ValueError, match="frames"):  # 2 frames of colours on a 3-frame item
        rd.add_mesh(np.zeros((3, V, 3), np.float32), it["faces"], vertex_colors=np.zeros((2, V, 3), np.float32))


# ---- guard bands ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,Hh", [(37, 29), (1, 1)])
def test_canaries_around_every_new_output(W, Hh):
    import torch

    base = LR.scene("points_mesh")
    sc = dict(base, W=W, H=Hh, cam=R.camera(W, Hh, fov_deg=40.0) if W > 1 else dict(R.camera(1, 1), fx=0.2, fy=0.2))
    K, F = 3, 1
    depth, raw_d, size_d = _canaried((K, F, Hh, W), torch.float32)
    prim, raw_p, size_p = _canaried((K, F, Hh, W), torch.int32)
    rgb, raw_c, size_c = _canaried((K, F, Hh, W, 3), torch.uint8)
    out, raw_o, size_o = _canaried((F, Hh, W, 3), torch.uint8)
    got = peel(sc, K, out=(depth, prim))
    pal = {i: torch.from_numpy(p).cuda() for i, p in _palettes(sc).items()}
    shade(sc, got, pal, rgb=rgb)
    composite(sc, rgb, prim, _alphas(sc), out=out)
    for raw, size in ((raw_d, size_d), (raw_p, size_p), (raw_c, size_c), (raw_o, size_o)):
        assert _intact(raw, size)
    assert bool((prim[0] >= 0).any()) and bool((prim[1] >= 0).any())
    proj = [(p.cpu().numpy(), xy.cpu().numpy().astype(np.int64)) for p, xy in got["proj"]]
    ref = LR.Layers(LR.collect(sc, proj), K)
    for k in range(K):
        assert np.array_equal(prim[k].cpu().numpy()[~ref.near_tie], ref.prim_id[k][~ref.near_tie]), k


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def test_rejected_arguments_launch_nothing():
    import torch

    L = G._lib()
    c = case("soup")
    sc, got = c["scene"], c["got"]
    W, Hh = sc["W"], sc["H"]
    pos, xy = got["proj"][0]
    f = got["faces"][0]
    V, Nf = int(pos.shape[1]), int(f.shape[0])
    fd, fi = got["depth"][0], got["prim"][0]  # a floor with covered pixels: a launched pass would draw behind it
    depth = torch.full((1, Hh, W), 7.0, dtype=torch.float32, device="cuda")
    prim = torch.full((1, Hh, W), 3, dtype=torch.int32, device="cuda")  # an id inside every range below: a launched pass would write
    rgb = torch.full((1, Hh, W, 3), SENTINEL, dtype=torch.uint8, device="cuda")
    col = torch.full((V, 3), 0.5, dtype=torch.float32, device="cuda")
    lights = np.ascontiguousarray(np.tile(G._lights()[:1], (9, 1)))
    layers_rgb = torch.full((9, 1, Hh, W, 3), 9, dtype=torch.uint8, device="cuda")
    layers_id = torch.full((9, 1, Hh, W), 3, dtype=torch.int32, device="cuda")
    big = torch.full((1, 4 * Hh, 4 * W, 3), 9, dtype=torch.uint8, device="cuda")
    one = np.ones(65, np.int32)
    bases65, alpha65 = np.arange(65, dtype=np.int32), np.ones(65, np.float32)
    bg = np.asarray(G.BG, np.float32)
    N = None

    def behind(xy_=P(xy), pos_=P(pos), f_=P(f), F=1, h=Hh, w=W, base=0, fd_=P(fd), fi_=P(fi), d=P(depth), p=P(prim)):
        return L.tamf_render_raster_behind(xy_, pos_, f_, F, V, Nf, h, w, base, fd_, fi_, d, p, N)

    def pbehind(xy_=P(xy), pos_=P(pos), h=Hh, w=W, size=3, fd_=P(fd), fi_=P(fi), d=P(depth), p=P(prim)):
        return L.tamf_render_points_behind(xy_, pos_, 1, V, h, w, size, 0, fd_, fi_, d, p, N)

    def mcol(p=P(prim), xy_=P(xy), pos_=P(pos), f_=P(f), h=Hh, w=W, c_=P(col), li=H(lights), n=3, o=P(rgb)):
        return L.tamf_render_shade_mesh_colors(p, xy_, pos_, N, f_, 1, V, Nf, h, w, 0, c_, 0, G.AMBIENT, li, n, o, N)

    def pcol(p=P(prim), h=Hh, w=W, count=V, c_=P(col), o=P(rgb)):
        return L.tamf_render_shade_points_colors(p, 1, h, w, 0, count, c_, 0, o, N)

    def comp(r=P(layers_rgb), i=P(layers_id), K=2, h=Hh, w=W, b=H(bases65), n=H(one), a=H(alpha65), items=2, bg_=H(bg), o=P(rgb)):
        return L.tamf_render_composite(r, i, K, 1, h, w, b, n, a, items, bg_, o, N)

    def res(i=P(big), h=Hh, w=W, s=2, o=P(rgb)):
        return L.tamf_render_resolve(i, 1, h, w, s, o, N)

    a0, a2, anan = np.float32([1.0, 0.0]), np.float32([1.0, 1.5]), np.float32([np.nan, 1.0])
    overlap, descending = np.int32([0, 0]), np.int32([5, 0])
    calls = [lambda: behind(fd_=N), lambda: behind(fi_=N), lambda: behind(xy_=N), lambda: behind(pos_=N), lambda: behind(f_=N), lambda: behind(d=N),
             lambda: behind(p=N), lambda: behind(w=0), lambda: behind(h=4097), lambda: behind(F=0), lambda: behind(base=-1),
             lambda: behind(fd_=P(depth)), lambda: behind(fi_=P(prim)),
             lambda: pbehind(fd_=N), lambda: pbehind(fi_=N), lambda: pbehind(xy_=N), lambda: pbehind(pos_=N), lambda: pbehind(d=N), lambda: pbehind(p=N),
             lambda: pbehind(size=2), lambda: pbehind(size=17), lambda: pbehind(w=0), lambda: pbehind(fd_=P(depth)),
             lambda: mcol(c_=N), lambda: mcol(p=N), lambda: mcol(xy_=N), lambda: mcol(pos_=N), lambda: mcol(f_=N), lambda: mcol(o=N), lambda: mcol(n=9),
             lambda: mcol(n=-1), lambda: mcol(li=N), lambda: mcol(w=0), lambda: mcol(h=4097),
             lambda: pcol(c_=N), lambda: pcol(p=N), lambda: pcol(o=N), lambda: pcol(w=0), lambda: pcol(count=0),
             lambda: comp(K=0), lambda: comp(K=9), lambda: comp(items=65), lambda: comp(items=0), lambda: comp(a=H(a0)), lambda: comp(a=H(a2)),
             lambda: comp(a=H(anan)), lambda: comp(b=H(overlap)), lambda: comp(b=H(descending)), lambda: comp(n=H(np.int32([0, 1]))), lambda: comp(r=N),
             lambda: comp(i=N), lambda: comp(b=N), lambda: comp(n=N), lambda: comp(a=N), lambda: comp(bg_=N), lambda: comp(o=N), lambda: comp(w=0),
             lambda: comp(h=4097), lambda: comp(bg_=H(np.float32([np.nan, 0, 0]))),
             lambda: res(s=5), lambda: res(s=1), lambda: res(s=0), lambda: res(w=2049), lambda: res(h=2049, s=2), lambda: res(w=1025, s=4), lambda: res(i=N),
             lambda: res(o=N), lambda: res(w=0)]
    for k, call in enumerate(calls):
        assert call() == INVALID_ARG, k
        assert L.tamf_render_last_error(), k
    torch.cuda.synchronize()
    assert bool((depth == 7.0).all()) and bool((prim == 3).all()) and bool((rgb == SENTINEL).all())
    for call in (behind, pbehind, mcol, pcol):  # the same arguments, valid: accepted, and they do write
        assert call() == 0
    assert comp(K=8, items=64) == 0 and res(s=4) == 0
    torch.cuda.synchronize()
    assert bool((prim != 3).any()) and bool((rgb != SENTINEL).any())


# ---- 8. the launcher --------------------------------------------------------------------------------------------------------------------
def test_render_samples_with_the_new_flags(tmp_path, monkeypatch):
    import test_render_launch_gpu as LG

    from oakink2_tamf_amd import render
    from oakink2_tamf_amd.launch import render_samples as L

    paths, cache, tree = LG._tree(str(tmp_path))
    for i in range(len(cache["interaction_segment_info_list"])):  # the objects INTO the hand: contact, and occlusion
        Ln, tsl, traj = cache["interaction_segment_len_list"][i], cache["interaction_segment_tsl_list"][i], cache["interaction_segment_obj_traj_list"][i]
        for k, o in enumerate(sorted(traj)):
            traj[o][:Ln, :3, 3] = tsl[:Ln] + np.asarray(((0.10, 0.0, -0.03), (0.06, 0.02, 0.04))[k], np.float32)
    with open(paths["cache"], "wb") as f:
        pickle.dump(cache, f)
    monkeypatch.chdir(tmp_path)
    data = ["--data.cache_dict_filepath", paths["cache"], "--data.obj_embedding_prefix", paths["emb"], "--data.obj_pointcloud_prefix", paths["pc"],
            "--debug.sample_refine_filepath", tree, "--render.width", "64", "--render.height", "64", "--max_clips", "1", "--render.every", "4",
            "--data.obj_model_loader", "oracle.fixtures:synthetic_object_mesh"]
    info, length = cache["interaction_segment_info_list"][0], cache["interaction_segment_len_list"][0]
    frames = list(range(0, length, 4))

    def run(tag, extra):
        out = tmp_path / tag
        assert L.main(data + extra + ["--out_dir", str(out), "--out_json", str(tmp_path / (tag + ".json"))]) == 0
        return L.clip_dir(str(out), info), json.load(open(tmp_path / (tag + ".json")))

    d_new, index = run("new", ["--render.contact_map", "--render.obj_alpha", "0.4", "--render.ssaa", "2", "--render.apng"])
    assert sorted(os.listdir(d_new)) == sorted(["frame_%04d.png" % f for f in frames] + ["sheet.png", "clip.apng"])
    clip = index["clips"][0]
    assert clip["apng"] == "clip.apng" and clip["frames"] == frames
    assert index["display"] == {"contact_map": True, "contact_far_mm": 30.0, "obj_alpha": 0.4, "layers": 4, "ssaa": 2, "apng": True, "apng_fps": 10}
    images = np.stack([render.read_png(os.path.join(d_new, "frame_%04d.png" % f)) for f in frames])
    assert images.shape == (len(frames), 64, 64, 3)
    anim, fps = render.read_apng(os.path.join(d_new, "clip.apng"))
    assert np.array_equal(anim, images) and fps == 10
    assert np.array_equal(render.read_png(os.path.join(d_new, "clip.apng")), images[0])
    # the same picture without the heat map: what differs is the hand, and the heat map gives it more than one hue
    d_flat, _ = run("flat", ["--render.obj_alpha", "0.4", "--render.ssaa", "2"])
    flat = np.stack([render.read_png(os.path.join(d_flat, "frame_%04d.png" % f)) for f in frames])
    hand = (images != flat).any(axis=-1)
    px = images[hand].astype(np.float64)
    ratio = px[:, 1] / np.maximum(px[:, 0], 1.0)  # green over red: 0.79 for the hand's own colour, 0.1 for the contact colour
    print(f"RENDER launcher: {int(hand.sum())} hand pixels recoloured, green / red from {ratio.min():.2f} to {ratio.max():.2f}")
    assert hand.sum() > 50 and ratio.max() - ratio.min() > 0.2
    # see-through objects show something behind them: the picture differs from the opaque one
    d_plain, plain_index = run("plain", [])
    assert "display" not in plain_index and "apng" not in plain_index["clips"][0]
    assert sorted(os.listdir(d_plain)) == sorted(["frame_%04d.png" % f for f in frames] + ["sheet.png"])
    # the new flags spelled at their defaults write the files of a run without them, byte for byte
    d_spelled, _ = run("spelled", ["--render.obj_alpha", "1.0", "--render.layers", "1", "--render.ssaa", "1", "--render.contact_far_mm", "30",
                                   "--render.apng_fps", "10"])
    for name in sorted(os.listdir(d_plain)):
        assert open(os.path.join(d_plain, name), "rb").read() == open(os.path.join(d_spelled, name), "rb").read(), name
    assert sorted(os.listdir(d_spelled)) == sorted(os.listdir(d_plain))
    opaque = np.stack([render.read_png(os.path.join(d_plain, "frame_%04d.png" % f)) for f in frames])
    d_see, _ = run("see", ["--render.obj_alpha", "0.4"])
    see = np.stack([render.read_png(os.path.join(d_see, "frame_%04d.png" % f)) for f in frames])
    assert (see != opaque).any(axis=-1).sum() > 50
    # an item without a point cloud cannot have a heat map: refused with a message, before anything is drawn
    import mano_fixture

    from oakink2_tamf_amd.launch import _score_common as C
    from oakink2_tamf_amd.launch.compute_score_siv import resolve_loader

    cfg = L.parse_args(data + ["--render.contact_map", "--out_dir", str(tmp_path / "refused")])
    item = dict(C.load_pairs(cfg, obj_model_loader=resolve_loader(cfg["data"]["obj_model_loader"]))[0][0])
    assert item.pop("obj_pointcloud") is not None
    arr = mano_fixture.synthetic_arrays(778)
    verts = np.tile(arr["v_template"][None], (LG.T, 1, 1)).astype(np.float32)
    with pytest.raises(SystemExit, match="obj_pointcloud"):
        L.render_clip(item, [(verts, L.HAND_COLOR)], arr["faces"], cfg, "cuda:0")
