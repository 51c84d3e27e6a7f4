"""GPU: the per-step scratch operands (Q | K, attention output, hidden activations, input-merge rows) hold nothing that a step needs
from an earlier one - whichever bytes they share.

scratch_layout (csrc/tamf_shapes.h) makes Q | K, the attention output and the input-merge rows views of the hidden operand's allocation
when ff >= 3 d.  What used to be allocation-time zeros beyond the rows a call writes - the clips between a call's batch and max_batch,
the clamped rows of a partial row tile (T = 160: 168 padded rows on 176-row tiles) - is then the data of another operand.  Here the
smallest architecture that aliases (d = 128, ff = 512, two heads, two layers: layer 2's QKV overwrites layer 1's hidden rows) runs
against the oracle, and with every scratch byte set to 0xFF (a NaN in every operand format) in front of the call: same bits, finite,
status word clear.  The poison comparison also runs on ARCH_TINY (ff = 256 < 3 d: separate buffers) - it checks the kernels, not the layout."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FWD_TOL = {"f32": 1e-5, "f16x3": 1e-5, "bf16x3": 6e-5, "bf16": 3e-2}  # the gates of tests/test_hip_forward.py
PRECS = list(FWD_TOL)
# (max_batch, max_frames, clips of the call): a full context of short clips; 2 clips of the dataset's length in a 3-clip context
SHAPES = {"b3_t20": (3, 20, 3), "b2of3_t160": (3, 160, 2)}
GUARD = 4096


def _archs():
    from oracle import mdm_oracle as O

    return {"G": O.Arch(latent_dim=128, ff_size=512, num_layers=2, num_heads=2),
            "R": O.Arch(latent_dim=128, ff_size=512, num_layers=2, num_heads=2, kind="R"),
            "tiny": O.ARCH_TINY}


@pytest.fixture(scope="module", autouse=True)
def hooks_library():
    """tamf_test_fill_scratch and the guard bands live in libtamf_hip_hooks.so: the contexts of this module are created through it"""
    from oakink2_tamf_amd.hip_backend import set_guard_bytes, use_test_hooks

    use_test_hooks(True)
    set_guard_bytes(0)
    yield
    set_guard_bytes(0)
    use_test_hooks(False)


def _arch_dict(a):
    return dict(input_dim=a.input_dim, obj_input_dim=a.obj_input_dim, hand_shape_dim=a.hand_shape_dim, obj_embed_dim=a.obj_embed_dim,
                latent_dim=a.latent_dim, ff_size=a.ff_size, num_layers=a.num_layers, num_heads=a.num_heads, clip_dim=a.clip_dim, h2o_dim=a.h2o_dim)


_CASE = {}


def _case(which, shape):
    """weights, conditioning, inputs and the oracle's output of one (architecture, shape), computed once per session and never modified"""
    from oracle import det
    from oracle import mdm_oracle as O

    key = (which, shape)
    if key not in _CASE:
        arch = _archs()[which]
        _, T, B = SHAPES[shape]
        tag = f"alias/{which}/{shape}"
        sd = O.det_state_dict(arch, tag=tag + "/w")
        cond = O.det_cond(B, T, tag=tag + "/c", arch=arch)
        c = {"arch": arch, "sd": sd, "cond": cond}
        if arch.kind == "R":
            c["x"] = torch.from_numpy(det.det_normal(tag + "/x", (B, T, arch.input_dim)))
            c["h2o"] = torch.from_numpy(det.det_normal(tag + "/h2o", (B, T, arch.h2o_dim)) * 0.05)
            c["ref"] = O.refine_forward(sd, arch, c["x"], c["h2o"], cond)
        else:
            c["x"] = torch.from_numpy(det.det_normal(tag + "/x", (B, arch.input_dim, 1, T)))
            c["t"] = torch.tensor([999, 0, 417][:B])
            c["ref"] = O.denoiser_forward(sd, arch, c["x"], c["t"], cond)
        _CASE[key] = c
    return _CASE[key]


def _ctx(c, shape, prec, n_steps=12, size=None):
    from oakink2_tamf_amd.hip_backend import TamfContext
    from oracle import mdm_oracle as O

    Bmax, Tmax, _ = SHAPES[shape]
    if size:
        Bmax, Tmax = size
    arch = c["arch"]
    ctx = TamfContext(_arch_dict(arch), Bmax, Tmax, precision=prec, kind=arch.kind)
    ctx.load_state_dict(c["sd"], max_timesteps=1000)
    if arch.kind == "G":
        tab = O.make_tables(n_steps, "cosine")
        ctx.set_schedule(tab.posterior_mean_coef1, tab.posterior_mean_coef2, tab.posterior_log_variance_clipped)
    _set_cond(ctx, c)
    return ctx


def _set_cond(ctx, c):
    cond = c["cond"]
    ctx.set_cond(cond.get("text_embedding") if c["arch"].kind == "G" else None, cond["hand_side"], cond["shape"], cond["obj_embedding"], cond["obj_traj"])


def _run(ctx, c):
    return (ctx.refine(c["x"], c["h2o"]) if c["arch"].kind == "R" else ctx.denoise(c["x"], c["t"])).clone()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_denoise_on_the_shared_scratch_matches_the_oracle_and_ignores_poison(shape, prec):
    """(a) one evaluation against oracle.denoiser_forward at the forward gates; (b) with every scratch byte 0xFF in front of the same call:
    the same bits, finite; (d) f16x3: the status word stays clear"""
    c = _case("G", shape)
    ctx = _ctx(c, shape, prec)
    out = _run(ctx, c)
    err = float((out.cpu() - c["ref"]).abs().max())
    print(f"scratch alias forward[{shape}, {prec}]: max|err| vs oracle {err:.3e}")
    assert torch.isfinite(out).all()
    assert err < FWD_TOL[prec] * max(1.0, float(c["ref"].abs().max())), (shape, prec, err)
    for _ in range(2):  # (the second round: poison over what the first poisoned call left)
        ctx.fill_scratch(0xFF)
        again = _run(ctx, c)
        assert torch.isfinite(again).all()
        assert torch.equal(again, out), (shape, prec, float((again - out).abs().max()))
    if prec == "f16x3":
        assert ctx.status_flags() == 0
    ctx.close()


@pytest.mark.parametrize("prec", ["f16x3", "f32", "bf16"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_a_12_step_loop_ignores_poison(shape, prec):
    """12 steps with a fixed seed = one replay of the 10-step graph plus two single steps; the graph is captured by the first call and
    replayed, with the scratch poisoned in between, by the second"""
    c = _case("G", shape)
    ctx = _ctx(c, shape, prec, n_steps=12)
    first = ctx.sample_loop(noise=None, seed=11, clip_id_base=3).clone()
    assert torch.isfinite(first).all()
    ctx.fill_scratch(0xFF)
    second = ctx.sample_loop(noise=None, seed=11, clip_id_base=3)
    assert torch.isfinite(second).all()
    assert torch.equal(first, second), (shape, prec, float((first - second).abs().max()))
    assert ctx.loop_stats()[0] == 1  # one capture: the second call replayed the first one's graph, views and all
    if prec == "f16x3":
        assert ctx.status_flags() == 0
    ctx.close()


@pytest.mark.parametrize("prec", ["f16x3", "f32"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_the_refine_trunk_ignores_poison(shape, prec):
    c = _case("R", shape)
    ctx = _ctx(c, shape, prec)
    out = _run(ctx, c)
    err = float((out.cpu() - c["ref"]).abs().max())
    assert torch.isfinite(out).all() and err < FWD_TOL[prec] * max(1.0, float(c["ref"].abs().max())), (shape, prec, err)
    ctx.fill_scratch(0xFF)
    assert torch.equal(_run(ctx, c), out)
    if prec == "f16x3":
        assert ctx.status_flags() == 0
    ctx.close()


@pytest.mark.parametrize("shape", list(SHAPES))
def test_separate_buffers_ignore_poison_too(shape):
    """ARCH_TINY (ff = 256 < 3 d) keeps an allocation per buffer: the same comparison there - the kernels, not the layout"""
    c = _case("tiny", shape)
    ctx = _ctx(c, shape, "f16x3", n_steps=12)
    out = _run(ctx, c)
    assert float((out.cpu() - c["ref"]).abs().max()) < FWD_TOL["f16x3"] * max(1.0, float(c["ref"].abs().max()))
    loop = ctx.sample_loop(noise=None, seed=5).clone()
    ctx.fill_scratch(0xFF)
    assert torch.equal(_run(ctx, c), out)
    ctx.fill_scratch(0xFF)
    assert torch.equal(ctx.sample_loop(noise=None, seed=5), loop) and torch.isfinite(loop).all()
    assert ctx.status_flags() == 0
    ctx.close()


@pytest.mark.parametrize("prec", ["f16x3", "f32"])
def test_guard_bands_cover_the_views_and_resize_keeps_the_bits(prec):
    """(c) guard-band mode: margins between and around the views, verified like an allocation's; resize to a larger size and back gives
    the bits of a fresh context of that size"""
    from oakink2_tamf_amd.hip_backend import TamfError, lib, set_guard_bytes

    shape = "b2of3_t160"
    c, tiny = _case("G", shape), _case("tiny", shape)
    set_guard_bytes(GUARD)
    try:
        ctx = _ctx(c, shape, prec, n_steps=12)
        t = _ctx(tiny, shape, prec, n_steps=12)
        n = ctx.check_guards()
        # ARCH_TINY has the same tensors and three workspace allocations more (Q | K, attention output, input-merge rows); the aliasing
        # context has three view records instead: without view margins it would report n_tiny - 3
        n_tiny = t.check_guards()
        t.close()
        assert n == n_tiny and n > n_tiny - 3
        out = _run(ctx, c)
        ctx.check_guards()
        loop = ctx.sample_loop(noise=None, seed=11, clip_id_base=3).clone()
        ctx.check_guards()
        ctx.fill_scratch(0xFF)  # the fill itself stays inside the views
        ctx.check_guards()
        assert torch.equal(_run(ctx, c), out)
        ctx.resize(5, 176)
        ctx.check_guards()
        ctx.resize(*SHAPES[shape][:2])
        _set_cond(ctx, c)
        assert torch.equal(_run(ctx, c), out)
        assert torch.equal(ctx.sample_loop(noise=None, seed=11, clip_id_base=3), loop)
        assert ctx.check_guards() == n
        # the margin between two views is a checked one: after the resize the workspaces' records are the last ones, in allocation order
        # (..., H_op, its views Q | K, attention output, h1, then eight more workspaces): 4 bytes right below the attention output
        assert lib().tamf_test_poke(ctx._h, n - 10, -4, 4) == 0
        with pytest.raises(TamfError, match=r"view A_op of H_op's allocation\] .* BELOW its start \(offsets -4 \.\. -1\)"):
            ctx.check_guards()
        ctx.close()
    finally:
        set_guard_bytes(0)
    # the same bits as a context created at that size without margins (other addresses, the views inside the hidden operand)
    fresh = _ctx(c, shape, prec, n_steps=12)
    assert torch.equal(_run(fresh, c), out)
    assert torch.equal(fresh.sample_loop(noise=None, seed=11, clip_id_base=3), loop)
    if prec == "f16x3":
        assert fresh.status_flags() == 0
    fresh.close()
