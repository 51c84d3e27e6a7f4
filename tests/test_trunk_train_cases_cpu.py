"""The case table of tests/trunk_train_cases.py without a device: every case passes the argument checks of its library's *_create and
values just outside each range do not (those that tests/test_refinetrain_cpu.py / tests/test_mdmtrain_cpu.py do not already assert);
the float64 restatement and the oracle agree at every case's architecture, so the reference of the GPU tests is valid there; the
float32 oracle's own error - the source of the gates - is measured and held against the fixture caps; and a Python mirror of the
weight-gradient split arithmetic asserts the table's comments."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "oakink2-tamf_amd"))
import trunk_train_cases as C  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
TAMF_ERR_INVALID, TAMF_ERR_HIP = -1, -3
CAP_FILES = {"R": ("refinetrain_tiny.npz", "refinetrain_l1_ff16.npz", "refinetrain_deep.npz", "refinetrain_e2e.npz"),
             "G": ("mdmtrain_l1_hd64.npz", "mdmtrain_l1_hd128.npz", "mdmtrain_tiny_hd64.npz", "mdmtrain_tiny_hd128.npz", "mdmtrain_losses.npz")}
MAX_FRAMES = {lib: C.MAX_S - C.PREFIX[lib] for lib in ("R", "G")}


def _caps(lib):
    """FIXTURE_TOL_MAX, FIXTURE_TOL_OUT_MAX of the library's GPU test module (the same files)"""
    z = [np.load(os.path.join(GOLDEN, f)) for f in CAP_FILES[lib]]
    return max(float(f["tol_rel"]) for f in z), max(float(f["tol_rel_out"]) for f in z)


def _create(lib, arch, max_batch, max_frames):
    """tamf_*train_create -> (status, last_error); a context that a device let it create is destroyed"""
    from oakink2_tamf_amd.hip_backend import _Arch

    if lib == "R":
        from oakink2_tamf_amd.model import segment_refine_train as mod
        st = _Arch(*[arch[k] for k in C.R.ARCH_NAMES[:8]], 0, arch["h2o_dim"], 1)
    else:
        from oakink2_tamf_amd.model import interaction_segment_mdm_train as mod
        st = _Arch(*[arch[k] for k in C.M.ARCH_NAMES], 0, 0)
    L = mod.lib()
    out = ctypes.c_void_p(0x5A5A5A5A)
    rc = getattr(L, mod.PREFIX + "create")(ctypes.byref(st), max_batch, max_frames, 0, ctypes.byref(out))
    msg = getattr(L, mod.PREFIX + "last_error")().decode()
    if rc == 0:
        getattr(L, mod.PREFIX + "destroy")(out)
    return rc, msg, out.value


def test_table_holds_the_cases():
    """the ids are unique, G has what R has plus its own cases, and every case is built from the smallest architecture"""
    ids = [c.id for c in C.ALL_CASES]
    assert len(ids) == len(set(ids))
    r, g = {c.id[2:] for c in C.CASES["R"]}, {c.id[2:] for c in C.CASES["G"]}
    assert g - r == {"hd128-h3", "hd128-h4", "t-edges"} and not r - g
    assert {"h3", "h5", "h8", "ff48", "ff80", "ff4096", "w1", "wodd", "w4096", "l64", "tmax", "tmax-1", "rows256", "rows257", "rows16384",
            "rows16512", "clips300", "nobj1", "nobj5"} == r
    for c in C.ALL_CASES:
        assert set(c.arch) == set(C.MODS[c.lib].ARCH_NAMES)
    assert C.UNCAPPED <= set(C.BY_ID)
    for lib in ("R", "G"):
        for name in C.DROPOUT_CASES + C.BATCH_BIT_CASES + (C.REPEAT_BIT_CASE,):
            assert f"{lib}-{name}" in C.BY_ID
    t = C.BY_ID["G-t-edges"].extras["t"]
    assert min(t) == 0 and 999 in t and max(t) == C.TIMESTEP_ROWS - 1
    assert C.BY_ID["R-nobj5"].extras["obj_num"][:5] == [1, 2, 3, 4, 5]
    assert [C.BY_ID[f"{lib}-tmax"].T for lib in ("R", "G")] == [1021, 1019]


@pytest.mark.parametrize("case", C.ALL_CASES, ids=lambda c: c.id)
def test_create_accepts_the_case(case):
    """the case passes every argument check of its library's create: the status is success on a machine with a device and the failure
    of the first device call (hipSetDevice) on one without - never TAMF_ERR_INVALID"""
    rc, msg, out = _create(case.lib, case.arch, case.B, case.T)
    assert rc in (0, TAMF_ERR_HIP), (case.id, rc, msg)
    if rc:
        assert msg.startswith("hipSetDevice") and out is None, (case.id, msg)


def test_the_python_step_accepts_the_last_timestep():
    """the table's largest t is what check_mdm_batch accepts and one more is refused: the wrapper's range is the library's"""
    import torch

    from oakink2_tamf_amd.model import interaction_segment_mdm_train as imt

    assert imt.MAX_TIMESTEP == C.TIMESTEP_ROWS - 1
    case = C.BY_ID["G-t-edges"]
    arch, _, inp, _, _ = C.build(case)
    batch = {k: torch.from_numpy(inp[k]) for k in ("text_embedding", "shape", "obj_embedding", "obj_traj")}
    batch["hand_side"] = inp["hand_side"]
    x = torch.from_numpy(inp["x_t"])
    got = imt.check_mdm_batch(x, torch.from_numpy(inp["t"]), batch, batch["text_embedding"], C.M.arch_dict(arch))
    assert got[4].tolist() == [0, 999, 4999]
    with pytest.raises(ValueError, match=r"timesteps must be in \[0, 4999\]"):
        imt.check_mdm_batch(x, torch.tensor([0, 999, 5000]), batch, batch["text_embedding"], C.M.arch_dict(arch))


R_HEADS = "the head dimension must be 64: latent_dim = 64 * num_heads, got latent_dim %d with %d heads"
G_HEADS = "the head dimension must be 64 or 128: latent_dim = 64 * num_heads or 128 * num_heads, in [64, 512], got latent_dim %d with %d heads"
FF_MSG = "ff_size must be a multiple of 16 in [16, 4096], got %d"


def test_create_refuses_just_outside_each_range():
    """what the two libraries' own CPU tests do not assert yet: ff_size 8 (both); R: 9 heads of 64 with a matching latent_dim is in
    test_refinetrain_cpu.py, here a latent_dim of 576 with 8 heads and a head dimension of 96; G: 9 heads (latent_dim 576 and 1152),
    5 heads of 128 (latent_dim 640 > 512), a head dimension of 96 at 2 heads; max_frames one past each library's limit at the case
    table's architecture.  The status, the whole message, and *out == NULL."""
    cases = [("R", dict(ff_size=8), {}, FF_MSG % 8), ("G", dict(ff_size=8), {}, FF_MSG % 8),
             ("R", dict(num_heads=8, latent_dim=576), {}, R_HEADS % (576, 8)), ("R", dict(num_heads=2, latent_dim=192), {}, R_HEADS % (192, 2)),
             ("G", dict(num_heads=9, latent_dim=576), {}, G_HEADS % (576, 9)), ("G", dict(num_heads=9, latent_dim=1152), {}, G_HEADS % (1152, 9)),
             ("G", dict(num_heads=5, latent_dim=640), {}, G_HEADS % (640, 5)), ("G", dict(num_heads=2, latent_dim=192), {}, G_HEADS % (192, 2)),
             ("G", dict(num_heads=8, latent_dim=576), {}, G_HEADS % (576, 8))]
    for lib in ("R", "G"):
        lim = MAX_FRAMES[lib]
        cases.append((lib, {}, dict(max_frames=lim + 1), f"max_frames = {lim + 1} outside [1, {lim}]"))
        cases.append((lib, dict(num_heads=8, latent_dim=512, ff_size=4096, num_layers=64), dict(max_frames=lim + 1, max_batch=65535),
                      f"max_frames = {lim + 1} outside [1, {lim}]"))
    for lib, arch, kw, text in cases:
        rc, msg, out = _create(lib, dict(C.BASE[lib], **arch), kw.get("max_batch", 2), kw.get("max_frames", 7))
        assert (rc, msg) == (TAMF_ERR_INVALID, text) and out is None, (lib, arch, kw, rc, msg)


def test_create_refusals_cover_the_issues_list():
    """every value just outside a range, on the case table's base architecture of either library, is refused with TAMF_ERR_INVALID:
    heads 0 and 9, ff_size 8, 24 and 4112, layers 0 and 65, each width 0 and 4097, max_frames one past the limit, max_batch 0 and 65536"""
    for lib in ("R", "G"):
        bad = [dict(num_heads=0), dict(num_heads=9, latent_dim=576), dict(ff_size=8), dict(ff_size=24), dict(ff_size=4112), dict(num_layers=0),
               dict(num_layers=65)] + [{k: v} for k in C.WIDTHS[lib] for v in (0, 4097)]
        for arch in bad:
            rc, msg, out = _create(lib, dict(C.BASE[lib], **arch), 2, 7)
            assert rc == TAMF_ERR_INVALID and out is None, (lib, arch, rc, msg)
        for kw in (dict(max_frames=MAX_FRAMES[lib] + 1), dict(max_batch=0), dict(max_batch=65536)):
            rc, msg, out = _create(lib, C.BASE[lib], kw.get("max_batch", 2), kw.get("max_frames", 7))
            assert rc == TAMF_ERR_INVALID and out is None, (lib, kw, rc, msg)
    rc, msg, _ = _create("G", dict(C.BASE["G"], latent_dim=96), 2, 7)
    assert (rc, msg) == (TAMF_ERR_INVALID, G_HEADS % (96, 1))


@pytest.mark.parametrize("case", C.ALL_CASES, ids=lambda c: c.id)
def test_oracle_agrees_and_gate_source(case):
    """float64 loss_and_grads through the restatement's own forward and through oracle_forward agree to the 1e-9 the fixtures'
    comparison uses (test_restatement_reproduces_fixture): the reference is valid at this architecture.  The same run measures the
    oracle's float32-against-float64 error, the source of the case's gates, and prints it with the side of the fixture cap its 4 x lies
    on and whether trunk_train_cases.UNCAPPED_GRAD / UNCAPPED_OUT lists the case (run with -s to read it).  Nothing is asserted on that
    side: the float32 error is a maximum over few elements and moves with the CPU's BLAS and thread count (the column sums over 16384
    rows ninefold between two machines), and either listing is safe - an unlisted case keeps the smaller of the two gates."""
    mod = C.MODS[case.lib]
    arch, sd, inp, obj_num, G = C.build(case)
    ref, m_g, m_o, err32 = C.measure_gates(case.lib, sd, arch, inp, G, obj_num)
    own = mod.loss_and_grads(sd, arch, inp, G, obj_num)
    assert mod.rel_err(own[0], ref[0]) <= 1e-9
    assert abs(own[1] - ref[1]) <= 1e-9 * abs(ref[1])
    err = mod.grad_rel_err(own[2], ref[2])
    assert set(err) == set(ref[2]) and max(err.values()) <= 1e-9, max(err, key=err.get)
    assert all(np.isfinite(g).all() for g in ref[2].values()) and np.isfinite(ref[0]).all()
    assert all(np.abs(g).max() > 0 for g in ref[2].values()), [k for k, g in ref[2].items() if not np.abs(g).max() > 0]
    cap, cap_out = _caps(case.lib)
    worst = max(err32, key=err32.get)
    print(f"GATE {case.id}: float32 oracle error: gradients {m_g / 4:.3e} ({worst}), output {m_o / 4:.3e}; 4 x: {m_g:.3e} (cap {cap:.3e}: "
          f"{'under' if m_g <= cap else 'ABOVE'}, {'not applied' if case.id in C.UNCAPPED_GRAD else 'applied'}), {m_o:.3e} (cap {cap_out:.3e}: "
          f"{'under' if m_o <= cap_out else 'ABOVE'}, {'not applied' if case.id in C.UNCAPPED_OUT else 'applied'})")


def test_split_arithmetic():
    """the mirror of TrunkStep::splits and the two chunk formulas against the numbers in the table's comments; the 16512-row case has
    empty splits, the 257-row case has 2 splits, and colsum2's boundaries differ from wgrad's"""
    assert [C.splits(r) for r in (1, 255, 256, 257, 512, 513, 16384, 16385, 16512, 65535 * 1024)] == [1, 1, 1, 2, 2, 3, 64, 64, 64, 64]
    seen = set()
    for case in C.ALL_CASES:
        if "splits" not in case.extras:
            continue
        rows, nsplit, chunk, empty, cchunk = case.extras["splits"]
        seen.add(rows)
        assert case.B * (case.T + C.PREFIX[case.lib]) == rows, case.id
        assert (C.splits(rows), C.wgrad_chunk(rows), C.first_empty_split(rows, C.wgrad_chunk(rows)), C.colsum_chunk(rows)) == (nsplit, chunk, empty, cchunk), case.id
        assert chunk % C.TG_K == 0 and nsplit * chunk >= rows and nsplit * cchunk >= rows  # every row is in a split
        assert C.first_empty_split(rows, cchunk) is None  # colsum2's unrounded chunk leaves no split empty
    assert seen == {256, 257, 16384, 16512}
    for lib in ("R", "G"):
        rows, nsplit, chunk, empty, cchunk = C.BY_ID[f"{lib}-rows16512"].extras["splits"]
        assert rows > C.MAX_SPLIT * C.SPLIT_ROWS and nsplit == C.MAX_SPLIT and empty == 58 and empty * chunk >= rows > (empty - 1) * chunk
        assert rows - (empty - 1) * chunk == 96  # the last split that holds rows holds 96
        assert chunk != cchunk
        assert C.BY_ID[f"{lib}-rows257"].extras["splits"][1] == 2 and C.BY_ID[f"{lib}-rows256"].extras["splits"][1] == 1
        assert C.BY_ID[f"{lib}-rows16384"].extras["splits"][3] is None
    # the constants are the header's
    with open(os.path.join(HERE, "..", "oakink2-tamf_amd", "csrc", "tamf_trunk_host.h")) as f:
        host = f.read()
    with open(os.path.join(HERE, "..", "oakink2-tamf_amd", "csrc", "tamf_trunk_grad.h")) as f:
        grad = f.read()
    assert f"constexpr int MAX_SPLIT = {C.MAX_SPLIT}, SPLIT_ROWS = {C.SPLIT_ROWS}, MAX_S = {C.MAX_S};" in host
    assert f"TG_K = {C.TG_K}," in grad
    assert "chunk = ((R + nsplit - 1) / nsplit + TG_K - 1) / TG_K * TG_K" in host and "D, R, (R + nsplit - 1) / nsplit, pa, pb" in host
