"""One case table for the two trunk training libraries (libtamf_refinetrain.so: "R", libtamf_mdmtrain.so: "G"): the architectures and
call shapes that tamf_*train_create accepts and the sweeps of tests/test_refinetrain_gpu.py / tests/test_mdmtrain_gpu.py never reach -
the head counts, the ff_size tails, the input widths at both ends of their range, 64 layers, the longest sequences, the row counts at
which the weight-gradient split changes, many one-frame clips, the object counts and G's timestep rows.  Every case is as small as its
edge allows.  tests/test_trunk_train_cases_cpu.py holds the table to the libraries' create checks and the oracle;
tests/test_refinetrain_ranges_gpu.py and tests/test_mdmtrain_ranges_gpu.py run the kernels over it (the bodies of those tests are here:
the two libraries take the same calls).

A case is (id, lib, arch, B, T, nobj, ragged, extras): arch holds every value of the library's ARCH_NAMES; extras may hold "obj_num" (the
per-clip object counts instead of seeded_inputs' ragged ones), "t" (G: the timesteps) and "splits" (below).

Gates.  A case's gates are 4 x the error of the oracle's float32 autograd against its float64 autograd on the same inputs (max over
tensors of |g32 - g64|_inf / |g64|_inf, and the same for the output), measured at test time and printed, never from the HIP result.
They are capped at the largest fixture gate as in the existing sweeps - except for the ids in UNCAPPED_GRAD (gradients) and UNCAPPED_OUT
(output), where the CPU run (test_trunk_train_cases_cpu.py::test_oracle_agrees_and_gate_source) shows the float32 oracle itself outside
the cap: there the measured 4 x stands alone.  The dropout cases measure the same way with the library's masks in both the float32 and the float64 restatement.
"""
import collections
import os
import sys
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mdm_train_restatement as M  # noqa: E402
import refine_train_restatement as R  # noqa: E402

MODS = {"R": R, "G": M}
PREFIX = {"R": 3, "G": M.PREFIX}
TIMESTEP_ROWS = 5000  # the rows of sequence_pos_encoder.pe: G's step takes t in [0, TIMESTEP_ROWS - 1]

# csrc/tamf_trunk_host.h, csrc/tamf_trunk_grad.h
MAX_S, MAX_SPLIT, SPLIT_ROWS, TG_K = 1024, 64, 256, 32


def splits(rows):
    """TrunkStep::splits"""
    return max(1, min(MAX_SPLIT, (rows + SPLIT_ROWS - 1) // SPLIT_ROWS))


def wgrad_chunk(rows):
    """the rows of one split of TrunkStep::wgrad: a multiple of the contraction step"""
    n = splits(rows)
    return ((rows + n - 1) // n + TG_K - 1) // TG_K * TG_K


def colsum_chunk(rows):
    """the rows of one split of TrunkStep::colsum2: not rounded"""
    n = splits(rows)
    return (rows + n - 1) // n


def first_empty_split(rows, chunk):
    """the first split that starts at or beyond the last row, or None"""
    s = (rows + chunk - 1) // chunk
    return s if s < splits(rows) else None


Case = collections.namedtuple("Case", "id lib arch B T nobj ragged extras")

BASE = {"R": R.arch_dict(R.ARCH_L1), "G": M.arch_dict(M.ARCH_L1_64)}  # latent 64, one head, ff 16, one layer, the fixtures' widths
WIDTHS = {"R": ("input_dim", "obj_input_dim", "hand_shape_dim", "obj_embed_dim", "h2o_dim"),
          "G": ("input_dim", "obj_input_dim", "hand_shape_dim", "obj_embed_dim", "clip_dim")}


def _case(lib, name, arch=None, B=2, T=6, nobj=2, ragged=False, **extras):
    return Case(f"{lib}-{name}", lib, dict(BASE[lib], **(arch or {})), B, T, nobj, ragged, extras)


def _table(lib):
    pre = PREFIX[lib]
    last = "clip_dim" if lib == "G" else "h2o_dim"
    out = []
    # heads: the dropout element (h S + q) S + k and the stat / delta strides at h >= 4; LayerNorm at 3, 5 and 8 column groups
    for H in (3, 5, 8):
        out.append(_case(lib, f"h{H}", dict(num_heads=H, latent_dim=64 * H, ff_size=48), T=14, ragged=True))
    if lib == "G":  # head dimension 128 at an odd head count and at its largest; LayerNorm at 6 and 8 column groups
        for H in (3, 4):
            out.append(_case(lib, f"hd128-h{H}", dict(num_heads=H, latent_dim=128 * H, ff_size=48), T=14, ragged=True))
    # ff tails: N = 48 and 80 leave 48 and 16 columns in the last 64-wide tile; 4096 is the largest N and K of the feed-forward maps
    for ff in (48, 80, 4096):
        out.append(_case(lib, f"ff{ff}", dict(ff_size=ff)))
    # widths: K = 1 (K + 1 = 2 columns of the weight gradient), odd K, K = 4096 (K + 1 = 4097: a 65th tile of one column)
    out.append(_case(lib, "w1", {k: 1 for k in WIDTHS[lib]}))
    out.append(_case(lib, "wodd", {"input_dim": 33, "obj_input_dim": 5, "hand_shape_dim": 7, "obj_embed_dim": 65, last: 31 if lib == "G" else 3}))
    out.append(_case(lib, "w4096", {k: 4096 for k in WIDTHS[lib]}, T=5))
    # depth: dropout sites up to 256
    out.append(_case(lib, "l64", dict(num_layers=64), B=1, T=2))
    # length: S = 1024 (64 full key tiles) and 1023 (a partial last tile); the largest dropout element of the attention site
    out.append(_case(lib, "tmax", B=1, T=MAX_S - pre))
    out.append(_case(lib, "tmax-1", B=1, T=MAX_S - pre - 1))
    # row splits of the weight gradients and the column sums over the B S token rows: (rows, nsplit, wgrad's chunk, its first empty
    # split, colsum2's chunk) by the formulas of TrunkStep::wgrad and TrunkStep::colsum2
    #   256 rows:    1 split  of 256 rows;                  colsum2 256
    #   257 rows:    2 splits of 160 rows (160 + 97);       colsum2 129 (129 + 128)
    #   16384 rows: 64 splits of 256 rows, none empty;      colsum2 256
    #   16512 rows: 65 > MAX_SPLIT -> 64 splits of 288 rows (ceil(16512 / 64) = 258 rounded up to 32): 57 full, split 57 with 96 rows,
    #               splits 58 .. 63 start beyond the last row and are empty; colsum2 258 (64 x 258 = 16512: none empty)
    out.append(_case(lib, "rows256", B=2, T=128 - pre, splits=(256, 1, 256, None, 256)))
    out.append(_case(lib, "rows257", B=1, T=257 - pre, splits=(257, 2, 160, None, 129)))
    out.append(_case(lib, "rows16384", B=64, T=256 - pre, splits=(16384, 64, 256, None, 256)))
    out.append(_case(lib, "rows16512", B=86, T=192 - pre, splits=(16512, 64, 288, 58, 258)))
    # many clips of one frame: 64-row GEMM tiles over many clips, 16-row attention tiles of S rows, grid z = 300
    out.append(_case(lib, "clips300", B=300, T=1))
    # objects
    out.append(_case(lib, "nobj1", nobj=1))
    out.append(_case(lib, "nobj5", B=6, nobj=5, obj_num=[1, 2, 3, 4, 5, 1]))
    if lib == "G":  # the timestep row gather at the table's first row, the diffusion's last step and the table's last row
        out.append(_case(lib, "t-edges", B=3, t=[0, 999, TIMESTEP_ROWS - 1]))
    return out


CASES = {lib: _table(lib) for lib in ("R", "G")}
ALL_CASES = CASES["R"] + CASES["G"]
BY_ID = {c.id: c for c in ALL_CASES}

# the cases whose measured gate (4 x the float32 oracle's error) lies above the largest fixture gate on the CPU run, for the gradients
# and for the output: no cap there (64 layers; every width 1, where input_merge.0.bias and the distance embedding's bias are sums of
# terms that cancel; the widest trunks; the 17- and 19-row clips of the 3- and 5-head cases, whose output gate the fixtures' 1.4e-6 / 2.2e-6 undercut)
UNCAPPED_GRAD = frozenset({"R-w1", "R-l64", "G-hd128-h4", "G-w1", "G-l64"})
UNCAPPED_OUT = frozenset({"R-h3", "R-h5", "R-l64", "G-h3", "G-h5"})
UNCAPPED = UNCAPPED_GRAD | UNCAPPED_OUT
DROPOUT_CASES = ("h8", "ff80", "tmax-1")  # p = 0.5 with the library's own masks
BATCH_BIT_CASES = ("h5", "ff80")          # a clip alone against the same clip inside a batch of 3
REPEAT_BIT_CASE = "rows16512"             # two identical calls


def arch_of(case):
    mod = MODS[case.lib]
    return mod.arch_of([case.arch[k] for k in mod.ARCH_NAMES])


def seed_of(case):
    return zlib.crc32(case.id.encode()) % 100000


def build(case):
    """-> (arch, sd, inputs, obj_num, G): seeded by the case's id"""
    mod, arch, seed = MODS[case.lib], arch_of(case), seed_of(case)
    sd = mod.seeded_state_dict(arch, seed)
    inp, obj_num = mod.seeded_inputs(arch, case.B, case.T, case.nobj, seed + 1, case.ragged)
    if "obj_num" in case.extras:
        obj_num = list(case.extras["obj_num"])
    if "t" in case.extras:
        inp["t"] = np.asarray(case.extras["t"], np.int64)
    shape = (case.B, case.T, arch.input_dim) if case.lib == "R" else (case.B, arch.input_dim, 1, case.T)
    G = np.random.default_rng(seed + 2).normal(size=shape).astype(np.float32)
    return arch, sd, inp, obj_num, G


def measure_gates(lib, sd, arch, inp, G, obj_num, masks=None, p=0.0):
    """float64 autograd, and 4 x (float32 autograd against it) for the gradients and the output -> (ref, gate, gate_out, {key: float32
    error}).  Without masks both runs go through the oracle; with masks through the restatement with the masks applied in both."""
    import torch

    mod = MODS[lib]
    kw = dict(forward=mod.oracle_forward) if masks is None else dict(masks=masks, p=p)
    ref = mod.loss_and_grads(sd, arch, inp, G, obj_num, **kw)
    r32 = mod.loss_and_grads(sd, arch, inp, G, obj_num, dtype=torch.float32, **kw)
    err = mod.grad_rel_err(r32[2], ref[2])
    return ref, 4 * max(err.values()), 4 * mod.rel_err(r32[0], ref[0]), err


def gates(case, cap, cap_out, sd, arch, inp, G, obj_num, masks=None, p=0.0):
    """the gates of a case: measured at test time, capped at the fixtures' unless the case is in UNCAPPED; printed"""
    ref, m_g, m_o, _ = measure_gates(case.lib, sd, arch, inp, G, obj_num, masks, p)
    free_g, free_o = case.id in UNCAPPED_GRAD, case.id in UNCAPPED_OUT
    print(f"{case.id}: gates measured at test time: gradients {m_g:.3e} (largest fixture gate {cap:.3e}{', not applied' if free_g else ''}), "
          f"output {m_o:.3e} ({cap_out:.3e}{', not applied' if free_o else ''})")
    return ref, (m_g if free_g else min(m_g, cap)), (m_o if free_o else min(m_o, cap_out))


# ---- the bodies of the GPU tests; tm: tests/test_refinetrain_gpu.py or tests/test_mdmtrain_gpu.py as a module ----
def _forward_args(tm, inp, rows=None):
    a = tm._batch(inp, rows)
    return a if isinstance(a, tuple) else (a,)


def check_parity(tm, case):
    """output and every parameter gradient against float64 autograd through the oracle; every gradient element written"""
    arch, sd, inp, obj_num, G = build(case)
    ref, tol, tol_out = gates(case, tm.FIXTURE_TOL_MAX, tm.FIXTURE_TOL_OUT_MAX, sd, arch, inp, G, obj_num)
    m, ts = tm._step(arch, sd, case.B, case.T)
    out, grads = tm._run(m, ts, inp, G, obj_num)  # (the gradient buffers start as NaN)
    ts.close()
    unwritten = {k: int(np.isnan(g).sum()) for k, g in grads.items() if np.isnan(g).any()}
    assert not unwritten and not np.isnan(out).any(), unwritten
    tm._check(case.id, (out, grads), ref, tol, tol_out)


def check_dropout(tm, case, p=0.5):
    """the library's own keep-masks injected into the float64 restatement"""
    arch, sd, inp, obj_num, G = build(case)
    m, ts = tm._step(arch, sd, case.B, case.T, p=p, seed=77)
    clip_ids = [5 + 3 * b for b in range(case.B)]
    got = tm._run(m, ts, inp, G, obj_num, clip_ids=clip_ids, step=4)
    masks = tm._masks(ts, arch, case.B, case.T, step=4, clip_ids=clip_ids)
    ts.close()
    assert not any(np.isnan(g).any() for g in got[1].values())
    kept = np.mean([float(v.float().mean()) for v in masks.values()])
    assert abs(kept - (1 - p)) < 0.05
    ref, tol, tol_out = gates(case, tm.FIXTURE_TOL_MAX, tm.FIXTURE_TOL_OUT_MAX, sd, arch, inp, G, obj_num, masks, p)
    tm._check(f"{case.id} p={p}", got, ref, tol, tol_out)


def check_head_masks_differ(tm, case, p=0.5):
    """the attention site's keep-masks of head 0 and head 4: the element index carries the head"""
    arch = arch_of(case)
    S = case.T + PREFIX[case.lib]
    assert arch.num_heads == 8
    m, ts = tm._step(arch, MODS[case.lib].seeded_state_dict(arch, seed_of(case)), case.B, case.T, p=p, seed=77)
    mask = ts.dropout_mask(4, 5, 1, arch.num_heads * S, S).cpu().numpy()
    ts.close()
    heads = mask.reshape(arch.num_heads, S, S)
    assert abs(float(heads.mean()) - (1 - p)) < 0.05
    assert not np.array_equal(heads[0], heads[4])
    assert len({heads[h].tobytes() for h in range(arch.num_heads)}) == arch.num_heads


def check_batch_bits(tm, case):
    """a clip's forward output alone equals its output inside a batch of 3, bit for bit"""
    import torch

    case3 = case._replace(B=3, ragged=True)
    arch, sd, inp, obj_num, _ = build(case3)
    m, ts = tm._step(arch, sd, 3, case.T)
    with torch.no_grad():
        full = ts.forward(*_forward_args(tm, inp), obj_num=obj_num).cpu().numpy()
        ts.discard_forward()
        alone = []
        for b in range(3):
            alone.append(ts.forward(*_forward_args(tm, inp, [b]), obj_num=[obj_num[b]]).cpu().numpy())
            ts.discard_forward()
    ts.close()
    assert np.isfinite(full).all()
    for b in range(3):
        assert np.array_equal(alone[b][0], full[b]), b


def check_repeat_bits(tm, case):
    """two identical calls give identical output and gradient bits (the gradient buffers are NaN again before the second)"""
    arch, sd, inp, obj_num, G = build(case)
    m, ts = tm._step(arch, sd, case.B, case.T)
    a = tm._run(m, ts, inp, G, obj_num)
    b = tm._run(m, ts, inp, G, obj_num)
    ts.close()
    assert not any(np.isnan(g).any() for g in b[1].values())
    assert np.array_equal(a[0], b[0]) and all(np.array_equal(a[1][k], b[1][k]) for k in a[1])
