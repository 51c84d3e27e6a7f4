"""HipAdamW (libtamf_optim.so) on the GPU against the float64 restatement of tests/optim_restatement.py.

The gate, per tensor and per quantity (p, exp_avg, exp_avg_sq, the gradient norm): 4 x the error of torch's own float32 CPU run of
clip_grad_norm_ + AdamW on the same inputs against the same float64 restatement, measured here and printed, and never below one
float32 ulp of the tensor's largest magnitude."""
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [p for p in (ROOT, os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests")) if p not in sys.path]

import optim_restatement as R  # noqa: E402

pytestmark = pytest.mark.gpu

CHUNK = 4096
SIZES = [1, 3, 4, 5, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 7, (512, 512)]
STEPS = 20
LR, MAX_NORM = 1e-3, 0.1
GUARD = 64  # canary floats on both sides of a guarded tensor
CANARY = 1234.5


def _numel(s):
    return int(np.prod(s))


@functools.lru_cache(maxsize=None)
def inputs():
    """the seeded parameters and the 20 steps of gradients at scale 10^U(-4, 1) / sqrt(numel): computed once, never modified"""
    rng = np.random.default_rng(2024)
    ps = [(0.1 * rng.standard_normal(s)).astype(np.float32) for s in SIZES]
    steps = []
    for _ in range(STEPS):
        steps.append([(rng.standard_normal(p.shape) * 10.0 ** rng.uniform(-4, 1) / np.sqrt(p.size)).astype(np.float32) for p in ps])
    for p in ps:
        p.setflags(write=False)
    for gs in steps:
        for g in gs:
            g.setflags(write=False)
    return ps, steps


@functools.lru_cache(maxsize=None)
def reference(weight_decay, n_steps=STEPS):
    """-> (float64 restatement (p, m, v) per tensor, torch's float32 CPU run of the reference's sequence (p, m, v) per tensor)"""
    import torch

    ps, steps = inputs()
    ref, state = R.run(ps, steps[:n_steps], lr=LR, weight_decay=weight_decay, max_norm=MAX_NORM)
    params, opt = R.torch_run(ps, steps[:n_steps], torch.float32, lr=LR, weight_decay=weight_decay, max_norm=MAX_NORM)
    ref64 = [(r, m, v) for r, (m, v, _) in zip(ref, state)]
    t32 = [(p.detach().numpy(), opt.state[p]["exp_avg"].numpy(), opt.state[p]["exp_avg_sq"].numpy()) for p in params]
    return ref64, t32


def gate(ref, yard):
    """4 x the yardstick's error against `ref`, not below one float32 ulp of ref's largest magnitude; -> (gate, yardstick error)"""
    ref = np.asarray(ref, np.float64)
    e = float(np.max(np.abs(np.asarray(yard, np.float64) - ref))) if ref.size else 0.0
    ulp = float(np.spacing(np.float32(np.max(np.abs(ref))))) if ref.size else 0.0
    return max(4.0 * e, ulp), e


def check(name, got, ref, yard):
    g, e = gate(ref, yard)
    err = float(np.max(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))))
    print(f"{name}: err {err:.3e} torch-f32 {e:.3e} gate {g:.3e} (max |ref| {float(np.max(np.abs(ref))):.3e})")
    assert np.isfinite(np.asarray(got)).all() and err <= g, (name, err, g)


class Slot:
    """p, grad, exp_avg, exp_avg_sq of one tensor on the device.  guarded: each is a slice at float offset 1 past a 64-float canary
    of a larger buffer, with a 64-float canary behind it - four addresses that are not 16-byte aligned."""

    def __init__(self, p_np, guarded=False, device="cuda:0"):
        import torch

        self.shape, self.n, self.guarded = p_np.shape, p_np.size, guarded
        self.bufs = []
        views = []
        for _ in range(4):
            if guarded:
                buf = torch.full((GUARD + 1 + self.n + GUARD,), CANARY, dtype=torch.float32, device=device)
                view = buf[GUARD + 1:GUARD + 1 + self.n].view(self.shape)
                assert view.data_ptr() % 16 != 0
            else:
                buf = torch.zeros(max(self.n, 1), dtype=torch.float32, device=device)
                view = buf[:self.n].view(self.shape)
                assert view.data_ptr() % 16 == 0
            self.bufs.append(buf)
            views.append(view)
        self.p = torch.nn.Parameter(views[0])
        self.g, self.m, self.v = views[1], views[2], views[3]
        with torch.no_grad():
            self.p.copy_(torch.from_numpy(np.ascontiguousarray(p_np)))
            self.g.zero_()
            self.m.zero_()
            self.v.zero_()
        self.p.grad = self.g

    def state(self):
        import torch

        return {"step": torch.tensor(0.0, dtype=torch.float32), "exp_avg": self.m, "exp_avg_sq": self.v}

    def set_grad(self, g_np):
        import torch

        self.g.copy_(torch.from_numpy(np.ascontiguousarray(g_np)).view(self.shape))

    def result(self):
        return tuple(t.detach().cpu().numpy().copy() for t in (self.p, self.m, self.v))

    def canaries_intact(self):
        if not self.guarded:
            return True
        return all(bool((b[:GUARD + 1] == CANARY).all()) and bool((b[GUARD + 1 + self.n:] == CANARY).all()) for b in self.bufs)


def hip_run(ps, steps, weight_decay=0.0, max_norm=MAX_NORM, guarded=False, norms=False):
    """the steps through HipAdamW -> ([(p, m, v)] per tensor, the slots, [grad_norms() before each step] when asked)"""
    from oakink2_tamf_amd.optim import HipAdamW

    slots = [Slot(p, guarded) for p in ps]
    opt = HipAdamW([s.p for s in slots], lr=LR, weight_decay=weight_decay, clip_max_norm=max_norm)
    for s in slots:
        opt.state[s.p] = s.state()
    seen = []
    for gs in steps:
        for s, g in zip(slots, gs):
            s.set_grad(g)
        if norms:
            seen.append(opt.grad_norms().cpu().numpy())
        opt.step()
    return [s.result() for s in slots], slots, seen


@functools.lru_cache(maxsize=None)
def aligned_run(weight_decay):
    ps, steps = inputs()
    out, slots, seen = hip_run(ps, steps, weight_decay, norms=True)
    return out, seen


def same_bits(a, b):
    return all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))


# ---- parity -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("weight_decay", [0.0, 0.01])
def test_parity_with_the_float64_restatement(weight_decay):
    ps, steps = inputs()
    norms64 = np.array([[R.grad_norm(g) for g in gs] for gs in steps])
    assert (norms64 > MAX_NORM * 1.01).any() and (norms64 < MAX_NORM * 0.99).any()  # clipped and unclipped steps both occur
    ref64, t32 = reference(weight_decay)
    out, _ = aligned_run(weight_decay)
    for i, s in enumerate(SIZES):
        for q, name in enumerate(("p", "exp_avg", "exp_avg_sq")):
            check(f"wd {weight_decay} numel {_numel(s)} {name}", out[i][q], ref64[i][q], t32[i][q])


def test_grad_norms_parity():
    import torch

    ps, steps = inputs()
    _, seen = aligned_run(0.0)
    assert len(seen) == STEPS and all(x.shape == (len(SIZES),) and x.dtype == np.float32 for x in seen)
    for i, s in enumerate(SIZES):
        ref = np.array([R.grad_norm(gs[i]) for gs in steps])
        yard = np.array([float(torch.linalg.vector_norm(torch.from_numpy(gs[i].copy()), 2.0)) for gs in steps])
        got = np.array([x[i] for x in seen], np.float64)
        # per step: every norm against its own gate (the steps' norms span five decades)
        for k in range(STEPS):
            g, e = gate(ref[k:k + 1], yard[k:k + 1])
            err = abs(got[k] - ref[k])
            assert np.isfinite(got[k]) and err <= g, (s, k, err, g)
        print(f"grad_norms numel {_numel(s)}: max rel err {np.max(np.abs(got - ref) / ref):.3e} torch-f32 {np.max(np.abs(yard - ref) / ref):.3e}")


# ---- guard bands and alignment ----------------------------------------------------------------------------------------------------

def test_unaligned_slices_keep_their_canaries_and_give_the_aligned_bits():
    ps, steps = inputs()
    out, slots, seen = hip_run(ps, steps, 0.01, guarded=True, norms=True)
    assert all(s.canaries_intact() for s in slots)
    ref, ref_seen = aligned_run(0.01)
    for i in range(len(SIZES)):
        assert same_bits(out[i], ref[i]), SIZES[i]
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(seen, ref_seen))


# ---- invariance -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", [6, 10, 11])  # numel 65, 2 CHUNK + 7, 512 x 512
def test_a_tensor_does_not_depend_on_its_table(which):
    ps, steps = inputs()
    n = 5
    alone, _, _ = hip_run([ps[which]], [[gs[which]] for gs in steps[:n]])
    again, _, _ = hip_run([ps[which]], [[gs[which]] for gs in steps[:n]])
    assert same_bits(alone[0], again[0])  # the same call gives the same bits
    others = [0, 2, 4, 7, 8, 9, 5]
    for pos in (0, 5):
        idx = others[:pos] + [which] + others[pos:]
        assert len(idx) == 8
        tab, _, _ = hip_run([ps[i] for i in idx], [[gs[i] for i in idx] for gs in steps[:n]])
        assert same_bits(tab[pos], alone[0]), pos


def test_two_identical_runs_give_identical_bits():
    ps, steps = inputs()
    a, _ = aligned_run(0.0)
    b, _, _ = hip_run(ps, steps, 0.0)
    assert all(same_bits(x, y) for x, y in zip(a, b))


# ---- skips and edges --------------------------------------------------------------------------------------------------------------

def test_tensors_without_gradient_or_elements_are_skipped():
    import torch

    from oakink2_tamf_amd.optim import HipAdamW

    ps, steps = inputs()
    dev = "cuda:0"
    a = torch.nn.Parameter(torch.from_numpy(ps[6].copy()).to(dev))
    none = torch.nn.Parameter(torch.from_numpy(ps[7].copy()).to(dev))
    empty = torch.nn.Parameter(torch.zeros(0, 7, device=dev))
    b = torch.nn.Parameter(torch.from_numpy(ps[9].copy()).to(dev))
    opt = HipAdamW([a, none, empty, b], lr=LR, clip_max_norm=MAX_NORM)
    for k in range(3):
        a.grad = torch.from_numpy(steps[k][6].copy()).to(dev)
        b.grad = torch.from_numpy(steps[k][9].copy()).to(dev)
        empty.grad = torch.zeros_like(empty)
        norms = opt.grad_norms().cpu().numpy()
        assert norms.shape == (4,) and norms[1] == 0 and norms[2] == 0 and norms[0] > 0 and norms[3] > 0
        opt.step()
    assert np.array_equal(none.detach().cpu().numpy(), ps[7]) and empty.numel() == 0
    assert opt.state.get(none) is None and opt.state.get(empty) is None
    assert float(opt.state[a]["step"]) == 3 and opt.state[a]["step"].device.type == "cpu" and opt.state[a]["step"].dtype == torch.float32
    alone, _, _ = hip_run([ps[6], ps[9]], [[gs[6], gs[9]] for gs in steps[:3]])
    assert np.array_equal(a.detach().cpu().numpy(), alone[0][0]) and np.array_equal(b.detach().cpu().numpy(), alone[1][0])


def test_all_zero_gradient():
    ps, _ = inputs()
    idx = [3, 8]
    zeros = [[np.zeros_like(ps[i]) for i in idx]] * 2
    out, _, seen = hip_run([ps[i] for i in idx], zeros, 0.01, norms=True)
    import torch

    ref, state = R.run([ps[i] for i in idx], zeros, lr=LR, weight_decay=0.01, max_norm=MAX_NORM)
    yard, _ = R.torch_run([ps[i] for i in idx], zeros, torch.float32, lr=LR, weight_decay=0.01, max_norm=MAX_NORM)
    for k in range(2):
        assert (seen[0] == 0).all()
        assert (out[k][1] == 0).all() and (out[k][2] == 0).all()
        check(f"zero gradient numel {ps[idx[k]].size} p", out[k][0], ref[k], yard[k].detach().numpy())


def test_one_nan_gradient_element_poisons_its_tensor_only():
    ps, steps = inputs()
    idx = [5, 10, 8, 2]
    base = [[gs[i] for i in idx] for gs in steps[:3]]
    clean, _, _ = hip_run([ps[i] for i in idx], base)
    bad = [list(gs) for gs in base]
    g = bad[1][1].copy()
    g[CHUNK + 3] = np.nan  # (in the second chunk of the 2 CHUNK + 7 tensor)
    bad[1][1] = g
    out, _, _ = hip_run([ps[i] for i in idx], bad)
    assert all(np.isnan(x).all() for x in out[1])
    for k in (0, 2, 3):
        assert same_bits(out[k], clean[k])


# ---- rebinding --------------------------------------------------------------------------------------------------------------------

def test_zero_grad_and_fresh_gradients_at_new_addresses():
    import torch

    from oakink2_tamf_amd.optim import HipAdamW

    ps, steps = inputs()
    idx = [6, 9, 10]
    dev = "cuda:0"
    params = [torch.nn.Parameter(torch.from_numpy(ps[i].copy()).to(dev)) for i in idx]
    opt = HipAdamW(params, lr=LR, clip_max_norm=MAX_NORM)
    keep, ptrs = [], set()
    for k in range(4):
        opt.zero_grad()  # set_to_none
        assert all(p.grad is None for p in params)
        for p, i in zip(params, idx):
            p.grad = torch.from_numpy(steps[k][i].copy()).to(dev)
            keep.append(p.grad)  # (kept alive, so that every step's gradients live at addresses of their own)
            ptrs.add(p.grad.data_ptr())
        opt.step()
    assert len(ptrs) == 4 * len(idx)
    fixed, _, _ = hip_run([ps[i] for i in idx], [[gs[i] for i in idx] for gs in steps[:4]])
    for p, f in zip(params, fixed):
        assert np.array_equal(p.detach().cpu().numpy().view(np.uint32), f[0].view(np.uint32))
    for p, f in zip(params, fixed):
        assert np.array_equal(opt.state[p]["exp_avg_sq"].cpu().numpy().view(np.uint32), f[2].view(np.uint32))


# ---- interchange with torch.optim.AdamW -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("first", ["hip", "torch"])
def test_state_dict_interchange_with_torch_adamw(first):
    """3 steps with one optimiser, state_dict() -> the other's load_state_dict, 3 more: 6 steps of the restatement inside the gate"""
    import torch

    from oakink2_tamf_amd.optim import HipAdamW

    ps, steps = inputs()
    idx = [1, 6, 8, 10]
    dev = "cuda:0"
    sub = [ps[i] for i in idx]
    grads = [[gs[i] for i in idx] for gs in steps[:6]]
    params = [torch.nn.Parameter(torch.from_numpy(p.copy()).to(dev)) for p in sub]

    def make(kind):
        return HipAdamW(params, lr=LR, weight_decay=0.01, clip_max_norm=MAX_NORM) if kind == "hip" else torch.optim.AdamW(params, lr=LR, weight_decay=0.01)

    def take(opt, some):
        for gs in some:
            for p, g in zip(params, gs):
                p.grad = torch.from_numpy(g.copy()).to(dev)
            if not isinstance(opt, HipAdamW):
                for p in params:
                    torch.nn.utils.clip_grad_norm_(p, MAX_NORM, 2.0)
            opt.step()

    one = make(first)
    take(one, grads[:3])
    sd = one.state_dict()
    assert all(float(s["step"]) == 3 and s["step"].device.type == "cpu" for s in sd["state"].values())
    two = make("torch" if first == "hip" else "hip")
    two.load_state_dict(sd)
    take(two, grads[3:])
    assert all(float(two.state[p]["step"]) == 6 for p in params)
    ref, state = R.run(sub, grads, lr=LR, weight_decay=0.01, max_norm=MAX_NORM)
    tp, topt = R.torch_run(sub, grads, torch.float32, lr=LR, weight_decay=0.01, max_norm=MAX_NORM)
    for k, p in enumerate(params):
        check(f"{first} first, numel {sub[k].size} p", p.detach().cpu().numpy(), ref[k], tp[k].detach().numpy())
        check(f"{first} first, numel {sub[k].size} exp_avg", two.state[p]["exp_avg"].cpu().numpy(), state[k][0], topt.state[tp[k]]["exp_avg"].numpy())
        check(f"{first} first, numel {sub[k].size} exp_avg_sq", two.state[p]["exp_avg_sq"].cpu().numpy(), state[k][1], topt.state[tp[k]]["exp_avg_sq"].numpy())


# ---- grad_norms() creates no state; a refused step changes nothing ------------------------------------------------------------------

def test_grad_norms_before_the_first_step_creates_no_state_and_a_refused_step_keeps_the_counters():
    import torch

    from oakink2_tamf_amd.hip_backend import TamfError
    from oakink2_tamf_amd.optim import HipAdamW

    ps, steps = inputs()
    idx = [4, 9]
    dev = "cuda:0"
    params = [torch.nn.Parameter(torch.from_numpy(ps[i].copy()).to(dev)) for i in idx]
    opt = HipAdamW(params, lr=LR, clip_max_norm=MAX_NORM)
    for p, i in zip(params, idx):
        p.grad = torch.from_numpy(steps[0][i].copy()).to(dev)
    first = opt.grad_norms().cpu().numpy()
    assert len(opt.state) == 0 and opt.state_dict()["state"] == {}  # (torch creates state in step() only)
    opt.step()
    assert all(float(opt.state[p]["step"]) == 1 for p in params)
    again = opt.grad_norms().cpu().numpy()  # (now on the table the step bound)
    assert np.array_equal(first.view(np.uint32), again.view(np.uint32)) and set(opt._tables) == {(0, 0), (0, "norms")}
    alone, _, seen = hip_run([ps[i] for i in idx], [[steps[0][i] for i in idx]], norms=True)
    assert np.array_equal(first.view(np.uint32), seen[0].view(np.uint32))
    assert all(np.array_equal(p.detach().cpu().numpy().view(np.uint32), a[0].view(np.uint32)) for p, a in zip(params, alone))
    before = [p.detach().clone() for p in params]
    opt.param_groups[0]["lr"] = float("nan")
    with pytest.raises(TamfError):
        opt.step()
    assert all(float(opt.state[p]["step"]) == 1 for p in params) and all(torch.equal(b, p.detach()) for b, p in zip(before, params))


def test_mixed_step_counts_and_grad_norms_do_not_rebind_each_other():
    """a parameter whose gradient was None for a step lags by one: the group steps through one table per count, grad_norms() through
    its own, and none of them is bound again while the pointers stay"""
    import torch

    from oakink2_tamf_amd.optim import HipAdamW

    ps, steps = inputs()
    idx = [6, 8]
    dev = "cuda:0"
    params = [torch.nn.Parameter(torch.from_numpy(ps[i].copy()).to(dev)) for i in idx]
    grads = [torch.zeros_like(p) for p in params]
    opt = HipAdamW(params, lr=LR, clip_max_norm=MAX_NORM)
    plan = [[steps[0][6], None], [steps[1][6], steps[1][8]], [steps[2][6], steps[2][8]], [steps[3][6], steps[3][8]]]
    binds = []
    for k, gs in enumerate(plan):
        for p, g, buf in zip(params, gs, grads):
            if g is None:
                p.grad = None
            else:
                buf.copy_(torch.from_numpy(g.copy()))
                p.grad = buf
        opt.grad_norms()
        opt.step()
        binds.append({key: tab.host for key, tab in opt._tables.items()})
    assert [float(opt.state[p]["step"]) for p in params] == [4, 3]
    assert set(binds[-1]) == {(0, 0), (0, 1), (0, "norms")}
    assert all(binds[3][key] is binds[2][key] for key in binds[3])  # (the host arrays of a bind: the same objects = not bound again)
    ref, state = R.run([ps[i] for i in idx], plan, lr=LR, max_norm=MAX_NORM)
    yard, yopt = R.torch_run([ps[i] for i in idx], plan, torch.float32, lr=LR, max_norm=MAX_NORM)
    for k, p in enumerate(params):
        check(f"mixed counts numel {ps[idx[k]].size} p", p.detach().cpu().numpy(), ref[k], yard[k].detach().numpy())
