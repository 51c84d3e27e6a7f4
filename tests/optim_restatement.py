"""The optimiser step of include/tamf_optim.h restated in numpy float64: the reference's per-parameter clip_grad_norm_(param, max_norm, 2.0)
followed by torch.optim.AdamW's single-tensor update, per tensor.  The yardstick of tests/test_optim_cpu.py (against torch in
float64) and tests/test_optim_gpu.py (against the HIP step and torch's float32 run)."""
import numpy as np


def grad_norm(g):
    g = np.asarray(g, np.float64)
    return float(np.sqrt(np.sum(g * g)))


def clip_coef(g, max_norm):
    """c = min(1, max_norm / (n + 1e-6)); None: no clipping.  A NaN norm gives a NaN coefficient, as torch.clamp keeps it."""
    if max_norm is None:
        return 1.0
    c = float(max_norm) / (grad_norm(g) + 1e-6)
    return c if (c < 1.0 or c != c) else 1.0


def adamw_step(p, g, m, v, t, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=None):
    """one step `t` (1-based) of one tensor -> (p, m, v), float64; the inputs are not modified"""
    b1, b2 = betas
    p, g, m, v = (np.array(x, np.float64) for x in (p, g, m, v))
    with np.errstate(invalid="ignore"):
        g = clip_coef(g, max_norm) * g
        p = p * (1.0 - lr * weight_decay)
        m = m + (g - m) * (1.0 - b1)
        v = b2 * v + (1.0 - b2) * g * g
        p = p - (lr / (1.0 - b1 ** t)) * m / (np.sqrt(v) / np.sqrt(1.0 - b2 ** t) + eps)
    return p, m, v


def run(ps, grads_per_step, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=None, state=None, lrs=None):
    """`len(grads_per_step)` steps of a list of tensors; grads_per_step[s][i] is tensor i's gradient at step s, or None (skipped, as
    torch skips a parameter without a gradient).  state: [(m, v, steps taken)] per tensor to continue from.  lrs: one lr per step.
    -> (ps, state) in float64."""
    ps = [np.array(p, np.float64) for p in ps]
    state = [(np.zeros_like(p), np.zeros_like(p), 0) for p in ps] if state is None else [(np.array(m, np.float64), np.array(v, np.float64), int(t)) for m, v, t in state]
    for s, grads in enumerate(grads_per_step):
        for i, g in enumerate(grads):
            if g is None or ps[i].size == 0:
                continue
            m, v, t = state[i]
            ps[i], m, v = adamw_step(ps[i], g, m, v, t + 1, lrs[s] if lrs is not None else lr, betas, eps, weight_decay, max_norm)
            state[i] = (m, v, t + 1)
    return ps, state


def torch_run(ps, grads_per_step, dtype, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=None, device="cpu", optimizer=None):
    """The reference's sequence itself in torch at `dtype` on `device`: per-parameter clip_grad_norm_ + torch.optim.AdamW.step().
    -> (params, optimizer); pass `optimizer` (and its params as ps) to continue a run."""
    import torch

    if optimizer is None:
        params = [torch.nn.Parameter(torch.as_tensor(np.array(p), dtype=dtype, device=device)) for p in ps]
        optimizer = torch.optim.AdamW(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    else:
        params = list(ps)
    for grads in grads_per_step:
        for p, g in zip(params, grads):
            p.grad = None if g is None else torch.as_tensor(np.array(g), dtype=dtype, device=device).reshape(p.shape)
        if max_norm is not None:
            for p in params:
                if p.grad is not None:
                    torch.nn.utils.clip_grad_norm_(p, max_norm, 2.0)
        optimizer.step()
    return params, optimizer


def rel_err(a, ref):
    """max |a - ref| over max |ref| (1 when ref is all zero), the figure the gates are stated in"""
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    if ref.size == 0:
        return 0.0
    return float(np.max(np.abs(a - ref)) / max(float(np.max(np.abs(ref))), 1e-300))
