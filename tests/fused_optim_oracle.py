"""fp64 oracle of AdamW / SGD + global-norm clipping + warmup-cosine schedule,
shared by test_fused_optim_cpu.py and test_fused_optim_gpu.py (not a test
module itself).  Written from the formulas, independent of the package; the CPU
test validates it against torch.optim.AdamW(float64) + clip_grad_norm_ +
LambdaLR before anything is compared against it."""
import math

import numpy as np
import torch


def sched_lr(base, t, kind="constant", warmup=0, total=0, lr_min=0.0):
    """Closed form of the learning rate of update t (1-based), in Python doubles."""
    if kind == "constant":
        return base
    if t <= warmup:
        return base * t / warmup
    if t >= total:
        return lr_min
    return lr_min + 0.5 * (base - lr_min) * (1.0 + math.cos(math.pi * (t - warmup) / (total - warmup)))


def oracle_adamw(p0, grads, decay=None, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.0,
                 grad_scale=1.0, max_norm=0.0, sched=None, t0=0, m0=None, v0=None):
    """``grads``: list of flat tensors, one per step.  ``decay``: per-element 0/1
    tensor (None = decay everything).  Returns a dict of fp64 results."""
    sched = sched or {}
    p = p0.double().clone()
    m = torch.zeros_like(p) if m0 is None else m0.double().clone()
    v = torch.zeros_like(p) if v0 is None else v0.double().clone()
    dec = torch.ones_like(p) if decay is None else decay.double()
    acc = torch.zeros_like(p)
    b1, b2 = betas
    lrs, norms, clips = [], [], []
    t = t0
    for g in grads:
        g = g.double()
        clip, norm = 1.0, 0.0
        if max_norm > 0:
            norm = grad_scale * float(g.norm())
            clip = min(1.0, max_norm / (norm + 1e-6))
        gs = (grad_scale * clip) * g
        t += 1
        lr_t = sched_lr(lr, t, **sched)
        m = b1 * m + (1 - b1) * gs
        v = b2 * v + (1 - b2) * gs * gs
        bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
        new = p * (1 - lr_t * wd * dec) - (lr_t / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps)
        acc += new - p
        p = new
        lrs.append(lr_t), norms.append(norm), clips.append(clip)
    return dict(p=p, m=m, v=v, acc=acc, lrs=lrs, norms=norms, clips=clips)


def torch_adamw(p0, grads, decay=None, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.0,
                grad_scale=1.0, max_norm=0.0, sched=None, dtype=torch.float64):
    """The same run through torch.optim.AdamW + clip_grad_norm_ + LambdaLR on the
    CPU in ``dtype``; returns p, m, v as flat tensors in the layout of ``p0``."""
    sched = sched or {}
    p0 = p0.detach().cpu()
    dec = torch.ones(p0.numel(), dtype=torch.bool) if decay is None else decay.cpu().bool()
    pd = torch.nn.Parameter(p0[dec].to(dtype).clone())
    pn = torch.nn.Parameter(p0[~dec].to(dtype).clone())
    groups = []
    if pd.numel():
        groups.append(dict(params=[pd], weight_decay=wd))
    if pn.numel():
        groups.append(dict(params=[pn], weight_decay=0.0))
    opt = torch.optim.AdamW(groups, lr=lr, betas=betas, eps=eps, foreach=False)
    lam = torch.optim.lr_scheduler.LambdaLR(
        opt, lambda e: sched_lr(lr, e + 1, **sched) / lr if lr else 1.0)
    live = [q for q in (pd, pn) if q.numel()]
    for g in grads:
        g = g.detach().cpu().to(dtype)
        pd.grad = g[dec] * grad_scale
        pn.grad = g[~dec] * grad_scale
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(live, max_norm)
        opt.step()
        lam.step()
    out = {}
    for name, key in (("p", None), ("m", "exp_avg"), ("v", "exp_avg_sq")):
        flat = torch.zeros(p0.numel(), dtype=dtype)
        for q, sel in ((pd, dec), (pn, ~dec)):
            if q.numel():
                flat[sel] = q.detach() if key is None else opt.state[q][key]
        out[name] = flat
    return out


def max_err(x, ref64):
    return float((x.detach().cpu().double() - ref64).abs().max())


def ulp_of(x64):
    """One fp32 ulp at the largest magnitude of ``x64``."""
    return float(np.spacing(np.float32(float(x64.abs().max()))))


def accuracy_report(native, torch32, ref):
    """Per-tensor (native error, torch fp32 error, bound) against the fp64 oracle.
    Bound: 4 x the fp32 torch.optim.AdamW error + one fp32 ulp of the largest
    magnitude (hardware reciprocal / square root and the norm's summation order)."""
    rows = {}
    for k in ("p", "m", "v"):
        en, et = max_err(native[k], ref[k]), max_err(torch32[k], ref[k])
        rows[k] = (en, et, 4.0 * et + ulp_of(ref[k]))
    return rows
