"""Exact-integer operands for the conv and GEMM kernel tests (helper, not a test
module; same role as tests/kernel_oracles.py).

With small integer operands every product and every partial sum of a conv or a
GEMM is an integer below 2^24: fp32 accumulation is exact in ANY order (MFMA
order, split-K, fp32 atomics, slab reduce, BN partial slots), and an output that
is an integer of magnitude <= 256 is exact in bf16.  The kernel is then compared
with the reference by ``torch.equal``, element by element, and a mismatch is
reported by its coordinates in the logical (NCHW / OIHW / row, column) axes.

The range conditions are always evaluated on the REFERENCE (``assert_exact_range``),
never on the kernel's output, and no element is ever left out of a comparison.
"""
from __future__ import annotations

import torch

# default operand ranges and densities
ACT = dict(lo=-2, hi=2, density=0.25)      # activations and output gradients
WGT = dict(lo=-1, hi=1, density=0.25)      # weights
ADD = dict(lo=-4, hi=4, density=1.0)       # addends and biases

COMPARED = [0]     # whole-tensor bitwise comparisons made by this process (for reports)


def sparse_ints(shape, lo, hi, density, generator):
    """fp32 tensor of integers drawn uniformly from [lo, hi], each kept with
    probability ``density``, else 0.  Drawn on the generator's device."""
    dev = generator.device
    v = torch.randint(lo, hi + 1, tuple(shape), generator=generator, device=dev)
    if density < 1.0:
        keep = torch.rand(tuple(shape), generator=generator, device=dev) < density
        v = v * keep
    return v.to(torch.float32)


def gen(seed: int) -> torch.Generator:
    """CPU generator: the operands of a case are the same on every machine."""
    return torch.Generator().manual_seed(seed)


def to_bf16(t, channels_last=False, device=None):
    """``t`` (fp32 integers) as bf16 on ``device``; asserts the round trip is lossless."""
    b = t.to(torch.bfloat16)
    assert torch.equal(b.to(t.dtype), t), "operand is not exact in bf16"
    if device is not None:
        b = b.to(device)
    if channels_last:
        b = b.contiguous(memory_format=torch.channels_last)
    return b


def assert_exact_range(ref, kind, what=""):
    """The condition that makes ``torch.equal`` legitimate, on the reference:
    every element an integer, |v| <= 256 (``bf16``: the store is exact) or
    |v| < 2^24 (``fp32``: every accumulation order is exact).  Returns max |v|."""
    assert kind in ("bf16", "fp32"), kind
    r = ref.detach().to(torch.float64)
    assert bool(torch.isfinite(r).all()), f"{what}: reference is not finite"
    assert bool((r == r.round()).all()), f"{what}: reference is not integer-valued"
    top = float(r.abs().max()) if r.numel() else 0.0
    bound = 256.0 if kind == "bf16" else float(2 ** 24)
    ok = top <= bound if kind == "bf16" else top < bound
    assert ok, (f"{what}: reference reaches |v| = {top:g}, outside the exact {kind} range "
                f"({bound:g}); lower the density of this shape")
    return top


def assert_equal_located(got, ref, axes, what=""):
    """``got`` == ``ref`` element by element (values compared in fp64 after an exact
    widening; shapes must agree).  On a mismatch the error names the count, the
    first 8 mismatches as (logical index, got, want), and per axis the distinct
    mismatching indices when there are at most 8 of them.  Indices are those of
    the logical view (``tensor[b, c, h, w]``), whatever the storage order."""
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    assert len(axes) == got.dim(), (what, axes, tuple(got.shape))
    COMPARED[0] += 1
    g = got.detach()
    r = ref.detach().to(g.device)
    if g.dtype == r.dtype and torch.equal(g, r):
        return
    g64, r64 = g.to(torch.float64), r.to(torch.float64)
    bad = g64 != r64
    bad |= torch.isnan(g64) != torch.isnan(r64)
    n = int(bad.sum())
    if n == 0:
        return
    idx = bad.nonzero().cpu()                  # [n, ndim], row-major in the logical axes
    gv, rv = g64[bad].cpu(), r64[bad].cpu()    # same (logical row-major) order
    first = ", ".join(
        f"({', '.join(f'{a}={int(i)}' for a, i in zip(axes, row))}): got {float(x):g} want "
        f"{float(y):g}" for row, x, y in zip(idx[:8], gv[:8], rv[:8]))
    where = []
    for d, a in enumerate(axes):
        u = torch.unique(idx[:, d]).tolist()
        if len(u) <= 8 and len(u) < got.shape[d]:
            where.append(f"{a} in {{{', '.join(str(int(v)) for v in u)}}}" if len(u) > 1
                         else f"{a}={int(u[0])}")
    loc = ("all mismatches at " + ", ".join(where)) if where else "mismatches spread over every axis"
    raise AssertionError(f"{what}: {n} of {got.numel()} elements differ; {loc}; first: {first}")


_CONV_CASES: dict = {}


def conv_case(row, seed=0, density=None):
    """Operands and fp64 references of one conv geometry, computed once on the CPU
    and shared by every test that names the row (treat the tensors as read-only).

    ``row`` = (B, CI, H, W, CO, k, stride, pad).  fp32 integer operands: ``x``,
    ``w``, ``dy``, ``bias`` [CO], ``add_y`` (output-shaped addend), ``add_x``
    (input-shaped), ``sub`` (stride 2: the addend of parity class (0, 0)),
    ``g0`` / ``b0`` (weight / bias gradient start values).  fp64 references: ``y``,
    ``y_epi`` = relu(y + bias + add_y), ``sums`` [2, CO] of y, ``dx``, ``dx_add``,
    ``dx_sub``, ``dw`` (one call's contribution), ``dw2`` = g0 + 2 dw, ``db1`` =
    b0 + colsum(dy).  ``density`` overrides the activations' and weights' 1/4."""
    key = (tuple(row), seed, density)
    if key in _CONV_CASES:
        return _CONV_CASES[key]
    import torch.nn.functional as F

    B, CI, H, W, CO, k, st, pd = row
    g = gen(seed)
    act = dict(ACT, density=density) if density is not None else ACT
    wgt = dict(WGT, density=density) if density is not None else WGT
    c = {}
    c["x"] = sparse_ints((B, CI, H, W), generator=g, **act)
    c["w"] = sparse_ints((CO, CI, k, k), generator=g, **wgt)
    xr = c["x"].double().requires_grad_(True)
    wr = c["w"].double().requires_grad_(True)
    y = F.conv2d(xr, wr, None, st, pd)
    c["dy"] = sparse_ints(tuple(y.shape), generator=g, **act)
    c["bias"] = sparse_ints((CO,), generator=g, **ADD)
    c["add_y"] = sparse_ints(tuple(y.shape), generator=g, **ADD)
    c["add_x"] = sparse_ints((B, CI, H, W), generator=g, **ADD)
    c["sub"] = sparse_ints((B, CI, (H + 1) // 2, (W + 1) // 2), generator=g, **ADD)
    c["g0"] = sparse_ints((CO, CI, k, k), generator=g, **ADD)
    c["b0"] = sparse_ints((CO,), generator=g, **ADD)
    y.backward(c["dy"].double())
    y = y.detach()
    c["y"] = y
    c["y_epi"] = torch.relu(y + c["bias"].double().view(1, -1, 1, 1) + c["add_y"].double())
    c["sums"] = torch.stack([y.sum(dim=(0, 2, 3)), (y * y).sum(dim=(0, 2, 3))])
    c["dx"] = xr.grad
    c["dx_add"] = xr.grad + c["add_x"].double()
    dxs = xr.grad.clone()
    dxs[:, :, ::2, ::2] += c["sub"].double()
    c["dx_sub"] = dxs
    c["dw"] = wr.grad
    c["dw2"] = c["g0"].double() + 2 * wr.grad
    c["db1"] = c["b0"].double() + c["dy"].double().sum(dim=(0, 2, 3))
    _CONV_CASES[key] = c
    return c


def conv_case_ranges(c, stride):
    """``assert_exact_range`` on every reference of a ``conv_case``; returns the
    largest |value| per pass."""
    top = {
        "fwd": assert_exact_range(c["y"], "bf16", "y"),
        "fwd_epilogue": assert_exact_range(c["y_epi"], "bf16", "relu(y + bias + addend)"),
        "bn_sums": assert_exact_range(c["sums"], "fp32", "BN sums"),
        "dgrad": assert_exact_range(c["dx"], "bf16", "dx"),
        "dgrad_addend": assert_exact_range(c["dx_add"], "bf16", "dx + addend"),
        "wgrad_twice": assert_exact_range(c["dw2"], "fp32", "g0 + 2 dw"),
        "dbias": assert_exact_range(c["db1"], "fp32", "b0 + colsum(dy)"),
    }
    # also before the epilogue's ReLU and before the start value is added
    assert_exact_range(c["y"] + c["bias"].double().view(1, -1, 1, 1) + c["add_y"].double(),
                       "bf16", "y + bias + addend")
    assert_exact_range(c["dw"], "fp32", "dw")
    if stride == 2:
        top["dgrad_sub_addend"] = assert_exact_range(c["dx_sub"], "bf16", "dx + sub addend")
    return top


def bn_sums(part, G, C):
    """[2, C] per-channel (sum, sum of squares) from the [2][G][C] BN partial slots."""
    G = int(G)
    return part[:2 * G * C].view(2, G, C).sum(1)
