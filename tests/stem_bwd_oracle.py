"""fp64 oracle and fp32 precision emulations of the CIFAR stem's backward
(BatchNorm + ReLU backward, then the 3x3/s1/p1 conv's weight gradient), shared by
test_stem_bwd_identity_cpu.py and the test_stem_bn_bwd_*_gpu.py files (not a test
module itself).  Plain torch on the CPU, independent of the package.

    dz = dy [y > 0]            S1 = sum dz     S2 = sum dz xhat,  xhat = (x0 - mean) inv
    k1 = gamma inv             Cc = -k1 inv S2 / M                Bc = -k1 S1 / M - Cc mean
    dx = k1 dz + Cc x0 + Bc    dW[co][k] = sum_p dx[p][co] patch[p][k]

Everything takes the kernel's own inputs: x0 (the conv's stored bf16 output), the
forward's fp32 mean / inv, the ReLU mask, dy, and the conv input x for the patches.
Weight gradients are [CO, CI*9] with unfold's (ci, r, s) column order.
"""
import torch
import torch.nn.functional as F

CELLS = [(1, 3, 1, 8), (3, 1, 5, 8), (2, 3, 8, 16), (9, 3, 16, 8), (5, 2, 7, 24)]
BIG = (64, 3, 32, 32)


def bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def patches(x):
    """[P, CI*9] 3x3/s1/p1 patch rows of the NCHW ``x``, same dtype."""
    B, CI, H, W = x.shape
    return F.unfold(x, 3, padding=1).permute(0, 2, 1).reshape(B * H * W, CI * 9)


def rows(t):
    """NCHW [B, C, H, W] -> [P, C]."""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def weight_cols(gw):
    """A [CO, CI, 3, 3] weight gradient as [CO, CI*9] in unfold's column order."""
    return gw.reshape(gw.shape[0], -1)


def oracle(x, x0, dy, keep, mean, inv, gamma):
    """fp64 (dW [CO, K], dgamma, dbeta) with dx unrounded."""
    d = torch.float64
    pt, X0, DZ = patches(x.to(d)), rows(x0.to(d)), rows(dy.to(d)) * rows(keep.to(d))
    mean, inv, gamma = mean.to(d), inv.to(d), gamma.to(d)
    M = X0.shape[0]
    S1 = DZ.sum(0)
    S2 = (DZ * (X0 - mean) * inv).sum(0)
    k1 = gamma * inv
    Cc = -k1 * inv * S2 / M
    Bc = -k1 * S1 / M - Cc * mean
    dx = k1 * DZ + Cc * X0 + Bc
    return dx.t() @ pt, S2, S1


def _coefs32(DZ, X0, mean, inv, gamma):
    M = X0.shape[0]
    S1 = DZ.sum(0)
    S2 = (DZ * (X0 - mean) * inv).sum(0)
    k1 = gamma * inv
    invM = torch.tensor(1.0 / M, dtype=torch.float32)
    Cc = -k1 * inv * S2 * invM
    Bc = -k1 * S1 * invM - Cc * mean
    return k1, Cc, Bc


def emul_unfused(x, x0, dy, keep, mean, inv, gamma):
    """Two-kernel form in fp32: dx rounded to bf16, then an fp32-accumulated weight
    gradient of bf16 operands."""
    f = torch.float32
    pt, X0, DZ = patches(x.to(f)), rows(x0.to(f)), rows(dy.to(f)) * rows(keep.to(f))
    k1, Cc, Bc = _coefs32(DZ, X0, mean.to(f), inv.to(f), gamma.to(f))
    dx = bf(k1 * DZ + Cc * X0 + Bc)
    return dx.t() @ pt


def emul_fused(x, x0, dy, keep, mean, inv, gamma):
    """One-pass form in fp32: G1, G2, G3 accumulated in fp32 from bf16 operands,
    the coefficients applied to the sums."""
    f = torch.float32
    pt, X0, DZ = patches(x.to(f)), rows(x0.to(f)), rows(dy.to(f)) * rows(keep.to(f))
    k1, Cc, Bc = _coefs32(DZ, X0, mean.to(f), inv.to(f), gamma.to(f))
    G1, G2, G3 = DZ.t() @ pt, X0.t() @ pt, pt.sum(0)
    return k1[:, None] * G1 + Cc[:, None] * G2 + Bc[:, None] * G3[None]


def row_rel_live(a, ref):
    """max over the rows whose reference is not zero of ||a_r - ref_r|| / ||ref_r||;
    rows whose reference is exactly zero (gamma = 0) must be exactly zero."""
    a, ref = a.detach().to("cpu", torch.float64), ref.detach().to("cpu", torch.float64)
    if a.dim() == 1:
        a, ref = a[None], ref[None]
    den = ref.norm(dim=-1)
    live = den > 0
    assert bool(live.any()), "no live reference row"
    assert bool((a[~live] == 0).all()), "a row with a zero reference is not zero"
    return float(((a - ref).norm(dim=-1)[live] / den[live]).max())


def cpu_case(shape, dc, gmode, seed=0, CO=64, eps=1e-5):
    """bf16-exact inputs of one cell, made on the CPU the way the forward makes them:
    (x, x0, dy, keep, mean, inv, gamma), all fp32 holding bf16 values except the
    fp32 statistics and gamma."""
    g = torch.Generator().manual_seed(seed)
    B, CI, H, W = shape
    x = bf(torch.randn(B, CI, H, W, generator=g) + dc)
    w = bf(torch.randn(CO, CI, 3, 3, generator=g) * 0.3)
    x0 = bf(F.conv2d(x.double(), w.double(), padding=1).float())
    X0 = rows(x0)
    mean = X0.mean(0)
    var = (X0 * X0).mean(0) - mean * mean
    inv = torch.rsqrt(var.clamp_min(0) + eps)
    gamma = torch.ones(CO)
    if gmode != "one":
        gamma = torch.randn(CO, generator=g)
    if gmode == "zeros":
        gamma[::5] = 0.0
    beta = torch.randn(CO, generator=g) * 0.5
    sc = gamma * inv
    sh = beta - mean * sc
    y = bf(torch.relu(x0 * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1)))
    keep = (y > 0).float()
    dy = bf(torch.randn(B, CO, H, W, generator=g))
    return x, x0, dy, keep, mean, inv, gamma
