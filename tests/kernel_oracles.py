"""fp64 oracles, row-wise error checkers, a NumPy Philox4x32-10 and precision-model
emulations for the ViT / loss / dropout kernels (csrc/attention.hip,
transformer.hip, xent.hip, dropout.hip) and for BatchNorm and pooling
(csrc/bn.hip, pool.hip).  Shared by test_kernel_oracles_cpu.py
and the *_edges_gpu.py / test_dropout_stream_gpu.py files (not a test module
itself).  Written from the formulas with plain torch / NumPy ops, independent
of the package; everything here runs on the CPU.

The emulations are NOT the code under test: each is the fp64 reference with the
kernel's documented rounding points inserted, so the CPU file can show that the
GPU tolerances hold for a correct implementation with a 3x margin.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

LN2 = math.log(2.0)


def bf(t):
    """Round to bf16 (round-to-nearest-even), keep the dtype."""
    return t.to(torch.bfloat16).to(t.dtype)


def f64(t):
    return t.detach().to("cpu", torch.float64)


# ------------------------------------------------------------------- checkers
def _rows(a, ref):
    a, ref = f64(a), f64(ref)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    if a.dim() == 1:
        a, ref = a[None], ref[None]
    return a, ref


def row_rel(a, ref):
    """max over rows (last dim) of ||a_r - ref_r|| / ||ref_r||."""
    a, ref = _rows(a, ref)
    err = (a - ref).norm(dim=-1)
    den = ref.norm(dim=-1)
    assert bool((den > 0).all()), "row_rel: a reference row is zero (use row_abs)"
    return float((err / den).max())


def row_abs(a, ref, den=None):
    """max over rows of ||a_r - ref_r|| / max_r ||ref_r||: for gradients, where
    single rows may be legitimately near zero.  2-D input is one group of rows;
    [G, R, D] input takes the max row norm per group g (attention: one group per
    (batch, head)) and returns the worst group.  ``den`` ([G]) replaces the
    groups' max row norms where the reference itself is a cancelled-out zero
    (see attention_cancel_scale)."""
    a, ref = _rows(a, ref)
    if a.dim() == 2:
        a, ref = a[None], ref[None]
    a, ref = a.reshape(-1, a.shape[-2], a.shape[-1]), ref.reshape(-1, *ref.shape[-2:])
    err = (a - ref).norm(dim=-1).amax(dim=-1)
    den = ref.norm(dim=-1).amax(dim=-1) if den is None else f64(den).reshape(-1)
    assert den.shape == err.shape and bool((den > 0).all()), "row_abs: a zero denominator"
    return float((err / den).max())


# --------------------------------------------------------------- Philox4x32-10
_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_MASK = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2,
    3", SC'11).  ``ctr``: four uint32 arrays (or ints) of one shape, ``key``: two
    uint32 scalars.  Returns the four output words as uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & _MASK for x in ctr]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c[0], _M1 * c[2]
        hi0, lo0 = p0 >> _S32, p0 & _MASK
        hi1, lo1 = p1 >> _S32, p1 & _MASK
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def dropout_threshold(p):
    return min(int(float(p) * 4294967296.0), 0xFFFFFFFF)


def dropout_mask_ref(nmask, p, seed, offset):
    """Keep mask (uint8 ndarray of ``nmask``) of the dropout stream: element i
    takes word i & 3 of philox(ctr = (g_lo, g_hi, off_lo, off_hi), key = (seed_lo,
    seed_hi)) with g = i >> 2, and is kept when the word >= uint32(p * 2^32)."""
    seed, offset = int(seed) & (2**64 - 1), int(offset) & (2**64 - 1)
    g = np.arange((nmask + 3) // 4, dtype=np.uint64)
    z = np.zeros_like(g)
    words = philox4x32_10((g & _MASK, g >> _S32, z + np.uint64(offset & 0xFFFFFFFF),
                           z + np.uint64(offset >> 32)),
                          (seed & 0xFFFFFFFF, seed >> 32))
    w = np.stack(words, axis=1).reshape(-1)[:nmask]
    return (w >= np.uint32(dropout_threshold(p))).astype(np.uint8)


# ------------------------------------------------------------------ attention
def split_qkv(qkv, H):
    """[B, N, 3*H*64] rows -> q, k, v as fp64 [B, H, N, 64]."""
    B, N, _ = qkv.shape
    return f64(qkv).view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)


def merge_heads(t):
    """[B, H, N, 64] -> [B, N, H*64]."""
    B, H, N, d = t.shape
    return t.permute(0, 2, 1, 3).reshape(B, N, H * d)


def attention_ref(qkv, H):
    """fp64 attention of bf16 qkv rows -> (out [B, N, D], lse2 [B, H, N]) with
    lse2 = log2 sum_j exp(s_ij * scale)."""
    q, k, v = split_qkv(qkv, H)
    s = q @ k.transpose(-1, -2) * 0.125
    lse = torch.logsumexp(s, dim=-1)
    out = torch.exp(s - lse[..., None]) @ v
    return merge_heads(out), lse / LN2


def attention_bwd_ref(qkv, dout, H):
    """fp64 gradient of attention_ref's out w.r.t. the qkv rows, [B, N, 3*D]."""
    x = f64(qkv).requires_grad_(True)
    B, N, _ = x.shape
    q, k, v = x.view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) * 0.125
    out = merge_heads(torch.softmax(s, dim=-1) @ v)
    out.backward(f64(dout))
    return x.grad


def attention_fwd_emul(qkv, H):
    """Forward precision model: the unnormalised P = exp(s - max) is rounded to
    bf16 before P.V, the row sum uses the unrounded P, the output is bf16."""
    q, k, v = split_qkv(qkv, H)
    s = q @ k.transpose(-1, -2) * 0.125
    mx = s.amax(dim=-1, keepdim=True)
    p = torch.exp(s - mx)
    ssum = p.sum(dim=-1, keepdim=True)
    out = bf((bf(p) @ v) / ssum)
    lse2 = (mx + torch.log(ssum)).squeeze(-1) / LN2
    return merge_heads(out), lse2


def attention_bwd_emul(qkv, out16, dout, lse2, H):
    """Backward precision model: di = rowsum(dO * O) from the bf16 output, P
    recomputed from lse2, dS = P * (dP - di) and P rounded to bf16 before the
    three output products, bf16 results."""
    q, k, v = split_qkv(qkv, H)
    B, N = qkv.shape[:2]
    do = f64(dout).view(B, N, H, 64).permute(0, 2, 1, 3)
    o = f64(out16).view(B, N, H, 64).permute(0, 2, 1, 3)
    di = (do * o).sum(-1, keepdim=True)
    p = torch.exp(q @ k.transpose(-1, -2) * 0.125 - f64(lse2)[..., None] * LN2)
    ds = bf(p * (do @ v.transpose(-1, -2) - di))
    dq = bf(ds @ k * 0.125)
    dk = bf(ds.transpose(-1, -2) @ q * 0.125)
    dv = bf(bf(p).transpose(-1, -2) @ do)
    return torch.stack([merge_heads(t) for t in (dq, dk, dv)], dim=2).reshape(B, N, -1)


def heads_rows(t, H):
    """[B, N, H*64] -> [B*H, N, 64]: row_abs groups per (batch, head)."""
    B, N, _ = t.shape
    return f64(t).view(B, N, H, 64).permute(0, 2, 1, 3).reshape(B * H, N, 64)


def attention_cancel_scale(qkv, dout, H):
    """Per-(b, head) size of the terms that CANCEL in dq and dk.

    dS_ij = P_ij (dP_ij - di_i) with di_i = sum_j P_ij dP_ij.  Where P is one-hot
    (N = 1, one dominant key, a loud token every query locks onto) dP_ij = di_i
    on the only key with weight, so the true dq and dk are zero up to exp(-gap)
    and a relative error against them measures nothing (the fp64 reference and
    the emulation disagree by O(1) there).  What a kernel can be held to is the
    size of what cancels: |dS_ij| <= P_ij (|dP_ij| + |di_i|), so
      den_q = scale * max_i sum_j P_ij (|dP_ij| + |di_i|) ||k_j||
      den_k = scale * max_j sum_i P_ij (|dP_ij| + |di_i|) ||q_i||.
    By the triangle inequality both are >= the largest reference row, so they
    are used ONLY in the cells named by attention_cancels()."""
    q, k, v = split_qkv(qkv, H)
    B, N = qkv.shape[:2]
    do = f64(dout).view(B, N, H, 64).permute(0, 2, 1, 3)
    p = torch.softmax(q @ k.transpose(-1, -2) * 0.125, dim=-1)
    dp = do @ v.transpose(-1, -2)
    di = (p * dp).sum(-1, keepdim=True)
    w = p * (dp.abs() + di.abs())
    den_q = 0.125 * (w @ k.norm(dim=-1, keepdim=True)).amax(dim=(-1, -2))
    den_k = 0.125 * (w.transpose(-1, -2) @ q.norm(dim=-1, keepdim=True)).amax(dim=(-1, -2))
    return den_q.reshape(-1), den_k.reshape(-1)


def attention_cancels(N, regime):
    return N == 1 or regime in ("loud", "onehot")


def attention_grad_errors(dqkv, dref, qkv, dout, H, regime):
    """(dq, dk, dv) row_abs errors of a [B, N, 3*D] gradient, rows = per-token
    64-vectors, one group per (batch, head); the checker of both the GPU test
    and the CPU floor."""
    B, N, _ = qkv.shape
    a, r = f64(dqkv).view(B, N, 3, H * 64), f64(dref).view(B, N, 3, H * 64)
    dens = attention_cancel_scale(qkv, dout, H) if attention_cancels(N, regime) else (None, None)
    return [row_abs(heads_rows(a[:, :, t], H), heads_rows(r[:, :, t], H), den)
            for t, den in enumerate((*dens, None))]


# ------------------------------------------------------------------ LayerNorm
def layernorm_ref(x, gamma, beta, eps, residual=None):
    """fp64 LayerNorm of bf16 rows -> (y, h); with ``residual`` h = bf16(x + r)
    is the value normalised (the fused add writes it as bf16), else h = x."""
    h = f64(x) if residual is None else bf(f64(x) + f64(residual))
    mean = h.mean(-1, keepdim=True)
    var = ((h - mean) ** 2).mean(-1, keepdim=True)
    y = (h - mean) / torch.sqrt(var + eps)
    if gamma is not None:
        y = y * f64(gamma)
    if beta is not None:
        y = y + f64(beta)
    return y, h


def layernorm_bwd_ref(h, dy, gamma, eps, dh=None, dtype=torch.float64):
    """Gradients of LayerNorm at the (bf16-exact) rows ``h``: (dx, dgamma, dbeta);
    ``dh`` is added to dx (the residual stream's own gradient).  ``dtype`` =
    float32 evaluates the same formula in fp32 (the dgamma / dbeta floor)."""
    h, dy = f64(h).to(dtype), f64(dy).to(dtype)
    D = h.shape[-1]
    mean = h.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((h - mean) ** 2).mean(-1, keepdim=True) + eps)
    xh = (h - mean) * rstd
    g = dy if gamma is None else dy * f64(gamma).to(dtype)
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    if dh is not None:
        dx = dx + f64(dh).to(dtype)
    return dx, (dy * xh).reshape(-1, D).sum(0), dy.reshape(-1, D).sum(0)


def layernorm_emul(x, gamma, beta, eps, residual=None):
    y, h = layernorm_ref(x, gamma, beta, eps, residual)
    return bf(y), h


def layernorm_bwd_emul(h, dy, gamma, eps, dh=None):
    dx, dg, db = layernorm_bwd_ref(h, dy, gamma, eps, dh)
    return bf(dx), dg, db


# -------------------------------------------------------------------- softmax
def softmax_ref(s, scale):
    return torch.softmax(f64(s) * scale, dim=-1)


def softmax_bwd_ref(p, dp, scale):
    """dS = scale * P * (dP - sum_j P_j dP_j) at the given P (the kernel's input)."""
    p, dp = f64(p), f64(dp)
    return scale * p * (dp - (p * dp).sum(-1, keepdim=True))


def softmax_emul(s, scale):
    return bf(softmax_ref(s, scale))


def softmax_bwd_emul(p, dp, scale):
    return bf(softmax_bwd_ref(p, dp, scale))


# ----------------------------------------------------------------------- GELU
_K0, _K1 = math.sqrt(2.0 / math.pi), 0.044715


def gelu_ref(x):
    x = f64(x)
    return 0.5 * x * (1.0 + torch.tanh(_K0 * (x + _K1 * x ** 3)))


def gelu_grad_ref(x):
    x = f64(x)
    t = torch.tanh(_K0 * (x + _K1 * x ** 3))
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * _K0 * (1.0 + 3.0 * _K1 * x * x)


def gelu_emul(x):
    return bf(gelu_ref(x))


def gelu_bwd_emul(x, dy):
    return bf(f64(dy) * gelu_grad_ref(x))


def gelu_grid(numel):
    """Deterministic bf16 grid over [-12, 12] plus {+-0, +-1e-3, +-40, +-200}."""
    special = torch.tensor([0.0, -0.0, 1e-3, -1e-3, 40.0, -40.0, 200.0, -200.0])
    if numel <= special.numel():
        return special[:numel].to(torch.bfloat16)
    grid = torch.linspace(-12.0, 12.0, numel - special.numel())
    return torch.cat([special, grid]).to(torch.bfloat16)


# -------------------------------------------------------------- cross-entropy
def xent_ref(logits, labels, smoothing=0.0, ignore_index=-100, gloss=1.0):
    """fp64 F.cross_entropy of the given logits -> (loss, dlogits * gloss).
    Labels outside [0, C) are mapped to ignore_index first (the kernels treat
    them as ignored; F.cross_entropy would raise)."""
    x = f64(logits).requires_grad_(True)
    y = labels.detach().cpu().clone()
    y[(y < 0) | (y >= x.shape[1])] = ignore_index
    loss = F.cross_entropy(x, y, label_smoothing=smoothing, ignore_index=ignore_index)
    (loss * gloss).backward()
    return loss.detach(), x.grad


def xent_hits_ref(logits, labels, ignore_index=-100):
    """Top-1 hits with NumPy's argmax (first occurrence of the maximum)."""
    x = f64(logits).numpy()
    y = labels.detach().cpu().numpy()
    ok = (y != ignore_index) & (y >= 0) & (y < x.shape[1])
    return int(((np.argmax(x, axis=1) == y) & ok).sum())


# ------------------------------------------------------------------ vit_embed
def vit_embed_ref(tok, cls, pos):
    """cat(cls, tok) + pos in fp64: [B, N + 1, D]."""
    tok = f64(tok)
    B, _, D = tok.shape
    c = f64(cls).reshape(1, 1, D).expand(B, 1, D)
    return torch.cat([c, tok], dim=1) + f64(pos).reshape(1, -1, D)


# ------------------------------------------------------------ input regimes
def attention_inputs(B, N, H, regime, seed=0):
    """bf16 qkv rows [B, N, 3*H*64] and a bf16 dout [B, N, H*64] on the CPU.
    Regimes: "sc1" / "sc3" = randn * sc; "loud" = last token's q, k, v x50;
    "onehot" = k = 8 * q[perm] (one dominant key per query: exact one-hot P)."""
    g = torch.Generator().manual_seed(seed * 1000 + N)
    sc = 3.0 if regime == "sc3" else 1.0
    x = torch.randn(B, N, 3, H, 64, generator=g) * sc
    if regime == "loud":
        x[:, N - 1] *= 50.0
    elif regime == "onehot":
        perm = torch.randperm(N, generator=g)
        x[:, :, 1] = 8.0 * x[:, perm, 0].to(torch.bfloat16).float()
    dout = torch.randn(B, N, H * 64, generator=g)
    return x.reshape(B, N, 3 * H * 64).to(torch.bfloat16), dout.to(torch.bfloat16)


def layernorm_inputs(rows, D, regime, seed=0):
    """(x, r, dy, dh) bf16 and (gamma, beta) fp32 on the CPU.  Regimes: "std" =
    randn * 2 + 0.5; "mean" = 50 + randn (mean^2 >> var)."""
    g = torch.Generator().manual_seed(seed * 7919 + rows * 31 + D)
    rn = lambda *s: torch.randn(*s, generator=g)
    x = (50.0 + rn(rows, D)) if regime == "mean" else (rn(rows, D) * 2 + 0.5)
    r = rn(rows, D)
    return (x.to(torch.bfloat16), r.to(torch.bfloat16), rn(rows, D).to(torch.bfloat16),
            rn(rows, D).to(torch.bfloat16), 1 + 0.1 * rn(D), 0.1 * rn(D))


# ------------------------------------------- cells and thresholds (GPU + CPU)
# The GPU files run these cells against these thresholds; the CPU file shows
# that the emulations above pass every cell at ONE THIRD of the threshold.
ATTN_N = (1, 15, 16, 17, 31, 32, 33, 129, 240, 241, 255, 256)
ATTN_REGIMES = ("sc1", "sc3", "loud", "onehot")
ATTN_CELLS = [(2, n, 2, r) for n in ATTN_N for r in ATTN_REGIMES] + [(3, 197, 12, "sc1"),
                                                                    (3, 197, 12, "sc3")]
# Emulation floors (max over the cells and three input seeds, per-token rows):
#   out   row_rel  sc1 0.0035  sc3 0.0031  loud 0.0042  onehot 0.0001
#   dq/dk row_abs  sc1 0.0043  sc3 0.0150  loud 0.0015  onehot 0.0000
#   dv    row_abs  <= 0.0035 everywhere
# A threshold is the nominal one (out 1e-2, gradients 2e-2) unless 3x its floor
# is larger; then it is 3x the floor.  The bf16 rounding of P at N >= 240 and of
# the loud rows puts the out floor just above 1e-2 / 3; at sc = 3 the bf16
# rounding of dS against near-cancelling rows puts dq / dk at 0.015.
ATTN_OUT_TOL = 1.3e-2     # row_rel, per (b, token, head); floor 0.0042
ATTN_DQK_TOL = {"sc1": 2e-2, "sc3": 4.5e-2, "loud": 2e-2, "onehot": 2e-2}   # sc3 floor 0.0150
ATTN_DV_TOL = 2e-2        # row_abs, rows = per-token 64-vectors, one group per (b, head)
ATTN_LSE_ATOL, ATTN_LSE_RTOL = 1e-3, 1e-5

# D -> (lanes LR, live chunks nc, MAXC template)
LN_DIMS = {16: (2, 1, 2), 48: (2, 3, 3), 96: (4, 3, 3), 384: (16, 3, 3), 2048: (64, 4, 4),
           40: (1, 5, 8), 1280: (32, 5, 8), 448: (8, 7, 8)}
LN_ROWS = (1, 37)
LN_REGIMES = ("std", "mean")
LN_MULTI_TRIP = (8200, 384)
LN_CELLS = [(r, d, g) for d in LN_DIMS for r in LN_ROWS for g in LN_REGIMES] + [
    (*LN_MULTI_TRIP, "std")]
LN_EPS = 1e-6
LN_Y_TOL = 1e-2           # row_rel on y and h
LN_DX_TOL = 1e-2          # row_abs on dx / dr
LN_PARAM_TOL = 1e-3       # max abs error of dgamma / dbeta over max |ref|

SOFTMAX_L = (1, 64, 65, 300, 512, 1024)
SOFTMAX_ROWS = 7          # not a multiple of the 4 rows per block
SOFTMAX_SCALE = 0.125
SOFTMAX_P_TOL = 1e-2      # row_rel on P; every row sums to 1 within the same
SOFTMAX_DS_TOL = 2e-2     # row_abs on dS

GELU_NUMEL = (8, 8 * 257, 64 * 3072)
GELU_Y_TOL = 1e-2         # rtol = atol, elementwise
GELU_DX_TOL = 2e-2


def ln_lanes(D):
    """(LR, nc) of csrc/transformer.hip for row length D."""
    nch, lr = D // 8, 64
    while lr > 1 and nch % lr:
        lr //= 2
    return lr, nch // lr


def softmax_inputs(L, seed=0):
    g = torch.Generator().manual_seed(seed * 101 + L)
    s = (torch.randn(SOFTMAX_ROWS, L, generator=g) * 30).to(torch.bfloat16)
    dp = torch.randn(SOFTMAX_ROWS, L, generator=g).to(torch.bfloat16)
    return s, dp


# ------------------------------------------------------------------ BatchNorm
# csrc/bn.hip works on [M, C] rows (M = N*H*W of a channels-last activation, or
# the rows of a BatchNorm1d input); the oracles take the logical [N, C, H, W] /
# [M, C] tensors and return results in the same shape.
BN_EPS = 1e-5


def _mc(t):
    """[N, C, H, W] or [M, C] -> fp64 [M, C]."""
    t = f64(t)
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) if t.dim() == 4 else t


def _unmc(t, like):
    if like.dim() == 4:
        N, C, H, W = like.shape
        return t.reshape(N, H, W, C).permute(0, 3, 1, 2)
    return t


def bn_ref(x, gamma, beta, eps=BN_EPS, residual=None, relu=False, training=True, running=None,
           dy=None, y_stored=None, dy_sums=None):
    """fp64 BatchNorm (+ residual) (+ ReLU) of bf16 inputs, forward and backward.

    Training: biased batch variance; ``rmean`` / ``rvar`` are the running
    statistics after an update with momentum 1 (the batch mean and the UNBIASED
    batch variance).  Eval (``training=False``): ``running = (mean, var)``
    normalises and the input gradient is dx = k1 * dz.

    The ReLU gradient mask is bf16(y) > 0 on the stored output (the rule
    documented in bn.hip): of ``y_stored`` when given (what the implementation
    under test wrote; an element whose pre-activation is 0 within rounding may
    legitimately land on either side), else of this reference's own y.

    ``dy_sums``: the gradient the two sums (dgamma, dbeta and the dx
    coefficients) are taken over when it is not ``dy`` itself (the fused stem
    reduces the unrounded pooled gradient and applies the bf16-rounded one).

    Returns a dict: y, pre (before the ReLU), mean, invstd, rmean, rvar and, with
    ``dy``, dx, dres (= dz), dgamma, dbeta and kdz = k1 * dz."""
    X = _mc(x)
    M, C = X.shape
    g, b = f64(gamma), f64(beta)
    if training:
        mean = X.mean(0)
        var = ((X - mean) ** 2).mean(0)
    else:
        mean, var = f64(running[0]), f64(running[1])
    inv = 1.0 / torch.sqrt(var + eps)
    xh = (X - mean) * inv
    pre = xh * g + b
    if residual is not None:
        pre = pre + _mc(residual)
    y = pre.clamp_min(0.0) if relu else pre
    out = dict(y=_unmc(y, x), pre=_unmc(pre, x), mean=mean, invstd=inv, rmean=mean,
               rvar=var * M / (M - 1) if M > 1 else var)
    if dy is None:
        return out
    dz, dzs = _mc(dy), _mc(dy if dy_sums is None else dy_sums)
    if relu:
        ys = bf(y) if y_stored is None else _mc(y_stored)
        dz = torch.where(ys > 0, dz, torch.zeros_like(dz))
        dzs = torch.where(ys > 0, dzs, torch.zeros_like(dzs))
    k1 = g * inv
    dbeta, dgamma = dzs.sum(0), (dzs * xh).sum(0)
    dx = k1 * (dz - dbeta / M - xh * dgamma / M) if training else k1 * dz
    out.update(dx=_unmc(dx, x), dres=_unmc(dz, x), dgamma=dgamma, dbeta=dbeta,
               kdz=_unmc(k1 * dz, x))
    return out


# Longest sequential fp32 run of the emulated sums.  No launch of csrc/bn.hip
# gives one thread more than 64 rows at the test cells (asserted by
# test_bn_edges_gpu.py::test_cells_are_the_ones_named); the partial sums of the
# runs are then added sequentially as well.  ``chunk=None`` is one run over all
# M rows: its error grows like sqrt(M) * ulp(sum) and reaches 9e-2 on invstd at
# M = 16820, |mean|/sigma = 64 -- three times that would bound nothing.
BN_EMUL_CHUNK = 64


def _seq_sum32(rows, chunk=None):
    """Sequential fp32 sum over the rows of a float32 [M, C] ndarray: one rounding
    per row and channel, the least accurate order a correct kernel could use.
    (An explicit loop: np.sum / torch.cumsum use pairwise or wider accumulation.)
    ``chunk``: sequential runs of that many rows, then a sequential sum of the
    runs' results."""
    assert rows.dtype == np.float32
    if chunk is not None and rows.shape[0] > chunk:
        M, C = rows.shape
        n = -(-M // chunk)
        pad = np.zeros((n * chunk, C), dtype=np.float32)     # + 0 is exact
        pad[:M] = rows
        acc = np.zeros((n, C), dtype=np.float32)
        for r in pad.reshape(n, chunk, C).transpose(1, 0, 2):
            acc = acc + r
        rows = acc
    acc = np.zeros(rows.shape[1], dtype=np.float32)
    for r in rows:
        acc = acc + r
    assert acc.dtype == np.float32
    return acc


def bn_emul(x, gamma, beta, eps=BN_EPS, residual=None, relu=False, training=True, running=None,
            dy=None, chunk=BN_EMUL_CHUNK, dy_sums=None):
    """bn_ref with the kernel's documented rounding points and nothing else:
    S = sum x and Q = sum x^2 in sequential fp32 (runs of ``chunk`` rows, see
    BN_EMUL_CHUNK; None = one run over all M rows), var = max(Q/M - mean^2, 0),
    folded scale / shift in fp32, y = bf16(relu(fma(x, scale, shift) + res));
    backward sums in sequential fp32, dx = bf16(A*dz + Cc*x + Bc) with fp32
    coefficients (Bc = Cc = 0 in eval mode), dres = dz.  Same dict as bn_ref."""
    f32 = np.float32
    X = _mc(x).numpy().astype(f32)            # bf16 values: exact
    M, C = X.shape
    g, b = f64(gamma).numpy().astype(f32), f64(beta).numpy().astype(f32)
    Mf, eps32 = f32(M), f32(eps)
    if training:
        mean = _seq_sum32(X, chunk) / Mf
        var = np.maximum(_seq_sum32(X * X, chunk) / Mf - mean * mean, f32(0))   # x*x exact in fp32
    else:
        mean = f64(running[0]).numpy().astype(f32)
        var = f64(running[1]).numpy().astype(f32)
    inv = (f32(1) / np.sqrt(var + eps32)).astype(f32)
    sc = g * inv
    sh = b - mean * sc
    pre = (X.astype(np.float64) * sc + sh).astype(f32)                    # one fma
    if residual is not None:
        pre = pre + _mc(residual).numpy().astype(f32)
    y32 = np.maximum(pre, f32(0)) if relu else pre
    assert y32.dtype == f32 and sc.dtype == f32 and sh.dtype == f32
    y = bf(torch.from_numpy(y32.astype(np.float64)))
    unb = var * Mf / f32(M - 1) if M > 1 else var
    t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    out = dict(y=_unmc(y, x), mean=t64(mean), invstd=t64(inv), rmean=t64(mean), rvar=t64(unb))
    if dy is None:
        return out
    dz = _mc(dy).numpy().astype(f32)
    dzs = dz if dy_sums is None else _mc(dy_sums).numpy().astype(f32)
    if relu:
        dz = np.where(y.numpy() > 0, dz, f32(0)).astype(f32)
        dzs = np.where(y.numpy() > 0, dzs, f32(0)).astype(f32)
    db = _seq_sum32(dzs, chunk)
    dg = _seq_sum32(dzs * (X - mean) * inv, chunk)
    k1 = g * inv
    if training:
        invM = f32(1) / Mf
        Cc = -k1 * inv * dg * invM
        Bc = -k1 * db * invM - Cc * mean
    else:
        Cc = Bc = np.zeros(C, dtype=f32)
    dx32 = k1 * dz + Cc * X + Bc
    assert dx32.dtype == f32 and dg.dtype == f32
    out.update(dx=_unmc(bf(t64(dx32)), x), dres=_unmc(t64(dz), x), dgamma=t64(dg), dbeta=t64(db))
    return out


BN_BASE_REGIMES = ("std", "off16", "off64", "tiny", "loud")
BN_REGIMES = BN_BASE_REGIMES + ("mixed", "const")
BN_EDGE_REGIMES = ("off256", "near1024")      # outside the asserted domain (recorded only)


def bn_inputs(N, C, H, W, regime, seed=0):
    """bf16 x, res, dy ([N, C, H, W], or [N, C] rows when H = W = 0), fp32 gamma,
    beta and running statistics (rm, rv) far from the batch's, on the CPU.

    Regimes: "std" randn*2 + 0.5; "off16" / "off64" / "off256" randn + offset
    (|mean|/sigma amplifies every error of the two sums); "tiny" randn*1e-3
    (variance below eps); "loud" randn*1e3 + 250; "mixed" the five base regimes
    interleaved channel by channel inside every 8-channel vector (a channel
    reading its neighbour's coefficients is off by orders of magnitude);
    "const" every second channel exactly 3.0 (zero variance); "near1024"
    bf16(randn + 1024), a nearly constant channel (the bf16 grid is 4 wide below
    1024 and 8 wide above).
    gamma is distinct per channel, negative on every 7th and exactly 0 on channel
    3; beta is distinct per channel."""
    g = torch.Generator().manual_seed(seed * 9973 + N * 131 + C * 7 + H * 3 + W)
    shape = (N, C, H, W) if H else (N, C)
    rn = lambda: torch.randn(*shape, generator=g)

    def draw(kind):
        z = rn()
        return {"std": z * 2 + 0.5, "off16": z + 16, "off64": z + 64, "off256": z + 256,
                "tiny": z * 1e-3, "loud": z * 1e3 + 250, "near1024": z + 1024}[kind]

    if regime == "mixed":
        x = torch.empty(shape)
        for i, kind in enumerate(BN_BASE_REGIMES):
            x[:, i::5] = draw(kind)[:, i::5]
    elif regime == "const":
        x = draw("std")
        x[:, 1::2] = 3.0
    else:
        x = draw(regime)
    res, dy = rn(), rn()
    gamma = 0.5 + torch.arange(C, dtype=torch.float32) / C
    gamma[::7] *= -1
    gamma[3] = 0.0
    beta = 0.5 * torch.randn(C, generator=g) + 1e-3 * torch.arange(C, dtype=torch.float32)
    rm = torch.randn(C, generator=g) * 3
    rv = torch.rand(C, generator=g) + 0.5
    if regime in ("off16", "off64", "off256", "near1024"):
        rm = rm + float(x.mean())             # far from the batch's, not absurdly so
    B = torch.bfloat16
    return dict(x=x.to(B), res=res.to(B), dy=dy.to(B), gamma=gamma, beta=beta, rm=rm, rv=rv)


def chan_rows(t):
    """[N, C, H, W] / [M, C] -> fp64 [C, 1, M]: every channel its own row_abs
    group, so one bad channel cannot hide in the others' norm."""
    return _mc(t).t().contiguous()[:, None, :]


def chan_rel(a, ref):
    """row_rel with channel = row ([C, M]); a channel whose reference is exactly
    zero (every element under the ReLU) must be exactly zero and is left out."""
    a2, r2 = chan_rows(a)[:, 0], chan_rows(ref)[:, 0]
    live = r2.norm(dim=-1) > 0
    assert bool((a2[~live] == 0).all()), "a channel with a zero reference is not exactly zero"
    return row_rel(a2[live], r2[live]) if bool(live.any()) else 0.0


def chan_abs(a, ref, den=None):
    """row_abs per channel: ||a_c - ref_c|| / ||ref_c|| (or / ||den_c|| with
    ``den`` a tensor of a's shape: BN's dx where the reference is a cancelled
    near-zero, e.g. M = 2 with xhat = +-1; den = k1 * dz bounds every term that
    cancels).  A channel whose denominator is exactly zero (gamma = 0, or a ReLU
    mask that is all zero) must be exactly zero in ``a`` and is left out."""
    a3, r3 = chan_rows(a), chan_rows(ref)
    dn = (r3 if den is None else chan_rows(den)).norm(dim=-1).reshape(-1)
    live = dn > 0
    assert bool((a3[~live] == 0).all()), "a channel with a zero reference is not exactly zero"
    if not bool(live.any()):
        return 0.0
    return row_abs(a3[live], r3[live], dn[live])


def param_err(a, ref):
    """(max abs error) / (max |ref|) of a per-channel vector (dgamma / dbeta)."""
    a, ref = f64(a), f64(ref)
    return float((a - ref).abs().max() / ref.abs().max())


def bn_stat_errs(mean, invstd, ref):
    """(mean error in units of sigma, relative invstd error), max over channels:
    |mean - mean_ref| * invstd_ref is what the mean's error does to xhat."""
    e_mean = float(((f64(mean) - ref["mean"]).abs() * ref["invstd"]).max())
    e_inv = float(((f64(invstd) - ref["invstd"]).abs() / ref["invstd"]).max())
    return e_mean, e_inv


def bn_running_errs(rm, rv, ref, eps=BN_EPS):
    """Running statistics after one update with momentum 1: the mean as in
    bn_stat_errs, the unbiased variance relative to (var + eps)."""
    e_mean = float(((f64(rm) - ref["rmean"]).abs() * ref["invstd"]).max())
    e_var = float(((f64(rv) - ref["rvar"]).abs() / (ref["rvar"] + eps)).max())
    return e_mean, e_var


def bn_mask_flip_err(y_stored, ref):
    """Elements whose stored-y ReLU mask differs from the fp64 mask may only be
    genuine near-zeros: returns max |pre| / rms(pre of the channel) over the
    flipped elements (0 without flips) and the number of flips."""
    ys, pre = _mc(y_stored), _mc(ref["pre"])
    flip = (ys > 0) != (bf(pre.clamp_min(0.0)) > 0)
    if not bool(flip.any()):
        return 0.0, 0
    scale = pre.pow(2).mean(0).sqrt().expand_as(pre)
    return float((pre[flip].abs() / scale[flip]).max()), int(flip.sum())


# ------------------------------------------------------------------- pooling
def maxpool_ref(x, k, s, p, relu_in=False, dy=None):
    """Max pool (floor mode) with the explicit first-maximum-in-scan-order rule:
    taps are visited (i, j) row-major and a tap wins only if strictly greater;
    padded taps never win.  Returns (y, tap, dx): tap = i*k + j as uint8, 255 for
    a window whose maximum is not positive under ``relu_in``; dx is the gather
    form (every input sums dy over the windows whose tap it is), fp64."""
    X = f64(x)
    N, C, H, W = X.shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    xp = F.pad(X, (p, p, p, p), value=float("-inf"))
    best = torch.full((N, C, Ho, Wo), float("-inf"), dtype=torch.float64)
    tap = torch.zeros((N, C, Ho, Wo), dtype=torch.int64)
    win = lambda t, i, j: t[:, :, i:i + s * (Ho - 1) + 1:s, j:j + s * (Wo - 1) + 1:s]
    for i in range(k):
        for j in range(k):
            v = win(xp, i, j)
            better = v > best
            best = torch.where(better, v, best)
            tap = torch.where(better, torch.full_like(tap, i * k + j), tap)
    if relu_in:
        tap = torch.where(best > 0, tap, torch.full_like(tap, 255))
    dx = None
    if dy is not None:
        dxp = torch.zeros_like(xp)
        for i in range(k):
            for j in range(k):
                win(dxp, i, j).add_(f64(dy) * (tap == i * k + j))
        dx = dxp[:, :, p:p + H, p:p + W]
    return best, tap.to(torch.uint8), dx


def maxpool_flat_index(tap, H, W, k, s, p):
    """The taps of maxpool_ref as F.max_pool2d's flat h*W + w input indices."""
    t = tap.to(torch.int64)
    Ho, Wo = t.shape[2:]
    ho = torch.arange(Ho).view(1, 1, Ho, 1)
    wo = torch.arange(Wo).view(1, 1, 1, Wo)
    return (ho * s - p + t // k) * W + (wo * s - p + t % k)


def gap_ref(x, dy=None):
    """fp64 global average pool [N, C, H, W] -> [N, C] and its gradient."""
    X = f64(x)
    y = X.mean(dim=(2, 3))
    dx = None if dy is None else (f64(dy) / (X.shape[2] * X.shape[3]))[:, :, None, None].expand_as(X)
    return y, dx


# HW = 1: three of the four waves idle; 29: crosses the 4-load trip (p + 12 < HW);
# C = 520: a second, partial 64-lane block of channel vectors
GAP_HW = {1: (1, 1), 3: (1, 3), 4: (2, 2), 5: (5, 1), 16: (4, 4), 17: (1, 17), 29: (29, 1),
          49: (7, 7)}
GAP_C = (8, 520, 2048)
GAP_OFFSETS = (0.0, 300.0)
GAP_Y_TOL = 1e-2      # row_rel, rows = samples
GAP_DX_TOL = 1e-2     # row_abs, rows = pixels


def gap_inputs(HW, C, offset, N=3):
    g = torch.Generator().manual_seed(HW * 1000 + C)
    H, W = GAP_HW[HW]
    x = (torch.randn(N, C, H, W, generator=g) + offset).to(torch.bfloat16)
    return x, torch.randn(N, C, generator=g).to(torch.bfloat16)


def gap_errors(y, dx, x, dy):
    y_ref, dx_ref = gap_ref(x, dy)
    return row_rel(y, y_ref), row_abs(_mc(dx), _mc(dx_ref))


def pool_int_inputs(shape, k, s, p, seed=0, lo=-1, hi=2):
    """Tie-heavy integer x in [lo, hi] and integer dy in [-2, 2] as bf16: every
    overlapping-window sum stays exact in bf16."""
    g = torch.Generator().manual_seed(seed * 577 + shape[1] * 13 + shape[2] * 5 + k)
    N, C, H, W = shape
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    x = torch.randint(lo, hi + 1, shape, generator=g).to(torch.bfloat16)
    dy = torch.randint(-2, 3, (N, C, Ho, Wo), generator=g).to(torch.bfloat16)
    return x, dy


# BatchNorm cells (tests/test_bn_edges_gpu.py): name -> (N, C, H, W)
BN_CELLS = {"min": (1, 8, 1, 2), "c24": (2, 24, 3, 5), "cs16": (2, 48, 5, 5),
            "cs32": (2, 96, 5, 5), "trip": (2, 64, 9, 9), "c1000": (2, 1000, 3, 3),
            "c1032": (2, 1032, 2, 3), "c2048": (3, 2048, 7, 7), "uneven": (2, 64, 23, 23),
            "wrap": (5, 64, 58, 58)}
BN_FULL_CELLS = ("trip", "c24", "c2048")       # every (relu, residual) x every regime
BN_SWEEP_REGIMES = ("std", "off64", "mixed")   # every cell, (relu, residual) = (T, F), (T, T)
BN_ACT = ((False, False), (True, False), (False, True), (True, True))
BN_UNFOLDED_CELLS = ("min", "c24", "trip", "c2048", "wrap")
BN_EVAL_CELLS = ("c24", "trip", "c2048")
BN_1D = ((30, 24), (162, 64))
BN_POOL_SHAPES = ((1, 64, 2, 1), (2, 64, 1, 7), (1, 128, 3, 2), (2, 64, 15, 17))
BN_POOL_REGIMES = ("std", "off16")


def bn_fold_cases():
    """(cell, regime, relu, residual) of the folded training path."""
    out = []
    for cell in BN_CELLS:
        for regime in BN_REGIMES:
            for relu, res in BN_ACT:
                full = cell in BN_FULL_CELLS
                sweep = regime in BN_SWEEP_REGIMES and relu
                if full or sweep:
                    out.append((cell, regime, relu, res))
    return out


def bn_unfolded_cases():
    return [(c, g, True, r) for c in BN_UNFOLDED_CELLS for g in ("std", "off64")
            for r in (False, True)]


def bn_errors(got, ref, M, relu, eps=BN_EPS):
    """Every error the BatchNorm tests bound, of whatever ``got`` holds (a dict
    with bn_ref's keys), against the fp64 ``ref``: the checker shared by the GPU
    tests and the CPU floors.  dx of an M <= 2 call is judged against ||k1*dz||
    (the reference itself is a cancelled near-zero there); "flip" is
    bn_mask_flip_err of the stored y."""
    e = {}
    if "y" in got:
        e["y"] = chan_rel(got["y"], ref["y"])
        e["flip"] = bn_mask_flip_err(got["y"], ref)[0] if relu else 0.0
    if "mean" in got:
        e["mean"], e["invstd"] = bn_stat_errs(got["mean"], got["invstd"], ref)
    if "rmean" in got:
        e["rmean"], e["rvar"] = bn_running_errs(got["rmean"], got["rvar"], ref, eps)
    if "dx" in got:
        e["dx"] = chan_abs(got["dx"], ref["dx"], ref["kdz"] if M <= 2 else None)
    if got.get("dres") is not None:
        e["dres"] = chan_abs(got["dres"], ref["dres"])
    for k in ("dgamma", "dbeta"):
        if k in got:
            e[k] = param_err(got[k], ref[k])
    return e


def bn_eval_cases():
    return [(c, g, relu, res) for c in BN_EVAL_CELLS for g in ("std", "off64")
            for relu, res in BN_ACT]


# Thresholds.  The starting values are LayerNorm's (LN_Y_TOL, LN_DX_TOL,
# LN_PARAM_TOL); the statistics start at the parameter tolerance: the mean's
# error in units of sigma, invstd and the unbiased running variance relative.
# "flip" bounds |pre| / rms(pre) of an element whose stored ReLU mask differs
# from the fp64 one.  A regime whose emulation floor (bn_emul, max over every
# cell, (relu, residual) pair and the two seeds the GPU file runs) is above a
# third of a starting value gets 3x the floor, rounded up to two digits; no value
# here comes from a kernel's output.
BN_TOL_START = dict(y=1e-2, flip=1e-2, dx=1e-2, dres=1e-2, dgamma=1e-3, dbeta=1e-3,
                    mean=1e-3, invstd=1e-3, rmean=1e-3, rvar=1e-3)
# y at M <= 18 is the max over ~1000 channels of the bf16 rounding of 12-18
# numbers (2^-8 at worst); eval-mode dx = bf16(k1 * dz) likewise
BN_STD_Y_TOL = 1.1e-2         # floor 3.654e-03 (c1032)
BN_STD_DX_TOL = 1.2e-2        # floor 3.695e-03 (c2048, eval mode)
BN_OFF16_Y_TOL = 1.1e-2       # floor 3.488e-03 (stem shape (1, 128, 3, 2), M = 6: as BN_STD_Y_TOL)
# |mean|/sigma = 64: ulp(Q) / (M var) = 2^-23 * 64^2 = 4.9e-4 per rounding of Q
BN_OFF64_Y_TOL = 3.3e-2       # floor 1.095e-02 (min: both rows equal, var = 0, invstd = 316:
                              #                  shift = beta - mean * scale rounds at ulp(2e4))
BN_OFF64_INVSTD_TOL = 3.9e-3  # floor 1.282e-03 (c1032)
BN_OFF64_RVAR_TOL = 7.7e-3    # floor 2.559e-03 (c1032)
BN_OFF64_DX_TOL = 1.3e-2      # floor 4.296e-03 (c1032)
BN_OFF64_DGAMMA_TOL = 2.0e-3  # floor 6.514e-04 (c1032)
# every fifth channel of "mixed" is an off64 channel
BN_MIXED_Y_TOL = 1.2e-2       # floor 3.698e-03 (wrap)
BN_MIXED_INVSTD_TOL = 3.7e-3  # floor 1.213e-03 (wrap)
BN_MIXED_RVAR_TOL = 7.3e-3    # floor 2.430e-03 (wrap)
BN_MIXED_DX_TOL = 1.1e-2      # floor 3.537e-03 (c1000)
BN_MIXED_DGAMMA_TOL = 3.3e-3  # floor 1.068e-03 (wrap)
# a constant channel: y = beta exactly, computed as fma(3, scale, beta - 3 * scale)
# with scale = gamma * 316; the error ulp(950 gamma) is measured against |beta|
BN_CONST_Y_TOL = 5.6e-2       # floor 1.863e-02 (c2048)
BN_TOL_RAISED = {
    "std": dict(y=BN_STD_Y_TOL, dx=BN_STD_DX_TOL),
    "off16": dict(y=BN_OFF16_Y_TOL),
    "off64": dict(y=BN_OFF64_Y_TOL, invstd=BN_OFF64_INVSTD_TOL, rvar=BN_OFF64_RVAR_TOL,
                  dx=BN_OFF64_DX_TOL, dgamma=BN_OFF64_DGAMMA_TOL),
    "mixed": dict(y=BN_MIXED_Y_TOL, invstd=BN_MIXED_INVSTD_TOL, rvar=BN_MIXED_RVAR_TOL,
                  dx=BN_MIXED_DX_TOL, dgamma=BN_MIXED_DGAMMA_TOL),
    "const": dict(y=BN_CONST_Y_TOL),
}


def bn_tol(regime):
    return {**BN_TOL_START, **BN_TOL_RAISED.get(regime, {})}


def bn_assert(errs, regime, margin=1.0, what=""):
    """Every error in ``errs`` (bn_errors) within its threshold / margin."""
    tol = bn_tol(regime)
    print(f"{what} {regime}: " + "  ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    bad = {k: (v, tol[k] / margin) for k, v in errs.items() if not v <= tol[k] / margin}
    assert not bad, f"{what} {regime}: (error, bound) {bad}"


def bn_pool_ref(d, y_stored, dp):
    """Reference of the fused BN + ReLU + max pool 3x3/s2/p1 stem, given the
    stored (bf16) BN output: the pooled y and taps (maxpool_ref with relu_in on
    the stored y), and the BN backward of the gathered dz: rounded to bf16 in the
    apply pass (the unfused dy was stored), unrounded in the pooled reduce.
    Returns (pooled y, taps, gathered dz, bn_ref dict)."""
    yp, tap, dz = maxpool_ref(y_stored, 3, 2, 1, relu_in=True, dy=dp)
    ref = bn_ref(d["x"], d["gamma"], d["beta"], relu=True, y_stored=y_stored, dy=bf(dz),
                 dy_sums=dz)
    return yp, tap, dz, ref


def bn_pool_dp(shape, seed=0):
    N, C, H, W = shape
    g = torch.Generator().manual_seed(seed * 31 + H * 7 + W)
    return torch.randn(N, C, (H - 1) // 2 + 1, (W - 1) // 2 + 1, generator=g).to(torch.bfloat16)
