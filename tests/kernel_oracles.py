"""fp64 oracles, row-wise error checkers, a NumPy Philox4x32-10 and precision-model
emulations for the ViT / loss / dropout kernels (csrc/attention.hip,
transformer.hip, xent.hip, dropout.hip).  Shared by test_kernel_oracles_cpu.py
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
