"""Precision model, input regimes, cells and checkers of the streaming attention
kernels (csrc/attention_stream.hip), on top of kernel_oracles.py.  Shared by
test_attention_stream_cpu.py and test_attention_stream_gpu.py (not a test module
itself); everything here runs on the CPU.

The fp64 references are kernel_oracles' (attention_ref / attention_bwd_ref) and
so are the thresholds: the CPU file shows that the streaming precision model
passes every GPU cell at one third of them.  The backward model is
ko.attention_bwd_emul unchanged: both routes recompute P from lse2.
"""
import functools

import torch

import kernel_oracles as ko

KT = 128                  # keys per staged tile (csrc/attn_plan.h kAttnStreamTile)

# N: the first streamed size (one key in the last tile, one query in the last
# block), the strip tail and the 32-row padding, both sides of each multiple of
# the 128-token tile / block, more than five tiles
STREAM_N = (257, 272, 383, 384, 385, 511, 512, 513, 577, 785, 1025)
# "loud_first": the loud regime flipped along the tokens.  The loud token is then
# token 0, so the running max is set in the first tile and every later tile
# contributes ~0, where the stock regime puts the jump in the last tile.
STREAM_REGIMES = ("sc1", "sc3", "loud", "loud_first", "onehot")
STREAM_CELLS = [(2, n, 2, r) for n in STREAM_N for r in STREAM_REGIMES] + [
    (3, 577, 12, "sc1"), (3, 577, 12, "sc3")]       # ViT-B/16 at 384^2: bh -> (b, h)
STREAM_CAP_CELL = (1, 4096, 1, "sc1")               # forward only
ROUTE_N = (1, 17, 197, 256)                         # sizes both routes take
ROUTE_CELLS = [(2, n, 2, r) for n in ROUTE_N for r in ko.ATTN_REGIMES]

# Emulation floors of stream_fwd_emul / ko.attention_bwd_emul against the fp64
# references (max over STREAM_CELLS, the cap cell and three input seeds, per-token
# rows; test_attention_stream_cpu.py asserts them at one third of each threshold):
#   out   row_rel  sc1 0.00363  sc3 0.00359  loud 0.00450 (N = 513, seed 1)
#                  loud_first 0.00428  onehot 0.00183
#   dq/dk row_abs  sc1 0.00445  sc3 0.01044  loud / loud_first 0.00111  onehot 0.00014
#   dv    row_abs  <= 0.00360 everywhere
#   lse2  max abs  1.4e-14
# The gradient and lse2 floors sit under one third of kernel_oracles' thresholds
# (ATTN_DQK_TOL, ATTN_DV_TOL, ATTN_LSE_*), which hold unchanged.  The out floor
# does not (0.00450 > ATTN_OUT_TOL / 3 = 0.00433: the bf16 rounding of P against
# a loud row, one more rescale per tile), so by kernel_oracles' rule the
# threshold is 3x the floor:
STREAM_OUT_TOL = 1.36e-2    # row_rel, per (b, token, head); floor 0.00450
assert STREAM_OUT_TOL >= ko.ATTN_OUT_TOL


def base_regime(regime):
    """loud_first is judged like loud (thresholds, attention_cancels)."""
    return "loud" if regime == "loud_first" else regime


@functools.lru_cache(maxsize=None)
def stream_inputs(B, N, H, regime, seed=0):
    """bf16 (qkv, dout) on the CPU; cached, callers must not write to them."""
    qkv, dout = ko.attention_inputs(B, N, H, base_regime(regime), seed)
    if regime == "loud_first":
        qkv, dout = qkv.flip(1).contiguous(), dout.flip(1).contiguous()
    return qkv, dout


@functools.lru_cache(maxsize=None)
def fwd_ref(B, N, H, regime, seed=0):
    return ko.attention_ref(stream_inputs(B, N, H, regime, seed)[0], H)


@functools.lru_cache(maxsize=None)
def bwd_ref(B, N, H, regime, seed=0):
    qkv, dout = stream_inputs(B, N, H, regime, seed)
    return ko.attention_bwd_ref(qkv, dout, H)


def stream_fwd_emul(qkv, H, kt=KT):
    """Streaming forward precision model: per key tile P = exp(s - m_new) is
    rounded to bf16 relative to the running max INCLUDING that tile before P.V,
    the running sum l (unrounded P) and the accumulated O are rescaled by
    exp(m_old - m_new), the output O / l is bf16."""
    q, k, v = ko.split_qkv(qkv, H)
    s = q @ k.transpose(-1, -2) * 0.125
    N = s.shape[-1]
    m = torch.full(s.shape[:-1] + (1,), -float("inf"), dtype=s.dtype)
    l = torch.zeros_like(m)
    o = torch.zeros_like(q)
    for t in range(0, N, kt):
        st = s[..., t:t + kt]
        m_new = torch.maximum(m, st.amax(dim=-1, keepdim=True))
        f = torch.exp(m - m_new)
        p = torch.exp(st - m_new)
        l = l * f + p.sum(dim=-1, keepdim=True)
        o = o * f + ko.bf(p) @ v[..., t:t + kt, :]
        m = m_new
    out = ko.bf(o / l)
    lse2 = (m + torch.log(l)).squeeze(-1) / ko.LN2
    return ko.merge_heads(out), lse2


# ------------------------------------------------------------------- checkers
def fwd_errors(out, lse2, B, N, H, regime, seed=0):
    """(out row_rel per (b, token, head), lse2 max abs error) against the fp64
    reference; shapes and finiteness asserted."""
    out_ref, lse_ref = fwd_ref(B, N, H, regime, seed)
    assert out.shape == (B, N, H * 64) and lse2.shape == (B, H, N)
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(lse2).all())
    e_out = ko.row_rel(out.view(B, N, H, 64), out_ref.view(B, N, H, 64))
    e_lse = float((ko.f64(lse2) - lse_ref).abs().max())
    return e_out, e_lse


def check_fwd(out, lse2, B, N, H, regime, margin=1.0, seed=0, out_tol=STREAM_OUT_TOL):
    """The _check_fwd of test_attention_edges_gpu.py: per-token rows, lse2 included.
    ROUTE_CELLS pass out_tol=ko.ATTN_OUT_TOL: the resident route's own check."""
    e_out, e_lse = fwd_errors(out, lse2, B, N, H, regime, seed)
    print(f"out row_rel {e_out:.5f}  lse2 max abs err {e_lse:.2e}")
    assert e_out <= out_tol * margin, e_out
    torch.testing.assert_close(ko.f64(lse2), fwd_ref(B, N, H, regime, seed)[1],
                               atol=ko.ATTN_LSE_ATOL * margin, rtol=ko.ATTN_LSE_RTOL * margin)


def bwd_errors(dqkv, B, N, H, regime, seed=0):
    qkv, dout = stream_inputs(B, N, H, regime, seed)
    assert dqkv.shape == qkv.shape and bool(torch.isfinite(dqkv.float()).all())
    return ko.attention_grad_errors(dqkv, bwd_ref(B, N, H, regime, seed), qkv, dout, H,
                                    base_regime(regime))


def check_bwd(dqkv, B, N, H, regime, margin=1.0, seed=0):
    """The _check_bwd of test_attention_edges_gpu.py."""
    eq, ek, ev = bwd_errors(dqkv, B, N, H, regime, seed)
    print(f"row_abs dq {eq:.5f} dk {ek:.5f} dv {ev:.5f}")
    tol = ko.ATTN_DQK_TOL[base_regime(regime)] * margin
    assert eq <= tol, eq
    assert ek <= tol, ek
    assert ev <= ko.ATTN_DV_TOL * margin, ev
