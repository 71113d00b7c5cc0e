"""csrc/attention.hip at its shape and dynamic-range edges, against the fp64
oracle of kernel_oracles.py, judged per token row (a whole-tensor norm hides one
wrong row or strip tail) and including lse2, which the backward trusts.

Shapes: the 16-token strip tail (N % 16), the 32-row LDS padding, one wave
handling two strips (N > 128), N = 1; NW = 8 waves throughout.  Regimes: sc = 1,
sc = 3 (peaky: exp2 arguments far below -126), a loud last token (the padding
rows of the staged images repeat it, so a leak through a ``< N`` mask shows) and
one dominant key per query (exact one-hot P, p * (dp - di) at p = 1).

Left out on purpose: a large common offset on K in the backward.  At K + 6 the
emulation of a correct kernel is itself 1.7-2.2 % off in dq (bf16 dS breaks the
cancellation in sum_j dS_j): inherent to the algorithm, not a kernel fault.
Thresholds and their emulation floors: kernel_oracles.py / test_kernel_oracles_cpu.py."""
import pytest
import torch

import kernel_oracles as ko

pytestmark = pytest.mark.gpu


def _nat():
    from distributed_ml_pytorch_amd.ops._ext import native

    return native()


def _check_fwd(out, lse2, qkv, H):
    B, N, _ = qkv.shape
    out_ref, lse_ref = ko.attention_ref(qkv, H)
    assert out.shape == (B, N, H * 64) and lse2.shape == (B, H, N)
    assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(lse2).all())
    e_out = ko.row_rel(out.view(B, N, H, 64), out_ref.view(B, N, H, 64))
    e_lse = float((ko.f64(lse2) - lse_ref).abs().max())
    print(f"out row_rel {e_out:.5f}  lse2 max abs err {e_lse:.2e}")
    assert e_out <= ko.ATTN_OUT_TOL, e_out
    torch.testing.assert_close(ko.f64(lse2), lse_ref, atol=ko.ATTN_LSE_ATOL,
                               rtol=ko.ATTN_LSE_RTOL)
    return out_ref


def _check_bwd(dqkv, qkv, dout, H, regime):
    assert dqkv.shape == qkv.shape and bool(torch.isfinite(dqkv.float()).all())
    dref = ko.attention_bwd_ref(qkv, dout, H)
    eq, ek, ev = ko.attention_grad_errors(dqkv, dref, qkv, dout, H, regime)
    print(f"row_abs dq {eq:.5f} dk {ek:.5f} dv {ev:.5f}")
    assert eq <= ko.ATTN_DQK_TOL[regime], eq
    assert ek <= ko.ATTN_DQK_TOL[regime], ek
    assert ev <= ko.ATTN_DV_TOL, ev


@pytest.mark.parametrize("B,N,H,regime", ko.ATTN_CELLS)
def test_attention_edges(B, N, H, regime):
    nat = _nat()
    qkv, dout = ko.attention_inputs(B, N, H, regime)
    q_d, do_d = qkv.cuda(), dout.cuda()
    out, lse2 = nat.attention_fwd(q_d, H)
    out_ref = _check_fwd(out, lse2, qkv, H)
    dqkv = nat.attention_bwd(q_d, out, do_d, lse2, H)
    _check_bwd(dqkv, qkv, dout, H, regime)
    if N > 1:
        # batches and heads carry different data: bh -> (b, h) indexing
        o = out_ref.view(B, N, H, 64)
        assert ko.row_rel(o.flip(0), o) > 0.5 and ko.row_rel(o.flip(2), o) > 0.5


@pytest.mark.parametrize("N", [17, 241])
def test_attention_bwd_noncontiguous_dout(N):
    """A transposed view as dout gives the bits of its contiguous copy."""
    nat = _nat()
    B, H = 2, 2
    qkv, dout = ko.attention_inputs(B, N, H, "sc1")
    q_d = qkv.cuda()
    out, lse2 = nat.attention_fwd(q_d, H)
    view = dout.cuda().transpose(0, 1).contiguous().transpose(0, 1)   # [B, N, D], strides of [N, B, D]
    assert not view.is_contiguous() and torch.equal(view, dout.cuda())
    a = nat.attention_bwd(q_d, out, view, lse2, H)
    b = nat.attention_bwd(q_d, out, view.contiguous(), lse2, H)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    _check_bwd(a, qkv, dout, H, "sc1")


@pytest.mark.parametrize("N,regime", [(33, "sc3"), (241, "loud")])
def test_attention_qkv_autograd(N, regime):
    """One autograd pass through attention_qkv: the same numbers as the bindings."""
    from distributed_ml_pytorch_amd.ops.functional import attention_qkv, fused_attention_supported

    B, H = 2, 2
    qkv, dout = ko.attention_inputs(B, N, H, regime)
    x = qkv.cuda().requires_grad_(True)
    assert fused_attention_supported(x, H)
    out = attention_qkv(x, H)
    out.backward(dout.cuda())
    out_ref, _ = ko.attention_ref(qkv, H)
    assert ko.row_rel(out.view(B, N, H, 64), out_ref.view(B, N, H, 64)) <= ko.ATTN_OUT_TOL
    _check_bwd(x.grad, qkv, dout, H, regime)
