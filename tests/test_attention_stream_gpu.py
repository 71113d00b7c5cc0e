"""csrc/attention_stream.hip, the streaming attention route (257 .. 4096 tokens),
through the bindings, autograd and a training step, against the fp64 oracle of
kernel_oracles.py with the cells, regimes and thresholds of
attention_stream_oracle.py (floors: test_attention_stream_cpu.py).  Judged per
token row, lse2 included, like test_attention_edges_gpu.py.

Shapes: the first streamed size (257: one key in the last tile, one query in the
last block), the 16-token strip tail, the 32-row padding, both sides of every
multiple of the 128-token tile / block, more than five tiles, the ViT-B/16-at-384
head count, and the 4096-token cap (forward).  Regimes: kernel_oracles' four plus
loud_first (the running max set in the first tile)."""
import pytest
import torch

import attention_stream_oracle as so
import kernel_oracles as ko

pytestmark = pytest.mark.gpu

RESIDENT, STREAM = 0, 1


def _nat():
    from distributed_ml_pytorch_amd.ops._ext import native

    return native()


def _run(B, N, H, regime, fwd_route=-1, bwd_route=-1):
    nat = _nat()
    qkv, dout = so.stream_inputs(B, N, H, regime)
    q_d, do_d = qkv.cuda(), dout.cuda()
    out, lse2 = nat.attention_fwd(q_d, H, fwd_route)
    dqkv = nat.attention_bwd(q_d, out, do_d, lse2, H, bwd_route)
    return out, lse2, dqkv


@pytest.mark.parametrize("B,N,H,regime", so.STREAM_CELLS)
def test_stream_edges(B, N, H, regime):
    out, lse2, dqkv = _run(B, N, H, regime)
    so.check_fwd(out, lse2, B, N, H, regime)
    so.check_bwd(dqkv, B, N, H, regime)
    # batches and heads carry different data: bh -> (b, h) indexing
    o = so.fwd_ref(B, N, H, regime)[0].view(B, N, H, 64)
    assert ko.row_rel(o.flip(0), o) > 0.5 and ko.row_rel(o.flip(2), o) > 0.5


def test_stream_forward_at_the_cap():
    B, N, H, regime = so.STREAM_CAP_CELL
    qkv, _ = so.stream_inputs(B, N, H, regime)
    out, lse2 = _nat().attention_fwd(qkv.cuda(), H)
    so.check_fwd(out, lse2, B, N, H, regime)


@pytest.mark.parametrize("B,N,H,regime", so.ROUTE_CELLS)
def test_routes_agree(B, N, H, regime):
    """At the sizes both routes take, the streaming route passes the resident
    route's checks, and either route's backward takes the other's out / lse2."""
    for fwd_route, bwd_route in ((STREAM, STREAM), (RESIDENT, STREAM), (STREAM, RESIDENT)):
        out, lse2, dqkv = _run(B, N, H, regime, fwd_route, bwd_route)
        so.check_fwd(out, lse2, B, N, H, regime, out_tol=ko.ATTN_OUT_TOL)
        so.check_bwd(dqkv, B, N, H, regime)
    # the automatic route is the resident one here, bit for bit
    auto, forced = _run(B, N, H, regime), _run(B, N, H, regime, RESIDENT, RESIDENT)
    assert torch.equal(auto[0].view(torch.int16), forced[0].view(torch.int16))
    assert torch.equal(auto[2].view(torch.int16), forced[2].view(torch.int16))


def test_stream_is_deterministic():
    a, b = _run(2, 577, 2, "sc1"), _run(2, 577, 2, "sc1")
    assert torch.equal(a[0].view(torch.int16), b[0].view(torch.int16))
    assert torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert torch.equal(a[2].view(torch.int16), b[2].view(torch.int16))


def test_stream_bwd_noncontiguous_dout():
    """A transposed view as dout gives the bits of its contiguous copy."""
    nat = _nat()
    B, N, H = 2, 385, 2
    qkv, dout = so.stream_inputs(B, N, H, "sc1")
    q_d = qkv.cuda()
    out, lse2 = nat.attention_fwd(q_d, H)
    view = dout.cuda().transpose(0, 1).contiguous().transpose(0, 1)   # [B, N, D], strides of [N, B, D]
    assert not view.is_contiguous() and torch.equal(view, dout.cuda())
    a = nat.attention_bwd(q_d, out, view, lse2, H)
    b = nat.attention_bwd(q_d, out, view.contiguous(), lse2, H)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))
    so.check_bwd(a, B, N, H, "sc1")


@pytest.mark.parametrize("N,regime", [(401, "sc3"), (577, "loud_first")])
def test_stream_attention_qkv_autograd(N, regime):
    """One autograd pass through attention_qkv: the bindings' numbers."""
    from distributed_ml_pytorch_amd.ops.functional import attention_qkv, fused_attention_supported

    B, H = 2, 2
    qkv, dout = so.stream_inputs(B, N, H, regime)
    x = qkv.cuda().requires_grad_(True)
    assert fused_attention_supported(x, H)
    out = attention_qkv(x, H)
    out.backward(dout.cuda())
    ref_out, ref_lse, ref_dqkv = _run(B, N, H, regime)
    assert torch.equal(out.detach().view(torch.int16), ref_out.view(torch.int16))
    assert torch.equal(x.grad.view(torch.int16), ref_dqkv.view(torch.int16))
    so.check_fwd(out.detach(), ref_lse, B, N, H, regime)
    so.check_bwd(x.grad, B, N, H, regime)


def test_stream_env_switch_forces_the_route(monkeypatch):
    """DMP_ATTN_STREAM=1 sends attention_qkv to the streaming kernels at 197 tokens."""
    from distributed_ml_pytorch_amd.ops.functional import attention_qkv

    B, N, H = 2, 197, 2
    qkv, _ = so.stream_inputs(B, N, H, "sc1")
    monkeypatch.setenv("DMP_ATTN_STREAM", "1")
    with torch.no_grad():
        got = attention_qkv(qkv.cuda(), H)
    want, _ = _nat().attention_fwd(qkv.cuda(), H, STREAM)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))


def test_stream_rejections():
    nat = _nat()
    z = lambda n: torch.zeros(1, n, 3 * 64, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="N <= 4096"):
        nat.attention_fwd(z(4097), 1)
    with pytest.raises(RuntimeError, match="resident"):
        nat.attention_fwd(z(257), 1, RESIDENT)
    with pytest.raises(RuntimeError, match="route"):
        nat.attention_fwd(z(197), 1, 2)
    out, lse2 = nat.attention_fwd(z(257), 1)
    with pytest.raises(RuntimeError, match="resident"):
        nat.attention_bwd(z(257), out, out, lse2, 1, RESIDENT)
    with pytest.raises(RuntimeError, match="route"):
        nat.attention_bwd(z(257), out, out, lse2, 1, 2)


# ------------------------------------------------------------------ the model
def _worker(dtype):
    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, Worker

    cfg = TrainConfig(model="vit_mini_long", batch_size=4, mode="asgd", ps="local", n_push=1,
                      n_pull=1, lr=0.01, evaluate=False, verbose=False, dtype=dtype, seed=5)
    return Worker(cfg, DistInfo(device=torch.device("cuda", 0)))


def _batch(w, n=4):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(n, *w.input_shape, generator=g)
    y = torch.randint(0, w.num_classes, (n,), generator=g)
    return w.prepare(x, y)


def test_vit_mini_long_step_is_native():
    """Two training steps of the 401-token model outside the oracle mode: no
    NativeCoverageError, a finite loss that does not grow, and every device
    kernel of the second step ours (the input copies aside)."""
    from torch.profiler import ProfilerActivity, profile

    from distributed_ml_pytorch_amd.ops._policy import stock_allowed

    with stock_allowed(False):
        w = _worker("bf16")
        x, y = _batch(w)
        loss1, _ = w.train_step(x, y)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            loss2, _ = w.train_step(x, y)
            torch.cuda.synchronize()
        w.finish()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert names, "profiler recorded no device work"
    is_copy = lambda n: n.startswith(("__amd_rocclr_copyBuffer", "Memcpy", "memcpy"))
    foreign = sorted({n for n in names if "dmp::" not in n and not is_copy(n)})
    assert not foreign, f"non-native device kernels in a vit_mini_long step: {foreign}"
    for k in ("attn_stream_fwd_kernel", "attn_stream_dq_kernel", "attn_stream_dkv_kernel"):
        assert any(k in n for n in names), (k, sorted(set(names)))
    l1, l2 = float(loss1.float().item()), float(loss2.float().item())
    print(f"loss {l1:.5f} -> {l2:.5f}")
    assert l1 == l1 and l2 == l2 and 0 < l2 <= l1, (l1, l2)


def test_vit_mini_long_gradients_match_fp32():
    """One backward on the native bf16 path (streaming attention) against the same
    weights on PyTorch's fp32 kernels (the oracle mode), as
    test_vit_native_gradients_match_fp32: every parameter's gradient within 5e-2."""
    from distributed_ml_pytorch_amd.ops._policy import stock_allowed
    from distributed_ml_pytorch_amd.ops.functional import softmax_cross_entropy

    grads = {}
    for dt in ("fp32", "bf16"):
        with stock_allowed(dt == "fp32"):
            w = _worker(dt)
            x, y = _batch(w)
            w.opt.zero_grad()
            loss, _ = softmax_cross_entropy(w.model(x), y)
            loss.backward()
            torch.cuda.synchronize()
            grads[dt] = {n: p.grad.detach().float().clone() for n, p in w.model.named_parameters()}
    rel = {n: float((grads["bf16"][n] - ref).norm() / (ref.norm() + 1e-12))
           for n, ref in grads["fp32"].items()}
    print("worst", max(rel.items(), key=lambda kv: kv[1]))
    bad = {n: r for n, r in rel.items() if r > 5e-2}
    assert not bad, bad
