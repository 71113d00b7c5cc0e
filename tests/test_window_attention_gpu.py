"""Shifted-window attention kernels (csrc/attention_window.hip) against an fp64
oracle written the way the paper's code reads: roll, partition, bias gather,
-100 mask, softmax, reverse.  Forward and backward bindings per cell, the
autograd Function against the bindings' bits, and the refusals."""
import pytest
import torch

import kernel_oracles as ko

# (ws, Hm, Wm, sh, heads, B)
CELLS = [(7, 14, 14, 3, 3, 2), (7, 7, 7, 0, 3, 2), (7, 14, 21, 3, 4, 1), (4, 8, 8, 2, 2, 2),
         (4, 4, 4, 0, 4, 2), (8, 16, 16, 4, 2, 1), (8, 8, 8, 0, 1, 3)]
REGIMES = {"sc1": 1.0, "sc3": 3.0}
# Emulation floors (window_ref(emul=True): bf16 P, bf16 dS, bf16 results; max over
# the cells, computed on the CPU by the first test below):
#   out    row_rel  sc1 0.0033  sc3 0.0031
#   dq/dk  row_abs  sc1 0.0041  sc3 0.0047      dv row_abs  0.0039 / 0.0029
#   dtable 0 (the sums take the unrounded dS; the kernel's are fp32)
# A threshold is the nominal one (out 1e-2, gradients 2e-2, kernel_oracles.py)
# unless 3x its floor is larger; no floor here reaches a third of its nominal.
OUT_TOL = 1e-2        # row_rel per (token, head); floor 0.0033
GRAD_TOL = 2e-2       # row_abs on dq / dk / dv, one group per (window, head); floor 0.0047
DTABLE_TOL = 2e-2     # max abs error per head over that head's largest reference entry


def inputs(ws, Hm, Wm, sh, heads, B, regime):
    g = torch.Generator().manual_seed(ws * 1000 + Hm * 10 + heads)
    qkv = (torch.randn(B, Hm, Wm, 3, heads, 32, generator=g) * REGIMES[regime]).bfloat16()
    dout = torch.randn(B, Hm, Wm, heads, 32, generator=g).bfloat16()
    return qkv, dout, torch.randn((2 * ws - 1) ** 2, heads, generator=g)


def partition(t, ws, sh):
    """[B, Hm, Wm, ...] -> rolled by -sh, [B * nW, ws * ws, ...]."""
    B, Hm, Wm = t.shape[:3]
    t = torch.roll(t, (-sh, -sh), (1, 2)).reshape(B, Hm // ws, ws, Wm // ws, ws, -1)
    return t.permute(0, 1, 3, 2, 4, 5).reshape(-1, ws * ws, t.shape[-1])


def logits(q, k, table, ws, Hm, Wm, sh, heads, B):
    c = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")).flatten(1)
    rel = c[:, :, None] - c[:, None, :] + ws - 1
    s = q @ k.transpose(-1, -2) * 32 ** -0.5 + table[rel[0] * (2 * ws - 1) + rel[1]].permute(2, 0, 1)
    if sh:
        img = torch.zeros(1, Hm, Wm, 1, dtype=s.dtype)
        for n, (ys, xs) in enumerate((y, x) for y in (slice(0, -ws), slice(-ws, -sh), slice(-sh, None))
                                     for x in (slice(0, -ws), slice(-ws, -sh), slice(-sh, None))):
            img[:, ys, xs] = n
        m = partition(img, ws, 0)[..., 0].repeat(B, 1)
        s = s + ((m[:, None, :] != m[:, :, None]) * -100.0)[:, None]
    return s


def heads_of(t, ws, sh, heads):
    """[B, Hm, Wm, heads * 32] -> fp64 [B * nW, heads, N, 32]."""
    return partition(t.to("cpu", torch.float64), ws, sh).unflatten(-1, (heads, 32)).transpose(1, 2)


def window_ref(qkv, dout, table, ws, Hm, Wm, sh, heads, B, emul=False):
    """(out, dqkv) as [B * nW, heads, N, 32] (dqkv stacked on dim 0) and dtable, in
    fp64; emul: with the kernels' rounding points (bf16 P, bf16 dS, bf16 results)."""
    q, k, v = (heads_of(qkv[:, :, :, i].flatten(3), ws, sh, heads) for i in range(3))
    do, tab = heads_of(dout.flatten(3), ws, sh, heads), ko.f64(table)
    r = ko.bf if emul else (lambda t: t)
    s = logits(q, k, tab, ws, Hm, Wm, sh, heads, B)
    e = torch.exp(s - s.amax(-1, keepdim=True))
    p = e / e.sum(-1, keepdim=True)
    out = r((r(e) @ v) / e.sum(-1, keepdim=True))
    dp = do @ v.transpose(-1, -2)
    ds = p * (dp - (p * dp).sum(-1, keepdim=True))
    dqkv = torch.stack([r(r(ds) @ k * 32 ** -0.5), r(r(ds).transpose(-1, -2) @ q * 32 ** -0.5),
                        r(r(p).transpose(-1, -2) @ do)])
    c = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")).flatten(1)
    rel = c[:, :, None] - c[:, None, :] + ws - 1
    dtable = torch.zeros_like(tab).index_add_(
        0, (rel[0] * (2 * ws - 1) + rel[1]).reshape(-1), ds.sum(0).permute(1, 2, 0).flatten(0, 1))
    return out, dqkv, dtable


def errors(out, dqkv, dtable, ref, ws, sh, heads):
    """row_rel of out, row_abs of dq / dk / dv, the worst head of dtable."""
    ro, rg, rt = ref
    eo = ko.row_rel(out.reshape(-1, 32), ro.reshape(-1, 32))
    eg = [ko.row_abs(dqkv[i].flatten(0, 1), rg[i].flatten(0, 1)) for i in range(3)]
    et = float(((ko.f64(dtable) - rt).abs().amax(0) / rt.abs().amax(0)).max())
    return eo, eg, et


def test_oracle_matches_autograd_and_emulation_floor():
    """The closed-form fp64 backward above is autograd's, and the emulation passes
    every cell at a third of the thresholds."""
    ws, Hm, Wm, sh, heads, B = CELLS[0]
    qkv, dout, table = inputs(*CELLS[0], "sc1")
    x, t = ko.f64(qkv).requires_grad_(), ko.f64(table).requires_grad_()
    q, k, v = (heads_of(x[:, :, :, i].flatten(3), ws, sh, heads) for i in range(3))
    o = torch.softmax(logits(q, k, t, ws, Hm, Wm, sh, heads, B), -1) @ v
    o.backward(heads_of(dout.flatten(3), ws, sh, heads))
    ref = window_ref(qkv, dout, table, ws, Hm, Wm, sh, heads, B)
    gx = torch.stack([heads_of(x.grad[:, :, :, i].flatten(3), ws, sh, heads) for i in range(3)])
    torch.testing.assert_close(ref[0], o.detach())
    torch.testing.assert_close(ref[1], gx)
    torch.testing.assert_close(ref[2], t.grad)
    for cell in CELLS:
        for regime in REGIMES:
            a = inputs(*cell, regime)
            eo, eg, et = errors(*window_ref(*a, *cell, emul=True), window_ref(*a, *cell), cell[0],
                                cell[3], cell[4])
            print(cell, regime, f"out {eo:.4f} dq {eg[0]:.4f} dk {eg[1]:.4f} dv {eg[2]:.4f} "
                                f"dtable {et:.1e}")
            assert eo < OUT_TOL / 3 and max(eg) < GRAD_TOL / 3 and et < DTABLE_TOL / 3


@pytest.mark.gpu
@pytest.mark.parametrize("regime", list(REGIMES))
@pytest.mark.parametrize("cell", CELLS, ids=lambda c: "ws{}_{}x{}_sh{}_h{}_b{}".format(*c))
def test_bindings_match_fp64_oracle(cell, regime):
    from distributed_ml_pytorch_amd.ops._ext import native

    ws, Hm, Wm, sh, heads, B = cell
    qkv, dout, table = inputs(*cell, regime)
    ref = window_ref(qkv, dout, table, ws, Hm, Wm, sh, heads, B)
    dev = lambda t: t.flatten(3).cuda()
    out = native().window_attention_fwd(dev(qkv), table.cuda(), heads, ws, sh)
    runs = []
    for _ in range(2):
        dtable = torch.zeros_like(table).cuda()
        runs.append((native().window_attention_bwd(dev(qkv), dev(dout), table.cuda(), dtable,
                                                   heads, ws, sh), dtable))
    (dqkv, dtable), (dqkv2, dtable2) = runs
    assert torch.equal(dqkv, dqkv2) and torch.equal(dtable, dtable2)
    assert all(bool(torch.isfinite(t).all()) for t in (out, dqkv, dtable))
    g = dqkv.cpu().view(B, Hm, Wm, 3, heads * 32)
    eo, eg, et = errors(heads_of(out.cpu(), ws, sh, heads),
                        [heads_of(g[:, :, :, i], ws, sh, heads) for i in range(3)], dtable.cpu(),
                        ref, ws, sh, heads)
    print(f"out {eo:.4f} dq {eg[0]:.4f} dk {eg[1]:.4f} dv {eg[2]:.4f} dtable {et:.1e}")
    assert eo < OUT_TOL and max(eg) < GRAD_TOL and et < DTABLE_TOL


@pytest.mark.gpu
def test_autograd_gives_the_bindings_bits():
    from distributed_ml_pytorch_amd.ops import functional as DF
    from distributed_ml_pytorch_amd.ops._ext import native

    ws, Hm, Wm, sh, heads, B = CELLS[0]
    qkv, dout, table = inputs(*CELLS[0], "sc1")
    x, t = qkv.flatten(3).cuda().requires_grad_(), table.cuda().requires_grad_()
    d = dout.flatten(3).cuda()
    assert DF.window_attention_supported(x, heads, ws, sh, t)
    out = DF.window_attention(x, heads, ws, sh, t)
    out.backward(d)
    dtable = torch.zeros_like(t)
    dqkv = native().window_attention_bwd(x.detach(), d, t.detach(), dtable, heads, ws, sh)
    assert torch.equal(out, native().window_attention_fwd(x.detach(), t.detach(), heads, ws, sh))
    assert torch.equal(x.grad, dqkv) and torch.equal(t.grad, dtable)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,dtype,heads,ws,sh", [
    ((1, 9, 9, 96), torch.bfloat16, 1, 9, 0),        # N = 81 > 64
    ((1, 10, 14, 96), torch.bfloat16, 1, 7, 0),      # map not divisible by the window
    ((1, 7, 7, 96), torch.bfloat16, 1, 7, 7),        # sh >= ws
    ((1, 7, 7, 192), torch.bfloat16, 1, 7, 0),       # head dim 64
    ((1, 7, 7, 96), torch.float32, 1, 7, 0),         # fp32 input
], ids=["N81", "indivisible", "shift", "dim64", "fp32"])
def test_bindings_refuse(shape, dtype, heads, ws, sh):
    from distributed_ml_pytorch_amd.ops import functional as DF
    from distributed_ml_pytorch_amd.ops._ext import native

    qkv = torch.zeros(shape, dtype=dtype, device="cuda")
    table = torch.zeros((2 * ws - 1) ** 2, heads, device="cuda")
    assert not DF.window_attention_supported(qkv, heads, ws, sh, table)
    with pytest.raises(RuntimeError):
        native().window_attention_fwd(qkv, table, heads, ws, sh)
    with pytest.raises(RuntimeError):
        native().window_attention_bwd(qkv, torch.zeros_like(qkv[..., :shape[-1] // 3]), table,
                                      None, heads, ws, sh)
