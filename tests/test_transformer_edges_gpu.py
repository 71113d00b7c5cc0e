"""csrc/transformer.hip against the fp64 oracles of kernel_oracles.py, row by row.

LayerNorm / add-LayerNorm: every lane width LR in {1, 2, 4, 8, 16, 32, 64}
and every chunk template (MAXC = 2, 3, 4, and 8 with 5 and 7 live chunks, where
``c < nc`` masks the rest), rows in {1, 37}, one multi-trip case over the 512
block cap, a large-mean regime a one-pass variance would fail, and the
gamma / beta / slots / dh variants.  Row softmax incl. MAXE = 8, tanh-GELU over
a grid with the saturating ends, token_row_scatter and vit_embed bit checks.
Thresholds and their emulation floors: kernel_oracles.py / test_kernel_oracles_cpu.py."""
import pytest
import torch

import kernel_oracles as ko

pytestmark = pytest.mark.gpu


def _nat():
    from distributed_ml_pytorch_amd.ops._ext import native

    return native()


def _param_err(a, ref):
    return float((ko.f64(a) - ref).abs().max() / ref.abs().max())


# ------------------------------------------------------------------ LayerNorm
@pytest.mark.parametrize("rows,D,regime", ko.LN_CELLS)
def test_layernorm_edges(rows, D, regime):
    """Plain and fused-add LayerNorm fwd/bwd through the bindings, dgamma / dbeta
    accumulated into non-zero buffers through persistent slots, twice."""
    from distributed_ml_pytorch_amd.ops.functional import LN_SLOTS, layernorm_supported

    nat = _nat()
    assert layernorm_supported(D) and ko.ln_lanes(D) == ko.LN_DIMS[D][:2]
    x, r, dy, dh, gamma, beta = ko.layernorm_inputs(rows, D, regime)
    xd, rd, dyd, dhd, gd, bd = (t.cuda() for t in (x, r, dy, dh, gamma, beta))
    slots = torch.zeros(LN_SLOTS * 2 * D, device="cuda")
    for res, add in ((None, None), (r, None), (r, dh)):
        y_ref, h_ref = ko.layernorm_ref(x, gamma, beta, ko.LN_EPS, res)
        outs = nat.layernorm_fwd(xd, gd, bd, ko.LN_EPS, None if res is None else rd)
        y, mean, rstd = outs[:3]
        assert len(outs) == (3 if res is None else 4)
        assert bool(torch.isfinite(y.float()).all())
        assert ko.row_rel(y, y_ref) <= ko.LN_Y_TOL
        hd = xd
        if res is not None:
            hd = outs[3]
            assert ko.row_rel(hd, h_ref) <= ko.LN_Y_TOL
        dx_ref, dg_ref, db_ref = ko.layernorm_bwd_ref(h_ref, dy, gamma, ko.LN_EPS, add)
        dg = torch.full((D,), 0.5, device="cuda")
        db = torch.full((D,), -0.25, device="cuda")
        for it in (1, 2):       # the second backward goes through the same slots
            dx = nat.layernorm_bwd(hd, dyd, gd, mean, rstd, dg, db, slots,
                                   None if add is None else dhd)
            assert bool(torch.isfinite(dx.float()).all())
            assert ko.row_abs(dx, dx_ref) <= ko.LN_DX_TOL
            assert float(slots.abs().max()) == 0.0          # back to exactly zero
            assert _param_err(dg - 0.5, it * dg_ref) <= ko.LN_PARAM_TOL
            assert _param_err(db + 0.25, it * db_ref) <= ko.LN_PARAM_TOL


@pytest.mark.parametrize("D", [48, 448, 2048])
@pytest.mark.parametrize("variant", ["no_affine", "no_slots", "gamma_only", "beta_none"])
def test_layernorm_variants(D, variant):
    """gamma / beta None, slots=None (a fresh zeroed buffer), a gradient wanted
    for gamma only: through the autograd wrappers, as the models call them."""
    from distributed_ml_pytorch_amd.ops.functional import LN_SLOTS, add_layer_norm, layer_norm

    rows = 37
    x, r, dy, dh, gamma, beta = ko.layernorm_inputs(rows, D, "std", seed=1)
    if variant == "no_affine":
        gamma = beta = None
    elif variant == "beta_none":
        beta = None
    xd = x.cuda().requires_grad_(True)
    rd = r.cuda().requires_grad_(True)
    gd = None if gamma is None else gamma.cuda().requires_grad_(True)
    bd = None if beta is None else beta.cuda().requires_grad_(variant != "gamma_only")
    slots = None if variant == "no_slots" else torch.zeros(LN_SLOTS * 2 * D, device="cuda")

    y = layer_norm(xd, gd, bd, ko.LN_EPS, slots)
    y.backward(dy.cuda())
    y_ref, h_ref = ko.layernorm_ref(x, gamma, beta, ko.LN_EPS)
    dx_ref, dg_ref, db_ref = ko.layernorm_bwd_ref(h_ref, dy, gamma, ko.LN_EPS)
    assert ko.row_rel(y, y_ref) <= ko.LN_Y_TOL
    assert ko.row_abs(xd.grad, dx_ref) <= ko.LN_DX_TOL
    if gd is not None:
        assert _param_err(gd.grad, dg_ref) <= ko.LN_PARAM_TOL
    if bd is not None:
        if variant == "gamma_only":
            assert bd.grad is None
        else:
            assert _param_err(bd.grad, db_ref) <= ko.LN_PARAM_TOL
    if slots is not None:
        assert float(slots.abs().max()) == 0.0

    # fused add, with and without the stream's own gradient dh
    for use_dh in (True, False):
        for t in (xd, rd, gd, bd):
            if t is not None:
                t.grad = None
        h, y = add_layer_norm(xd, rd, gd, bd, ko.LN_EPS, slots)
        y_ref, h_ref = ko.layernorm_ref(x, gamma, beta, ko.LN_EPS, r)
        assert ko.row_rel(h, h_ref) <= ko.LN_Y_TOL and ko.row_rel(y, y_ref) <= ko.LN_Y_TOL
        if use_dh:
            torch.autograd.backward([y, h], [dy.cuda(), dh.cuda()])
        else:
            y.backward(dy.cuda())
        dx_ref, dg_ref, db_ref = ko.layernorm_bwd_ref(h_ref, dy, gamma, ko.LN_EPS,
                                                      dh if use_dh else None)
        assert ko.row_abs(xd.grad, dx_ref) <= ko.LN_DX_TOL
        assert ko.row_abs(rd.grad, dx_ref) <= ko.LN_DX_TOL
        if gd is not None:
            assert _param_err(gd.grad, dg_ref) <= ko.LN_PARAM_TOL
        if bd is not None and variant != "gamma_only":
            assert _param_err(bd.grad, db_ref) <= ko.LN_PARAM_TOL
        if slots is not None:
            assert float(slots.abs().max()) == 0.0


# -------------------------------------------------------------------- softmax
@pytest.mark.parametrize("L", ko.SOFTMAX_L)
def test_softmax_edges(L):
    nat = _nat()
    s, dp = ko.softmax_inputs(L)
    p = nat.softmax_fwd(s.cuda(), ko.SOFTMAX_SCALE)
    assert bool(torch.isfinite(p.float()).all())
    assert ko.row_rel(p, ko.softmax_ref(s, ko.SOFTMAX_SCALE)) <= ko.SOFTMAX_P_TOL
    assert float((ko.f64(p).sum(-1) - 1).abs().max()) <= ko.SOFTMAX_P_TOL
    ds = nat.softmax_bwd(p, dp.cuda(), ko.SOFTMAX_SCALE)
    assert bool(torch.isfinite(ds.float()).all())
    if L == 1:      # P = 1: dS is exactly zero
        assert float(ds.float().abs().max()) == 0.0
    else:
        assert ko.row_abs(ds, ko.softmax_bwd_ref(p, dp, ko.SOFTMAX_SCALE)) <= ko.SOFTMAX_DS_TOL


# ----------------------------------------------------------------------- GELU
@pytest.mark.parametrize("numel", ko.GELU_NUMEL)
def test_gelu_edges(numel):
    nat = _nat()
    x = ko.gelu_grid(numel)
    dy = torch.randn(numel, generator=torch.Generator().manual_seed(numel)).to(torch.bfloat16)
    y = nat.gelu_fwd(x.cuda())
    dx = nat.gelu_bwd(x.cuda(), dy.cuda())
    assert bool(torch.isfinite(y.float()).all()) and bool(torch.isfinite(dx.float()).all())
    torch.testing.assert_close(ko.f64(y), ko.gelu_ref(x), rtol=ko.GELU_Y_TOL, atol=ko.GELU_Y_TOL)
    torch.testing.assert_close(ko.f64(dx), ko.f64(dy) * ko.gelu_grad_ref(x),
                               rtol=ko.GELU_DX_TOL, atol=ko.GELU_DX_TOL)


# ------------------------------------------------------- token_row_scatter
@pytest.mark.parametrize("B,N,D", [(3, 5, 16), (1, 1, 8), (4, 197, 768)])
def test_token_row_scatter_bits(B, N, D):
    nat = _nat()
    g = torch.randn(B, D, generator=torch.Generator().manual_seed(B * N)).to(torch.bfloat16)
    for tok in sorted({0, N // 2, N - 1}):
        out = nat.token_row_scatter(g.cuda(), N, tok)
        want = torch.zeros(B, N, D, dtype=torch.bfloat16)
        want[:, tok] = g
        assert out.shape == (B, N, D)
        assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16))


# ------------------------------------------------------------------ vit_embed
@pytest.mark.parametrize("B,N,D", [(1, 1, 8), (11, 3, 40), (9, 4, 264)])
def test_vit_embed_edges(B, N, D):
    """D/8 not a multiple of 32, B not a multiple of 8, a second blockIdx.y."""
    nat = _nat()
    g = torch.Generator().manual_seed(B * 100 + D)
    tok = torch.randn(B, N, D, generator=g).to(torch.bfloat16)
    cls = torch.randn(1, 1, D, generator=g).to(torch.bfloat16)
    pos = torch.randn(1, N + 1, D, generator=g).to(torch.bfloat16)
    h = nat.vit_embed_fwd(tok.cuda(), cls.cuda(), pos.cuda())
    assert h.shape == (B, N + 1, D)
    # one bf16 rounding of the exact sum
    torch.testing.assert_close(ko.f64(h), ko.vit_embed_ref(tok, cls, pos), rtol=2.0 ** -7, atol=0)

    dh = torch.randn(B, N + 1, D, generator=g).to(torch.bfloat16)
    dpos0 = torch.randn((N + 1) * D, generator=g)
    dcls0 = torch.randn(D, generator=g)
    dpos, dcls = dpos0.cuda(), dcls0.cuda()
    dtok = nat.vit_embed_bwd(dh.cuda(), dpos, dcls, True)
    assert torch.equal(dtok.cpu().view(torch.int16), dh[:, 1:].contiguous().view(torch.int16))
    sums = ko.f64(dh).sum(0)
    torch.testing.assert_close(ko.f64(dpos), dpos0.double() + sums.reshape(-1),
                               rtol=1e-5, atol=1e-4)
    torch.testing.assert_close(ko.f64(dcls), dcls0.double() + sums[0], rtol=1e-5, atol=1e-4)
    # tok needs no gradient: no dtok, the same sums
    dpos2, dcls2 = dpos0.cuda(), dcls0.cuda()
    assert nat.vit_embed_bwd(dh.cuda(), dpos2, dcls2, False) is None
    assert torch.equal(dpos2, dpos) and torch.equal(dcls2, dcls)


def test_vit_embed_autograd_without_token_grad():
    from distributed_ml_pytorch_amd.ops.functional import vit_embed

    B, N, D = 11, 3, 40
    g = torch.Generator().manual_seed(5)
    tok = torch.randn(B, N, D, generator=g).to(torch.bfloat16)
    cls = torch.randn(1, 1, D, generator=g)
    pos = torch.randn(1, N + 1, D, generator=g)
    dh = torch.randn(B, N + 1, D, generator=g).to(torch.bfloat16)
    for tok_grad in (False, True):
        td = tok.cuda().requires_grad_(tok_grad)
        cd, pd = cls.cuda().requires_grad_(True), pos.cuda().requires_grad_(True)
        h = vit_embed(td, cd, pd)
        torch.testing.assert_close(ko.f64(h), ko.vit_embed_ref(tok, ko.bf(cls), ko.bf(pos)),
                                   rtol=2.0 ** -7, atol=0)
        h.backward(dh.cuda())
        sums = ko.f64(dh).sum(0)
        torch.testing.assert_close(ko.f64(pd.grad), sums[None], rtol=1e-5, atol=1e-4)
        torch.testing.assert_close(ko.f64(cd.grad), sums[:1][None], rtol=1e-5, atol=1e-4)
        if tok_grad:
            assert torch.equal(td.grad.cpu().view(torch.int16),
                               dh[:, 1:].contiguous().view(torch.int16))
        else:
            assert td.grad is None
