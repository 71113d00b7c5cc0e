"""CPU checks of tests/kernel_oracles.py: Philox known answers, the fp64
references against torch's own ops, and the tolerance floors -- for every
(shape, regime) cell the GPU edge tests run, the precision-model emulation of a
correct kernel must pass the GPU test's own checker at ONE THIRD of the GPU
threshold.  No threshold is derived from a kernel's output."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import kernel_oracles as ko


# --------------------------------------------------------------------- Philox
@pytest.mark.parametrize("ctr,key,out", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox_known_answers(ctr, key, out):
    got = tuple(int(w) for w in ko.philox4x32_10(ctr, key))
    assert got == out, [hex(w) for w in got]


def test_philox_vectorised_matches_scalar():
    ctr = [np.array([0, 0xFFFFFFFF, 0x243F6A88], dtype=np.uint32) for _ in range(4)]
    ctr[1] = np.array([0, 0xFFFFFFFF, 0x85A308D3], dtype=np.uint32)
    ctr[2] = np.array([0, 0xFFFFFFFF, 0x13198A2E], dtype=np.uint32)
    ctr[3] = np.array([0, 0xFFFFFFFF, 0x03707344], dtype=np.uint32)
    key = (0xA4093822, 0x299F31D0)
    vec = ko.philox4x32_10(ctr, key)
    for i in range(3):
        one = ko.philox4x32_10([c[i] for c in ctr], key)
        assert [int(w[i]) for w in vec] == [int(w) for w in one]


def test_dropout_mask_ref_stream():
    """Element i takes word i & 3 of group i >> 2; the tail of a partial group,
    both key words, both offset words and the threshold are all wired."""
    seed, off, p = 0x123456789ABCDEF0 >> 2, 2**33 + 5, 0.3
    m = ko.dropout_mask_ref(11, p, seed, off)
    assert m.dtype == np.uint8 and m.shape == (11,)
    thr = ko.dropout_threshold(p)
    assert thr == int(0.3 * 2**32)
    for i in (0, 3, 4, 10):
        w = ko.philox4x32_10((i >> 2, 0, off & 0xFFFFFFFF, off >> 32),
                             (seed & 0xFFFFFFFF, seed >> 32))[i & 3]
        assert m[i] == (1 if int(w) >= thr else 0)
    assert np.array_equal(m, ko.dropout_mask_ref(12, p, seed, off)[:11])
    big = ko.dropout_mask_ref(40000, p, seed, off)
    assert abs(big.mean() - 0.7) < 0.01
    for other in (ko.dropout_mask_ref(40000, p, seed ^ (1 << 40), off),    # key high word
                  ko.dropout_mask_ref(40000, p, seed, off ^ (1 << 33)),    # offset high word
                  ko.dropout_mask_ref(40000, p, seed, off + 1)):
        assert 0.3 < (other != big).mean() < 0.55
    assert ko.dropout_mask_ref(64, 0.0, seed, 0).all()


# ----------------------------------------------------------------- checkers
def test_row_checkers_see_one_bad_row():
    ref = torch.randn(1000, 64, generator=torch.Generator().manual_seed(0)).double()
    a = ref.clone()
    a[123] = 0
    whole = float((a - ref).norm() / ref.norm())
    assert whole < 5e-2                      # the whole-tensor norm barely moves
    assert ko.row_rel(a, ref) == pytest.approx(1.0)
    assert ko.row_abs(a, ref) > 0.5
    # row_abs: groups are judged against their own largest row
    g = torch.stack([ref[:10], ref[10:20] * 1e-3])
    b = g.clone()
    b[1, 3] = 0
    assert ko.row_abs(b, g) > 0.5
    assert ko.row_abs(b.reshape(20, 64), g.reshape(20, 64)) < 2e-3


# --------------------------------------------- references vs torch's own ops
def test_references_match_torch():
    g = torch.Generator().manual_seed(1)
    qkv, dout = ko.attention_inputs(2, 17, 2, "sc3")
    out, lse2 = ko.attention_ref(qkv, 2)
    q, k, v = ko.split_qkv(qkv, 2)
    sd = F.scaled_dot_product_attention(q, k, v)
    torch.testing.assert_close(out, ko.merge_heads(sd), rtol=1e-10, atol=1e-12)
    s = q @ k.transpose(-1, -2) / 8
    torch.testing.assert_close(lse2, torch.log2(torch.exp(s).sum(-1)), rtol=1e-10, atol=1e-10)
    # the emulation's lse2 is the same quantity
    torch.testing.assert_close(ko.attention_fwd_emul(qkv, 2)[1], lse2, rtol=1e-12, atol=1e-10)

    x, r, dy, dh, gamma, beta = ko.layernorm_inputs(5, 48, "std")
    xr = ko.f64(x).requires_grad_(True)
    gr, br = ko.f64(gamma).requires_grad_(True), ko.f64(beta).requires_grad_(True)
    yr = F.layer_norm(xr, (48,), gr, br, ko.LN_EPS)
    (yr * ko.f64(dy)).sum().backward()
    y, h = ko.layernorm_ref(x, gamma, beta, ko.LN_EPS)
    dx, dg, db = ko.layernorm_bwd_ref(h, dy, gamma, ko.LN_EPS)
    for a, b in ((y, yr.detach()), (dx, xr.grad), (dg, gr.grad), (db, br.grad)):
        torch.testing.assert_close(a, b, rtol=1e-9, atol=1e-11)

    xg = ko.gelu_grid(8 * 257)
    xr = ko.f64(xg).requires_grad_(True)
    yr = F.gelu(xr, approximate="tanh")
    yr.sum().backward()
    torch.testing.assert_close(ko.gelu_ref(xg), yr.detach(), rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(ko.gelu_grad_ref(xg), xr.grad, rtol=1e-10, atol=1e-12)

    s, dp = ko.softmax_inputs(65)
    sr = ko.f64(s).requires_grad_(True)
    pr = torch.softmax(sr * 0.125, -1)
    (pr * ko.f64(dp)).sum().backward()
    torch.testing.assert_close(ko.softmax_bwd_ref(pr.detach(), dp, 0.125), sr.grad,
                               rtol=1e-9, atol=1e-12)

    tok = torch.randn(3, 4, 8, generator=g).to(torch.bfloat16)
    cls = torch.randn(1, 1, 8, generator=g).to(torch.bfloat16)
    pos = torch.randn(1, 5, 8, generator=g).to(torch.bfloat16)
    ref = ko.vit_embed_ref(tok, cls, pos)
    want = torch.cat([cls.double().expand(3, 1, 8), tok.double()], 1) + pos.double()
    assert torch.equal(ref, want)


def test_xent_ref_ignores_out_of_range_labels_and_numpy_argmax_is_first():
    x = torch.tensor([[1.0, 3.0, 3.0, 0.0], [2.0, 2.0, 1.0, 0.0], [0.0, 1.0, 2.0, 5.0]])
    y = torch.tensor([1, 7, 3])
    loss, grad = ko.xent_ref(x, y)
    want = F.cross_entropy(x[[0, 2]].double(), y[[0, 2]])
    torch.testing.assert_close(loss, want)
    assert float(grad[1].abs().max()) == 0.0
    assert ko.xent_hits_ref(x, torch.tensor([1, 0, 3])) == 3     # first max wins
    assert ko.xent_hits_ref(x, torch.tensor([2, 1, 3])) == 1


# ------------------------------------------------------------ tolerance floors
@pytest.mark.parametrize("B,N,H,regime", ko.ATTN_CELLS)
def test_attention_floor(B, N, H, regime):
    qkv, dout = ko.attention_inputs(B, N, H, regime)
    out_ref, lse_ref = ko.attention_ref(qkv, H)
    out_em, lse_em = ko.attention_fwd_emul(qkv, H)
    f_out = ko.row_rel(out_em.view(B, N, H, 64), out_ref.view(B, N, H, 64))
    dref = ko.attention_bwd_ref(qkv, dout, H)
    dem = ko.attention_bwd_emul(qkv, out_em, dout, lse_em, H)
    f = ko.attention_grad_errors(dem, dref, qkv, dout, H, regime)
    print(f"attention floor B{B} N{N} H{H} {regime}: out {f_out:.5f} dq {f[0]:.5f} "
          f"dk {f[1]:.5f} dv {f[2]:.5f}")
    assert f_out <= ko.ATTN_OUT_TOL / 3
    assert f[0] <= ko.ATTN_DQK_TOL[regime] / 3
    assert f[1] <= ko.ATTN_DQK_TOL[regime] / 3
    assert f[2] <= ko.ATTN_DV_TOL / 3


@pytest.mark.parametrize("rows,D,regime", ko.LN_CELLS)
def test_layernorm_floor(rows, D, regime):
    assert ko.ln_lanes(D) == ko.LN_DIMS[D][:2]
    x, r, dy, dh, gamma, beta = ko.layernorm_inputs(rows, D, regime)
    for res in (None, r):
        y_ref, h = ko.layernorm_ref(x, gamma, beta, ko.LN_EPS, res)
        y_em, _ = ko.layernorm_emul(x, gamma, beta, ko.LN_EPS, res)
        assert ko.row_rel(y_em, y_ref) <= ko.LN_Y_TOL / 3
        for add in (None, dh):
            dx_ref, dg_ref, db_ref = ko.layernorm_bwd_ref(h, dy, gamma, ko.LN_EPS, add)
            dx_em, _, _ = ko.layernorm_bwd_emul(h, dy, gamma, ko.LN_EPS, add)
            assert ko.row_abs(dx_em, dx_ref) <= ko.LN_DX_TOL / 3
    # dgamma / dbeta: fp32 sums of products of the same bf16 inputs
    _, dg32, db32 = ko.layernorm_bwd_ref(h, dy, gamma, ko.LN_EPS, None, dtype=torch.float32)
    for a, ref in ((dg32, dg_ref), (db32, db_ref)):
        floor = float((a.double() - ref).abs().max() / ref.abs().max())
        assert floor <= ko.LN_PARAM_TOL / 3, floor


@pytest.mark.parametrize("L", ko.SOFTMAX_L)
def test_softmax_floor(L):
    s, dp = ko.softmax_inputs(L)
    p_ref = ko.softmax_ref(s, ko.SOFTMAX_SCALE)
    p_em = ko.softmax_emul(s, ko.SOFTMAX_SCALE)
    assert ko.row_rel(p_em, p_ref) <= ko.SOFTMAX_P_TOL / 3
    assert float((p_em.sum(-1) - 1).abs().max()) <= ko.SOFTMAX_P_TOL / 3
    ds_ref = ko.softmax_bwd_ref(p_em, dp, ko.SOFTMAX_SCALE)
    ds_em = ko.softmax_bwd_emul(p_em, dp, ko.SOFTMAX_SCALE)
    if L == 1:      # P = 1: dS is exactly zero, and the GPU test asks for that
        assert float(ds_ref.abs().max()) == 0.0 and float(ds_em.abs().max()) == 0.0
    else:
        assert ko.row_abs(ds_em, ds_ref) <= ko.SOFTMAX_DS_TOL / 3


@pytest.mark.parametrize("numel", ko.GELU_NUMEL)
def test_gelu_floor(numel):
    x = ko.gelu_grid(numel)
    assert x.numel() == numel
    if numel > 8:
        assert float(x.min()) == -200.0 and float(x.max()) == 200.0
    dy = torch.randn(numel, generator=torch.Generator().manual_seed(numel)).to(torch.bfloat16)
    y_ref, y_em = ko.gelu_ref(x), ko.gelu_emul(x)
    assert bool(torch.isfinite(y_ref).all())
    torch.testing.assert_close(y_em, y_ref, rtol=ko.GELU_Y_TOL / 3, atol=ko.GELU_Y_TOL / 3)
    dx_ref = ko.f64(dy) * ko.gelu_grad_ref(x)
    torch.testing.assert_close(ko.gelu_bwd_emul(x, dy), dx_ref, rtol=ko.GELU_DX_TOL / 3,
                               atol=ko.GELU_DX_TOL / 3)
