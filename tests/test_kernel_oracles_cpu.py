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


# ------------------------------------------------------- BatchNorm and pooling
def _bn_case(shape, regime, relu, res, seed=0, training=True, emul=True, **kw):
    N, C, H, W = shape
    d = ko.bn_inputs(N, C, H, W, regime, seed)
    args = dict(residual=d["res"] if res else None, relu=relu, dy=d["dy"], training=training,
                running=None if training else (d["rm"], d["rv"]))
    em = ko.bn_emul(d["x"], d["gamma"], d["beta"], **args, **kw) if emul else None
    ref = ko.bn_ref(d["x"], d["gamma"], d["beta"], **args,
                    y_stored=em["y"] if emul else None)
    return d, em, ref


def test_bn_inputs_regimes():
    d = ko.bn_inputs(4, 40, 5, 5, "mixed")
    x, gamma, beta = d["x"].double(), d["gamma"], d["beta"]
    assert gamma.unique().numel() == 40 and beta.unique().numel() == 40
    assert float(gamma[3]) == 0.0 and int((gamma == 0).sum()) == 1
    assert bool((gamma[::7] < 0).all()) and int((gamma < 0).sum()) == 6
    mean, std = x.mean(dim=(0, 2, 3)), x.std(dim=(0, 2, 3))
    # the five base regimes inside every 8-channel vector
    for c in range(40):
        want = {0: (0.5, 2.0), 1: (16.0, 1.0), 2: (64.0, 1.0), 3: (0.0, 1e-3), 4: (250.0, 1e3)}[c % 5]
        assert abs(float(mean[c]) - want[0]) < 0.5 * want[1] and 0.7 < float(std[c]) / want[1] < 1.3
    c = ko.bn_inputs(2, 16, 3, 3, "const")["x"].double()
    assert bool((c[:, 1::2] == 3.0).all()) and float(c[:, ::2].std()) > 1.0
    n = ko.bn_inputs(2, 8, 9, 9, "near1024")["x"].double()
    assert set(n.unique().tolist()) <= {1016.0, 1020.0, 1024.0, 1032.0}    # the bf16 grid there
    assert ko.bn_inputs(30, 24, 0, 0, "std")["x"].shape == (30, 24)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("relu,res", ko.BN_ACT)
def test_bn_ref_matches_torch(training, relu, res):
    """bn_ref against F.batch_norm in fp64: forward, running statistics (momentum
    1) and every gradient, training and eval; eval-mode dx is k1 * dz."""
    for shape in ((3, 16, 5, 4), (11, 8, 0, 0)):
        d, _, ref = _bn_case(shape, "std", relu, res, training=training, emul=False)
        x = ko.f64(d["x"]).requires_grad_(True)
        r = ko.f64(d["res"]).requires_grad_(True)
        g, b = ko.f64(d["gamma"]).requires_grad_(True), ko.f64(d["beta"]).requires_grad_(True)
        rm, rv = ko.f64(d["rm"]).clone(), ko.f64(d["rv"]).clone()
        y = F.batch_norm(x, rm, rv, g, b, training, 1.0, ko.BN_EPS)
        if res:
            y = y + r
        if relu:
            y = F.relu(y)
        (y * ko.f64(d["dy"])).sum().backward()
        close = lambda a, w: torch.testing.assert_close(a, w, rtol=1e-9, atol=1e-10)
        close(ref["y"], y.detach())
        close(ref["dx"], x.grad)
        close(ref["dgamma"], g.grad)
        close(ref["dbeta"], b.grad)
        if res:
            close(ref["dres"], r.grad)
        if training:
            close(ref["rmean"], rm)
            close(ref["rvar"], rv)
        else:
            close(ref["dx"], ko._unmc(ko._mc(ref["dres"]) * ko.f64(d["gamma"]) * ref["invstd"],
                                      d["x"]))


def test_bn_emul_is_really_fp32():
    """At |mean|/sigma = 64 two-moment fp32 statistics are off by about
    2^-23 * 64^2 = 5e-4 on invstd: an emulation whose accumulator were silently
    wider would sit orders of magnitude below.  One run over all M rows (the
    literal worst order) is worse still, and grows with M."""
    for cell in ("c24", "trip", "wrap"):
        _, em, ref = _bn_case(ko.BN_CELLS[cell], "off64", False, False)
        e = ko.bn_stat_errs(em["mean"], em["invstd"], ref)[1]
        assert 1e-4 < e <= ko.BN_OFF64_INVSTD_TOL / 3, (cell, e)
    _, em1, ref = _bn_case(ko.BN_CELLS["wrap"], "off64", False, False, chunk=None)
    e1 = ko.bn_stat_errs(em1["mean"], em1["invstd"], ref)[1]
    print(f"wrap off64 invstd error: one sequential run {e1:.2e}, 64-row runs {e:.2e}")
    assert e1 > 10 * e
    _, em16, ref16 = _bn_case(ko.BN_CELLS["trip"], "off16", False, False)
    assert 3e-6 < ko.bn_stat_errs(em16["mean"], em16["invstd"], ref16)[1] < 1e-4


def test_chan_checkers_see_one_bad_channel():
    d, em, ref = _bn_case(ko.BN_CELLS["trip"], "mixed", True, True)
    bad = {k: v.clone() if torch.is_tensor(v) else v for k, v in em.items()}
    # channel 9 (a "loud" channel: tiny k1) takes channel 10's dx and y
    bad["dx"][:, 9], bad["y"][:, 9] = em["dx"][:, 10], em["y"][:, 10]
    e = ko.bn_errors(bad, ref, 162, True)
    assert e["dx"] > 0.5 and e["y"] > 0.5
    whole = float((ko.f64(bad["dx"]) - ref["dx"]).norm() / ref["dx"].norm())
    assert whole < 1e-2                      # the whole-tensor norm does not notice
    # gamma == 0 on channel 3: dx must be exactly zero there
    assert float(ref["dx"][:, 3].abs().max()) == 0.0
    bad = dict(em, dx=em["dx"].clone())
    bad["dx"][0, 3, 0, 0] = 1e-3
    with pytest.raises(AssertionError):
        ko.bn_errors(bad, ref, 162, True)


@pytest.mark.parametrize("cell,regime,relu,res", ko.bn_fold_cases())
def test_bn_floor(cell, regime, relu, res):
    """Training mode: the folded, unfolded and mode-1 GPU tests run these cells
    (two steps: seeds 0 and 1)."""
    shape = ko.BN_CELLS[cell]
    for seed in (0, 1):
        _, em, ref = _bn_case(shape, regime, relu, res, seed)
        if not res:
            em["dres"] = None
        e = ko.bn_errors(em, ref, shape[0] * shape[2] * shape[3], relu)
        ko.bn_assert(e, regime, 3.0, f"floor {cell} relu={relu} res={res} seed={seed}")


@pytest.mark.parametrize("cell,regime,relu,res", ko.bn_eval_cases())
def test_bn_eval_floor(cell, regime, relu, res):
    shape = ko.BN_CELLS[cell]
    _, em, ref = _bn_case(shape, regime, relu, res, training=False)
    got = {k: em[k] for k in ("y", "dx", "dgamma", "dbeta")}
    got["dres"] = em["dres"] if res else None
    ko.bn_assert(ko.bn_errors(got, ref, shape[0] * shape[2] * shape[3], relu), regime, 3.0,
                 f"eval floor {cell}")


@pytest.mark.parametrize("M,C", ko.BN_1D)
@pytest.mark.parametrize("regime", ["std", "off64"])
@pytest.mark.parametrize("training", [True, False])
def test_bn1d_floor(M, C, regime, training):
    _, em, ref = _bn_case((M, C, 0, 0), regime, True, False, training=training)
    got = {k: em[k] for k in ("y", "dx", "dgamma", "dbeta")}
    ko.bn_assert(ko.bn_errors(got, ref, M, True), regime, 3.0, "1d floor")


@pytest.mark.parametrize("shape", ko.BN_POOL_SHAPES)
@pytest.mark.parametrize("regime", ko.BN_POOL_REGIMES)
def test_bn_pool_floor(shape, regime):
    """The fused stem: BN emulation -> pool of its stored y -> BN backward of the
    gathered, bf16-rounded dz."""
    d = ko.bn_inputs(*shape, regime)
    fwd = ko.bn_emul(d["x"], d["gamma"], d["beta"], relu=True)
    dp = ko.bn_pool_dp(shape)
    yp, tap, dz, ref = ko.bn_pool_ref(d, fwd["y"], dp)
    em = ko.bn_emul(d["x"], d["gamma"], d["beta"], relu=True, dy=ko.bf(dz), dy_sums=dz)
    assert torch.equal(em["y"], fwd["y"])
    em["dres"] = None
    ko.bn_assert(ko.bn_errors(em, ref, shape[0] * shape[2] * shape[3], True), regime, 3.0,
                 f"stem floor {shape}")


POOL_KSP = [(2, 2, 0), (3, 2, 1), (3, 3, 0), (5, 2, 2), (2, 3, 0)]
POOL_SHAPES = [(2, 8, 9, 7), (1, 16, 3, 3), (2, 6, 9, 7)]


@pytest.mark.parametrize("k,s,p", POOL_KSP)
@pytest.mark.parametrize("shape", POOL_SHAPES + [(2, 64, 15, 17)])
def test_maxpool_ref_matches_torch(shape, k, s, p):
    """First maximum in scan order on tie-heavy integers, against
    F.max_pool2d(return_indices=True) and its autograd; all-negative inputs with
    padding (a padded tap that won would show)."""
    for lo, hi in ((-1, 2), (-3, -1)):
        x, dy = ko.pool_int_inputs(shape, k, s, p, lo=lo, hi=hi)
        y, tap, dx = ko.maxpool_ref(x, k, s, p, dy=dy)
        xr = x.double().requires_grad_(True)
        yr, ir = F.max_pool2d(xr, k, s, p, return_indices=True)
        (yr * dy.double()).sum().backward()
        assert torch.equal(y, yr.detach())
        assert torch.equal(ko.maxpool_flat_index(tap, shape[2], shape[3], k, s, p), ir)
        assert torch.equal(dx, xr.grad)
        assert torch.equal(ko.bf(dx), dx)        # exact in bf16
        # relu_in: tap 255 exactly where the window maximum is not positive
        _, tap_r, dx_r = ko.maxpool_ref(x, k, s, p, relu_in=True, dy=dy)
        assert torch.equal(tap_r == 255, ~(y > 0))
        assert torch.equal(tap_r[y > 0], tap[y > 0])
        xr.grad = None
        (F.max_pool2d(F.relu(xr), k, s, p) * dy.double()).sum().backward()
        assert torch.equal(dx_r, xr.grad)


def test_gap_ref_matches_torch():
    x = torch.randn(3, 8, 5, 6, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(3, 8, dtype=torch.float64)
    x.mean(dim=(2, 3)).backward(dy)
    y, dx = ko.gap_ref(x, dy)
    torch.testing.assert_close(y, x.detach().mean(dim=(2, 3)))
    torch.testing.assert_close(dx, x.grad)


@pytest.mark.parametrize("HW", list(ko.GAP_HW))
@pytest.mark.parametrize("C", ko.GAP_C)
def test_gap_floor(HW, C):
    for offset in ko.GAP_OFFSETS:
        x, dy = ko.gap_inputs(HW, C, offset)
        y, dx = ko.gap_ref(x, dy)
        e_y, e_dx = ko.gap_errors(ko.bf(y), ko.bf(dx), x, dy)
        assert e_y <= ko.GAP_Y_TOL / 3 and e_dx <= ko.GAP_DX_TOL / 3, (e_y, e_dx)
