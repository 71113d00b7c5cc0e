"""csrc/bn.hip at its edge shapes and over its numeric range, against the fp64
oracle tests/kernel_oracles.py::bn_ref: the folded and unfolded training paths,
every ReLU-mask mode, eval mode (running statistics: dx = k1 * dz), BatchNorm1d,
the fused BN + ReLU + max pool stem and, recorded only, the edge of the
two-moment variance's domain.  Thresholds and cells live in kernel_oracles.py;
test_kernel_oracles_cpu.py shows a correct implementation passes each at a third.

The backward reference takes its ReLU mask from the stored y of the run under
test (bn.hip's rule); that the stored mask differs from the fp64 one only at
genuine near-zeros is checked with the forward (the "flip" error)."""
import functools

import pytest
import torch

import kernel_oracles as ko

pytestmark = pytest.mark.gpu

CL = torch.channels_last
EPS = ko.BN_EPS
SLOTS, TAIL = 64, 4          # csrc/bn_slots.h


def _nat():
    from distributed_ml_pytorch_amd.ops._ext import native

    return native()


def _dev(t):
    t = t.cuda()
    return t.contiguous(memory_format=CL) if t.dim() == 4 else t


@functools.lru_cache(maxsize=None)
def _inputs(shape, regime, seed=0):
    return ko.bn_inputs(*shape, regime, seed)


def _rows(shape):
    return shape[0] * shape[2] * shape[3] if shape[2] else shape[0]


def _case_id(c):
    return f"{c[0]}-{c[1]}-relu{int(c[2])}-res{int(c[3])}"


# ------------------------------------------------------------------ dispatch
def _num_partials(M, C):
    g = M * (C // 8) // (256 * 8)
    return min(max(g, 1), 2048, M)


def _bwd_partials(M, C):
    G = _num_partials(M, C)
    if G >= 256:
        return G
    return max(G, min(M * (C // 8) // (256 * 2), 2048, M))


def _fold_cs(C):
    return 64 if C % 64 == 0 else 32 if C % 32 == 0 else 16 if C % 16 == 0 else 8


def _fold_grid(M, C):
    cs = _fold_cs(C)
    nsl, vecs = C // cs, M * (cs // 8)
    nrb = -(-vecs // (256 * 4))
    if nrb * nsl < 512:
        nrb = -(-vecs // 256)
    return max(1, min(nrb, max(1, 1024 // nsl), M)), nsl


def test_cells_are_the_ones_named():
    """bn_num_partials, bn_bwd_partials, fold_cs and fold_grid of bn.hip at their
    default knobs, recomputed: every cell sits on the edge it is named for."""
    geo = {}
    for name, (N, C, H, W) in ko.BN_CELLS.items():
        M, tpr = N * H * W, C // 8
        G, Gb = _num_partials(M, C), _bwd_partials(M, C)
        geo[name] = dict(M=M, tpr=tpr, rpi=256 // tpr, cs=_fold_cs(C), G=G, Gb=Gb,
                         rpb=-(-M // G), rpb_b=-(-M // Gb), grid=_fold_grid(M, C))
        g = geo[name]
        # no thread sums more than BN_EMUL_CHUNK rows in one run (the emulation's model)
        for rows_per_blk in (g["rpb"], g["rpb_b"]):
            assert -(-rows_per_blk // g["rpi"]) <= ko.BN_EMUL_CHUNK, name
    g = geo["min"]       # the smallest legal call
    assert (g["M"], g["tpr"], g["rpi"], g["cs"]) == (2, 1, 256, 8)
    g = geo["c24"]       # thread 255 idle, fewer rows than row-lanes
    assert (g["M"], g["tpr"], g["rpi"]) == (30, 3, 85) and 255 // 3 == 85 and g["M"] < g["rpi"]
    assert (geo["cs16"]["cs"], geo["cs16"]["grid"][1]) == (16, 3)
    assert (geo["cs32"]["cs"], geo["cs32"]["grid"][1]) == (32, 3)
    g = geo["trip"]      # one 4-row trip, then a ragged tail of 1 or 2 rows
    assert (g["M"], g["rpi"], g["G"]) == (162, 32, 1)
    lanes = [len(range(r0, 162, 32)) for r0 in range(32)]
    assert set(lanes) == {5, 6} and all(r0 + 3 * 32 < 162 for r0 in range(32))
    g = geo["c1000"]
    assert (g["tpr"], g["rpi"], g["cs"], g["grid"][1]) == (125, 2, 8, 125)
    g = geo["c1032"]
    assert (g["tpr"], g["rpi"], 256 - g["tpr"], g["cs"]) == (129, 1, 127, 8)
    g = geo["c2048"]     # the last reduce block starts past M
    assert (g["M"], g["rpi"], g["G"], g["rpb"]) == (147, 1, 18, 9)
    assert (g["G"] - 1) * g["rpb"] == 153 >= g["M"]
    g = geo["uneven"]    # the last reduce block is short
    assert (g["M"], g["G"], g["rpb"]) == (1058, 4, 265) and g["M"] - 3 * 265 == 263
    g = geo["wrap"]      # more reduce blocks than slots, both directions
    assert (g["M"], g["G"], g["Gb"]) == (16820, 65, 262) and g["G"] > SLOTS
    assert -(-g["Gb"] // SLOTS) == 5 and g["Gb"] // SLOTS == 4     # slots shared 4- and 5-fold
    # the largest tensor stays small
    assert max(N * C * H * W * 2 for N, C, H, W in ko.BN_CELLS.values()) < 2.2e6


# ------------------------------------------------------------------- helpers
def _layer(C, d, relu, one_d=False):
    from distributed_ml_pytorch_amd.ops import functional as DF
    from distributed_ml_pytorch_amd.ops import layers as L

    bn = (L.BatchNorm1d if one_d else L.BatchNorm2d)(C, eps=EPS, momentum=1.0, relu=relu).cuda()
    with torch.no_grad():
        bn.weight.copy_(d["gamma"])
        bn.bias.copy_(d["beta"])
    # the layer's persistent slot buffers, their reserved tail words marked
    n = 2 * SLOTS * C + TAIL
    for attr in ("_dmp_fslots", "_dmp_bslots"):
        buf = torch.zeros(n, dtype=torch.float32, device="cuda")
        buf[-TAIL:] = torch.tensor([1.5, -2.5, 3.5, -4.5])
        DF.mark_slots(buf, False)            # a recycled address may still be listed dirty
        object.__setattr__(bn, attr, buf)
    return bn


def _slots_clean(buf, what):
    assert float(buf[:-TAIL].abs().max()) == 0.0, f"{what}: slot sums left behind"
    assert buf[-TAIL:].tolist() == [1.5, -2.5, 3.5, -4.5], f"{what}: reserved tail words written"


def _step(bn, d, res, check_slots=False):
    """One forward / backward through the layer -> dict of bn_ref's keys (CPU)."""
    x = _dev(d["x"]).requires_grad_(True)
    r = _dev(d["res"]).requires_grad_(True) if res else None
    with torch.no_grad():                # beta is drawn per seed
        bn.weight.copy_(d["gamma"])
        bn.bias.copy_(d["beta"])
    bn.weight.grad = bn.bias.grad = None
    y = bn(x, residual=r)
    assert y.dtype == torch.bfloat16 and y.shape == x.shape
    if check_slots:      # the forward apply zeroed the backward slots
        _slots_clean(bn._dmp_bslots, "after the forward, backward slots")
    y.backward(_dev(d["dy"]))
    if check_slots:      # the backward apply zeroed the forward slot sums it read
        _slots_clean(bn._dmp_fslots, "after the backward, forward slots")
        assert bn._dmp_bslots[-TAIL:].tolist() == [1.5, -2.5, 3.5, -4.5]
    torch.cuda.synchronize()
    return dict(y=y.detach().cpu(), dx=x.grad.cpu(), dres=r.grad.cpu() if res else None,
                dgamma=bn.weight.grad.cpu(), dbeta=bn.bias.grad.cpu(),
                rmean=bn.running_mean.cpu(), rvar=bn.running_var.cpu())


def _ref(d, got, relu, res, training=True):
    return ko.bn_ref(d["x"], d["gamma"], d["beta"], EPS, d["res"] if res else None, relu,
                     training, None if training else (d["rm"], d["rv"]), dy=d["dy"],
                     y_stored=got["y"])


def _finite(got):
    for k, v in got.items():
        if v is not None:
            assert bool(torch.isfinite(v.float()).all()), f"{k} is not finite"


def _check_training(bn, shape, regime, relu, res, what, check_slots=False):
    """Two steps back to back (seeds 0 and 1) on the layer's persistent slots."""
    for seed in (0, 1):
        d = _inputs(shape, regime, seed)
        got = _step(bn, d, res, check_slots)
        _finite(got)
        ref = _ref(d, got, relu, res)
        ko.bn_assert(ko.bn_errors(got, ref, _rows(shape), relu), regime, 1.0,
                     f"{what} step {seed}")


def _mask_bits(y):
    """The 1-bit ReLU mask of a stored y: [M, C/8] bytes, bit k = channel c0 + k."""
    nz = (_mc_dev(y).view(torch.int16) != 0).to(torch.int32)
    M, C = nz.shape
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.int32, device=nz.device)
    return (nz.view(M, C // 8, 8) * w).sum(-1).to(torch.uint8)


def _mc_dev(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]) if t.dim() == 4 else t


def _fresh_slots(C):
    return torch.zeros(2 * SLOTS * C + TAIL, dtype=torch.float32, device="cuda")


# ------------------------------------------------------- folded training path
@pytest.mark.parametrize("cell,regime,relu,res", ko.bn_fold_cases(),
                         ids=[_case_id(c) for c in ko.bn_fold_cases()])
def test_fold_training(cell, regime, relu, res):
    """bn_fwd_fold / bn_bwd_fold (the default training path).  First the
    binding itself, for the statistics it returns (mean, invstd, folded scale /
    shift, running statistics at momentum 1) and the ReLU bit mask; then two
    steps through the layer with its persistent slot buffers: y, dx, dres,
    dgamma, dbeta and the running statistics, and after every pass the slot
    buffer that pass is to leave zeroed (the forward apply zeroes the backward
    slots, the backward apply the forward slots) with the reserved tail words
    untouched."""
    from distributed_ml_pytorch_amd.ops import functional as DF

    assert DF._BN_FOLD and DF._BN_BITMASK, "the folded path with bit masks is the default"
    shape = ko.BN_CELLS[cell]
    C, M = shape[1], _rows(shape)
    d = _inputs(shape, regime, 0)
    x, r = _dev(d["x"]), _dev(d["res"]) if res else None
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    want_mask = relu and res
    y, stats, mask = _nat().bn_fwd_fold(x, _fresh_slots(C), False, r, d["gamma"].cuda(),
                                        d["beta"].cuda(), rm, rv, 1.0, EPS, relu, want_mask, None)
    torch.cuda.synchronize()
    stats = stats.cpu().double()
    got = dict(y=y.cpu(), mean=stats[0], invstd=stats[1], rmean=rm.cpu(), rvar=rv.cpu())
    _finite(got)
    ref = ko.bn_ref(d["x"], d["gamma"], d["beta"], EPS, d["res"] if res else None, relu)
    ko.bn_assert(ko.bn_errors(got, ref, M, relu), regime, 1.0, f"{cell} bn_fwd_fold")
    # folded coefficients: scale = gamma * invstd, shift = beta - mean * scale, from
    # the published mean / invstd (fp32: a few ulp of the larger term)
    sc = d["gamma"].double() * stats[1]
    torch.testing.assert_close(stats[2], sc, rtol=1e-6, atol=0)
    bound = 1e-6 * (d["beta"].double().abs() + (stats[0] * sc).abs()) + 1e-30
    assert bool(((stats[3] - (d["beta"].double() - stats[0] * sc)).abs() <= bound).all())
    if want_mask:
        assert torch.equal(mask, _mask_bits(y))
    else:
        assert mask is None or mask.numel() == 0

    bn = _layer(C, d, relu)
    _check_training(bn, shape, regime, relu, res, f"{cell} layer", check_slots=True)


# ------------------------------------------------------ mask exactness, bit for bit
@pytest.mark.parametrize("regime", ko.BN_REGIMES)
@pytest.mark.parametrize("cell", ko.BN_FULL_CELLS)
def test_relu_mask_is_the_stored_y(cell, regime):
    """bn.hip claims the mask recomputed from x and the folded scale / shift
    (mode 2) is the mask of the stored y, and so is the bit mask (mode 3): dres of
    a direct bn_bwd_fold call equals where(stored y > 0, dy, 0) exactly."""
    shape = ko.BN_CELLS[cell]
    C = shape[1]
    d = _inputs(shape, regime, 0)
    nat = _nat()
    x, r, dy = _dev(d["x"]), _dev(d["res"]), _dev(d["dy"])
    gamma, beta = d["gamma"].cuda(), d["beta"].cuda()
    zeros = lambda: torch.zeros(C, device="cuda")
    for mode, res in ((2, None), (3, r)):
        fs, bs = _fresh_slots(C), _fresh_slots(C)
        y, stats, mask = nat.bn_fwd_fold(x, fs, False, res, gamma, beta, None, None, 0.1, EPS,
                                         True, mode == 3, bs)
        if mode == 3:
            assert torch.equal(mask, _mask_bits(y))
        dx, dres = nat.bn_bwd_fold(x, dy, None, gamma, stats, zeros(), zeros(), True, True, bs,
                                   mask if mode == 3 else None, fs)
        torch.cuda.synchronize()
        want = torch.where(y > 0, dy, torch.zeros_like(dy))
        assert torch.equal(dres, want), f"mode {mode}: dres is not dy under the stored y's mask"
        assert 0 < int((y > 0).sum()) < y.numel()
        assert float(fs[:-TAIL].abs().max()) == 0.0      # zeroed by the backward apply


# -------------------------------------------------------- mode 1 (mask from y)
@pytest.mark.parametrize("regime", ["std", "off64"])
def test_mode1_mask_from_saved_y(regime, monkeypatch):
    from distributed_ml_pytorch_amd.ops import functional as DF

    monkeypatch.setattr(DF, "_BN_BITMASK", False)
    shape = ko.BN_CELLS["trip"]
    bn = _layer(shape[1], _inputs(shape, regime, 0), True)
    _check_training(bn, shape, regime, True, True, "trip mode 1", check_slots=True)


# ------------------------------------------------------------- unfolded path
@pytest.mark.parametrize("cell,regime,relu,res", ko.bn_unfolded_cases(),
                         ids=[_case_id(c) for c in ko.bn_unfolded_cases()])
def test_unfolded_training(cell, regime, relu, res, monkeypatch):
    """DMP_BN_FOLD=0: bn_fwd / bn_bwd with their separate finalize kernels, which
    re-zero the slots they read."""
    from distributed_ml_pytorch_amd.ops import functional as DF

    monkeypatch.setattr(DF, "_BN_FOLD", False)
    shape = ko.BN_CELLS[cell]
    C, M = shape[1], _rows(shape)
    d = _inputs(shape, regime, 0)
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    slots = _fresh_slots(C)
    y, stats, _ = _nat().bn_fwd(_dev(d["x"]), _dev(d["res"]) if res else None, d["gamma"].cuda(),
                                d["beta"].cuda(), rm, rv, 1.0, EPS, True, relu, slots, relu and res)
    torch.cuda.synchronize()
    stats = stats.cpu().double()
    got = dict(y=y.cpu(), mean=stats[0], invstd=stats[1], rmean=rm.cpu(), rvar=rv.cpu())
    ref = ko.bn_ref(d["x"], d["gamma"], d["beta"], EPS, d["res"] if res else None, relu)
    ko.bn_assert(ko.bn_errors(got, ref, M, relu), regime, 1.0, f"{cell} bn_fwd")
    assert float(slots.abs().max()) == 0.0               # re-zeroed by the finalize

    bn = _layer(C, d, relu)
    _check_training(bn, shape, regime, relu, res, f"{cell} unfolded layer")
    _slots_clean(bn._dmp_fslots, "unfolded forward slots")
    _slots_clean(bn._dmp_bslots, "unfolded backward slots")


def test_fwd_from_partials():
    """bn_fwd_from_partials fed with slot sums the test builds from the fp64 S
    and Q, spread unevenly over the 64 slots."""
    shape, regime = ko.BN_CELLS["trip"], "std"
    C, M = shape[1], _rows(shape)
    d = _inputs(shape, regime, 0)
    X = ko._mc(d["x"])
    w = torch.rand(SLOTS, 1, dtype=torch.float64, generator=torch.Generator().manual_seed(5))
    w[7] = 0.0                                            # an unused slot
    w = w / w.sum()
    part = torch.zeros(2 * SLOTS * C + TAIL, dtype=torch.float32)
    part[:SLOTS * C] = (w * X.sum(0)).float().reshape(-1)
    part[SLOTS * C:2 * SLOTS * C] = (w * (X * X).sum(0)).float().reshape(-1)
    part = part.cuda()
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    y, stats, mask = _nat().bn_fwd_from_partials(
        _dev(d["x"]), part, SLOTS, _dev(d["res"]), d["gamma"].cuda(), d["beta"].cuda(), rm, rv,
        1.0, EPS, True, True)
    torch.cuda.synchronize()
    stats = stats.cpu().double()
    got = dict(y=y.cpu(), mean=stats[0], invstd=stats[1], rmean=rm.cpu(), rvar=rv.cpu())
    ref = ko.bn_ref(d["x"], d["gamma"], d["beta"], EPS, d["res"], True)
    ko.bn_assert(ko.bn_errors(got, ref, M, True), regime, 1.0, "bn_fwd_from_partials")
    assert torch.equal(mask, _mask_bits(y))
    assert float(part.abs().max()) == 0.0                # re-zeroed by the finalize


# ------------------------------------------------------------------ eval mode
def _check_eval(bn, d, shape, regime, relu, res, what):
    with torch.no_grad():
        bn.running_mean.copy_(d["rm"])
        bn.running_var.copy_(d["rv"])
    bn.eval()
    got = _step(bn, d, res)
    _finite(got)
    assert torch.equal(got.pop("rmean"), d["rm"]) and torch.equal(got.pop("rvar"), d["rv"])
    ref = _ref(d, got, relu, res, training=False)
    ko.bn_assert(ko.bn_errors(got, ref, _rows(shape), relu), regime, 1.0, what)


@pytest.mark.parametrize("fold", [True, False], ids=["fold", "nofold"])
@pytest.mark.parametrize("cell,regime,relu,res", ko.bn_eval_cases(),
                         ids=[_case_id(c) for c in ko.bn_eval_cases()])
def test_eval_mode(cell, regime, relu, res, fold, monkeypatch):
    """Running statistics far from the batch's: the forward normalises with them
    and the input gradient is k1 * dz -- mean and invstd do not depend on x.
    (Before the batch_stats flag of bn_bwd the batch-statistics formula was
    applied here: per-channel dx error 3.4 - 3.6 at c24 against the bound 0.012.)"""
    from distributed_ml_pytorch_amd.ops import functional as DF

    monkeypatch.setattr(DF, "_BN_FOLD", fold)
    shape = ko.BN_CELLS[cell]
    d = _inputs(shape, regime, 0)
    bn = _layer(shape[1], d, relu)
    _check_eval(bn, d, shape, regime, relu, res, f"eval {cell}")


def test_eval_backward_after_a_training_step():
    """A folded training backward leaves its sums in the layer's backward slots
    (the next folded forward zeroes them).  An eval-mode backward reduces into
    the same buffer: it must not add to what was left."""
    shape, regime = ko.BN_CELLS["trip"], "std"
    d0, d1 = _inputs(shape, regime, 0), _inputs(shape, regime, 1)
    bn = _layer(shape[1], d0, True)
    _step(bn, d0, True)
    assert float(bn._dmp_bslots[:-TAIL].abs().max()) > 0.0
    _check_eval(bn, d1, shape, regime, True, True, "eval after a training step")


# ---------------------------------------------------------------- BatchNorm1d
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("regime", ["std", "off64"])
@pytest.mark.parametrize("M,C", ko.BN_1D)
def test_batchnorm1d(M, C, regime, training):
    shape = (M, C, 0, 0)
    d = _inputs(shape, regime, 0)
    bn = _layer(C, d, True, one_d=True)
    if training:
        _check_training(bn, shape, regime, True, False, "1d", check_slots=True)
    else:
        _check_eval(bn, d, shape, regime, True, False, "1d eval")


# ------------------------------------------- fused BN + ReLU + max pool stem
@pytest.mark.parametrize("regime", ko.BN_POOL_REGIMES)
@pytest.mark.parametrize("shape", ko.BN_POOL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bn_relu_maxpool_stem(shape, regime):
    """bn_relu_maxpool_fwd / maxpool_bn_bwd against the unfused kernels (pooled
    output bit-identical) and against bn_ref + maxpool_ref: the taps and the x
    kept at the winning taps exactly, everything else at the BN thresholds."""
    nat = _nat()
    N, C, H, W = shape
    M = N * H * W
    d = _inputs(shape, regime, 0)
    x, gamma, beta = _dev(d["x"]), d["gamma"].cuda(), d["beta"].cuda()
    assert nat.bn_maxpool_supported(C, 3, 2, 1)
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    fs, bs = _fresh_slots(C), _fresh_slots(C)
    yp, idx, stats, xm = nat.bn_relu_maxpool_fwd(x, fs, False, gamma, beta, rm, rv, 1.0, EPS, bs,
                                                 3, 2, 1)
    # the unfused pair
    y_u, stats_u, _ = nat.bn_fwd_fold(x, _fresh_slots(C), False, None, gamma, beta, None, None,
                                      0.1, EPS, True, False, None)
    yp_u, idx_u = nat.maxpool_fwd(y_u, 3, 2, 1, False, True)
    torch.cuda.synchronize()
    assert torch.equal(yp, yp_u) and torch.equal(idx, idx_u)
    assert torch.equal(stats, stats_u)

    dp = ko.bn_pool_dp(shape)
    yp_ref, tap, dz, ref = ko.bn_pool_ref(d, y_u.cpu(), dp)
    assert torch.equal(yp.cpu().double(), yp_ref)
    assert torch.equal(idx.cpu(), tap)
    # xm: the raw x of every window's winning tap (0 where no tap won)
    xp = torch.nn.functional.pad(d["x"].double(), (1, 1, 1, 1))
    Ho, Wo = tap.shape[2:]
    ho, wo = torch.arange(Ho).view(1, 1, Ho, 1), torch.arange(Wo).view(1, 1, 1, Wo)
    t = tap.long().clamp(max=8)
    flat = (ho * 2 + t // 3) * (W + 2) + (wo * 2 + t % 3)
    xm_ref = xp.reshape(N, C, -1).gather(2, flat.reshape(N, C, -1)).reshape(tap.shape)
    xm_ref = torch.where(tap == 255, torch.zeros_like(xm_ref), xm_ref)
    assert torch.equal(xm.cpu().double(), xm_ref)

    st = stats.cpu().double()
    fwd = dict(y=y_u.cpu(), mean=st[0], invstd=st[1], rmean=rm.cpu(), rvar=rv.cpu())
    dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    dx = nat.maxpool_bn_bwd(x, _dev(dp), idx, xm, gamma, stats, dg, db, bs, fs, 3, 2, 1)
    torch.cuda.synchronize()
    got = dict(fwd, dx=dx.cpu(), dgamma=dg.cpu(), dbeta=db.cpu())
    _finite(got)
    ko.bn_assert(ko.bn_errors(got, ref, M, True), regime, 1.0, f"stem {shape}")
    assert float(fs[:-TAIL].abs().max()) == 0.0          # zeroed by the backward apply
    # the unfused backward agrees: dy = maxpool_bwd(dp) stored as bf16
    dy_u = nat.maxpool_bwd(_dev(dp), idx_u, H, W, 3, 2, 1)
    assert torch.equal(dy_u.cpu().double(), ko.bf(dz))


# ------------------------------------------------------- domain edge, recorded
@pytest.mark.parametrize("regime", ("off16", "off64") + ko.BN_EDGE_REGIMES)
@pytest.mark.parametrize("cell", ["uneven", "wrap"])
def test_domain_edge_recorded(cell, regime):
    """var = Q/M - mean^2 in fp32 loses 2 log2(|mean|/sigma) bits: asserted up to
    64 (the tests above), recorded here at 256 and for a nearly constant channel,
    where the variance cancels to 0 or to twice its value.  Asserted: everything
    stays finite (the clamp max(var, 0)) and the kernel's invstd is no further
    from fp64 than 3x the emulation's on the same input."""
    shape = ko.BN_CELLS[cell]
    C, M = shape[1], _rows(shape)
    d = _inputs(shape, regime, 0)
    x, dy = _dev(d["x"]), _dev(d["dy"])
    gamma, beta = d["gamma"].cuda(), d["beta"].cuda()
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    fs, bs = _fresh_slots(C), _fresh_slots(C)
    nat = _nat()
    y, stats, _ = nat.bn_fwd_fold(x, fs, False, None, gamma, beta, rm, rv, 1.0, EPS, True, False,
                                  bs)
    dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    dx, _ = nat.bn_bwd_fold(x, dy, None, gamma, stats, dg, db, True, False, bs, None, fs)
    torch.cuda.synchronize()
    st = stats.cpu().double()
    _finite(dict(y=y, dx=dx, stats=stats, rm=rm, rv=rv, dg=dg, db=db))
    ref = ko.bn_ref(d["x"], d["gamma"], d["beta"], EPS, None, True)
    em = ko.bn_emul(d["x"], d["gamma"], d["beta"], EPS, None, True)
    e_k = ko.bn_stat_errs(st[0], st[1], ref)
    e_e = ko.bn_stat_errs(em["mean"], em["invstd"], ref)
    y_k = float((y.cpu().double() - ref["y"]).abs().max())
    y_e = float((em["y"] - ref["y"]).abs().max())
    print(f"domain {cell} {regime}: invstd rel err kernel {e_k[1]:.2e} emulation {e_e[1]:.2e}  "
          f"mean err/sigma kernel {e_k[0]:.2e}  max |y - ref| kernel {y_k:.3g} emulation {y_e:.3g}")
    assert e_k[1] <= 3 * e_e[1], (e_k, e_e)
