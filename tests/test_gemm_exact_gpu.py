"""Native MFMA GEMM (csrc/gemm.hip) on exact-integer operands (tests/exact_ints.py):
every mode, store epilogue and tile config compared with an fp64 matmul by
``torch.equal``, a mismatch reported by (row, column).

Operands are small integers, so every product and partial sum is an integer far
below 2^24 (fp32 accumulation exact in any order: MFMA order, split-K atomics,
slab reduce, BN partial slots) and every bf16 output an integer <= 256 (exact
store); both conditions are asserted on the reference of every case.

Shapes: tails in every dimension, at least two tiles and a partial last one per
dimension for the smallest tiles ((257, 136, 72)) and the 256-wide ones
((300, 256, 264)); MANY derives per config a grid of 17 x 16 tiles (more tiles
than CUs) of 3 k-tiles each, the last tile row and the last k-tile partial.
"""
import pytest
import torch

import exact_ints as ei

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(300, 256, 264), (257, 136, 72)]       # M, K, N (also read by test_exact_ints_cpu.py)
# small output, long reduction (the cfg 4 / 9 / -1 picks with 24-196 splits of
# test_small_output_long_reduction_wgrad): M, N, K, ldb
LONG_K = (16, 150, 6400, 152)
LONG_K_PICKS = [(4, 96), (9, 24), (-1, 196)]
STRIDED = (200, 256, 136, 520, 8)                # M, K, N, row stride of x's buffer, column offset
BN_SLOTS, BN_TAIL = 64, 4                        # csrc/bn_slots.h


def _nat():
    from distributed_ml_pytorch_amd.ops._ext import native

    return native()


def _cfgs(mode):
    nat = _nat()
    return [-1] + [c[0] for c in nat.gemm_configs() if nat.gemm_config_ok(mode, c[0])]


def _mm(a, b):
    """fp64 reference product on the GPU (exact for these integers)."""
    return a.double() @ b.double()


def fwd_operands(M, K, N, seed=11):
    g = ei.gen(seed)
    return dict(x=ei.sparse_ints((M, K), generator=g, **ei.ACT),
                w=ei.sparse_ints((N, K), generator=g, **ei.WGT),
                b=ei.sparse_ints((N,), generator=g, **ei.ADD),
                r=ei.sparse_ints((M, N), generator=g, **ei.ADD))


def dgrad_operands(M, K, N, seed=12):
    g = ei.gen(seed)
    return dict(dy=ei.sparse_ints((M, N), generator=g, **ei.ACT),
                w=ei.sparse_ints((N, K), generator=g, **ei.WGT),
                h=ei.sparse_ints((M, K), generator=g, **ei.ADD))


def wgrad_operands(M, K, N, seed=13):
    g = ei.gen(seed)
    return dict(x=ei.sparse_ints((M, K), generator=g, **ei.ACT),
                dy=ei.sparse_ints((M, N), generator=g, **ei.ACT),
                g0=ei.sparse_ints((N, K), generator=g, **ei.ADD),
                b0=ei.sparse_ints((N,), generator=g, **ei.ADD))


def _dev16(d):
    return {k: ei.to_bf16(v, device=DEV) for k, v in d.items()}


@pytest.mark.parametrize("M,K,N", SHAPES)
def test_fwd_exact(M, K, N):
    """Establishes the premise first (plain store, every config): a bf16 MFMA with
    fp32 accumulate reproduces integer dot products bit for bit.  Then bias +
    addend, ReLU, the pre-activation half of the GELU epilogue and the BN partial
    sums of the store epilogue."""
    nat = _nat()
    o = _dev16(fwd_operands(M, K, N))
    x, w, b, r = o["x"], o["w"], o["b"], o["r"]
    ref = _mm(x, w.t())
    ref_b = ref + b.double()
    ref_br = ref_b + r.double()
    for t in (ref, ref_b, ref_br):
        ei.assert_exact_range(t, "bf16", f"fwd {M}x{K}x{N}")
    s_ref = torch.stack([ref.sum(0), (ref * ref).sum(0)])
    ei.assert_exact_range(s_ref, "fp32", "fwd BN sums")
    assert float((ref != 0).double().mean()) > 0.3, "reference too sparse to catch a lost term"
    parts = 0
    for cfg in _cfgs(0):
        y = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        nat.gemm(0, 0, cfg, x, w, y)
        ei.assert_equal_located(y, ref, ("m", "n"), f"fwd plain cfg {cfg}")
        y = torch.empty_like(y)
        nat.gemm(0, 0, cfg, x, w, y, bias=b, aux=r)
        ei.assert_equal_located(y, ref_br, ("m", "n"), f"fwd bias+addend cfg {cfg}")
        y = torch.empty_like(y)
        nat.gemm(0, 0, cfg, x, w, y, bias=b, aux=r, relu=True)
        ei.assert_equal_located(y, ref_br.clamp_min(0), ("m", "n"), f"fwd relu cfg {cfg}")
        y = torch.empty_like(y)
        nat.gemm(0, 0, cfg, x, w, y, relu=True)
        ei.assert_equal_located(y, ref.clamp_min(0), ("m", "n"), f"fwd plain relu cfg {cfg}")
        y, g2 = torch.empty_like(y), torch.empty_like(y)
        nat.gemm(0, 1, cfg, x, w, y, c2=g2, bias=b)
        ei.assert_equal_located(y, ref_b, ("m", "n"), f"fwd gelu pre-activation cfg {cfg}")
        if cfg >= 0 and N % 8 == 0:
            part = torch.zeros(2 * BN_SLOTS * N + BN_TAIL, device=DEV)
            y = torch.empty_like(y)
            nat.gemm(0, 0, cfg, x, w, y, part=part)
            ei.assert_equal_located(y, ref, ("m", "n"), f"fwd +part cfg {cfg}")
            ei.assert_equal_located(ei.bn_sums(part, BN_SLOTS, N), s_ref, ("moment", "n"),
                                    f"fwd BN partial sums cfg {cfg}")
            parts += 1
    assert parts > 0


@pytest.mark.parametrize("M,K,N", SHAPES)
def test_dgrad_exact(M, K, N):
    """dX[M, K] = dY[M, N] @ W[N, K]: plain, addend, dReLU (epi 4), and W read
    through a row stride wider than its row (padded, and a width that is no
    multiple of 8 inside a padded row)."""
    nat = _nat()
    o = _dev16(dgrad_operands(M, K, N))
    dy, w, h = o["dy"], o["w"], o["h"]
    ref = _mm(dy, w)
    ref_a = ref + h.double()
    ref_r = ref * (h.double() > 0)
    for t in (ref, ref_a):
        ei.assert_exact_range(t, "bf16", f"dgrad {M}x{K}x{N}")
    wide = torch.zeros(N, K + 8, device=DEV, dtype=torch.bfloat16)
    wide[:, :K] = w
    wide[:, K:] = 3                      # padding a correct kernel never multiplies in
    Kc = K - 4                           # 8-column pieces: the last one runs into the padding
    for cfg in _cfgs(1):
        dx = torch.empty(M, K, device=DEV, dtype=torch.bfloat16)
        nat.gemm(1, 0, cfg, dy, w, dx)
        ei.assert_equal_located(dx, ref, ("m", "k"), f"dgrad plain cfg {cfg}")
        dx = torch.empty_like(dx)
        nat.gemm(1, 0, cfg, dy, w, dx, aux=h)
        ei.assert_equal_located(dx, ref_a, ("m", "k"), f"dgrad addend cfg {cfg}")
        dx = torch.empty_like(dx)
        nat.gemm(1, 4, cfg, dy, w, dx, aux=h)
        ei.assert_equal_located(dx, ref_r, ("m", "k"), f"dgrad drelu cfg {cfg}")
        dx = torch.empty_like(dx)
        nat.gemm(1, 0, cfg, dy, wide[:, :K], dx)
        ei.assert_equal_located(dx, ref, ("m", "k"), f"dgrad padded stride cfg {cfg}")
        dxc = torch.empty(M, Kc, device=DEV, dtype=torch.bfloat16)
        nat.gemm(1, 0, cfg, dy, w[:, :Kc], dxc)
        ei.assert_equal_located(dxc, ref[:, :Kc], ("m", "k"), f"dgrad width {Kc} cfg {cfg}")


@pytest.mark.parametrize("M,K,N", SHAPES)
@pytest.mark.parametrize("splits,slab", [(1, False), (3, False), (3, True)])
def test_wgrad_exact(M, K, N, splits, slab):
    """gW[N, K] += dY^T X and gb[N] += colsum(dY), called twice on a non-zero
    integer start: every config x split-K through atomics or the slab x both
    block -> (tile, k-range) deals."""
    nat = _nat()
    o = wgrad_operands(M, K, N)
    x, dy = ei.to_bf16(o["x"], device=DEV), ei.to_bf16(o["dy"], device=DEV)
    g0, b0 = o["g0"].to(DEV), o["b0"].to(DEV)
    ref_w = g0.double() + 2 * _mm(dy.t(), x)
    ref_b = b0.double() + 2 * dy.double().sum(0)
    ei.assert_exact_range(ref_w, "fp32", "wgrad")
    ei.assert_exact_range(ref_b, "fp32", "wgrad dbias")
    try:
        for xcd_k in (0, 1):
            nat.gemm_set_xcd_k(xcd_k)
            for cfg in _cfgs(2):
                g, gb = g0.clone(), b0.clone()
                for _ in range(2):
                    nat.gemm(2, 3, cfg, dy, x, g, dbias=gb, splits=splits, slab=slab)
                what = f"wgrad cfg {cfg} splits {splits} slab {slab} xcd_k {xcd_k}"
                ei.assert_equal_located(g, ref_w, ("n", "k"), what)
                ei.assert_equal_located(gb, ref_b, ("n",), what + " dbias")
    finally:
        nat.gemm_set_xcd_k(1)


def long_k_operands(seed=14):
    M, N, K, ldb = LONG_K
    g = ei.gen(seed)
    return dict(a=ei.sparse_ints((K, M), generator=g, **ei.ACT),
                b=ei.sparse_ints((K, ldb), generator=g, **ei.ACT),
                c0=ei.sparse_ints((M, N), generator=g, **ei.ADD),
                d0=ei.sparse_ints((M,), generator=g, **ei.ADD))


@pytest.mark.parametrize("cfg,splits", LONG_K_PICKS)
def test_wgrad_long_reduction_exact(cfg, splits):
    """Small output, 6400-row reduction split 24-196 ways, the second operand a
    150-column slice of 152-wide rows; accumulated twice with dbias."""
    nat = _nat()
    M, N, K, ldb = LONG_K
    o = long_k_operands()
    a = ei.to_bf16(o["a"], device=DEV)
    b = ei.to_bf16(o["b"], device=DEV)[:, :N]
    ref = o["c0"].to(DEV).double() + 2 * _mm(a.t(), b)
    ref_d = o["d0"].to(DEV).double() + 2 * a.double().sum(0)
    ei.assert_exact_range(ref, "fp32", "long-k wgrad")
    ei.assert_exact_range(ref_d, "fp32", "long-k dbias")
    try:
        for xcd_k in (0, 1):
            nat.gemm_set_xcd_k(xcd_k)
            c, d = o["c0"].to(DEV), o["d0"].to(DEV)
            for _ in range(2):
                nat.gemm(2, 3, cfg, a, b, c, dbias=d, splits=splits)
            what = f"long-k wgrad cfg {cfg} splits {splits} xcd_k {xcd_k}"
            ei.assert_equal_located(c, ref, ("m", "n"), what)
            ei.assert_equal_located(d, ref_d, ("m",), what + " dbias")
    finally:
        nat.gemm_set_xcd_k(1)


def test_strided_operands_exact():
    """Column slices of a wider buffer as the row-major operand, the addend and the
    output of the forward, and as dY of the data gradient."""
    nat = _nat()
    M, K, N, ld, off = STRIDED
    g = ei.gen(15)
    big = ei.to_bf16(ei.sparse_ints((M, ld), generator=g, **ei.ACT), device=DEV)
    w = ei.to_bf16(ei.sparse_ints((N, K), generator=g, **ei.WGT), device=DEV)
    x = big[:, off:off + K]
    ref = _mm(x, w.t())
    ei.assert_exact_range(ref, "bf16", "strided fwd")
    wd = ei.to_bf16(ei.sparse_ints((K, N), generator=g, **ei.WGT), device=DEV)
    ref_d = _mm(x, wd)                    # x as a [M, K] dY against W [K, N]
    ei.assert_exact_range(ref_d, "bf16", "strided dgrad")
    for cfg in _cfgs(0):
        y = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        nat.gemm(0, 0, cfg, x, w, y)
        ei.assert_equal_located(y, ref, ("m", "n"), f"strided fwd cfg {cfg}")
        ybig = torch.full((M, N + 16), 7.0, device=DEV, dtype=torch.bfloat16)
        nat.gemm(0, 0, cfg, x, w, ybig[:, 8:8 + N])
        ei.assert_equal_located(ybig[:, 8:8 + N], ref, ("m", "n"), f"strided output cfg {cfg}")
        assert bool((ybig[:, :8] == 7).all()) and bool((ybig[:, 8 + N:] == 7).all()), \
            f"cfg {cfg} wrote outside its output columns"
    for cfg in _cfgs(1):
        dx = torch.empty(M, N, device=DEV, dtype=torch.bfloat16)
        nat.gemm(1, 0, cfg, x, wd, dx)
        ei.assert_equal_located(dx, ref_d, ("m", "k"), f"strided dgrad cfg {cfg}")


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_many_tiles_exact(mode):
    """Per MFMA config a 17 x 16 tile grid (272 tiles: more than the chip has CUs,
    so blocks of several waves of the grid run back to back) of 3 k-tiles each,
    the last tile row and the last k-tile partial: sizes from the config table."""
    nat = _nat()
    info = {c[0]: c for c in nat.gemm_configs()}          # id, BM, BN, threads, stages, BK
    ran = 0
    for cfg in [c for c in _cfgs(mode) if c >= 0]:
        _, BM, BN, _, _, BK = info[cfg][:6]
        R = 2 * BK + 8                                    # reduction: 3 k-tiles, the last one 8 deep
        P, Q = 17 * BM - 5, 16 * BN                       # output rows, columns
        if mode == 2:
            P = 17 * BM - 8                               # k-strided operand: width % 8
        g = ei.gen(100 + cfg)
        if mode == 0:
            a = ei.to_bf16(ei.sparse_ints((P, R), generator=g, **ei.ACT), device=DEV)
            b = ei.to_bf16(ei.sparse_ints((Q, R), generator=g, **ei.WGT), device=DEV)
            bias = ei.to_bf16(ei.sparse_ints((Q,), generator=g, **ei.ADD), device=DEV)
            ref = _mm(a, b.t()) + bias.double()
            ei.assert_exact_range(ref, "bf16", f"many-tiles fwd cfg {cfg}")
            out = torch.empty(P, Q, device=DEV, dtype=torch.bfloat16)
            nat.gemm(0, 0, cfg, a, b, out, bias=bias)
        elif mode == 1:
            a = ei.to_bf16(ei.sparse_ints((P, R), generator=g, **ei.ACT), device=DEV)
            b = ei.to_bf16(ei.sparse_ints((R, Q), generator=g, **ei.WGT), device=DEV)
            ref = _mm(a, b)
            ei.assert_exact_range(ref, "bf16", f"many-tiles dgrad cfg {cfg}")
            out = torch.empty(P, Q, device=DEV, dtype=torch.bfloat16)
            nat.gemm(1, 0, cfg, a, b, out)
        else:
            a = ei.to_bf16(ei.sparse_ints((R, P), generator=g, **ei.ACT), device=DEV)
            b = ei.to_bf16(ei.sparse_ints((R, Q), generator=g, **ei.ACT), device=DEV)
            ref = 2 * _mm(a.t(), b) + 1
            ei.assert_exact_range(ref, "fp32", f"many-tiles wgrad cfg {cfg}")
            out = torch.ones(P, Q, device=DEV)
            nat.gemm(2, 3, cfg, a, b, out)
            nat.gemm(2, 3, cfg, a, b, out)
        ei.assert_equal_located(out, ref, ("row", "col"), f"many tiles mode {mode} cfg {cfg}")
        ran += 1
    assert ran > 0
