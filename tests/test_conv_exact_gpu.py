"""The conv kernel families on exact-integer operands (tests/exact_ints.py): every
pass of every config id the enumerators offer for a shape, compared with an fp64
CPU reference by ``torch.equal``; a mismatch is reported by its (b, c, h, w) or
(co, ci, r, s) coordinates.

With integer operands of magnitude <= 2 (weights <= 1) at density 1/4 every
partial sum is an integer far below 2^24 (fp32 exact in any order: MFMA order,
split-K atomics, slab reduce, BN slots) and every bf16 output an integer <= 256;
``exact_ints.conv_case_ranges`` asserts this on the references of every row (also
on the CPU, tests/test_exact_ints_cpu.py).  No element is masked out anywhere.

Shapes are the smallest at which each tile can still go wrong, derived from the
host-side planners (csrc/halo_plan.h halo_tiling / plan_s2 / plan_wgrad_halo and
the implicit-GEMM tile table, BM 64-256 x BN 64-128):

* row tiles (TB = 1) never straddle an image, so a partial last tile exists only
  for whole-image tiles (TB > 1): those rows have a B that is no multiple of the
  TBs that occur, and = 1 (mod TB) for at least one row of every config (8x8:
  2/4/8 images per tile -> B = 9, 5; 4x4: 4/8/16 -> B = 17; 7x7: 2/4/5/9/10 ->
  B = 11; 14x14 and 16x16: 2 -> B = 3; 5x7: 6/7 -> B = 8; 9x11: 2/4/5 -> B = 3),
  and B = 1 rows stand next to them (test_tables_give_every_config_its_edges);
* the halo weight gradient splits its tiles over blocks (plan_wgrad_halo): the
  rows give every variant more than one split (slab ids 3000+ are only offered
  then) and, for the smaller targets, several tiles per split;
* reduction channels of one, two and three 64-channel chunks (64, 128, 192) and
  more, CO != CI in most rows so that a swapped channel count cannot pass;
* implicit GEMM: B * OH * OW is no multiple of 64 / 128 / 256 and spans at least
  two 256-pixel tiles; odd 9 x 11 maps at stride 1 and 2, 1x1, 5x5.
"""
import pytest
import torch

import exact_ints as ei

pytestmark = pytest.mark.gpu
CL = torch.channels_last
DEV = "cuda"
BN_SLOTS, BN_TAIL = 64, 4            # csrc/bn_slots.h

# rows: B, CI, H, W, CO, k, stride, pad  (module level: tests/test_exact_ints_cpu.py
# builds the same operands and checks the range conditions without a GPU)
HALO_S1 = [
    (3, 64, 32, 32, 64, 3, 1, 1),      # persistent 64-channel ids 115-117; 12 tiles of 256
    (1, 64, 16, 16, 64, 3, 1, 1),      # B = 1: one 256-pixel tile / two of 128
    (3, 128, 16, 16, 64, 3, 1, 1),     # 512-pixel tile holds 2 images: one alone in the last
    (9, 256, 8, 8, 128, 3, 1, 1),      # 2 / 4 / 8 images per tile, one alone in the last
    (1, 192, 8, 8, 64, 3, 1, 1),       # B = 1, three chunks
    (5, 64, 8, 8, 64, 3, 1, 1),        # persistent id 116 on whole images: 2 per tile, one alone
    (3, 192, 4, 4, 128, 3, 1, 1),      # under-full whole-image tiles, three chunks
    (17, 512, 4, 4, 512, 3, 1, 1),     # ResNet-18 stage 4: 4 / 8 / 16 images per tile, one alone
    (1, 64, 4, 4, 192, 3, 1, 1),       # B = 1 on the position-major map
    (1, 64, 56, 56, 64, 3, 1, 1),      # 224-pixel tiles (4 rows of 56), 14 per image
    (2, 64, 56, 56, 128, 3, 1, 1),     # two images of them, CO != CI
    (1, 128, 28, 28, 128, 3, 1, 1),    # 7 / 4-row tiles of 28
    (3, 256, 14, 14, 64, 3, 1, 1),     # padded whole-image tiles (1 / 2 images)
    (11, 512, 7, 7, 128, 3, 1, 1),     # 2 / 4 / 5 / 9 / 10 images per tile
    (8, 64, 5, 7, 64, 3, 1, 1),        # odd map, 7 images per 256-pixel tile
    (3, 64, 9, 11, 128, 3, 1, 1),      # odd map, 2 / 4 / 5 images per tile
]
IGEMM = [
    (9, 64, 9, 11, 128, 3, 2, 1),      # odd stride 2: 5 x 6 outputs, M = 270
    (3, 128, 9, 11, 256, 3, 1, 1),     # M = 297, two 128-wide channel tiles
    (7, 192, 7, 7, 128, 1, 1, 0),      # 1x1, M = 343, three k chunks
    (9, 64, 9, 11, 128, 1, 2, 0),      # 1x1 / 2 (projection shortcut)
    (6, 64, 7, 7, 192, 5, 1, 2),       # 5x5 (AlexNet conv2 kind), M = 294
    (1, 64, 17, 19, 64, 3, 1, 1),      # B = 1, M = 323
]
S2 = [
    (5, 64, 16, 16, 128, 3, 2, 1),     # 8 x 8 class grid: 1 / 2 / 4 images per tile
    (17, 256, 8, 8, 512, 3, 2, 1),     # 4 x 4 class grid: 4 / 8 / 16 images per tile
    (5, 256, 16, 16, 256, 3, 2, 1),    # halo wgrad: 3 tiles of 128 over 2 splits
    (8, 64, 8, 8, 64, 3, 2, 1),        # 112-pixel tiles hold 7 class grids: one image alone
    (1, 128, 56, 56, 128, 3, 2, 1),    # 28-pixel class rows: the 112-pixel tiles
    (1, 128, 32, 32, 64, 3, 2, 1),     # B = 1, row tiles of the 16 x 16 class grid, 128-wide N tiles
]
GEMM1X1 = [
    (3, 256, 7, 7, 64, 1, 1, 0),
    (1, 64, 9, 11, 192, 1, 1, 0),
]
SMALL = [
    (5, 3, 9, 11, 64, 3, 1, 1),        # VALU kernels (stem3_route false), 495 pixels
    (3, 3, 8, 16, 64, 3, 1, 1),        # MFMA stem (stem3_route true), partial blocks
    (2, 1, 16, 8, 64, 3, 1, 1),        # MFMA stem with CI = 1
    (2, 3, 40, 36, 64, 7, 2, 3),       # 7x7 / 2 on the VALU kernels
    (3, 1, 28, 28, 128, 5, 1, 2),
]
STEM = [(1, 3, 8, 224, 64, 7, 2, 3), (2, 3, 8, 224, 64, 7, 2, 3)]
LAYER = [
    (3, 64, 16, 16, 128, 3, 1, 1),
    (3, 64, 16, 16, 128, 3, 2, 1),
    (3, 128, 7, 7, 64, 1, 1, 0),
]
ALL_ROWS = list(dict.fromkeys(HALO_S1 + IGEMM + S2 + GEMM1X1 + SMALL + STEM + LAYER))

AX_Y = ("b", "co", "oh", "ow")
AX_X = ("b", "ci", "h", "w")
AX_W = ("co", "ci", "r", "s")
_DEVCASE: dict = {}


def _ids(rows):
    return ["x".join(str(v) for v in r) for r in rows]


@pytest.fixture(scope="module")
def nat():
    from distributed_ml_pytorch_amd.ops._ext import native

    return native()


class _Switch:
    """conv_halo_pm(on) for the duration of a block, the previous value restored"""

    def __init__(self, nat, on):
        self.nat, self.on = nat, on

    def __enter__(self):
        self.prev = self.nat.conv_halo_pm(self.on)

    def __exit__(self, *exc):
        self.nat.conv_halo_pm(self.prev)


def _case(row):
    """The row's reference (range-checked) and its operands on the GPU: bf16
    channels_last activations / weights, fp32 bias and gradient start values,
    fp64 references.  Built once per row."""
    if row in _DEVCASE:
        return _DEVCASE[row]
    c = ei.conv_case(row)
    ei.conv_case_ranges(c, row[6])
    d = {}
    for k in ("x", "w", "dy", "add_y", "add_x", "sub"):
        d[k] = ei.to_bf16(c[k], channels_last=True, device=DEV)
    d["bias"] = c["bias"].to(DEV)
    d["b0"] = c["b0"].to(DEV)
    d["g0"] = c["g0"].to(DEV).contiguous(memory_format=CL)
    for k in ("y", "y_epi", "sums", "dx", "dx_add", "dx_sub", "dw2", "db1"):
        d[k] = c[k].to(DEV)
    _DEVCASE[row] = d
    return d


def _pm_states(row):
    """both states of the position-major switch on 4 x 4 maps, else the default"""
    return (True, False) if (row[2], row[3]) == (4, 4) else (None,)


class _Pm:
    def __init__(self, nat, on):
        self.sw = _Switch(nat, on) if on is not None else None

    def __enter__(self):
        if self.sw is not None:
            self.sw.__enter__()

    def __exit__(self, *exc):
        if self.sw is not None:
            self.sw.__exit__(*exc)


def _check_fwd(nat, row, d, cfgs, tag):
    B, CI, H, W, CO, k, st, pd = row
    for cfg in cfgs:
        y, part, G = nat.conv_fwd(d["x"], d["w"], st, pd, True, cfg)
        ei.assert_equal_located(y, d["y"], AX_Y, f"{tag} fwd cfg {cfg}")
        ei.assert_equal_located(ei.bn_sums(part, G, CO), d["sums"], ("moment", "co"),
                                f"{tag} fwd BN partial sums cfg {cfg}")
        y2, _, _ = nat.conv_fwd(d["x"], d["w"], st, pd, False, cfg, None, d["bias"], True,
                                d["add_y"])
        ei.assert_equal_located(y2, d["y_epi"], AX_Y, f"{tag} fwd bias+addend+relu cfg {cfg}")


def _check_dgrad(nat, row, d, cfgs, tag):
    B, CI, H, W, CO, k, st, pd = row
    for cfg in cfgs:
        dx = nat.conv_dgrad(d["dy"], d["w"], H, W, st, pd, cfg)
        ei.assert_equal_located(dx, d["dx"], AX_X, f"{tag} dgrad cfg {cfg}")
        dxa = nat.conv_dgrad(d["dy"], d["w"], H, W, st, pd, cfg, None, d["add_x"])
        ei.assert_equal_located(dxa, d["dx_add"], AX_X, f"{tag} dgrad + addend cfg {cfg}")
        if st == 2:
            dxs = nat.conv_dgrad(d["dy"], d["w"], H, W, st, pd, cfg, addend=d["sub"],
                                 addend_sub=True)
            ei.assert_equal_located(dxs, d["dx_sub"], AX_X,
                                    f"{tag} dgrad + subsampled addend cfg {cfg}")


def _check_wgrad(nat, row, d, cfgs, tag):
    """accumulated twice into the non-zero integer start g0"""
    B, CI, H, W, CO, k, st, pd = row
    for cfg in cfgs:
        dw = d["g0"].clone(memory_format=torch.preserve_format)
        nat.conv_wgrad(d["dy"], d["x"], dw, st, pd, cfg)
        nat.conv_wgrad(d["dy"], d["x"], dw, st, pd, cfg)
        ei.assert_equal_located(dw, d["dw2"], AX_W, f"{tag} wgrad x2 cfg {cfg}")


# ------------------------------------------------------------ 3x3 / 1 halo tiles
@pytest.mark.parametrize("row", HALO_S1, ids=_ids(HALO_S1))
def test_halo_fwd(nat, row):
    B, CI, H, W, CO, k, st, pd = row
    d = _case(row)
    cfgs = list(nat.conv_halo_configs(H, W, CI, 3, 3, 1, 1))
    assert cfgs, "no halo config applies"
    for on in _pm_states(row):
        with _Pm(nat, on):
            _check_fwd(nat, row, d, cfgs, f"halo pm={on}")


@pytest.mark.parametrize("row", HALO_S1, ids=_ids(HALO_S1))
def test_halo_dgrad(nat, row):
    B, CI, H, W, CO, k, st, pd = row
    d = _case(row)
    cfgs = list(nat.conv_halo_configs(H, W, CO, 3, 3, 1, 1))     # gathers dY: CO channels
    assert cfgs, "no halo config applies"
    for on in _pm_states(row):
        with _Pm(nat, on):
            _check_dgrad(nat, row, d, cfgs, f"halo pm={on}")


def _wh_ids(nat, row):
    B, CI, H, W, CO, k, st, pd = row
    return list(nat.conv_wgrad_halo_configs(B, H, W, CI, CO, 3, 3, st, pd))


@pytest.mark.parametrize("row", HALO_S1 + S2, ids=_ids(HALO_S1 + S2))
def test_halo_wgrad(nat, row):
    """halo weight gradient at stride 1 and 2: atomic (1000+) and slab (3000+) ids"""
    d = _case(row)
    cfgs = _wh_ids(nat, row)
    assert cfgs, "no halo wgrad config applies"
    _check_wgrad(nat, row, d, cfgs, "halo")


# --------------------------------------------------------- implicit-GEMM tiles
_ROWS_IDS = (24, 25, 26, 27)        # row-staged epilogue: forward and stride-1 dgrad only


@pytest.mark.parametrize("row", IGEMM, ids=_ids(IGEMM))
def test_igemm_fwd_dgrad(nat, row):
    d = _case(row)
    ids = [c[0] for c in nat.conv_configs()]
    _check_fwd(nat, row, d, ids, "igemm")
    _check_dgrad(nat, row, d, [c for c in ids if row[6] == 1 or c not in _ROWS_IDS], "igemm")


@pytest.mark.parametrize("row", IGEMM, ids=_ids(IGEMM))
def test_igemm_wgrad(nat, row):
    from distributed_ml_pytorch_amd.ops.conv import _wgrad_candidates

    B, CI, H, W, CO, k, st, pd = row
    d = _case(row)
    cands = _wgrad_candidates(CI * k * k, CO)
    assert cands
    _check_wgrad(nat, row, d, cands, "igemm")
    for cfg in (cands[0], cands[-1]):           # the fused bias-gradient variant
        dw = d["g0"].clone(memory_format=torch.preserve_format)
        db = d["b0"].clone()
        nat.conv_wgrad(d["dy"], d["x"], dw, st, pd, cfg, db)
        nat.conv_wgrad(d["dy"], d["x"], dw, st, pd, cfg)
        ei.assert_equal_located(dw, d["dw2"], AX_W, f"igemm wgrad + dbias cfg {cfg}")
        ei.assert_equal_located(db, d["db1"], ("co",), f"igemm dbias cfg {cfg}")


# --------------------------------------------------- 3x3 / 2 parity-class dgrad
@pytest.mark.parametrize("row", S2, ids=_ids(S2))
def test_s2_dgrad(nat, row):
    B, CI, H, W, CO, k, st, pd = row
    d = _case(row)
    cfgs = list(nat.conv_dgrad_s2_configs(H, W, H // 2, W // 2, CO, CI, 3, 3, 2, 1))
    assert cfgs, "no stride-2 halo config applies"
    _check_dgrad(nat, row, d, cfgs, "s2")


# ------------------------------------------------------------ 1x1 GEMM route
@pytest.mark.parametrize("row", GEMM1X1, ids=_ids(GEMM1X1))
def test_gemm1x1_route(row):
    from distributed_ml_pytorch_amd.ops import conv as C

    B, CI, H, W, CO, k, st, pd = row
    d = _case(row)
    part = torch.zeros(2 * C.BN_SLOTS * CO + C.BN_TAIL, device=DEV)
    y = C._gemm1x1_fwd(d["x"], d["w"], part)
    ei.assert_equal_located(y, d["y"], AX_Y, "gemm1x1 fwd")
    ei.assert_equal_located(ei.bn_sums(part, C.BN_SLOTS, CO), d["sums"], ("moment", "co"),
                            "gemm1x1 BN partial sums")
    ei.assert_equal_located(C._gemm1x1_dgrad(d["dy"], d["w"]), d["dx"], AX_X, "gemm1x1 dgrad")
    ei.assert_equal_located(C._gemm1x1_dgrad(d["dy"], d["w"], d["add_x"]), d["dx_add"], AX_X,
                            "gemm1x1 dgrad + addend")
    g = d["g0"].clone(memory_format=torch.preserve_format)
    C._gemm1x1_wgrad(d["dy"], d["x"], g)
    C._gemm1x1_wgrad(d["dy"], d["x"], g)
    ei.assert_equal_located(g, d["dw2"], AX_W, "gemm1x1 wgrad x2")


# --------------------------------------------------- few-channel and stem kernels
@pytest.mark.parametrize("row", SMALL, ids=_ids(SMALL))
def test_small_conv(nat, row):
    B, CI, H, W, CO, k, st, pd = row
    d = _case(row)
    for name, x in (("channels_last", d["x"]), ("nchw", d["x"].contiguous())):
        y, part, G = nat.conv_small_fwd(x, d["w"], st, pd, True)
        ei.assert_equal_located(y, d["y"], AX_Y, f"small fwd {name}")
        ei.assert_equal_located(ei.bn_sums(part, G, CO), d["sums"], ("moment", "co"),
                                f"small BN partial sums {name}")
        dw = d["g0"].clone(memory_format=torch.preserve_format)
        nat.conv_small_wgrad(d["dy"], x, dw, st, pd)
        nat.conv_small_wgrad(d["dy"], x, dw, st, pd)
        ei.assert_equal_located(dw, d["dw2"], AX_W, f"small wgrad x2 {name}")


def test_small_table_covers_both_routes(nat):
    routes = {bool(nat.stem3_route(r[1], r[5], r[5], r[4], r[6], r[7], r[3])) for r in SMALL}
    assert routes == {True, False}


@pytest.mark.parametrize("row", STEM, ids=_ids(STEM))
def test_stem(nat, row):
    B, CI, H, W, CO, k, st, pd = row
    assert nat.stem_supported(H, W)
    d = _case(row)
    y, part, xs = nat.stem_fwd(d["x"], d["w"], True)
    ei.assert_equal_located(y, d["y"], AX_Y, "stem fwd")
    ei.assert_equal_located(ei.bn_sums(part, 64, 64), d["sums"], ("moment", "co"),
                            "stem BN partial sums")
    dw = d["g0"].clone(memory_format=torch.preserve_format)
    nat.stem_wgrad(d["dy"], xs, dw)
    nat.stem_wgrad(d["dy"], xs, dw)
    ei.assert_equal_located(dw, d["dw2"], AX_W, "stem wgrad x2")


# ------------------------------------------------------------------ layer level
@pytest.mark.parametrize("row", LAYER, ids=_ids(LAYER))
def test_layer_tuner_picks(row):
    """ops.layers.Conv2d forward + backward through the tuner's own picks, integer
    master weights behind a FlatArena shadow."""
    from distributed_ml_pytorch_amd.ops import layers as L
    from distributed_ml_pytorch_amd.parallel.arena import FlatArena

    B, CI, H, W, CO, k, st, pd = row
    c = ei.conv_case(row)
    d = _case(row)
    conv = L.Conv2d(CI, CO, k, stride=st, padding=pd, bias=False).cuda()
    with torch.no_grad():
        conv.weight.copy_(c["w"])
    FlatArena(conv, device=DEV)
    ei.assert_equal_located(conv.weight._dmp_w16.float(), c["w"], AX_W, "layer bf16 shadow")
    x = d["x"].clone(memory_format=torch.preserve_format).requires_grad_(True)
    y = conv(x)
    ei.assert_equal_located(y, d["y"], AX_Y, "layer fwd")
    y.backward(d["dy"])
    ei.assert_equal_located(x.grad, d["dx"], AX_X, "layer x.grad")
    ei.assert_equal_located(conv.weight.grad, c["dw"], AX_W, "layer weight.grad")


# --------------------------------------------------------------- coverage check
# (B, CI, H, W, CO, k, stride, pad) of every conv the native MFMA path runs:
# ResNet-18 on CIFAR (batch 128) and ResNet-50 v1.5 on 224 x 224 (batch 32); the
# stride-2 1x1 projection shortcuts run at stride 1 on the subsampled alias
def _workload_rows():
    rows = []
    Bc, Bi = 128, 32
    for c, h in ((64, 32), (128, 16), (256, 8), (512, 4)):
        rows.append((Bc, c, h, h, c, 3, 1, 1))
        if c > 64:
            rows.append((Bc, c // 2, 2 * h, 2 * h, c, 3, 2, 1))
            rows.append((Bc, c // 2, h, h, c, 1, 1, 0))
    for p, h, cin in ((64, 56, 64), (128, 28, 256), (256, 14, 512), (512, 7, 1024)):
        hin = h if p == 64 else 2 * h
        rows.append((Bi, cin, hin, hin, p, 1, 1, 0))            # first block's conv1
        rows.append((Bi, 4 * p, h, h, p, 1, 1, 0))              # later blocks' conv1
        rows.append((Bi, p, h, h, p, 3, 1, 1))
        if p > 64:
            rows.append((Bi, p, 2 * h, 2 * h, p, 3, 2, 1))
        rows.append((Bi, p, h, h, 4 * p, 1, 1, 0))              # conv3
        rows.append((Bi, cin, h, h, 4 * p, 1, 1, 0))            # projection shortcut
    return rows


def _offered(nat, row):
    """ids the tuner's enumerators (ops/conv.py _fwd_cfg / _dgrad_cfg / _wgrad_cfg)
    offer for one layer, per pass (the GEMM route aside)"""
    from distributed_ml_pytorch_amd.ops import conv as C

    B, CI, H, W, CO, k, st, pd = row
    OH, OW = (H + 2 * pd - k) // st + 1, (W + 2 * pd - k) // st + 1
    fwd = set(C._igemm_candidates(CO)) | set(nat.conv_halo_configs(H, W, CI, k, k, st, pd))
    dg = set(C._igemm_candidates(CI, fwd=st == 1))
    if (OH, OW) == (H, W):
        dg |= set(nat.conv_halo_configs(H, W, CO, k, k, st, pd))
    elif st == 2:
        dg |= set(nat.conv_dgrad_s2_configs(H, W, OH, OW, CO, CI, k, k, st, pd))
    wg = set(C._wgrad_candidates(CI * k * k, CO))
    wg |= set(nat.conv_wgrad_halo_configs(B, H, W, CI, CO, k, k, st, pd))
    return {"fwd": fwd, "dgrad": dg, "wgrad": wg}


def _exercised(nat):
    """ids the tests above run, per pass, from the same tables and enumerators"""
    from distributed_ml_pytorch_amd.ops import conv as C

    ids = {c[0] for c in nat.conv_configs()}
    ex = {"fwd": set(ids), "dgrad": set(), "wgrad": set()}
    for r in IGEMM:
        ex["dgrad"] |= {c for c in ids if r[6] == 1 or c not in _ROWS_IDS}
        ex["wgrad"] |= set(C._wgrad_candidates(r[1] * r[5] * r[5], r[4]))
    for r in HALO_S1:
        ex["fwd"] |= set(nat.conv_halo_configs(r[2], r[3], r[1], 3, 3, 1, 1))
        ex["dgrad"] |= set(nat.conv_halo_configs(r[2], r[3], r[4], 3, 3, 1, 1))
    for r in S2:
        ex["dgrad"] |= set(nat.conv_dgrad_s2_configs(r[2], r[3], r[2] // 2, r[3] // 2, r[4], r[1],
                                                     3, 3, 2, 1))
    for r in HALO_S1 + S2:
        ex["wgrad"] |= set(_wh_ids(nat, r))
    return ex


# ------------------------------------------- what the tables give each config
# Python mirror of csrc/halo_plan.h (halo_tiling, the BM of each halo id, the
# split rule of plan_wgrad_halo); the plans themselves are pinned by
# tests/golden/halo_plans.txt, and an id the mirror gets wrong would show up
# below as an id the enumerator offers although the mirror finds no tiling.
_HALO_BM = {100: 256, 101: 128, 102: 64, 103: 128, 104: 256, 105: 128, 106: 256, 107: 64,
            108: 128, 109: 256, 110: 256, 111: 128, 112: 128, 113: 256, 114: 512, 115: 256,
            116: 128, 117: 256, 118: 224, 119: 224, 120: 112, 121: 112, 122: 112, 123: 448,
            124: 224, 125: 112}
_S2_BM = {200: 128, 201: 256, 202: 128, 203: 256, 204: 64, 205: 112, 206: 256, 207: 128,
          208: 128, 209: 112}
_WH_TR = (1, 1, 1, 3, 3, 1, 1, 1)
_WH_BM = (0, 0, 0, 0, 0, 0, 224, 224)


def _tiling(bm, H, W, padded):
    """(TH, TB, MV) of a bm-pixel tile on an H x W map, or None"""
    img = H * W
    if bm <= img:
        TB, TH = 1, bm // W
        while TH > 0 and img % (TH * W):
            TH -= 1
        if TH == 0:
            return None
    else:
        TH, TB = H, bm // img
    MV = TB * TH * W
    return (TH, TB, MV) if (8 * (bm - MV) <= bm if padded else MV == bm) else None


def _wh_split(cfg, row):
    """(variant, BM, splits, tiles per split) of a halo weight-gradient id"""
    B, CI, H, W, CO, k, st, pd = row
    i = cfg % 1000
    var, rest = i // 12, i % 12
    bm = _WH_BM[var] or 64 << (rest // 4)
    if st == 2:
        H, W = H // 2, W // 2
    TH, TB, MV = _tiling(bm, H, W, True)
    ntiles = -(-B * H * W // MV)
    per = (CI // 64) * (CO // 64) * (3 // _WH_TR[var])
    sp = min(max((128 << (rest % 4)) // per, 1), ntiles)
    tps = -(-ntiles // sp)
    return var, bm, -(-ntiles // tps), tps


def test_tables_give_every_config_its_edges(nat):
    """Host side only.  Every halo-family id the tables exercise meets, in some row:
    B = 1; and, where the id ever tiles whole images (TB > 1), a batch that leaves
    one image alone in the last tile.  Every halo weight-gradient tile (variant,
    BM) runs with more than one split and with several tiles per split, slab ids
    included.  Reduction channels of one, two and three chunks, CO != CI."""
    seen = {}
    for r in HALO_S1:
        B, CI, H, W, CO = r[:5]
        for C in (CI, CO):
            for cfg in nat.conv_halo_configs(H, W, C, 3, 3, 1, 1):
                t = _tiling(_HALO_BM[cfg], H, W, not 115 <= cfg <= 117)
                assert t is not None, (cfg, r)
                seen.setdefault(cfg, []).append((B, t[1]))
    for r in S2:
        B, CI, H, W, CO = r[:5]
        for cfg in nat.conv_dgrad_s2_configs(H, W, H // 2, W // 2, CO, CI, 3, 3, 2, 1):
            t = _tiling(_S2_BM[cfg], H // 2, W // 2, False)
            assert t is not None, (cfg, r)
            seen.setdefault(cfg, []).append((B, t[1]))
    for cfg, uses in seen.items():
        assert any(B == 1 for B, _ in uses), f"cfg {cfg}: no B = 1 row"
        if any(TB > 1 for _, TB in uses):
            assert any(TB > 1 and B > TB and B % TB == 1 for B, TB in uses), \
                f"cfg {cfg}: no row leaves one image alone in the last tile: {uses}"
    tiles = {}
    for r in HALO_S1 + S2:
        for cfg in _wh_ids(nat, r):
            var, bm, splits, tps = _wh_split(cfg, r)
            t = tiles.setdefault((r[6], var, bm), dict(split=False, deep=False, slab=False))
            t["split"] |= splits > 1
            t["deep"] |= splits > 1 and tps >= 2
            t["slab"] |= cfg >= 3000
            assert cfg < 3000 or splits > 1, (cfg, r)
    for key, t in tiles.items():
        assert t["split"] and t["deep"], (key, t)
        assert t["slab"] == (key[1] in (0, 5, 6)), (key, t)
    rows = HALO_S1 + IGEMM + S2
    assert {64, 128, 192} <= {r[1] for r in rows}
    assert sum(r[1] != r[4] for r in rows) > len(rows) // 2


# ids offered at workload size that no small geometry can reach, with the reason
# (none: every tile family, the 224-pixel row tiles included, fits a B <= 2 map)
WORKLOAD_ONLY: dict = {"fwd": {}, "dgrad": {}, "wgrad": {}}


def test_table_covers_workload_configs(nat):
    """Host-side enumerators only (no kernel launch): every config id offered for a
    real ResNet-18 (CIFAR, batch 128) or ResNet-50 (224 x 224, batch 32) layer is
    exercised by this module's tables for the same pass."""
    ex = _exercised(nat)
    missing = {}
    for row in _workload_rows():
        for p, offered in _offered(nat, row).items():
            gap = offered - ex[p] - set(WORKLOAD_ONLY[p])
            if gap:
                missing[(p, row)] = sorted(gap)
    assert not missing, missing
    # the tables reach both kinds of halo weight-gradient id and every family
    assert any(i >= 3000 for i in ex["wgrad"]) and any(1000 <= i < 3000 for i in ex["wgrad"])
    assert {115, 116, 117} <= ex["fwd"] and {115, 116, 117} <= ex["dgrad"]
    assert any(200 <= i < 300 for i in ex["dgrad"])
