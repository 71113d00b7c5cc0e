"""CPU side of the exact-integer conv / GEMM tests (tests/exact_ints.py):

* the range conditions that make ``torch.equal`` legitimate, for every shape row
  of tests/test_conv_exact_gpu.py and tests/test_gemm_exact_gpu.py, on the
  operands those tests build (same seeds) and fp64 references;
* the mismatch locator, on reference copies with planted errors.
"""
import pytest
import torch

import exact_ints as ei
import test_conv_exact_gpu as tc
import test_gemm_exact_gpu as tg

_TOP: dict = {}


def _note(top):
    for k, v in top.items():
        _TOP[k] = max(_TOP.get(k, 0.0), v)


@pytest.mark.parametrize("row", tc.ALL_ROWS, ids=tc._ids(tc.ALL_ROWS))
def test_conv_reference_ranges(row):
    """forward, forward + bias + addend + ReLU, data gradient (+ addends), weight
    gradient after two accumulating calls on a non-zero integer start, bias
    gradient, and the per-channel sum / sum of squares: all inside the exact
    ranges; the operands survive the bf16 round trip."""
    c = ei.conv_case(row)
    for k in ("x", "w", "dy", "add_y", "add_x", "sub"):
        ei.to_bf16(c[k])
    top = ei.conv_case_ranges(c, row[6])
    _note(top)
    print(f"{row}: " + ", ".join(f"{k} {v:g}" for k, v in top.items()))
    # a lost contribution cannot hide among zeros: where the reduction is long
    # enough the references are mostly non-zero
    B, CI, H, W, CO, k, st, pd = row
    if c["y"].shape[0] * c["y"].shape[2] * c["y"].shape[3] >= 1024 and CI >= 64:
        assert float((c["dw"] != 0).double().mean()) > 0.6
    if CI * k * k >= 576:
        assert float((c["y"] != 0).double().mean()) > 0.6
        assert float((c["dx"] != 0).double().mean()) > 0.5


@pytest.mark.parametrize("M,K,N", tg.SHAPES)
def test_gemm_reference_ranges(M, K, N):
    o = tg.fwd_operands(M, K, N)
    for v in o.values():
        ei.to_bf16(v)
    y = o["x"].double() @ o["w"].double().t()
    top = {"gemm_fwd": ei.assert_exact_range(y + o["b"].double() + o["r"].double(), "bf16"),
           "gemm_bn_sums": ei.assert_exact_range(torch.stack([y.sum(0), (y * y).sum(0)]), "fp32")}
    ei.assert_exact_range(y, "bf16")
    ei.assert_exact_range(y + o["b"].double(), "bf16")
    o = tg.dgrad_operands(M, K, N)
    dx = o["dy"].double() @ o["w"].double()
    ei.assert_exact_range(dx, "bf16")
    top["gemm_dgrad"] = ei.assert_exact_range(dx + o["h"].double(), "bf16")
    o = tg.wgrad_operands(M, K, N)
    top["gemm_wgrad_twice"] = ei.assert_exact_range(
        o["g0"].double() + 2 * o["dy"].double().t() @ o["x"].double(), "fp32")
    ei.assert_exact_range(o["b0"].double() + 2 * o["dy"].double().sum(0), "fp32")
    _note(top)
    print(f"gemm {(M, K, N)}: " + ", ".join(f"{k} {v:g}" for k, v in top.items()))


def test_gemm_long_reduction_range():
    M, N, K, ldb = tg.LONG_K
    o = tg.long_k_operands()
    ref = o["c0"].double() + 2 * o["a"].double().t() @ o["b"].double()[:, :N]
    _note({"gemm_long_k_wgrad_twice": ei.assert_exact_range(ref, "fp32")})
    ei.assert_exact_range(o["d0"].double() + 2 * o["a"].double().sum(0), "fp32")


def test_zz_headroom_report():
    """prints the largest |value| per pass over the tables (run with -s)"""
    print("largest |reference| per pass: " + ", ".join(f"{k} {v:g}" for k, v in sorted(_TOP.items())))


# ------------------------------------------------------------------ the helpers
def test_sparse_ints_and_round_trip():
    g = ei.gen(3)
    t = ei.sparse_ints((64, 1000), -2, 2, 0.25, g)
    assert t.dtype == torch.float32 and bool((t == t.round()).all())
    assert float(t.min()) == -2 and float(t.max()) == 2
    nz = float((t != 0).float().mean())
    assert 0.18 < nz < 0.22, nz                    # 1/4 kept, 1/5 of those drew a zero
    d = ei.sparse_ints((1000,), -4, 4, 1.0, g)
    assert float(d.abs().max()) == 4
    assert torch.equal(ei.sparse_ints((5, 7), -2, 2, 0.25, ei.gen(9)),
                       ei.sparse_ints((5, 7), -2, 2, 0.25, ei.gen(9)))
    assert torch.equal(ei.to_bf16(t).float(), t)
    with pytest.raises(AssertionError, match="not exact in bf16"):
        ei.to_bf16(torch.tensor([257.0]))


def test_exact_range_rejects():
    ei.assert_exact_range(torch.tensor([256.0, -256.0, 0.0]), "bf16")
    ei.assert_exact_range(torch.tensor([2.0 ** 24 - 1]), "fp32")
    for bad, kind in ((torch.tensor([257.0]), "bf16"), (torch.tensor([0.5]), "bf16"),
                      (torch.tensor([2.0 ** 24], dtype=torch.float64), "fp32"),
                      (torch.tensor([float("nan")]), "fp32")):
        with pytest.raises(AssertionError):
            ei.assert_exact_range(bad, kind)


def test_bn_sums():
    part = torch.arange(2 * 4 * 3 + 4, dtype=torch.float32)
    s = ei.bn_sums(part, 4, 3)
    assert torch.equal(s, part[:24].view(2, 4, 3).sum(1))


# ------------------------------------------------------------------ the locator
def _msg(got, ref, axes):
    with pytest.raises(AssertionError) as e:
        ei.assert_equal_located(got, ref, axes, "planted")
    return str(e.value)


@pytest.mark.parametrize("channels_last", [False, True])
def test_locator_reports_planted_errors(channels_last):
    c = ei.conv_case((4, 64, 32, 32, 64, 3, 1, 1))

    def stored(t):
        t = t.to(torch.bfloat16)
        return t.contiguous(memory_format=torch.channels_last) if channels_last else t

    y, dw = c["y"], c["dw"]
    ax_y, ax_w = ("b", "co", "oh", "ow"), ("co", "ci", "r", "s")
    ei.assert_equal_located(stored(y), y, ax_y, "equal")
    ei.assert_equal_located(stored(y), stored(y).clone(), ax_y, "equal")
    # one element
    got = stored(y).clone()
    got[2, 5, 31, 7] += 1
    m = _msg(got, y, ax_y)
    assert "1 of %d elements" % y.numel() in m
    assert "all mismatches at b=2, co=5, oh=31, ow=7" in m
    want = float(y[2, 5, 31, 7])
    assert f"(b=2, co=5, oh=31, ow=7): got {want + 1:g} want {want:g}" in m
    # one whole tap of a weight gradient
    gw = dw.float()
    gw = gw.contiguous(memory_format=torch.channels_last) if channels_last else gw.clone()
    assert bool((dw[:, :, 0, 2] != 0).any())
    gw[:, :, 0, 2] = 0
    n = int((dw[:, :, 0, 2] != 0).sum())
    m = _msg(gw, dw, ax_w)
    assert f"{n} of {dw.numel()} elements" in m
    assert "all mismatches at r=0, s=2" in m
    # one image
    got = stored(y).clone()
    got[3] = 0
    m = _msg(got, y, ax_y)
    assert "all mismatches at b=3" in m
    assert f"{int((y[3] != 0).sum())} of {y.numel()}" in m
    # two columns of the last row: the set of indices per axis
    got = stored(y).clone()
    got[:, :, 31, 30:] += 2
    m = _msg(got, y, ax_y)
    assert "oh=31" in m and "ow in {30, 31}" in m
    # NaN and shape errors are mismatches too
    got = stored(y).clone()
    got[0, 0, 0, 0] = float("nan")
    assert "b=0, co=0, oh=0, ow=0" in _msg(got, y, ax_y)
    with pytest.raises(AssertionError):
        ei.assert_equal_located(stored(y)[:, :, :, :31], y, ax_y, "shape")
