"""The one-pass stem backward kernels (csrc/conv_small.hip stem3_bn_bwd_kernel +
stem3_bn_bwd_finalize_kernel), called through their binding, against the fp64
oracle of tests/stem_bwd_oracle.py built from the kernel's own inputs: x0 and stats
as the native forward produced them, the mask from the native y > 0, dx unrounded.

Tolerance: row-relative error of dW, dgamma and dbeta <= 1e-4 -- about 10x the
worst cell of the fp32 CPU emulation (test_stem_bwd_identity_cpu.py; the kernel
sums across blocks by atomics, in another order than a matmul) and 30-200x below
the error of the two-kernel form, so a wrong or missing term fails.  Each cell also
runs that two-kernel form (bn_bwd_fold, then conv_small_wgrad) on the same inputs,
prints both errors and asserts fused <= unfused.
"""
import functools

import pytest
import torch

from stem_bwd_oracle import CELLS, oracle, row_rel_live, weight_cols

pytestmark = pytest.mark.gpu

CL = torch.channels_last
TOL = 1e-4
REGIMES = ["plain", "dc", "gamma", "beta_masked", "dy_zero", "zero_w_row"]
SLOT_FLOATS = 2 * 64 * 64 + 4


def _native():
    from distributed_ml_pytorch_amd.ops._ext import native
    return native()


def _scratch():
    return torch.zeros(_native().stem3_bn_bwd_scratch_floats(), dtype=torch.float32, device="cuda")


@functools.lru_cache(maxsize=None)
def _case(shape, regime):
    """Inputs through the native forward, and the fp64 oracle (computed once)."""
    N = _native()
    B, CI, H, W = shape
    g = torch.Generator().manual_seed(1000 * sum(shape) + REGIMES.index(regime))
    x = torch.randn(B, CI, H, W, generator=g) + (4.0 if regime == "dc" else 0.0)
    w = torch.randn(64, CI, 3, 3, generator=g) * 0.3
    gamma = 1.0 + 0.2 * torch.randn(64, generator=g)
    beta = 0.3 * torch.randn(64, generator=g)
    dy = torch.randn(B, 64, H, W, generator=g)
    if regime == "gamma":
        gamma = torch.randn(64, generator=g)
        gamma[::7] = 0.0
        gamma[1::7] = -gamma[1::7].abs() - 0.1
    if regime == "beta_masked":
        beta[::4] = -10.0
    if regime == "dy_zero":
        dy[:, 3::5] = 0.0
    if regime == "zero_w_row":
        w[5] = 0.0
        beta[5] = 0.5
    x = x.to("cuda", torch.bfloat16).contiguous(memory_format=CL)
    w16 = w.to("cuda", torch.bfloat16).contiguous(memory_format=CL)
    dy = dy.to("cuda", torch.bfloat16).contiguous(memory_format=CL)
    gamma, beta = gamma.cuda(), beta.cuda()
    slots = torch.zeros(SLOT_FLOATS, dtype=torch.float32, device="cuda")
    x0, part, _ = N.conv_small_fwd(x, w16, 1, 1, True, slots)
    y, stats, _ = N.bn_fwd_fold(x0, part, True, None, gamma, beta, None, None, 0.1, 1e-5, True,
                                False, None)
    torch.cuda.synchronize()
    st = stats.view(4, 64).cpu()
    ref = oracle(x.float().cpu(), x0.float().cpu(), dy.float().cpu(), (y > 0).float().cpu(),
                 st[0], st[1], gamma.cpu())
    return dict(x=x, x0=x0, dy=dy, stats=stats, gamma=gamma, part=part, ref=ref, CI=CI)


def _fused(c, dw=True, affine=True, scratch=None, calls=1, zero_buf=None):
    N = _native()
    gw = torch.zeros(64, c["CI"], 3, 3, dtype=torch.float32, device="cuda").contiguous(
        memory_format=CL) if dw else None
    dg = torch.zeros(64, device="cuda") if affine else None
    db = torch.zeros(64, device="cuda") if affine else None
    scratch = _scratch() if scratch is None else scratch
    for _ in range(calls):
        N.stem3_bn_bwd(c["dy"], c["x0"], c["x"], c["stats"], c["gamma"], dg, db, gw, scratch,
                       zero_buf)
    torch.cuda.synchronize()
    return gw, dg, db, scratch


def _unfused(c):
    N = _native()
    gw = torch.zeros(64, c["CI"], 3, 3, dtype=torch.float32, device="cuda").contiguous(
        memory_format=CL)
    dg, db = torch.zeros(64, device="cuda"), torch.zeros(64, device="cuda")
    bs = torch.zeros(SLOT_FLOATS, dtype=torch.float32, device="cuda")
    dx, _ = N.bn_bwd_fold(c["x0"], c["dy"], None, c["gamma"], c["stats"], dg, db, True, False, bs,
                          None, None)
    N.conv_small_wgrad(dx, c["x"], gw, 1, 1)
    torch.cuda.synchronize()
    return gw, dg, db


def _errors(out, ref, scale=1.0):
    gw, dg, db = out[:3]
    rw, rg, rb = ref
    return (row_rel_live(weight_cols(gw), scale * rw), row_rel_live(dg, scale * rg),
            row_rel_live(db, scale * rb))


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("shape", CELLS, ids=lambda s: "x".join(map(str, s)))
def test_against_fp64_and_two_kernel_form(shape, regime):
    c = _case(shape, regime)
    ef = _errors(_fused(c), c["ref"])
    eu = _errors(_unfused(c), c["ref"])
    print(f"{shape} {regime}: fused dW {ef[0]:.3e} dgamma {ef[1]:.3e} dbeta {ef[2]:.3e} | "
          f"two-kernel dW {eu[0]:.3e} dgamma {eu[1]:.3e} dbeta {eu[2]:.3e}")
    assert max(ef) <= TOL, ef
    assert ef[0] <= eu[0], (ef, eu)


@pytest.mark.parametrize("shape", [CELLS[0], CELLS[3]], ids=lambda s: "x".join(map(str, s)))
def test_two_calls_on_one_scratch_double_the_gradients(shape):
    """The finalize kernel re-zeroes the scratch: a second call adds exactly once more."""
    c = _case(shape, "plain")
    out = _fused(c, calls=2)
    assert max(_errors(out, c["ref"], scale=2.0)) <= TOL
    assert not bool(out[3].any()), "scratch not re-zeroed"


def test_graph_replays_equal_eager_calls():
    c = _case(CELLS[3], "dc")
    N = _native()
    gw = torch.zeros(64, c["CI"], 3, 3, dtype=torch.float32, device="cuda").contiguous(
        memory_format=CL)
    dg, db, scratch = torch.zeros(64, device="cuda"), torch.zeros(64, device="cuda"), _scratch()

    def call():
        N.stem3_bn_bwd(c["dy"], c["x0"], c["x"], c["stats"], c["gamma"], dg, db, gw, scratch, None)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call()                                   # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t in (gw, dg, db):
        t.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        call()
    for t in (gw, dg, db):
        t.zero_()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize()
    eager = _fused(c, calls=3)
    assert max(_errors((gw, dg, db), c["ref"], scale=3.0)) <= TOL
    assert max(_errors((gw, dg, db), (weight_cols(eager[0]).double().cpu(),
                                      eager[1].double().cpu(), eager[2].double().cpu()))) <= TOL
    assert not bool(scratch.any())


def test_frozen_parameters_are_skipped():
    c = _case(CELLS[2], "plain")
    gw, dg, db, _ = _fused(c, dw=False)
    assert gw is None
    assert row_rel_live(dg, c["ref"][1]) <= TOL and row_rel_live(db, c["ref"][2]) <= TOL
    gw, dg, db, _ = _fused(c, affine=False)
    assert dg is None and db is None
    assert row_rel_live(weight_cols(gw), c["ref"][0]) <= TOL


def test_forward_slot_sums_are_zeroed():
    c = _case(CELLS[4], "plain")
    part = torch.full((SLOT_FLOATS,), 3.0, dtype=torch.float32, device="cuda")
    _fused(c, zero_buf=part)
    assert not bool(part[:2 * 64 * 64].any())
