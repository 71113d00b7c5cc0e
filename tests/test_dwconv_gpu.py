"""Depthwise conv kernels (csrc/dwconv.hip) through ``ops.layers.Conv2d`` against
``F.conv2d(..., groups=C)`` in fp64 on the CPU over the same bf16-rounded operands.

Exact-integer operands (tests/exact_ints.py): ``y`` / ``dx`` are integers of
magnitude under 256 and ``dW`` / ``db`` sums far below 2^24, so every pass must be
``torch.equal``; with ``alias`` the layer hands its input back as a second output
and the gradient sent into it must arrive in ``dx`` (the data-gradient epilogue's
addend), again exactly.  Gaussian operands: one bf16 rounding plus fp32 accumulation in
any order, ``|y - ref| <= 2^-8 |ref| + K*K 2^-23 sum|x w|`` (the same for ``dx``) and
``|dW - ref| <= P 2^-23 sum|dy x|``, ``P = N H W``, right-hand sides on the reference.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import exact_ints as ei

pytestmark = [pytest.mark.gpu, pytest.mark.strict_native]

SHAPES = [      # (N, H, W, C)
    pytest.param((1, 1, 1, 8), id="1x1x1x8-all-padding"),
    pytest.param((2, 2, 3, 8), id="2x2x3x8-map-under-kernel"),
    pytest.param((1, 7, 7, 96), id="1x7x7x96-map-equals-kernel"),
    pytest.param((3, 9, 11, 40), id="3x9x11x40-ragged"),
    # W = 20 is one tile for every K (tiles are up to 32 columns wide); at 33 every kernel,
    # forward / dgrad and wgrad, has more than one tile along W for every K
    pytest.param((2, 33, 33, 136), id="2x33x33x136-multi-tile-W-33-not-20"),
]


@functools.lru_cache(maxsize=None)
def case(shape, K, kind, bias):
    """Operands (bf16-exact fp32) and fp64 references of one case, computed once."""
    N, H, W, C = shape
    g = ei.gen(1000 * K + H)
    if kind == "ints":
        x, dy = (ei.sparse_ints((N, C, H, W), generator=g, **ei.ACT) for _ in range(2))
        w = ei.sparse_ints((C, 1, K, K), generator=g, **ei.WGT)
        b = ei.sparse_ints((C,), generator=g, **ei.ADD) if bias else None
    else:
        x, dy = (torch.randn(N, C, H, W, generator=g).bfloat16().float() for _ in range(2))
        w = torch.randn(C, 1, K, K, generator=g).bfloat16().float()
        b = torch.randn(C, generator=g) if bias else None
    c = dict(x=x, w=w, b=b, dy=dy)
    for tag, f in (("", lambda t: t.double()), ("abs_", lambda t: t.double().abs())):
        xr, wr = f(x).requires_grad_(True), f(w).requires_grad_(True)
        br = f(b).requires_grad_(True) if bias else None
        y = F.conv2d(xr, wr, br, padding=K // 2, groups=C)
        y.backward(f(dy))
        c.update({tag + "y": y.detach(), tag + "dx": xr.grad, tag + "dw": wr.grad,
                  tag + "db": br.grad if bias else None})
    return c


def run_layer(c, K, xgrad, da=None):
    """(y, dx, dW, db) of the layer; ``da``: run with ``alias=True`` and send this
    gradient into the aliased input."""
    from distributed_ml_pytorch_amd.ops.layers import Conv2d

    C = c["w"].shape[0]
    layer = Conv2d(C, C, K, padding=K // 2, groups=C, bias=c["b"] is not None).cuda()
    with torch.no_grad():
        layer.weight.copy_(c["w"])
        if c["b"] is not None:
            layer.bias.copy_(c["b"])
    x = c["x"].cuda().bfloat16().contiguous(memory_format=torch.channels_last)
    x.requires_grad_(xgrad)
    if da is None:
        y = layer(x)
        y.backward(c["dy"].cuda().bfloat16())
    else:
        y, xa = layer(x, alias=True)
        torch.autograd.backward([y, xa], [c["dy"].cuda().bfloat16(), da.cuda().bfloat16()])
    return y.detach(), x.grad, layer.weight.grad, layer.bias.grad if c["b"] is not None else None


@pytest.mark.parametrize("bias,xgrad,alias", [(True, True, True), (False, True, False),
                                              (False, False, False)])
@pytest.mark.parametrize("K", [3, 5, 7])
@pytest.mark.parametrize("shape", SHAPES)
def test_exact_integer_operands(shape, K, bias, xgrad, alias):
    c = case(shape, K, "ints", bias)
    da, ref_dx = None, c["dx"]
    if alias:
        da = ei.sparse_ints(tuple(c["x"].shape), generator=ei.gen(7), **ei.ADD)
        ref_dx = c["dx"] + da.double()
    y, dx, dw, db = run_layer(c, K, xgrad, da)
    axes = ("n", "c", "h", "w")
    ei.assert_exact_range(c["y"], "bf16", "y")
    ei.assert_equal_located(y.float().cpu().double(), c["y"], axes, "y")
    if xgrad:
        ei.assert_exact_range(ref_dx, "bf16", "dx")
        ei.assert_equal_located(dx.float().cpu().double(), ref_dx, axes, "dx")
    else:
        assert dx is None
    ei.assert_exact_range(c["dw"], "fp32", "dw")
    assert dw.dtype == torch.float32
    ei.assert_equal_located(dw.cpu().double(), c["dw"], ("c", "one", "r", "s"), "dw")
    if bias:
        ei.assert_exact_range(c["db"], "fp32", "db")
        ei.assert_equal_located(db.cpu().double(), c["db"], ("c",), "db")


@pytest.mark.parametrize("bias,xgrad", [(True, True), (False, False)])
@pytest.mark.parametrize("K", [3, 5, 7])
@pytest.mark.parametrize("shape", SHAPES)
def test_gaussian_operands_within_derived_bounds(shape, K, bias, xgrad):
    c = case(shape, K, "gauss", bias)
    y, dx, dw, db = run_layer(c, K, xgrad)
    P = shape[0] * shape[1] * shape[2]

    def check(got, ref, bound, what):
        err = (got.cpu().double() - ref).abs()
        worst = float((err - bound).max())
        print(f"{what}: max err {float(err.max()):.3e}, max (err - bound) {worst:.3e}")
        assert worst <= 0, what

    check(y.float(), c["y"], 2.0 ** -8 * c["y"].abs() + K * K * 2.0 ** -23 * c["abs_y"], "y")
    if xgrad:
        check(dx.float(), c["dx"], 2.0 ** -8 * c["dx"].abs() + K * K * 2.0 ** -23 * c["abs_dx"],
              "dx")
    check(dw, c["dw"], P * 2.0 ** -23 * c["abs_dw"], "dw")
    if bias:
        check(db, c["db"], P * 2.0 ** -23 * c["abs_db"], "db")


def test_weight_gradient_is_bitwise_reproducible():
    from distributed_ml_pytorch_amd.ops._ext import native

    shape, K = (2, 33, 33, 136), 7
    assert min(native().dwconv_plan(shape[1], shape[2], shape[3], K)[3:6]) >= 2, "one tile"
    c = case(shape, K, "gauss", True)
    x, dy = (c[k].cuda().bfloat16().contiguous(memory_format=torch.channels_last)
             for k in ("x", "dy"))
    outs = []
    for _ in range(2):
        dw = torch.zeros(shape[3], 1, K, K, device="cuda")
        db = torch.zeros(shape[3], device="cuda")
        native().dwconv_wgrad(dy, x, dw, db)
        outs.append((dw, db))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_captured_step_survives_a_larger_no_grad_forward():
    """A captured forward + backward holds the layer's slab by address: an evaluation
    at a larger batch in between must neither replace it nor change the replayed dW."""
    from distributed_ml_pytorch_amd.ops.layers import Conv2d
    from distributed_ml_pytorch_amd.parallel.arena import attach_arena

    C, K = 64, 7
    c = case((2, 8, 8, C), K, "ints", True)
    layer = Conv2d(C, C, K, padding=K // 2, groups=C).cuda()
    with torch.no_grad():
        layer.weight.copy_(c["w"])
        layer.bias.copy_(c["b"])
    arena = attach_arena(layer, shadow_dtype=torch.bfloat16, channels_last=True)
    x = c["x"].cuda().bfloat16().contiguous(memory_format=torch.channels_last)
    dy = c["dy"].cuda().bfloat16().contiguous(memory_format=torch.channels_last)

    def step():            # the gradients accumulate straight into the arena
        layer(x).backward(dy)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):          # eager warm-up: the slab is allocated here
        step()
    torch.cuda.current_stream().wait_stream(side)
    slab = layer.__dict__["_dmp_dw_slab"]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        step()
    with torch.no_grad():                  # "evaluation": 64 images instead of 2
        layer(torch.randn(64, C, 8, 8, device="cuda").bfloat16().contiguous(
            memory_format=torch.channels_last))
    assert layer.__dict__["_dmp_dw_slab"] is slab
    junk = [torch.full((slab.numel(),), float("nan"), device="cuda") for _ in range(4)]
    for _ in range(2):
        arena.g32.fill_(0.0)
        g.replay()
        torch.cuda.synchronize()
        ei.assert_equal_located(layer.weight.grad.cpu().double(), c["dw"],
                                ("c", "one", "r", "s"), "dw")
        ei.assert_equal_located(layer.bias.grad.cpu().double(), c["db"], ("c",), "db")
    del junk


def test_depthwise_layer_stays_native():
    from distributed_ml_pytorch_amd.ops._policy import stock_allowed, stock_log
    from distributed_ml_pytorch_amd.ops.layers import Conv2d

    before = stock_log()
    with stock_allowed(False):
        layer = Conv2d(96, 96, 7, padding=3, groups=96).cuda()
        x = torch.randn(2, 96, 7, 7, device="cuda").bfloat16().contiguous(
            memory_format=torch.channels_last).requires_grad_(True)
        layer(x).float().sum().backward()
        with torch.no_grad():
            assert layer(x).grad_fn is None
    assert stock_log() == before
    assert x.grad is not None and layer.weight.grad is not None
