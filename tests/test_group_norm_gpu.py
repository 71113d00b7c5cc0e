"""GroupNorm (+ residual) (+ ReLU) of csrc/group_norm.hip through ``group_norm_act``
against an fp64 oracle written as the formulas of the kernel header.

Bounds (the margin of the LAMB tests): the CPU path of ``ops/functional.py`` runs
on the same bf16 inputs and its largest absolute error against the oracle is
taken per tensor, ``E_cpu``.  bf16 outputs: within ``4 E_cpu + 1 bf16 ulp`` of the
oracle value; mean, rstd: ``4 E_cpu + 2^-22 |oracle|``; dgamma, dbeta: ``4 E_cpu +
P 2^-23 sum|terms|``, ``P = N H W``.  The rstd bound at ``randn + 32`` is the one
that tells centred from raw-moment variance: ``E[x^2] - mean^2`` in fp32 loses about
``2^-24 * 32^2 = 6e-5`` of a variance near 1, 250 times ``2^-22``, while the CPU
path's centred form sits at a few fp32 ulps.

The ReLU mask of the backward is the saved ``y > 0`` by specification, so the
oracle's backward takes the mask of the implementation it is compared with; a
pre-activation within rounding of zero is covered by the bound on ``y`` itself.
"""
import pytest
import torch

from distributed_ml_pytorch_amd.ops._policy import NativeCoverageError

pytestmark = [pytest.mark.gpu, pytest.mark.strict_native]

EPS = 1e-5
SMALL = [(2, 64, 4, 4, 32), (3, 32, 7, 7, 8), (2, 64, 5, 3, 8), (2, 96, 7, 7, 4),
         (1, 128, 2, 2, 1), (2, 16, 1, 1, 16)]
STREAM = (2, 64, 33, 17, 32)            # route forced: two parts, the last one ragged
LARGE = (1, 64, 112, 112, 32)           # streams by the planner's own choice
EPILOGUES = {"plain": (False, False), "relu": (True, False), "residual": (False, True),
             "residual_relu": (True, True)}
CASES = [(c, e, s) for c in SMALL for e in EPILOGUES for s in (0.0, 32.0)] + \
        [(c, "residual_relu", s) for c in (STREAM, LARGE) for s in (0.0, 32.0)]


def oracle(x, r, gamma, beta, dy, G, relu, mask=None):
    """fp64 forward, and the backward under ``mask`` (the saved y > 0) when given."""
    N, C, H, W = x.shape
    xg = x.double().reshape(N, G, -1)
    mean = xg.mean(-1)
    d = xg - mean[..., None]
    rstd = ((d * d).mean(-1) + EPS) ** -0.5
    xhat = (d * rstd[..., None]).reshape(x.shape)
    ga, be = gamma.double().view(1, C, 1, 1), beta.double().view(1, C, 1, 1)
    y = xhat * ga + be + (r.double() if r is not None else 0.0)
    out = {"y": y.clamp_min(0) if relu else y, "mean": mean, "rstd": rstd}
    if mask is None:
        return out
    dz = dy.double() * mask if relu else dy.double()
    t = dz * ga

    def gmean(v):
        return v.reshape(N, G, -1).mean(-1).repeat_interleave(C // G, 1).view(N, C, 1, 1)

    out["dx"] = rstd.repeat_interleave(C // G, 1).view(N, C, 1, 1) * (
        t - gmean(t) - xhat * gmean(t * xhat))
    out["dres"] = dz
    out["dbeta"], out["dbeta_abs"] = dz.sum((0, 2, 3)), dz.abs().sum((0, 2, 3))
    out["dgamma"], out["dgamma_abs"] = (dz * xhat).sum((0, 2, 3)), (dz * xhat).abs().sum((0, 2, 3))
    return out


def run(x, r, gamma, beta, dy, G, relu, dev):
    """``group_norm_act`` forward + backward on ``dev``: every output, on the CPU."""
    from distributed_ml_pytorch_amd.ops.functional import group_norm_act

    def leaf(t):            # a fresh leaf on dev (``.to`` of a CPU tensor is the tensor itself)
        fmt = torch.channels_last if t.dim() == 4 else torch.contiguous_format
        return t.to(dev).clone(memory_format=fmt).requires_grad_(True)

    xs, rs = leaf(x), leaf(r) if r is not None else None
    g, b = leaf(gamma), leaf(beta)
    y = group_norm_act(xs, G, g, b, EPS, relu=relu, residual=rs)
    y.backward(dy.to(dev))
    out = {"y": y.detach(), "dx": xs.grad, "dgamma": g.grad, "dbeta": b.grad}
    if rs is not None:
        out["dres"] = rs.grad
    return {k: v.cpu() for k, v in out.items()}


def bf16_ulp(v):
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -120))) - 7)


@pytest.mark.parametrize("cell,epilogue,shift", CASES,
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_group_norm_matches_fp64_oracle(cell, epilogue, shift, monkeypatch):
    from distributed_ml_pytorch_amd.ops._ext import native

    N, C, H, W, G = cell
    relu, has_res = EPILOGUES[epilogue]
    if cell == STREAM:
        monkeypatch.setenv("DMP_GN_ROUTE", "stream")
    plan = native().gn_plan(N, C, H, W, G, 1 if cell == STREAM else -1)
    if cell in (STREAM, LARGE):
        assert plan["route"] == "stream" and plan["parts"] >= 2
        assert cell == LARGE or (H * W) % plan["part_pixels"] != 0
    else:
        assert plan["route"] == "resident"

    g = torch.Generator().manual_seed(N * 1000 + C + H)
    x = (torch.randn(N, C, H, W, generator=g) + shift).bfloat16()
    r = torch.randn(N, C, H, W, generator=g).bfloat16() if has_res else None
    dy = torch.randn(N, C, H, W, generator=g).bfloat16()
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)

    cpu = run(x, r, gamma, beta, dy, G, relu, "cpu")
    xf = x.float().reshape(N, G, -1)                  # the CPU path's statistics
    cpu["mean"] = xf.mean(-1)
    dc = xf - cpu["mean"][..., None]
    cpu["rstd"] = torch.rsqrt((dc * dc).mean(-1) + EPS)
    gpu = run(x, r, gamma, beta, dy, G, relu, "cuda")
    _, stats = native().gn_fwd(x.cuda().contiguous(memory_format=torch.channels_last), None,
                               gamma.cuda(), beta.cuda(), G, EPS, False,
                               1 if plan["route"] == "stream" else -1)
    gpu["mean"], gpu["rstd"] = stats[0].cpu(), stats[1].cpu()

    ref_cpu = oracle(x, r, gamma, beta, dy, G, relu, mask=cpu["y"] > 0)
    ref = oracle(x, r, gamma, beta, dy, G, relu, mask=gpu["y"] > 0)
    P = N * H * W
    worst = {}
    for k, got in gpu.items():
        e_cpu = (cpu[k].double() - ref_cpu[k]).abs().max()
        if k in ("y", "dx", "dres"):
            slack = bf16_ulp(ref[k])
        elif k in ("mean", "rstd"):
            slack = 2.0 ** -22 * ref[k].abs()
        else:
            slack = P * 2.0 ** -23 * ref[k + "_abs"]
        ratio = (got.double() - ref[k]).abs() / (4 * e_cpu + slack + 1e-300)   # 0 / 0 -> 0
        worst[k] = float(ratio.max())
    print("worst native/bound", cell, epilogue, shift,
          " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert all(v <= 1.0 for v in worst.values()), worst
    if H * W == 1:                                        # variance 0: rstd = eps^-1/2 above
        assert torch.equal(gpu["dx"], torch.zeros_like(gpu["dx"]))


@pytest.mark.parametrize("cell,route", [((2, 96, 7, 7, 4), ""), (STREAM, "stream")])
def test_backward_repeats_bit_equal(cell, route, monkeypatch):
    monkeypatch.setenv("DMP_GN_ROUTE", route)
    N, C, H, W, G = cell
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, C, H, W, generator=g).bfloat16()
    r = torch.randn(N, C, H, W, generator=g).bfloat16()
    dy = torch.randn(N, C, H, W, generator=g).bfloat16()
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    a = run(x, r, gamma, beta, dy, G, True, "cuda")
    b = run(x, r, gamma, beta, dy, G, True, "cuda")
    assert all(torch.equal(a[k], b[k]) for k in a)


def test_refusals(monkeypatch):
    from distributed_ml_pytorch_amd.ops.functional import group_norm_act

    def gn(N, C, H, W, G, dtype=torch.bfloat16):
        x = torch.zeros(N, C, H, W, dtype=dtype, device="cuda")
        return group_norm_act(x, G, torch.ones(C, device="cuda"), torch.zeros(C, device="cuda"), EPS)

    from distributed_ml_pytorch_amd.ops._policy import stock_allowed

    with stock_allowed(False):                  # whatever process-wide switch an earlier test left
        with pytest.raises(NativeCoverageError):
            gn(2, 24, 4, 4, 8)                      # cpg 3
        with pytest.raises(NativeCoverageError):
            gn(2, 12, 4, 4, 3)                      # C % 8 != 0
        with pytest.raises(NativeCoverageError):
            gn(2, 64, 4, 4, 32, torch.float32)      # fp32 outside the oracle mode
    monkeypatch.setenv("DMP_GN_ROUTE", "resident")
    with pytest.raises(RuntimeError, match="resident"):
        gn(*LARGE)                              # a forced route is never replaced
