"""Layer-scale residual add (csrc/layer_scale.hip) against its CPU expression
``(x.float() + (gamma * r.float()) * s).to(bf16)``: the rounding is pinned, so ``h``
and ``dr`` match bit for bit with any operands; ``dgamma`` is exact with integer
operands and within ``P 2^-23 sum|dh r s|`` (fp32 accumulation in any order over
the ``P`` rows) with Gaussians.
"""
import pytest
import torch

import exact_ints as ei

pytestmark = [pytest.mark.gpu, pytest.mark.strict_native]

SHAPES = [(3, 8), (2, 5, 7, 40), (4, 49, 96)]      # leading dim = samples, last = C
SCALES = {"unscaled": None, "scaled": (0.0, 1.0, 2.0)}


def operands(shape, kind, scaled):
    g = ei.gen(sum(shape))
    C = shape[-1]
    if kind == "ints":
        x, r, dh = (ei.sparse_ints(shape, generator=g, **ei.ADD).bfloat16() for _ in range(3))
        gamma = ei.sparse_ints((C,), generator=g, **ei.ADD)
    else:
        x, r, dh = (torch.randn(shape, generator=g).bfloat16() for _ in range(3))
        gamma = torch.randn(C, generator=g)
    s = None
    if scaled:
        s = torch.tensor([SCALES["scaled"][b % 3] for b in range(shape[0])])
    return x, r, dh, gamma, s


@pytest.mark.parametrize("kind", ["ints", "gauss"])
@pytest.mark.parametrize("variant", list(SCALES))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_layer_scale_add_matches_cpu_expression(shape, variant, kind):
    from distributed_ml_pytorch_amd.ops.functional import layer_scale_add

    x, r, dh, gamma, s = operands(shape, kind, variant == "scaled")
    sv = s.view(-1, *([1] * (len(shape) - 1))) if s is not None else None
    # CPU: the specification, in fp32 with separately rounded products
    t = gamma * r.float()
    h_ref = (x.float() + (t * sv if s is not None else t)).to(torch.bfloat16)
    u = dh.float() * gamma
    dr_ref = (u * sv if s is not None else u).to(torch.bfloat16)
    prod = dh.double() * r.double() * (sv.double() if s is not None else 1.0)
    dg_ref = prod.reshape(-1, shape[-1]).sum(0)
    dg_abs = prod.abs().reshape(-1, shape[-1]).sum(0)

    xg, rg = x.cuda().requires_grad_(True), r.cuda().requires_grad_(True)
    gg = gamma.cuda().requires_grad_(True)
    h = layer_scale_add(xg, rg, gg, s.cuda() if s is not None else None)
    h.backward(dh.cuda())
    assert torch.equal(h.detach().cpu(), h_ref)
    assert torch.equal(rg.grad.cpu(), dr_ref)
    assert torch.equal(xg.grad.cpu(), dh)                       # dx is dh itself
    if s is not None:
        dropped = (s == 0)
        assert dropped.any()
        assert torch.equal(h.detach().cpu()[dropped].view(torch.int16),
                           x[dropped].view(torch.int16))       # bitwise, signed zeros too
    if kind == "ints":
        ei.assert_exact_range(dg_ref, "fp32", "dgamma")
        assert torch.equal(gg.grad.cpu().double(), dg_ref)
    else:
        P = h_ref.numel() // shape[-1]
        err = (gg.grad.cpu().double() - dg_ref).abs()
        print("dgamma max err", float(err.max()), "bound min", float((P * 2.0 ** -23 * dg_abs).min()))
        assert bool((err <= P * 2.0 ** -23 * dg_abs).all())
