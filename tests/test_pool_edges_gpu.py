"""csrc/pool.hip at its edge shapes: the global average pool against fp64
(kernel_oracles.gap_ref) and the max pool, forward taps and gather-form
backward, EXACTLY against kernel_oracles.maxpool_ref on tie-heavy integers."""
import pytest
import torch

import kernel_oracles as ko

pytestmark = pytest.mark.gpu

CL = torch.channels_last

def _nat():
    from distributed_ml_pytorch_amd.ops._ext import native

    return native()


def _dev(t):
    return t.cuda().contiguous(memory_format=CL)


# --------------------------------------------------------- global average pool
@pytest.mark.parametrize("offset", ko.GAP_OFFSETS, ids=["randn", "plus300"])
@pytest.mark.parametrize("C", ko.GAP_C)
@pytest.mark.parametrize("HW", list(ko.GAP_HW))
def test_global_avg_pool(HW, C, offset):
    from distributed_ml_pytorch_amd.ops.functional import global_avg_pool

    x, dy = ko.gap_inputs(HW, C, offset)
    xd = _dev(x).requires_grad_(True)
    y = global_avg_pool(xd)
    assert y.shape == dy.shape and y.dtype == torch.bfloat16
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    e_y, e_dx = ko.gap_errors(y, xd.grad.cpu(), x, dy)
    print(f"gap HW{HW} C{C} +{offset}: y row_rel {e_y:.2e}  dx row_abs {e_dx:.2e}")
    assert e_y <= ko.GAP_Y_TOL and e_dx <= ko.GAP_DX_TOL


# -------------------------------------------------------------------- max pool
KSP = [(2, 2, 0), (3, 2, 1), (3, 3, 0), (5, 2, 2), (2, 3, 0)]   # the last: stride > window
SHAPES = [(2, 8, 9, 7), (1, 16, 3, 3), (2, 6, 9, 7)]            # C = 6: one channel per lane


def _pool_exact(x, dy, k, s, p, relu_in=False, nchw_out=False):
    """maxpool_fwd / maxpool_bwd on x against maxpool_ref: y, the taps and dx equal."""
    nat = _nat()
    N, C, H, W = x.shape
    y, idx = nat.maxpool_fwd(_dev(x), k, s, p, nchw_out, relu_in)
    dyd = dy.cuda().contiguous() if nchw_out else _dev(dy)
    dx = nat.maxpool_bwd(dyd, idx, H, W, k, s, p)
    torch.cuda.synchronize()
    y_ref, tap, dx_ref = ko.maxpool_ref(x, k, s, p, relu_in=relu_in, dy=dy)
    assert y.is_contiguous() if (nchw_out and C % 8 == 0) else y.is_contiguous(memory_format=CL)
    assert torch.equal(y.cpu().double(), y_ref)
    assert torch.equal(idx.cpu(), tap)
    assert torch.equal(dx.cpu().double(), dx_ref)
    return y_ref, dx_ref


@pytest.mark.parametrize("k,s,p", KSP)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_max_pool_exact(shape, k, s, p):
    """Integers in {-1, 0, 1, 2} (ties in most windows; the first maximum in scan
    order wins) and integer dy in {-2..2}: overlapping-window sums are exact."""
    x, dy = ko.pool_int_inputs(shape, k, s, p)
    y_ref, dx_ref = _pool_exact(x, dy, k, s, p)
    if s > k:       # some inputs belong to no window: their gradient is an exact 0
        assert float(dx_ref[:, :, k::s].abs().max()) == 0.0
    # all negative: with p > 0 a padded tap that won would show as 0 / a tap out of range
    x, dy = ko.pool_int_inputs(shape, k, s, p, seed=1, lo=-3, hi=-1)
    y_ref, _ = _pool_exact(x, dy, k, s, p)
    assert float(y_ref.max()) < 0.0


@pytest.mark.parametrize("k,s,p", KSP)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_max_pool_relu_in(shape, k, s, p):
    """A non-negative input taken through relu: windows whose maximum is 0 record
    tap 255 and pass no gradient; through the functional ops, d/dx of
    max_pool2d(relu(x)) is the reference's."""
    from distributed_ml_pytorch_amd.ops import functional as DF

    x, dy = ko.pool_int_inputs(shape, k, s, p, seed=2, lo=-3, hi=1)
    x[0, 0] = -1.0                      # one plane whose every window is all zeros
    xr = x.clamp(min=0)
    _, dx_ref = _pool_exact(xr, dy, k, s, p, relu_in=True)
    _, tap, _ = ko.maxpool_ref(xr, k, s, p, relu_in=True)
    assert 0 < int((tap == 255).sum()) < tap.numel()

    xd = _dev(x).requires_grad_(True)
    h = DF.set_nonneg(DF.relu(xd))
    y = DF.max_pool2d(h, k, s, p)
    assert DF.nonneg(y)
    y.backward(_dev(dy))
    torch.cuda.synchronize()
    assert torch.equal(xd.grad.cpu().double(), dx_ref)


@pytest.mark.parametrize("k,s,p", KSP)
@pytest.mark.parametrize("nchw_out", [False, True])
def test_max_pool_nchw_out(k, s, p, nchw_out):
    """C = 8: y written NCHW-contiguous and its NCHW gradient read in place."""
    shape = SHAPES[0]
    x, dy = ko.pool_int_inputs(shape, k, s, p, seed=3)
    _pool_exact(x, dy, k, s, p, nchw_out=nchw_out)
