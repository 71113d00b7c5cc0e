"""csrc/dropout.hip: the keep mask is a pure function of (seed, offset, element
index) -- pinned byte for byte against the NumPy Philox4x32-10 of
kernel_oracles.py -- and the element-wise backward follows the FORWARD's memory
format, however the gradient arrives.

Left untested on purpose: the high word of the group counter (ctr.y) is
non-zero only past 2^34 mask elements, 16 GiB of mask bytes."""
import numpy as np
import pytest
import torch

import kernel_oracles as ko

pytestmark = pytest.mark.gpu

SEED = 0x123456789ABCDEF0 >> 2          # both 32-bit key words non-zero
OFFSETS = (0, 1, 2**33 + 5)             # the last: a non-zero high offset word
PS = (0.3, 0.5, 0.0)
DTYPES = [torch.bfloat16, torch.float32]
SHAPE = (3, 7, 5, 3)                    # N*C = 21 (not a multiple of 4), 315 elements (not of 8)


def _nat():
    from distributed_ml_pytorch_amd.ops._ext import native

    return native()


def _input(shape, dtype, seed=0):
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
    x = torch.where(x.abs() < 0.05, torch.full_like(x, 0.5), x)      # no zeros: y == 0 <=> dropped
    return x.to(dtype)


def _check_y(y, x, keep, p):
    """y == x * keep * scale to one rounding of the output type."""
    want = x.double() * keep.double() / (1.0 - p)
    rtol = 2.0 ** -7 if x.dtype == torch.bfloat16 else 1e-6
    torch.testing.assert_close(y.cpu().double(), want, rtol=rtol, atol=0)
    assert torch.equal(y.cpu() == 0, keep == 0)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_dropout_mask_is_the_philox_stream(mode, dtype):
    nat = _nat()
    assert SEED & 0xFFFFFFFF and SEED >> 32
    if mode == 0:
        x = _input((1003,), dtype)                       # 1003: not a multiple of 8 (or 4)
    else:
        x = _input(SHAPE, dtype)
    xd = x.cuda()
    if mode == 2:
        xd = xd.contiguous(memory_format=torch.channels_last)
    nmask = x.numel() if mode == 0 else SHAPE[0] * SHAPE[1]
    for p in PS:
        for off in OFFSETS:
            state = torch.tensor([off, 0], dtype=torch.int64, device="cuda")
            y, mask = nat.dropout_fwd(xd, p, SEED, state, mode)
            ref = ko.dropout_mask_ref(nmask, p, SEED, off)
            got = mask.cpu().numpy()
            assert got.dtype == np.uint8 and got.shape == (nmask,)
            assert np.array_equal(got, ref), (p, off, int((got != ref).sum()))
            # the offset advances by exactly 1 per launch, the ticket returns to 0
            assert state.tolist() == [off + 1, 0]
            keep = torch.from_numpy(ref)
            if mode != 0:
                keep = keep.view(SHAPE[0], SHAPE[1], 1, 1).expand(SHAPE)
            assert y.shape == x.shape
            if mode == 2:
                assert y.is_contiguous(memory_format=torch.channels_last)
            _check_y(y, x, keep.reshape(x.shape), p)
            if p == 0.0:
                assert ref.all()
        # a second launch on the same state: the next offset's mask
        state = torch.tensor([7, 0], dtype=torch.int64, device="cuda")
        for k in range(3):
            _, mask = nat.dropout_fwd(xd, p, SEED, state, mode)
            assert np.array_equal(mask.cpu().numpy(), ko.dropout_mask_ref(nmask, p, SEED, 7 + k))
        assert state.tolist() == [10, 0]


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
def test_dropout_plane_masks_agree_across_layouts(dtype):
    """Modes 1 (NCHW) and 2 (channels_last) give the same plane mask and the
    same logical output for the same logical tensor."""
    nat = _nat()
    x = _input(SHAPE, dtype, seed=1).cuda()
    outs = []
    for mode, xin in ((1, x), (2, x.contiguous(memory_format=torch.channels_last))):
        state = torch.tensor([2**33 + 5, 0], dtype=torch.int64, device="cuda")
        outs.append(nat.dropout_fwd(xin, 0.5, SEED, state, mode))
    (y1, m1), (y2, m2) = outs
    assert torch.equal(m1, m2)
    assert torch.equal(y1, y2)          # logical comparison across layouts
    per_plane = (y1 != 0).float().mean(dim=(2, 3))
    assert bool(((per_plane == 0) | (per_plane == 1)).all())
    assert 0 < float(per_plane.mean()) < 1


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
@pytest.mark.parametrize("grad_cl", [False, True], ids=["g_nchw", "g_cl"])
@pytest.mark.parametrize("x_cl", [False, True], ids=["x_nchw", "x_cl"])
def test_elementwise_dropout_backward_follows_forward_format(x_cl, grad_cl, dtype):
    """mode 0 draws mask[i] in MEMORY order of the forward input.  Whatever dense
    format the incoming gradient has (a reshape copy before a Linear hands back
    NCHW, a native conv channels_last), x.grad == g * keep * scale logically."""
    from distributed_ml_pytorch_amd.ops import layers as L

    shape, p = (4, 6, 5, 3), 0.3
    CL = torch.channels_last
    x = _input(shape, dtype, seed=2).cuda()
    if x_cl:
        x = x.contiguous(memory_format=CL)
    x.requires_grad_(True)
    layer = L.Dropout(p, seed=SEED).cuda()
    y = layer(x)
    keep = (y.detach() != 0)
    # the mask is the stream in the forward's memory order
    ref = torch.from_numpy(ko.dropout_mask_ref(x.numel(), p, SEED, 0)).bool()
    mem = keep.permute(0, 2, 3, 1) if x_cl else keep
    assert torch.equal(mem.reshape(-1).cpu(), ref)
    _check_y(y.detach(), x.detach().cpu(), keep.cpu(), p)

    g = _input(shape, dtype, seed=3).cuda()
    g = g.contiguous(memory_format=CL) if grad_cl else g.contiguous()
    assert g.is_contiguous() != grad_cl and g.is_contiguous(memory_format=CL) == grad_cl
    y.backward(g)
    assert x.grad.shape == x.shape
    _check_y(x.grad, g.cpu(), keep.cpu(), p)
    assert layer._state.tolist() == [1, 0]
