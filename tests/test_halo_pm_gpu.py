"""Position-major halo tiles on 4 x 4 maps (csrc/halo_pm.h, conv_halo_kernel<.., PM>):
one fragment = one pixel position across 16 images, padding taps not issued.

Against fp32 PyTorch at the tolerances of test_halo_conv_configs, against the dense
kernel of the same cfg id BIT FOR BIT (the skipped products are exact zeros and the
order of the others is unchanged; only the BN partial sums change their summation
order), and an integer one-hot conv that has no tolerance at all.

Shapes: B 1 / 16 / 17 / 33 (under-full tile, exact tile, second tile holding one
image), K = 32 / 64 / 96 reduction channels (one, two, an odd number of chunks
through the two-stage ring), N = 64 / 128 output channels.
"""
import itertools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
CL = torch.channels_last
H = W = 4
CASES = list(itertools.product((1, 16, 17, 33), (32, 64, 96), (64, 128)))


def _rel(a, b):
    return float((a.float() - b.float()).norm() / (b.float().norm() + 1e-12))


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


def _pm_cfgs(nat, K):
    cfgs = [c for c in nat.conv_halo_configs(H, W, K, 3, 3, 1, 1)
            if nat.conv_halo_pm_ok(c, H, W, K, 3, 3, 1, 1)]
    assert 100 in cfgs, "cfg 100 must run position-major on 4 x 4 maps"
    return cfgs


def _sums(part, G, CO):
    return part[:2 * int(G) * CO].view(2, int(G), CO).sum(1)


def test_switch_and_applicability(nat):
    prev = nat.conv_halo_pm(True)
    try:
        assert nat.conv_halo_pm(False) is True
        assert nat.conv_halo_pm(True) is False
    finally:
        nat.conv_halo_pm(prev)
    assert nat.conv_halo_pm_ok(100, 4, 4, 512, 3, 3, 1, 1)
    assert not nat.conv_halo_pm_ok(100, 8, 8, 256, 3, 3, 1, 1)
    assert not nat.conv_halo_pm_ok(100, 4, 4, 512, 3, 3, 2, 1)
    assert not nat.conv_halo_pm_ok(102, 4, 4, 512, 3, 3, 1, 1)


@pytest.mark.parametrize("B,K,N", CASES)
def test_forward(nat, B, K, N):
    torch.manual_seed(B * 1000 + K + N)
    x = torch.randn(B, K, H, W, device="cuda").to(torch.bfloat16).contiguous(memory_format=CL)
    w = (torch.randn(N, K, 3, 3, device="cuda") / (K * 9) ** 0.5).to(torch.bfloat16)
    w = w.contiguous(memory_format=CL)
    yr = F.conv2d(x.float(), w.float(), None, 1, 1)
    for cfg in _pm_cfgs(nat, K):
        with _Switch(nat, True):
            y, part, G = nat.conv_fwd(x, w, 1, 1, True, cfg)
            y0 = nat.conv_fwd(x, w, 1, 1, False, cfg)[0]        # no statistics: eval forward
        with _Switch(nat, False):
            yd, partd, Gd = nat.conv_fwd(x, w, 1, 1, True, cfg)
        rel = _rel(y, yr)
        print(f"fwd B{B} K{K} N{N} cfg{cfg}: rel {rel:.3e}")
        assert rel < 1e-2, cfg
        ps, yf = _sums(part, G, N), y.float()
        torch.testing.assert_close(ps[0], yf.sum(dim=(0, 2, 3)), rtol=1e-3, atol=1e-2)
        torch.testing.assert_close(ps[1], (yf * yf).sum(dim=(0, 2, 3)), rtol=1e-3, atol=1e-2)
        # PM against dense: the outputs bit for bit, the sums to their tolerance
        assert torch.equal(y, yd), (cfg, float((y.float() - yd.float()).abs().max()))
        assert torch.equal(y0, yd), cfg
        torch.testing.assert_close(ps, _sums(partd, Gd, N), rtol=1e-3, atol=1e-2)


@pytest.mark.parametrize("B,K,N", CASES)
def test_data_gradient(nat, B, K, N):
    """dX [B, N, 4, 4] from dY [B, K, 4, 4]: plain, with a residual addend, and with
    an addend behind a deferred ReLU bit mask."""
    torch.manual_seed(B * 1000 + K + N + 7)
    dy = torch.randn(B, K, H, W, device="cuda").to(torch.bfloat16).contiguous(memory_format=CL)
    w = (torch.randn(K, N, 3, 3, device="cuda") / (K * 9) ** 0.5).to(torch.bfloat16)
    w = w.contiguous(memory_format=CL)
    dxr = F.conv_transpose2d(dy.float(), w.float(), None, 1, 1)
    add = torch.randn(B, N, H, W, device="cuda").to(torch.bfloat16).contiguous(memory_format=CL)
    mask = torch.randint(0, 256, (B * H * W * N // 8,), device="cuda", dtype=torch.uint8)
    bits = torch.stack([(mask >> k) & 1 for k in range(8)], 1).view(B, H, W, N).permute(0, 3, 1, 2)
    refs = (dxr, dxr + add.float(), dxr + torch.where(bits.bool(), add.float(), 0.0))
    for cfg in _pm_cfgs(nat, K):
        outs = {}
        for on in (True, False):
            with _Switch(nat, on):
                outs[on] = (nat.conv_dgrad(dy, w, H, W, 1, 1, cfg),
                            nat.conv_dgrad(dy, w, H, W, 1, 1, cfg, None, add),
                            nat.conv_dgrad(dy, w, H, W, 1, 1, cfg, None, add, addend_mask=mask))
        for name, got, dense, ref in zip(("plain", "addend", "masked"), outs[True], outs[False], refs):
            rel = _rel(got, ref)
            print(f"dgrad {name} B{B} K{K} N{N} cfg{cfg}: rel {rel:.3e}")
            assert rel < 1e-2, (cfg, name)
            assert torch.equal(got, dense), (cfg, name)


@pytest.mark.parametrize("tap", range(9))
def test_one_hot_taps_exact(nat, tap):
    """x[b, p, 0] = 16 b + p (integers <= 255, exact in bf16), one weight of 1 at
    `tap` from channel 0 to channel 0: y[..., 0] is x shifted with zero fill, exactly;
    a wrong permutation or validity bit has no tolerance to hide in."""
    B, K, N = 16, 32, 64
    r, s = divmod(tap, 3)
    x = torch.zeros(B, K, H, W, device="cuda")
    x[:, 0] = (16 * torch.arange(B, device="cuda").view(B, 1, 1) +
               torch.arange(H * W, device="cuda").view(1, H, W)).float()
    xb = x.to(torch.bfloat16).contiguous(memory_format=CL)
    assert torch.equal(xb.float(), x)
    w = torch.zeros(N, K, 3, 3, device="cuda")
    w[0, 0, r, s] = 1.0
    wb = w.to(torch.bfloat16).contiguous(memory_format=CL)
    # y[b, h, w] = x[b, h + r - 1, w + s - 1], zero outside the image
    want = F.pad(x[:, 0], (1, 1, 1, 1))[:, r:r + H, s:s + W]
    # dx[b, h, w] = dy[b, h - (r - 1), w - (s - 1)]: the mirrored tap
    want_dx = F.pad(x[:, 0], (1, 1, 1, 1))[:, 2 - r:2 - r + H, 2 - s:2 - s + W]
    w_dg = torch.zeros(K, N, 3, 3, device="cuda")
    w_dg[0, 0, r, s] = 1.0
    w_dg = w_dg.to(torch.bfloat16).contiguous(memory_format=CL)
    with _Switch(nat, True):
        for cfg in _pm_cfgs(nat, K):
            y = nat.conv_fwd(xb, wb, 1, 1, True, cfg)[0].float()
            assert torch.equal(y[:, 0], want), (cfg, tap)
            assert not y[:, 1:].any(), (cfg, tap)
            dx = nat.conv_dgrad(xb, w_dg, H, W, 1, 1, cfg).float()
            assert torch.equal(dx[:, 0], want_dx), (cfg, tap)
            assert not dx[:, 1:].any(), (cfg, tap)
