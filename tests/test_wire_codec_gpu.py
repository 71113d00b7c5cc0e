"""The wire codecs on the GPU (native kernels) against the same codecs on the CPU
(the torch expressions of parallel/wire.py and wire8.py): bit for bit."""
import pytest
import torch

from distributed_ml_pytorch_amd.parallel import wire

pytestmark = pytest.mark.gpu

CODECS = {"fp32": wire.FP32, "bf16": wire.BF16, "mx8": wire.MX8}


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8),
                                              b.contiguous().view(torch.uint8))


# n = 64: the smallest arena; 65,540: several blocks of the grid, n % 32 == 4 (a short
# last MX8 block).  Both scales make the product exact, so the fused multiply-add of
# the fp32 / bf16 kernels, the two roundings of the MX8 kernel and torch's CPU add all
# round once, to the same bits.
@pytest.mark.parametrize("scale", [1.0, 0.5])
@pytest.mark.parametrize("n", [64, 65_540])
@pytest.mark.parametrize("name", sorted(CODECS))
def test_handoff_then_apply_matches_cpu(name, n, scale):
    c = CODECS[name]
    g = torch.Generator().manual_seed(n)
    # magnitudes over many binades: MX8 blocks with different scales
    acc0 = torch.randn(n, generator=g) * torch.exp2(torch.randint(-12, 4, (n,), generator=g))
    master0 = torch.randn(n, generator=g)

    def run(device):
        acc, master = acc0.clone().to(device), master0.clone().to(device)   # never the inputs
        buf = c.new_payload(n, device)
        c.handoff(acc, buf)
        c.apply(master, buf, scale)
        return buf.cpu(), acc.cpu(), master.cpu()

    payload, resid, master = run("cuda")
    payload_ref, resid_ref, master_ref = run("cpu")
    assert same_bits(payload, payload_ref)
    # what stays in the accumulator: zeros, or the MX8 quantisation residual
    assert same_bits(resid, resid_ref)
    assert bool(resid.any()) == (name == "mx8")
    assert same_bits(master, master_ref)
    assert not torch.equal(master, master0)
