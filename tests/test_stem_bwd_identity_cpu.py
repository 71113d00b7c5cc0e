"""The algebra behind the one-pass stem backward (csrc/conv_small.hip
stem3_bn_bwd_*), pinned without a GPU: the BatchNorm backward is affine per
channel, so the stem's weight gradient is k1 G1 + Cc G2 + Bc G3 with three sums
over the pixels, and dx need never exist.

Both forms are emulated in fp32 (bf16 operands, fp32 sums) against the fp64
oracle of tests/stem_bwd_oracle.py.  The fused form must stay within 3e-5
row-relative (3x the worst cell of the emulation, 9.3e-6); today's form, which
rounds dx to bf16 on the way, must be at least 100x worse than that in every
cell: the change drops a rounding, it does not add error.
"""
import pytest
import torch

from stem_bwd_oracle import BIG, CELLS, cpu_case, emul_fused, emul_unfused, oracle, row_rel_live

FUSED_TOL = 3e-5


@pytest.mark.parametrize("gmode", ["one", "random", "zeros"])
@pytest.mark.parametrize("dc", [0.0, 4.0])
@pytest.mark.parametrize("shape", CELLS + [BIG], ids=lambda s: "x".join(map(str, s)))
def test_fused_form_is_closer_to_fp64(shape, dc, gmode):
    torch.manual_seed(0)
    case = cpu_case(shape, dc, gmode, seed=sum(shape) + int(dc))
    ref, _, _ = oracle(*case)
    e_fused = row_rel_live(emul_fused(*case), ref)
    e_unfused = row_rel_live(emul_unfused(*case), ref)
    print(f"{shape} dc={dc} gamma={gmode}: fused {e_fused:.3e} unfused {e_unfused:.3e}")
    assert e_fused <= FUSED_TOL
    assert e_unfused >= 100 * e_fused
