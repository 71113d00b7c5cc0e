"""The wire codecs (parallel/wire.py): payload sizes, header codes and lookups."""
import pytest
import torch

from distributed_ml_pytorch_amd.parallel import messaging as M
from distributed_ml_pytorch_amd.parallel import wire

# (nelem, alloc, dtype) the central PS receives a push of n elements into, and the
# header's dtype code, as ParameterServer._recv_payload and the clients computed
# them before the codecs existed: a dense payload is padded to whole float4 items,
# an MX8 payload is wire8.layout(n) bytes with no padding of its own
EXPECTED = {
    ("fp32", 64): (64, 64, torch.float32, 0),
    ("fp32", 66): (66, 68, torch.float32, 0),
    ("fp32", 65_540): (65_540, 65_540, torch.float32, 0),
    ("bf16", 64): (64, 64, torch.bfloat16, 1),
    ("bf16", 66): (66, 68, torch.bfloat16, 1),
    ("bf16", 65_540): (65_540, 65_540, torch.bfloat16, 1),
    ("mx8", 64): (68, 68, torch.uint8, 3),
    ("mx8", 66): (84, 84, torch.uint8, 3),
    ("mx8", 65_540): (67_604, 67_604, torch.uint8, 3),
}
CODECS = {"fp32": wire.FP32, "bf16": wire.BF16, "mx8": wire.MX8}


@pytest.mark.parametrize("name,n", sorted(EXPECTED))
def test_payload_shape_and_header(name, n):
    c = CODECS[name]
    nelem, alloc, dtype, code = EXPECTED[name, n]
    assert c.payload_shape(n) == (nelem, alloc, dtype)
    header = M.make_header(M.MessageCode.GradientUpdate, 1, 2, 3, n, c.header)
    assert header.tolist() == [int(M.MessageCode.GradientUpdate), 1, 2, 3, n, code]
    assert wire.codec(M.parse_header(header)[5]) is c
    buf = c.new_payload(n, "cpu")
    assert (buf.numel(), buf.dtype) == (nelem, dtype)
    assert wire.codec(buf) is c and wire.codec(dtype) is c


def test_mx8_payload_pad_bytes_are_zero():
    acc = torch.randn(66)
    buf = wire.MX8.new_payload(66, "cpu")
    wire.MX8.handoff(acc, buf)
    assert buf[66:80].eq(0).all() and buf[83:].eq(0).all()    # between codes and scales, tail


def test_copy_as_never_aliases():
    master = torch.randn(8)
    for dt in (torch.float32, torch.bfloat16):
        snap = wire.copy_as(master, dt)
        assert snap.dtype == dt and snap.data_ptr() != master.data_ptr()
        assert torch.equal(snap, master.to(dt))


def test_unknown_wire_is_an_error():
    with pytest.raises(KeyError):
        wire.codec(torch.int32)
