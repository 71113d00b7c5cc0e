"""``ops._grads.GradSink``: where a native backward puts a parameter gradient
(the arena's flat grad buffer + ready callback, or a returned temporary)."""
import pytest
import torch
import torch.nn as nn

from distributed_ml_pytorch_amd.ops._grads import GradSink, notify
from distributed_ml_pytorch_amd.parallel.arena import FlatArena

CL = torch.channels_last
LAYOUTS = ("any", "cl", "rows")


@pytest.fixture
def net():
    torch.manual_seed(0)
    model = nn.Sequential(nn.Conv2d(8, 8, 3), nn.BatchNorm2d(8), nn.Flatten(), nn.Linear(8, 4))
    arena = FlatArena(model, device="cpu")
    ready = []
    arena.set_grad_ready_callback(ready.append)
    return model, arena, ready


@pytest.mark.parametrize("layout", LAYOUTS)
def test_arena_conv_weight(net, layout):
    model, arena, ready = net
    w = model[0].weight                       # params[0], channels-last [8, 8, 3, 3]
    sink = GradSink(w, True, layout)
    assert sink.arena and sink.hooked
    assert sink.buf.data_ptr() == w.grad.data_ptr()
    assert sink.buf.dtype == torch.float32
    if layout == "rows":
        assert sink.buf.shape == (8, 72)
        sink.buf[3, (1 * 3 + 2) * 8 + 5] = 7.0          # column (r, s, ci) = (1, 2, 5)
        assert float(w.grad[3, 5, 1, 2]) == 7.0
        assert int((w.grad != 0).sum()) == 1
    else:
        assert sink.buf.shape == w.shape
    assert ready == []                        # nothing fires before done()
    assert sink.done() is None
    assert ready == [0]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("index", [1, 2, 3, 4, 5])
def test_arena_contiguous_params(net, layout, index):
    """Conv bias, BN gamma / beta, Linear weight / bias: 1-D and 2-D arena views."""
    model, arena, ready = net
    p = arena.params[index]
    sink = GradSink(p, True, layout)
    if layout == "cl":                        # not a channels-last 4-D grad: temporary
        assert not sink.arena and sink.buf.shape == p.shape and not sink.buf.any()
        assert sink.done().shape == p.shape and ready == []
        return
    assert sink.arena and sink.buf.shape == p.shape
    assert sink.buf.data_ptr() == p.grad.data_ptr()
    assert sink.done() is None
    assert ready == [index]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_plain_parameter(layout, dtype):
    called = []
    p = nn.Parameter(torch.randn(8, 6, 3, 5).to(dtype))
    sink = GradSink(p, True, layout)
    assert not sink.arena and not sink.hooked
    assert sink.buf.dtype == torch.float32 and not sink.buf.any()
    if layout == "rows":
        assert sink.buf.shape == (8, 90) and sink.buf.is_contiguous()
        sink.buf.copy_(torch.arange(8 * 90).view(8, 90))
        want = torch.arange(8 * 90, dtype=torch.float32).view(8, 3, 5, 6).permute(0, 3, 1, 2)
    else:
        assert sink.buf.shape == p.shape
        assert sink.buf.is_contiguous(memory_format=CL) == (layout == "cl")
        sink.buf.copy_(torch.arange(p.numel()).view(p.shape))
        want = torch.arange(p.numel(), dtype=torch.float32).view(p.shape)
    p._dmp_grad_ready = called.append         # a hook alone does not make it an arena grad
    out = sink.done()
    assert out.shape == p.shape and out.dtype == p.dtype
    assert torch.equal(out, want.to(dtype))
    assert called == []


def test_plain_2d_and_1d_rows():
    for shape in [(4, 8), (4,)]:
        p = nn.Parameter(torch.randn(shape))
        sink = GradSink(p, True, "rows")
        assert sink.buf.shape == p.shape and not sink.buf.any()
        assert sink.done().shape == p.shape


def test_temporary_dtype():
    p = nn.Parameter(torch.randn(8).to(torch.bfloat16))
    assert GradSink(p, True).buf.dtype == torch.float32
    sink = GradSink(p, True, dtype=None)      # the BatchNorm sites: the parameter's own
    assert sink.buf.dtype == torch.bfloat16
    assert sink.done() is sink.buf            # no cast, no reshape


@pytest.mark.parametrize("layout", LAYOUTS)
def test_detached_grad_falls_back(net, layout):
    model, arena, ready = net
    w = model[0].weight
    w.grad = None
    sink = GradSink(w, True, layout)
    assert not sink.arena and not sink.buf.any()
    out = sink.done()
    assert out.shape == w.shape and out.dtype == w.dtype
    assert ready == []                        # autograd's accumulate hook reports it instead


def test_wrong_layout_falls_back(net):
    model, arena, ready = net
    w, lw = model[0].weight, model[3].weight
    w.grad = torch.zeros(w.shape)             # NCHW-contiguous: not what a "cl" kernel writes
    assert not GradSink(w, True, "cl").arena
    assert GradSink(w, True, "rows").arena    # contiguous rows are fine as they are
    assert GradSink(w, True, "any").arena
    lw.grad = torch.zeros(8, 4).t()           # transposed: no dense rows
    sink = GradSink(lw, True, "rows")
    assert not sink.arena and sink.buf.shape == lw.shape and sink.buf.is_contiguous()
    assert ready == []


def test_not_needed(net):
    model, arena, ready = net
    w = model[0].weight
    for sink in (GradSink(w, False), GradSink(None, True), GradSink(None, False, "rows")):
        assert sink.buf is None and not sink.arena and not sink.hooked
        assert sink.done() is None
    assert ready == []


def test_frozen_arena_parameter_is_left_alone(net):
    """The one rule for every site: no gradient needed, no write and no notify,
    even though the parameter has an arena slot."""
    model, arena, ready = net
    gamma = model[1].weight
    gamma.requires_grad_(False)
    for layout in LAYOUTS:
        sink = GradSink(gamma, gamma.requires_grad, layout)
        assert sink.buf is None and sink.done() is None
    assert ready == [] and not gamma.grad.any()


def test_no_callback_set():
    model = nn.Sequential(nn.Conv2d(8, 8, 3), nn.Linear(8, 4))
    FlatArena(model, device="cpu")
    for p, layout in [(model[0].weight, "cl"), (model[0].weight, "rows"), (model[1].bias, "any")]:
        sink = GradSink(p, True, layout)
        assert sink.arena and not sink.hooked
        assert sink.done() is None
    notify(model[0].weight, None)             # silent too
