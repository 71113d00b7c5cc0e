"""Parameter gradients of the native backwards, through both of their ways out:
accumulated into the arena's flat grad buffer (ready callback fired by the
backward) or returned to autograd (callback fired by its accumulate hook).

Default tile picks throughout (tuner off: nothing is timed).  Only public API,
plus ``ops.conv``'s ``_*_cfg`` pickers to force the GEMM route of a 1x1 conv."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last
MODELS = [("resnet18", 8), ("resnet50", 2), ("alexnet", 4), ("lenet", 8), ("vit_tiny", 4),
          ("mlp", 8)]
# every Function whose backward owns a parameter gradient
FUNCTIONS = {"_NativeConv", "_SmallConv", "_StemConv", "_Im2colConv", "_ArenaLinear",
             "_GapLinear", "_BNAct", "_BNReLUPool", "_VitEmbed"}
LN_FUNCTIONS = {"_LayerNormStream", "_AddLayerNorm"}


@pytest.fixture(autouse=True)
def _default_picks(monkeypatch):
    from distributed_ml_pytorch_amd.ops.tuner import TUNER

    monkeypatch.setattr(TUNER, "enabled", False)


def _functions(root):
    """Names of the autograd Functions in the graph under ``root``."""
    seen, names, todo = set(), set(), [root.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        names.add(type(fn).__name__.removesuffix("Backward"))
        todo += [f for f, _ in fn.next_functions]
    return names


def _rel(a, b):
    return float((a.float() - b.float()).norm() / (b.float().norm() + 1e-12))


def _bf16_exact(t):
    return t.to(torch.bfloat16).float()


def _ready_means_final(model, x):
    """One backward with the ready callback cloning each reported gradient (the
    clone is ordered behind whatever was enqueued when the callback fired).
    Returns (Function names, unreported trainable indices, indices whose clone
    differs from the final gradient)."""
    from distributed_ml_pytorch_amd.parallel.arena import FlatArena

    model = model.cuda().train()
    arena = FlatArena(model, device="cuda")
    early = {}

    def ready(i):
        if i not in early:
            early[i] = arena.params[i].grad.clone()
    arena.set_grad_ready_callback(ready)
    arena.zero_grad()
    y = model(x)
    c = torch.randn(y.shape, device="cuda")
    loss = (y.float() * c).sum()
    names = _functions(loss)
    loss.backward()
    torch.cuda.synchronize()
    trainable = [i for i, p in enumerate(arena.params) if p.requires_grad]
    missing = [i for i in trainable if i not in early]
    changed = [i for i in trainable if i in early
               and not torch.equal(early[i], arena.params[i].grad)]
    dead = [i for i in trainable if not bool(arena.params[i].grad.any())]
    return names, missing, changed, dead


@functools.lru_cache(maxsize=None)
def _model_run(name, batch):
    from distributed_ml_pytorch_amd.models import build_model

    torch.manual_seed(0)
    model, shape, _ = build_model(name)
    x = torch.randn(batch, *shape, device="cuda").to(torch.bfloat16).contiguous(memory_format=CL)
    return _ready_means_final(model, x)


@pytest.mark.parametrize("name,batch", MODELS)
def test_ready_means_final(name, batch):
    names, missing, changed, dead = _model_run(name, batch)
    assert not missing, f"{name}: gradients never reported ready: {missing}"
    assert not changed, f"{name}: gradients written after they were reported ready: {changed}"
    assert not dead, f"{name}: all-zero gradients (nothing to compare): {dead}"


def test_every_parameter_owning_function_ran():
    ran = set()
    for name, batch in MODELS:
        ran |= _model_run(name, batch)[0]
    assert FUNCTIONS <= ran, FUNCTIONS - ran
    assert LN_FUNCTIONS & ran


def test_ready_means_final_gemm_route(monkeypatch):
    """A 1x1 conv with every pass forced onto the GEMM route."""
    from distributed_ml_pytorch_amd.ops import conv as C
    from distributed_ml_pytorch_amd.ops import layers as L

    for pick in ("_fwd_cfg", "_dgrad_cfg", "_wgrad_cfg"):
        monkeypatch.setattr(C, pick, lambda *a: C._GEMM_ROUTE)
    torch.manual_seed(0)
    x = torch.randn(2, 64, 5, 5, device="cuda").to(torch.bfloat16).contiguous(memory_format=CL)
    names, missing, changed, dead = _ready_means_final(L.Conv2d(64, 128, 1, bias=False),
                                                       x.requires_grad_(True))
    assert "_NativeConv" in names and not (missing or changed or dead)


# ------------------------------------------------ returned path == arena path
def _conv_case(ci, co, k, pad, bias, hw, fn):
    from distributed_ml_pytorch_amd.ops import layers as L

    def oracle(x, w, b=None):
        return F.conv2d(x, w, b, padding=pad)
    return (lambda: L.Conv2d(ci, co, k, padding=pad, bias=bias)), (2, ci, hw, hw), oracle, fn


def _linear_case():
    from distributed_ml_pytorch_amd.ops import layers as L

    return (lambda: L.Linear(120, 84, bias=False)), (33, 120), lambda x, w: x @ w.t(), \
        "_ArenaLinear"


def _bn_case():
    from distributed_ml_pytorch_amd.ops import layers as L

    def oracle(x, g, b):
        return F.batch_norm(x, None, None, g, b, True, 0.1, 1e-5)
    return (lambda: L.BatchNorm2d(8)), (2, 8, 4, 4), oracle, "_BNAct"


def _ln_case():
    from distributed_ml_pytorch_amd.models.vit import LayerNorm

    def oracle(x, g, b):
        return F.layer_norm(x, (64,), g, b, 1e-5)
    return (lambda: LayerNorm(64)), (2, 5, 64), oracle, "_LayerNorm"


LAYERS = {
    "conv3x3": lambda: _conv_case(64, 64, 3, 1, False, 8, "_NativeConv"),
    "conv3x3_bias": lambda: _conv_case(64, 64, 3, 1, True, 8, "_NativeConv"),
    "conv_small": lambda: _conv_case(3, 64, 3, 1, False, 8, "_SmallConv"),
    "conv5x5_padded_rows": lambda: _conv_case(1, 10, 5, 0, False, 12, "_Im2colConv"),
    "conv5x5_bias": lambda: _conv_case(8, 16, 5, 0, True, 12, "_Im2colConv"),
    "linear": _linear_case,
    "batchnorm": _bn_case,
    "layernorm": _ln_case,
}


@pytest.mark.parametrize("case", sorted(LAYERS))
def test_returned_path_equals_arena_path(case):
    """The same backward twice: into the arena grad views, then with every
    ``p.grad = None`` (gradients returned to autograd), both against the fp32
    oracle on the same bf16 operands."""
    from distributed_ml_pytorch_amd.parallel.arena import FlatArena

    make, xshape, oracle, fn = LAYERS[case]()
    torch.manual_seed(0)
    layer = make().cuda().train()
    with torch.no_grad():
        for p in layer.parameters():          # masters == their bf16 shadows
            p.copy_(_bf16_exact(p + 0.25 * torch.randn_like(p)))
    arena = FlatArena(layer, device="cuda")
    ready = []
    arena.set_grad_ready_callback(ready.append)
    params = arena.params
    x = torch.randn(*xshape, device="cuda").to(torch.bfloat16)
    if x.dim() == 4:
        x = x.contiguous(memory_format=CL)
    leaves = [p.detach().float().requires_grad_(True) for p in params]
    yr = oracle(x.float(), *leaves)
    c = _bf16_exact(torch.randn(yr.shape, device="cuda"))   # dY exact in bf16
    want = torch.autograd.grad((yr * c).sum(), leaves)
    yr = yr.detach()
    got = []
    for attached in (True, False):
        if not attached:
            for p in params:
                p.grad = None
        del ready[:]
        arena.zero_grad()
        y = layer(x)
        assert y.dtype == torch.bfloat16 and _rel(y, yr) < 1e-2
        loss = (y.float() * c).sum()
        assert fn in _functions(loss)
        loss.backward()
        torch.cuda.synchronize()
        assert sorted(set(ready)) == list(range(len(params))), (attached, ready)
        got.append([p.grad.clone() for p in params])
    for i, p in enumerate(params):
        assert p.grad.data_ptr() != arena.g32.data_ptr() + 4 * arena.slots[i].offset
        for g, path in zip((got[0][i], got[1][i]), ("arena", "returned")):
            assert g.shape == p.shape and g.dtype == p.dtype
            print(f"{case} param {i} {path}: rel {_rel(g, want[i]):.3e}")
            assert _rel(g, want[i]) < 1e-2, (case, i, path)
