"""Model EMA on the CPU path (parallel/fused_optim.py, parallel/ema.py): the
readable specification of the EMA kernels, against the NumPy oracle of
ema_oracle.py.  Every comparison is bit equality."""
import copy
import logging
import types

import numpy as np
import pytest
import torch

import ema_oracle as eo
from distributed_ml_pytorch_amd.parallel.arena import attach_arena
from distributed_ml_pytorch_amd.parallel.asgd import Asynchronous
from distributed_ml_pytorch_amd.parallel.clients import LocalPSClient
from distributed_ml_pytorch_amd.parallel.ddp import FusedAdamW, FusedSGD
from distributed_ml_pytorch_amd.parallel.ema import ModelEma
from distributed_ml_pytorch_amd.parallel.fused_optim import FusedOptimCore, ema_coeffs
from distributed_ml_pytorch_amd.utils import checkpoint as ck

DECAY = 0.97


def _eq(t, a):
    """Bit equality of a torch tensor and a NumPy float32 array."""
    return np.array_equal(eo.to_np(t).view(np.uint32), np.asarray(a, np.float32).view(np.uint32))


def test_oracle_coefficients():
    # warm-up: (1 + u) / (10 + u) until it passes the decay; the interval skips steps
    assert eo.coeffs(0.9, 1, True, 1) == (1, np.float32(2 / 11), np.float32(1 - 2 / 11))
    assert eo.coeffs(0.9, 3, True, 6)[0] == 2 and eo.coeffs(0.9, 3, True, 6)[1] == np.float32(0.25)
    assert eo.coeffs(0.9, 3, True, 7) == (2, np.float32(1), np.float32(0))
    u, D, O = eo.coeffs(0.9, 1, True, 200)
    d32 = np.float32(0.9)
    assert D == d32 and O == np.float32(1.0 - np.float64(d32))
    # the CPU path publishes the same scalars
    for every in (1, 3):
        for warm in (False, True):
            for t in range(1, 130):
                u, D, O = eo.coeffs(DECAY, every, warm, t)
                assert ema_coeffs(DECAY, every, warm, t) == (u, float(D), float(O))


def _raw(n, seed=0):
    g = torch.Generator().manual_seed(seed)
    return types.SimpleNamespace(numel=n, device=torch.device("cpu"), params=[], slots=[],
                                 p32=torch.randn(n, generator=g), g32=torch.zeros(n), w16=None)


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("every", [1, 3])
def test_core_cpu_path_against_oracle(kind, warm, every):
    n, steps = 64 * 3, 40
    kw = dict(weight_decay=0.01, momentum=0.9 if kind == "sgd" else 0.0)
    off_a, on_a = _raw(n), _raw(n)
    off = FusedOptimCore(off_a, kind, 0.05, **kw)
    on = FusedOptimCore(on_a, kind, 0.05, ema_decay=DECAY, ema_every=every, ema_warmup=warm, **kw)
    assert off.ema is None and off.ema_updates == 0
    e = eo.to_np(on_a.p32).copy()
    assert _eq(on.ema, e)
    state = []
    for core in (off, on):
        state.append((torch.zeros(n), torch.zeros(n) if kind == "sgd" else None))
    gen = torch.Generator().manual_seed(1)
    for t in range(1, steps + 1):
        g = torch.randn(n, generator=gen)
        for core, a, (acc, mom) in zip((off, on), (off_a, on_a), state):
            a.g32.copy_(g)
            core.step(a, acc, mom, 0.0)
        u, D, O = eo.coeffs(DECAY, every, warm, t)
        before = e
        e = eo.update(e, eo.to_np(on_a.p32), D, O)
        assert _eq(on.ema, e), t
        if t % every:
            assert np.array_equal(e, before)
        assert on.ema_updates == u == t // every
    assert torch.equal(off_a.p32, on_a.p32)
    assert torch.equal(state[0][0], state[1][0])
    if kind == "sgd":
        assert torch.equal(state[0][1], state[1][1])
    else:
        assert torch.equal(off.m, on.m) and torch.equal(off.v, on.v)
    assert not _eq(on.ema, eo.to_np(on_a.p32))


def test_options_are_refused():
    a = _raw(64)
    for kw in (dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(ema_decay=0.5, ema_every=0),
               dict(ema_every=2), dict(ema_warmup=True), dict(ema_decay=1.0 - 1e-12)):
        with pytest.raises(ValueError, match="EMA"):
            FusedOptimCore(a, "sgd", 0.1, **kw)


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 6, 3, padding=1)
        self.bn = torch.nn.BatchNorm2d(6)
        self.fc = torch.nn.Linear(6, 4)

    def forward(self, x):
        return self.fc(torch.relu(self.bn(self.conv(x))).mean((2, 3)))


def _batch(i):
    g = torch.Generator().manual_seed(100 + i)
    return torch.randn(8, 3, 5, 5, generator=g) * (1 + i % 3), torch.randint(0, 4, (8,), generator=g)


def _train(model, opt, i):
    x, y = _batch(i)
    opt.zero_grad()
    torch.nn.functional.cross_entropy(model(x), y).backward()
    opt.local_step()
    opt.comm_step()


def _net_opt(which="sgd", seed=0, **kw):
    torch.manual_seed(seed)
    model = _Net()
    ema = dict(ema_decay=DECAY, ema_every=2, ema_warmup=True)
    ema.update(kw)
    if which == "async":
        opt = Asynchronous(model.parameters(), lr=0.05, n_push=3, n_pull=2, model=model,
                           client=LocalPSClient(staleness=0), momentum=0.9, **ema)
    elif which == "adamw":
        arena = attach_arena(model, shadow_dtype=None)
        opt = FusedAdamW(model.parameters(), arena, 0.01, model=model, **ema)
    else:
        arena = attach_arena(model, shadow_dtype=None)
        opt = FusedSGD(model.parameters(), arena, 0.05, 0.9, model=model, **ema)
    return model, opt


@pytest.mark.parametrize("which", ["sgd", "adamw"])
def test_model_ema_buffers_and_applied(which):
    model, opt = _net_opt(which)
    avg = opt.ema
    assert isinstance(avg, ModelEma)
    assert avg.names == ["bn.running_mean", "bn.running_var"]       # integer buffers stay live
    e = {k: eo.to_np(model.state_dict()[k]).copy() for k in avg.names}
    ep = eo.to_np(opt.arena.p32).copy()
    for t in range(1, 8):
        _train(model, opt, t)
        _, D, O = eo.coeffs(DECAY, 2, True, t)
        for k in avg.names:
            e[k] = eo.update(e[k], eo.to_np(model.state_dict()[k]), D, O)
        ep = eo.update(ep, eo.to_np(opt.arena.p32), D, O)
    assert _eq(opt.core.ema, ep)
    for k, v in zip(avg.names, avg._views()):
        assert _eq(v, e[k]), k
        assert not _eq(model.state_dict()[k], e[k])
    assert int(model.bn.num_batches_tracked) == 7
    # a second model holding the averaged values is what applied() must compute
    twin = copy.deepcopy(model)
    with torch.no_grad():
        for p, q, s in zip(twin.parameters(), model.parameters(), opt.arena.slots):
            # the arena's own layout of this parameter (4-D: channels-last)
            p.copy_(torch.as_strided(opt.core.ema, q.shape, q.stride(), s.offset))
        twin.bn.running_mean.copy_(torch.from_numpy(e["bn.running_mean"]))
        twin.bn.running_var.copy_(torch.from_numpy(e["bn.running_var"]))
    live = {k: v.clone() for k, v in model.state_dict().items()}
    p0, e0, f0, v0 = opt.arena.p32.clone(), opt.core.ema.clone(), avg.flat.clone(), opt.arena.version
    x, _ = _batch(50)
    model.eval(), twin.eval()
    with torch.no_grad():
        out_live = model(x)
        with avg.applied():
            assert opt.arena.version > v0
            assert torch.equal(opt.arena.p32, e0) and torch.equal(opt.core.ema, p0)
            assert int(model.bn.num_batches_tracked) == 7
            out_ema = model(x)
            with pytest.raises(RuntimeError, match="already active"):
                with avg.applied():
                    pass
        assert torch.equal(out_ema, twin(x))
        assert not torch.equal(out_ema, out_live)
        assert torch.equal(model(x), out_live)
    model.train()
    assert torch.equal(opt.arena.p32, p0) and torch.equal(opt.core.ema, e0)
    assert torch.equal(avg.flat, f0)
    for k, v in model.state_dict().items():
        assert torch.equal(v, live[k]), k


def test_async_pull_landing_is_no_ema_event():
    model, opt = _net_opt("async")
    a = opt.arena
    e0 = eo.to_np(opt.core.ema).copy()
    assert _eq(a.p32, e0)                       # initialised after client.init()
    seen, landed = [], 0
    for t in range(1, 13):
        before = a.p32.clone()
        if seen and not np.array_equal(eo.to_np(before), seen[-1]):
            landed += 1                          # a landing moved p32 between two steps
        x, y = _batch(t)
        opt.zero_grad()
        with pytest.raises(RuntimeError, match="compute half"):
            with opt.ema.applied():
                pass
        torch.nn.functional.cross_entropy(model(x), y).backward()
        opt.local_step()
        seen.append(eo.to_np(a.p32).copy())
        opt.comm_step()
    opt.finish()
    assert landed >= 3
    assert _eq(opt.core.ema, eo.replay(e0, seen, DECAY, 2, True))
    assert opt.core.ema_updates == 6


def _state(model, opt):
    return dict(p=opt.arena.p32.clone(), e=opt.core.ema.clone(), f=opt.ema.flat.clone(),
                mom=opt.mom.clone(), acc=opt.acc.clone(),
                rm=model.bn.running_mean.clone(), u=opt.core.ema_updates)


def test_worker_checkpoint_roundtrip(tmp_path, caplog):
    kw = dict(ema_every=3, max_grad_norm=5.0)
    full_m, full = _net_opt("async", **kw)
    for t in range(1, 13):
        _train(full_m, full, t)
    m1, o1 = _net_opt("async", **kw)
    for t in range(1, 7):
        _train(m1, o1, t)
    path = str(tmp_path / "w.pt")
    ck.save_worker_checkpoint(path, m1, o1, 6)
    m2, o2 = _net_opt("async", seed=9, **kw)
    assert ck.load_worker_checkpoint(path, m2, o2) == 6
    assert o2.core.ema_updates == 2 and torch.equal(o2.core.ema, o1.core.ema)
    assert torch.equal(o2.ema.flat, o1.ema.flat)
    for t in range(7, 13):
        _train(m2, o2, t)
    want, got = _state(full_m, full), _state(m2, o2)
    for k in want:
        assert torch.equal(torch.as_tensor(want[k]), torch.as_tensor(got[k])), k
    assert got["u"] == 4

    # a checkpoint without EMA into an EMA run: the average restarts from the
    # loaded parameters and buffers, and says so
    m3, o3 = _net_opt("async", ema_decay=0.0, ema_every=1, ema_warmup=False, max_grad_norm=5.0)
    assert o3.ema is None and o3.core.ema is None
    for t in range(1, 4):
        _train(m3, o3, t)
    bare = str(tmp_path / "bare.pt")
    ck.save_worker_checkpoint(bare, m3, o3, 3)
    m4, o4 = _net_opt("async", seed=5, **kw)
    with caplog.at_level(logging.WARNING):
        ck.load_worker_checkpoint(bare, m4, o4)
    assert "EMA" in caplog.text
    assert torch.equal(o4.arena.p32, o3.arena.p32) and torch.equal(o4.core.ema, o3.arena.p32)
    assert torch.equal(o4.ema._views()[0], m3.bn.running_mean)
    assert o4.core.t == 3 and o4.core.ema_updates == 1

    # EMA state in a checkpoint is ignored when EMA is off
    m5, o5 = _net_opt("async", seed=6, ema_decay=0.0, ema_every=1, ema_warmup=False,
                      max_grad_norm=5.0)
    ck.load_worker_checkpoint(path, m5, o5)
    assert o5.ema is None and o5.core.ema is None and o5.core.t == 6
    assert torch.equal(o5.arena.p32, o1.arena.p32)
    assert "ema" not in o5.core.state_dict() and "ema_updates" not in o5.core.state_dict()


def test_cli_and_config_refusals():
    from distributed_ml_pytorch_amd.cli import build_parser, config_from_args
    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, Worker

    def cfg(*argv):
        return config_from_args(build_parser().parse_args(list(argv)))

    c = cfg("--model-ema", "0.999", "--model-ema-every", "32", "--model-ema-warmup")
    assert (c.model_ema, c.model_ema_every, c.model_ema_warmup) == (0.999, 32, True)
    c = cfg()
    assert (c.model_ema, c.model_ema_every, c.model_ema_warmup) == (0.0, 1, False)
    for argv in (["--model-ema", "1.0"], ["--model-ema", "-0.5"], ["--model-ema-every", "4"],
                 ["--model-ema-warmup"], ["--model-ema", "0.9", "--model-ema-every", "0"],
                 ["--model-ema-every", "1"]):
        with pytest.raises(ValueError, match="model-ema"):
            cfg(*argv)
    info = DistInfo(device=torch.device("cpu"))
    for kw in (dict(model_ema=1.0), dict(model_ema=0.9, model_ema_every=0),
               dict(model_ema_every=2), dict(model_ema_warmup=True)):
        with pytest.raises(ValueError, match="model-ema"):
            Worker(TrainConfig(model="mlp", cuda=False, mode="single", **kw), info)


def test_virtual_workers_refuse_model_ema():
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig
    from distributed_ml_pytorch_amd.runtime.virtual import VirtualWorkers

    cfg = TrainConfig(model="mlp", cuda=False, mode="asgd", ps="local", model_ema=0.9,
                      evaluate=False, verbose=False)
    with pytest.raises(ValueError, match="model-ema"):
        VirtualWorkers(cfg, 2, torch.device("cpu"))


def test_worker_evaluates_the_average():
    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, Worker

    cfg = TrainConfig(model="mlp", batch_size=16, cuda=False, mode="single", lr=0.1,
                      model_ema=0.9, model_ema_every=2, evaluate=False, verbose=False)
    w = Worker(cfg, DistInfo(device=torch.device("cpu")))
    assert w.opt.core is not None and w.opt.ema is not None
    g = torch.Generator().manual_seed(0)
    x = torch.randn(16, *w.input_shape, generator=g)
    y = torch.randint(0, w.num_classes, (16,), generator=g)
    for _ in range(4):
        w.train_step(x, y)
    assert w.opt.core.ema_updates == 2
    p0 = w.arena.p32.clone()
    live = w.evaluate([(x, y)])
    avg = w.evaluate([(x, y)], ema=True)
    assert live[0] != avg[0]
    assert torch.equal(w.arena.p32, p0)
    plain = Worker(TrainConfig(model="mlp", cuda=False, mode="single", evaluate=False,
                               verbose=False), DistInfo(device=torch.device("cpu")))
    assert getattr(plain.opt, "core", None) is None           # defaults: the by-value path
    with pytest.raises(ValueError, match="model_ema"):
        plain.evaluate([(x, y)], ema=True)
