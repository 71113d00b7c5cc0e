"""Model EMA on the GPU: the EMA instantiations of the fused step kernels, the
hyper-block words, arena_swap, ema_buffers (csrc/optim.hip), graph replay, the
bindings' argument checks and the Worker paths (parallel/ema.py).

Every criterion is bit equality.  The EMA is compared with the formula
``e.mul(D).add(p.mul(O))`` applied in torch on the CPU to the kernel's own
read-back parameters (three fp32 roundings; ema_oracle.py is the same in NumPy,
checked against the CPU path by test_ema_cpu.py), never with another run's
parameters: the split weight-gradient reductions use atomics, so two training
runs need not agree bitwise.
"""
import types

import numpy as np
import pytest
import torch

import ema_oracle as eo

pytestmark = pytest.mark.gpu

DEV = "cuda"
DECAY = 0.97
LR = 1e-2
D_W, O_W, U_W = 17, 18, 19          # hyper-block words (csrc/optim.hip)


def _nat():
    from distributed_ml_pytorch_amd.ops._ext import native

    return native()


def _raw_arena(n, shadow=True, seed=0):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    return types.SimpleNamespace(numel=n, device=torch.device(DEV, 0), params=[], slots=[],
                                 p32=p.to(DEV), g32=torch.zeros(n, device=DEV),
                                 w16=torch.zeros(n, dtype=torch.bfloat16, device=DEV) if shadow
                                 else None)


def _core(arena, kind, mask=None, **kw):
    from distributed_ml_pytorch_amd.parallel.fused_optim import FusedOptimCore

    core = FusedOptimCore(arena, kind, LR, weight_decay=0.05,
                          momentum=0.9 if kind == "sgd" else 0.0, **kw)
    if kind == "adamw":
        core.mask = mask
    return core


def _mask(n):
    nb = n // 64
    return (torch.rand(nb, generator=torch.Generator().manual_seed(7)) < 0.6).to(torch.uint8).to(DEV)


def _cpu_ema(e, p, D, O):
    """The specification, in torch on the CPU."""
    return e if O == 0 else e.mul(D).add(p.mul(O))


# one mask block / lanes of one wave / grid-stride tail with an odd block count /
# more float4s than one trip of the 2048 x 256 grid
SIZES = [64, 256, 64 * 1021, 64 * 40000]


@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("full", [True, False], ids=["full", "nulls"])
@pytest.mark.parametrize("kind", ["adamw", "sgd"])
@pytest.mark.parametrize("n", SIZES)
def test_step_kernels_update_the_average(n, kind, full, every):
    """acc, w16 and the decay mask present and null; K = 3 runs with the decay warm-up."""
    warm = every == 3
    runs = []
    for ema in (False, True):
        a = _raw_arena(n, shadow=full)
        kw = dict(ema_decay=DECAY, ema_every=every, ema_warmup=warm) if ema else {}
        core = _core(a, kind, mask=_mask(n) if full else None, **kw)
        acc = torch.zeros(n, device=DEV) if full else None
        mom = torch.zeros(n, device=DEV) if kind == "sgd" else None
        runs.append((a, core, acc, mom))
    (a0, c0, acc0, mom0), (a1, c1, acc1, mom1) = runs
    assert c0.ema is None and torch.equal(c1.ema, a1.p32)
    e = a1.p32.cpu()
    gen = torch.Generator().manual_seed(n + 1)
    for t in range(1, 6):
        g = torch.randn(n, generator=gen).to(DEV)
        for a, c, acc, mom in runs:
            a.g32.copy_(g)
            c.step(a, acc, mom, 0.0)
        u, D, O = eo.coeffs(DECAY, every, warm, t)
        h = c1.hyper.cpu()
        assert (float(h[D_W]), float(h[O_W]), int(h.view(torch.int32)[U_W])) == \
            (float(D), float(O), u)
        before = e
        e = _cpu_ema(e, a1.p32.cpu(), float(D), float(O))
        got = c1.ema.cpu()
        assert torch.equal(got, e), (t, int((got != e).sum()))
        if t % every:
            assert torch.equal(got, before)                 # a step between two updates
        assert np.array_equal(got.numpy(), eo.update(before.numpy(), a1.p32.cpu().numpy(), D, O))
    assert c1.ema_updates == 5 // every and c0.ema_updates == 0
    assert not torch.equal(c1.ema, a1.p32)
    # nothing else moved: the EMA-off run of the same inputs
    assert torch.equal(a0.p32, a1.p32)
    if full:
        assert torch.equal(acc0, acc1) and torch.equal(a0.w16, a1.w16)
        assert torch.equal(a1.w16, a1.p32.bfloat16())
    if kind == "sgd":
        assert torch.equal(mom0, mom1)
    else:
        assert torch.equal(c0.m, c1.m) and torch.equal(c0.v, c1.v)
    assert torch.equal(c0.hyper[:17], c1.hyper[:17])
    assert not c0.hyper[17:].any()                          # EMA off: none of the words is written


@pytest.mark.parametrize("warm", [False, True])
@pytest.mark.parametrize("every", [1, 3])
def test_hyper_words_follow_the_oracle(every, warm):
    a = _raw_arena(64)
    core = _core(a, "sgd", ema_decay=DECAY, ema_every=every, ema_warmup=warm)
    nat = _nat()
    for t in range(1, 41):
        nat.optim_hyper(core.hyper, None, None)
        h = core.hyper.cpu()
        hi = h.view(torch.int32)
        u, D, O = eo.coeffs(DECAY, every, warm, t)
        assert int(hi[0]) == t and int(hi[U_W]) == u
        assert h[D_W].numpy().view(np.uint32) == D.view(np.uint32), (t, float(h[D_W]), D)
        assert h[O_W].numpy().view(np.uint32) == O.view(np.uint32), (t, float(h[O_W]), O)
    assert float(h[20]) == float(np.float32(DECAY)) and int(hi[21]) == every and int(hi[22]) == warm
    assert core.ema_updates == 40 // every


@pytest.mark.parametrize("shadow", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_arena_swap(n, shadow):
    nat = _nat()
    g = torch.Generator().manual_seed(n)
    p0, e0 = torch.randn(n, generator=g), torch.randn(n, generator=g)
    p, e = p0.to(DEV), e0.to(DEV)
    w16 = p.bfloat16() if shadow else None
    w0 = w16.clone() if shadow else None
    nat.arena_swap(p, e, w16)
    assert torch.equal(p.cpu(), e0) and torch.equal(e.cpu(), p0)
    if shadow:
        assert torch.equal(w16, p.bfloat16()) and not torch.equal(w16, w0)
    nat.arena_swap(p, e, w16)
    assert torch.equal(p.cpu(), p0) and torch.equal(e.cpu(), e0)
    if shadow:
        assert torch.equal(w16, w0)


def _buffer_table(sizes=(1, 6, 64, 2048)):
    """Live buffers carved out of one allocation at odd element offsets, and a
    flat EMA tensor with entries at offsets 0, 1, 7, 71."""
    g = torch.Generator().manual_seed(3)
    pool = torch.randn(sum(sizes) + 3 * len(sizes), generator=g).to(DEV)
    live, offs, at, off = [], [], 1, 0
    for s in sizes:
        live.append(pool[at:at + s])
        at += s + 3
        offs.append(off)
        off += s
    flat = torch.randn(off, generator=g).to(DEV)
    table = torch.tensor([[b.data_ptr(), o, b.numel()] for b, o in zip(live, offs)],
                         dtype=torch.int64).to(DEV)
    assert any(o % 2 for o in offs) and any(b.data_ptr() % 16 for b in live)
    return pool, live, offs, flat, table


def test_ema_buffers_kernel():
    nat = _nat()
    pool, live, offs, flat, table = _buffer_table()
    core = _core(_raw_arena(64), "sgd", ema_decay=DECAY, ema_every=2, ema_warmup=True)
    pool0 = pool.clone()
    want = flat.cpu()
    for t in range(1, 5):
        nat.optim_hyper(core.hyper, None, None)
        nat.ema_buffers(table, flat, core.hyper, 0)
        _, D, O = eo.coeffs(DECAY, 2, True, t)
        before = want
        want = want.clone()
        for b, o in zip(live, offs):
            want[o:o + b.numel()] = _cpu_ema(before[o:o + b.numel()], b.cpu(), float(D), float(O))
        assert torch.equal(flat.cpu(), want), t
        if t % 2:
            assert torch.equal(want, before)
        assert torch.equal(pool, pool0)                      # the live side is only read
    # exchange, and back
    f0 = flat.clone()
    nat.ema_buffers(table, flat, core.hyper, 1)
    for b, o in zip(live, offs):
        assert torch.equal(b, f0[o:o + b.numel()])
        at = (b.data_ptr() - pool.data_ptr()) // 4
        assert torch.equal(flat[o:o + b.numel()], pool0[at:at + b.numel()])
    gaps = torch.ones_like(pool, dtype=torch.bool)
    for b in live:
        at = (b.data_ptr() - pool.data_ptr()) // 4
        gaps[at:at + b.numel()] = False
    assert torch.equal(pool[gaps], pool0[gaps])              # nothing outside the entries
    nat.ema_buffers(table, flat, core.hyper, 1)
    assert torch.equal(pool, pool0) and torch.equal(flat, f0)
    # a row that does not fit in flat is skipped on the device
    bad = table.clone()
    bad[3, 1] = flat.numel() - 5
    nat.ema_buffers(bad[3:], flat, core.hyper, 1)
    assert torch.equal(pool, pool0) and torch.equal(flat, f0)


def test_graph_replay_is_bitwise_eager():
    n, steps = 64 * 1021, 9
    kw = dict(ema_decay=DECAY, ema_every=3, ema_warmup=True)
    ea, ga = _raw_arena(n), _raw_arena(n)
    eager, graphed = _core(ea, "adamw", mask=_mask(n), **kw), _core(ga, "adamw", mask=_mask(n), **kw)
    acc_e, acc_g = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    gen = torch.Generator().manual_seed(2)
    grads = [torch.randn(n, generator=gen).to(DEV) for _ in range(steps)]
    for g in grads:
        ea.g32.copy_(g)
        eager.step(ea, acc_e)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.step(ga, acc_g)
    for g in grads:
        ga.g32.copy_(g)
        graph.replay()
    torch.cuda.synchronize()
    assert graphed.t == steps and graphed.ema_updates == 3
    for x, y in ((ea.p32, ga.p32), (eager.ema, graphed.ema), (eager.m, graphed.m),
                 (eager.v, graphed.v), (acc_e, acc_g), (ea.w16, ga.w16)):
        assert torch.equal(x, y)
    assert not torch.equal(graphed.ema, ga.p32)


def test_bindings_refuse_bad_arguments():
    nat = _nat()
    n = 256
    a = _raw_arena(n)
    core = _core(a, "adamw", mask=_mask(n), ema_decay=DECAY)
    adam = (a.g32, a.p32, None, core.m, core.v, a.w16, core.mask, core.hyper, 0.0, 1e-8)
    sgd = (a.g32, a.p32, None, None, a.w16, core.hyper, 0.0, 0.0, 0.0, False)
    strided = torch.zeros(2 * n, device=DEV)[::2]           # n elements, not contiguous
    for bad in (core.ema.double(), core.ema[:128], core.ema.cpu(), a.p32, strided):
        with pytest.raises(RuntimeError, match="ema"):
            nat.adamw_fused_step(*adam, bad)
        with pytest.raises(RuntimeError, match="ema"):
            nat.asgd_fused_step_dev(*sgd, bad)
        with pytest.raises(RuntimeError, match="ema"):
            nat.arena_swap(a.p32, bad, a.w16)
    _, _, _, flat, table = _buffer_table()
    for bad in (table.int(), table[:, :2].contiguous(), table.cpu(), table.t()):
        with pytest.raises(RuntimeError, match="table"):
            nat.ema_buffers(bad, flat, core.hyper, 0)
    with pytest.raises(RuntimeError, match="flat"):
        nat.ema_buffers(table, flat.double(), core.hyper, 0)
    with pytest.raises(RuntimeError, match="hyper block"):
        nat.ema_buffers(table, flat, core.hyper[:20], 0)
    with pytest.raises(RuntimeError, match="mode"):
        nat.ema_buffers(table, flat, core.hyper, 2)


# ------------------------------------------------------------------- workers
EVERY = 2
WORKERS = {"resnet18": dict(model="resnet18", mode="asgd", ps="local", n_push=1, n_pull=1, lr=0.01,
                            momentum=0.9),
           "vit_tiny": dict(model="vit_tiny", mode="single", optimizer="adamw", lr=1e-3,
                            weight_decay=0.05)}


def _worker(name, **kw):
    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, Worker

    cfg = dict(batch_size=8, model_ema=DECAY, model_ema_every=EVERY, model_ema_warmup=True,
               evaluate=False, verbose=False)
    cfg.update(WORKERS[name])
    cfg.update(kw)
    w = Worker(TrainConfig(**cfg), DistInfo(device=torch.device(DEV, 0)))
    g = torch.Generator().manual_seed(0)
    x = torch.randn(8, *w.input_shape, generator=g)
    y = torch.randint(0, w.num_classes, (8,), generator=g)
    return w, w.prepare(x, y)


def _record_steps(w):
    """Read p32 and the averaged buffers back right after every local_step, before
    the push / pull / land half of the step can overwrite the parameters."""
    seen = []
    comm = w.opt.comm_step

    def recording():
        seen.append((w.arena.p32.cpu(), [b.cpu().clone() for b in w.opt.ema.live]))
        return comm()

    w.opt.comm_step = recording
    return seen


def _replay(w, e, bufs, seen, t0=0):
    for i, (p, live) in enumerate(seen):
        _, D, O = eo.coeffs(DECAY, EVERY, True, t0 + i + 1)
        e = _cpu_ema(e, p, float(D), float(O))
        bufs = [_cpu_ema(b, l, float(D), float(O)) for b, l in zip(bufs, live)]
    return e, bufs


@pytest.mark.parametrize("name", list(WORKERS))
def test_worker_average_follows_its_own_parameters(name, monkeypatch):
    w, (x, y) = _worker(name)
    assert w.enable_graph(True)
    avg = w.opt.ema
    assert bool(avg.live) == (name == "resnet18")
    assert all(b.dtype == torch.float32 for b in avg.live)
    e0, b0 = w.opt.core.ema.cpu(), [v.cpu().clone() for v in avg._views()]
    assert torch.equal(e0, w.arena.p32.cpu())
    seen = _record_steps(w)
    for _ in range(6):
        w.train_step(x, y)
    torch.cuda.synchronize()
    assert w.graph is not None and len(seen) == 6
    assert w.opt.core.t == 6 and w.opt.core.ema_updates == 3
    e, bufs = _replay(w, e0, b0, seen)
    assert torch.equal(w.opt.core.ema.cpu(), e)
    for name_b, v, want in zip(avg.names, avg._views(), bufs):
        assert torch.equal(v.cpu(), want), name_b
    assert not torch.equal(w.opt.core.ema, w.arena.p32)
    # evaluation on the average, and everything back in place afterwards
    p0, w0 = w.arena.p32.clone(), w.arena.w16.clone()
    live0 = {k: v.clone() for k, v in w.model.state_dict().items()}
    ema0, flat0 = w.opt.core.ema.clone(), avg.flat.clone()
    plain = w.evaluate([(x, y)])
    averaged = w.evaluate([(x, y)], ema=True)
    assert plain[0] != averaged[0]
    assert w.evaluate([(x, y)]) == plain
    assert torch.equal(w.arena.p32, p0) and torch.equal(w.arena.w16, w0)
    assert torch.equal(w.opt.core.ema, ema0) and torch.equal(avg.flat, flat0)
    for k, v in w.model.state_dict().items():
        assert torch.equal(v, live0[k]), k
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(RuntimeError, match="graph capture"):
            with avg.applied():
                pass
    assert torch.equal(w.arena.p32, p0) and torch.equal(w.opt.core.ema, ema0)
    w.train_step(x, y)                                  # the captured step still replays
    w.finish()
    assert w.opt.core.t == 7


def _is_copy(name: str) -> bool:
    return name.startswith(("__amd_rocclr_copyBuffer", "Memcpy", "memcpy"))


@pytest.mark.strict_native
@pytest.mark.parametrize("name", list(WORKERS))
def test_ema_steps_run_only_native_kernels(name):
    """One profiled eager step with the stock oracle mode OFF.  The ViT worker
    runs vit_mini_long here, as tests/test_drop_path_gpu.py does: vit_tiny's head
    dim 16 is outside the fused attention and raises in this mode, EMA or not."""
    from torch.profiler import ProfilerActivity, profile

    kw = dict(model="vit_mini_long") if name == "vit_tiny" else {}
    w, (x, y) = _worker(name, model_ema_every=1, **kw)
    w.train_step(x, y)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        w.train_step(x, y)
        torch.cuda.synchronize()
    w.finish()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert names, "profiler recorded no device work"
    foreign = sorted({n for n in names if "dmp::" not in n and not _is_copy(n)})
    assert not foreign, f"{name}: non-native device kernels in a training step: {foreign}"
    step = "asgd_fused_step_dev_kernel<true" if name == "resnet18" else \
        "adamw_fused_step_kernel<true"
    assert any(step in n for n in names), (step, sorted(set(names)))
    assert any("ema_buffers_kernel" in n for n in names) == (name == "resnet18")


def test_worker_checkpoint_roundtrip_gpu(tmp_path):
    from distributed_ml_pytorch_amd.utils import checkpoint as ck

    w1, (x, y) = _worker("resnet18")
    for _ in range(6):
        w1.train_step(x, y)
    path = str(tmp_path / "w.pt")
    ck.save_worker_checkpoint(path, w1.model, w1.opt, 6)
    # what was saved: finish() lands the outstanding pull and moves p32 after it
    p1, e1, f1 = w1.arena.p32.clone(), w1.opt.core.ema.clone(), w1.opt.ema.flat.clone()
    w1.finish()
    w2, _ = _worker("resnet18", seed=5)
    assert not torch.equal(w2.arena.p32, p1)
    assert ck.load_worker_checkpoint(path, w2.model, w2.opt) == 6
    assert w2.opt.core.t == 6 and w2.opt.core.ema_updates == 3
    assert torch.equal(w2.arena.p32, p1)
    assert torch.equal(w2.opt.core.ema, e1) and not torch.equal(e1, p1)
    assert torch.equal(w2.opt.ema.flat, f1)
    e0, b0 = w2.opt.core.ema.cpu(), [v.cpu().clone() for v in w2.opt.ema._views()]
    seen = _record_steps(w2)
    for _ in range(6):
        w2.train_step(x, y)
    w2.finish()
    e, bufs = _replay(w2, e0, b0, seen, t0=6)
    assert w2.opt.core.t == 12 and w2.opt.core.ema_updates == 6
    assert torch.equal(w2.opt.core.ema.cpu(), e)
    for v, want in zip(w2.opt.ema._views(), bufs):
        assert torch.equal(v.cpu(), want)
