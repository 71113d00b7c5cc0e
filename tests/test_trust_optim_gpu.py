"""LAMB and LARS on the GPU (csrc/optim_trust.hip): the three-launch step against
the fp64 oracle of test_trust_optim_cpu.py on an arena whose tensors sit on the
kernels' edges, pad elements, graph replay and reproducibility, the bindings'
refusals and the Worker path.

Accuracy bound, the project's own (fused_optim_oracle.accuracy_report): the
native error against the fp64 oracle is at most 4 x the error of the fp32 CPU
path against the same oracle, plus one fp32 ulp of the largest magnitude.
profiles/lamb_lars.txt holds the worst ratios measured on an MI355X.
"""
import functools
import math

import pytest
import torch

from fused_optim_oracle import max_err, ulp_of
from test_trust_optim_cpu import CASES, core_pads, make_arena, make_core, oracle, run

pytestmark = pytest.mark.gpu

DEV = "cuda"
KINDS = ["lamb", "lars"]
EMA = 0.9


def _nat():
    from distributed_ml_pytorch_amd.ops._ext import native

    return native()


@functools.lru_cache(maxsize=None)
def _reference(kind, wd, clip, ema):
    """(fp64 oracle, error of the fp32 CPU path against it), computed once."""
    arena, grads = make_arena()
    p0 = arena.p32.clone()
    core = make_core(arena, kind, wd, clip, ema_decay=ema)
    cpu = run(core, arena, grads, acc=torch.zeros(arena.numel))
    ref = oracle(kind, arena.slots, p0, grads, wd, clip, ema)
    return ref, {k: max_err(x, ref[k]) for k, x in cpu.items()}


def _gpu_run(kind, wd=0.05, clip=False, acc=True, ema=0.0, steps=None, **attrs):
    arena, grads = make_arena(DEV)
    core = make_core(arena, kind, wd, clip, ema_decay=ema)
    for k, v in attrs.items():
        setattr(core, k, v)
    a = torch.zeros(arena.numel, device=DEV) if acc else None
    return arena, core, run(core, arena, grads[:steps], a)


@pytest.mark.parametrize("ema", [0.0, EMA], ids=["noema", "ema"])
@pytest.mark.parametrize("acc", [False, True], ids=["noacc", "acc"])
@pytest.mark.parametrize("wd,clip", CASES)
@pytest.mark.parametrize("kind", KINDS)
def test_three_steps_against_fp64_oracle(kind, wd, clip, acc, ema):
    ref, cpu_err = _reference(kind, wd, clip, ema)
    arena, _, got = _gpu_run(kind, wd, clip, acc, ema)
    assert set(got) == set(cpu_err) - (set() if acc else {"acc"})
    rows = {k: (max_err(x, ref[k]), cpu_err[k], 4.0 * cpu_err[k] + ulp_of(ref[k]))
            for k, x in got.items()}
    for k, (en, ec, bound) in rows.items():
        print(f"{kind} wd={wd} clip={clip} acc={acc} ema={ema} {k}: native err {en:.3e}  "
              f"cpu-fp32 err {ec:.3e}  bound {bound:.3e}  ratio {en / bound:.3f}")
    for k, (en, ec, bound) in rows.items():
        assert en <= bound, (k, en, ec, bound)
    assert torch.equal(arena.w16, arena.p32.to(torch.bfloat16))
    assert (core_pads(arena, arena.p32) == 0).all()


@pytest.mark.parametrize("kind", KINDS)
def test_pad_elements_never_enter_a_norm(kind):
    """1e30 in every pad element of p32 and g32 before the steps: the same trust
    values and the same parameters bit for bit, and the pads keep what they hold."""
    _, _, clean = _gpu_run(kind)
    arena, grads = make_arena(DEV)
    pad = torch.ones(arena.numel, dtype=torch.bool)
    for s in arena.slots:
        pad[s.offset:s.offset + s.numel] = False
    pad = pad.to(DEV)
    arena.p32[pad] = 1e30
    dirty = run(make_core(arena, kind, 0.05, False), arena,
                [torch.where(pad.cpu(), torch.tensor(1e30), g) for g in grads],
                torch.zeros(arena.numel, device=DEV))
    assert torch.equal(dirty["trust"], clean["trust"])
    assert torch.equal(dirty["p"][~pad], clean["p"][~pad])
    assert (dirty["p"][pad] == 1e30).all() and (dirty["acc"][pad] == 0).all()


@pytest.mark.parametrize("kind", KINDS)
def test_graph_replay_and_fresh_runs_are_bitwise_equal(kind):
    """Three replays of ONE captured step equal three eager steps, a second fresh
    run equals the first, and so does a run on three workgroups (grid-strided
    chunks): partial k covers the same elements whatever the grid."""
    _, _, eager = _gpu_run(kind, clip=True, ema=EMA)
    _, _, again = _gpu_run(kind, clip=True, ema=EMA)
    _, _, narrow = _gpu_run(kind, clip=True, ema=EMA, trust_grid_cap=3)
    arena, grads = make_arena(DEV)
    core = make_core(arena, kind, 0.05, True, ema_decay=EMA)
    acc = torch.zeros(arena.numel, device=DEV)
    mom = torch.zeros_like(arena.p32) if kind == "lars" else None
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        core.step(arena, acc, mom)
    trust = []
    for g in grads:
        arena.g32.copy_(g)
        graph.replay()
        trust.append(core.trust_ratios()[:, 0])
    assert core.t == len(grads)                         # the capture itself applied nothing
    state = dict(mom=mom) if kind == "lars" else dict(m=core.m, v=core.v)
    replayed = dict(p=arena.p32, trust=torch.stack(trust), acc=acc, e=core.ema, **state)
    for other in (again, narrow, replayed):
        assert set(other) == set(eager)
        for k in eager:
            assert torch.equal(other[k], eager[k]), k


def test_bindings_refuse_bad_arguments():
    nat = _nat()
    arena, core, _ = _gpu_run("lamb", steps=1)
    n, chunk = arena.numel, nat.trust_chunk()
    good = dict(g=arena.g32, p=arena.p32, acc=None, m=core.m, v=core.v, w16=arena.w16,
                chunks=core.chunks, tens=core.tens, partials=core.trust_partials,
                trust=core.trust, hyper=core.hyper, wd=0.0, eps=1e-6)
    nat.lamb_fused_step(**good)
    bad = {
        "chunks_on_host": dict(chunks=core.chunks.cpu()),
        "chunks_int64": dict(chunks=core.chunks.long()),
        "tens_two_columns": dict(tens=core.tens[:, :2].contiguous()),
        "partials_short": dict(partials=core.trust_partials[:-2]),
        "trust_short": dict(trust=core.trust.flatten()[:-4]),
        "n_not_64": {k: good[k][:n - 4] for k in ("g", "p", "m", "v", "w16")},
    }
    for name, kw in bad.items():
        with pytest.raises(RuntimeError):
            nat.lamb_fused_step(**{**good, **kw})
            pytest.fail(f"{name} was accepted")
    lars = {k: v for k, v in good.items() if k not in ("m", "v", "eps")}
    lars.update(mom=torch.zeros_like(arena.p32), momentum=0.9, trust_coef=0.001, lars_eps=0.0)
    with pytest.raises(RuntimeError):
        nat.lars_fused_step(**{**lars, "partials": core.trust_partials[:-2]})
    # the host-side check of the tables, before they reach the device
    chunks, tens = core.chunks.cpu(), core.tens.cpu()
    nat.trust_check_tables(chunks, tens, n)
    long_chunk, crossing, unaligned = chunks.clone(), chunks.clone(), chunks.clone()
    long_chunk[0, 2] = chunk + 1
    crossing[-1, 1] = n - 64
    crossing[-1, 2] = 65
    unaligned[0, 1] = 4
    for t in (long_chunk, crossing, unaligned, chunks.long()):
        with pytest.raises(RuntimeError):
            nat.trust_check_tables(t, tens, n)
    with pytest.raises(RuntimeError):
        nat.trust_check_tables(chunks, tens, n - 4)


def _is_copy(name: str) -> bool:
    return name.startswith(("__amd_rocclr_copyBuffer", "Memcpy", "memcpy"))


@pytest.mark.strict_native
@pytest.mark.parametrize("model,batch", [("mlp", 16), ("convnext_mini", 8)])
def test_worker_trains_with_lamb_on_native_kernels_only(model, batch):
    from torch.profiler import ProfilerActivity, profile

    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, Worker

    cfg = TrainConfig(model=model, batch_size=batch, optimizer="lamb", lr=2e-3, weight_decay=0.01,
                      clip_grad_norm=1.0, mode="single", evaluate=False, verbose=False)
    w = Worker(cfg, DistInfo(device=torch.device(DEV, 0)))
    gen = torch.Generator().manual_seed(0)
    x, y = w.prepare(torch.randn(batch, *w.input_shape, generator=gen),
                     torch.randint(0, w.num_classes, (batch,), generator=gen))
    losses = [float(w.train_step(x, y)[0].float().item())]
    with profile(activities=[ProfilerActivity.CUDA]) as prof:       # one eager step
        loss, _ = w.train_step(x, y)
        torch.cuda.synchronize()
    losses.append(float(loss.float().item()))
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    foreign = sorted({n for n in names if "dmp::" not in n and not _is_copy(n)})
    assert not foreign, f"non-native device kernels in a LAMB step of {model}: {foreign}"
    for k in ("lamb_stage1_kernel", "trust_reduce_kernel", "lamb_stage2_kernel"):
        assert any(k in n for n in names), (k, sorted(set(names)))
    assert w.enable_graph()
    graphs = []
    for _ in range(18):
        loss, _ = w.train_step(x, y)
        losses.append(float(loss.float().item()))
        graphs.append(w.graph)
    w.finish()
    assert graphs[1] is not None and all(g is graphs[1] for g in graphs[1:])   # captured once
    assert all(math.isfinite(v) for v in losses), losses
    assert losses[-1] < losses[0], losses
    r = w.opt.core.trust_ratios()
    assert torch.isfinite(r).all() and (r[:, 0] > 0).all() and (r[:, 0] != 1).any()
