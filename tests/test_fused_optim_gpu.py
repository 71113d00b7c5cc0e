"""Fused AdamW / device-hyper SGD kernels, the device-side schedule and clipping,
graph safety and the Worker paths on the GPU (csrc/optim.hip,
parallel/fused_optim.py).

Accuracy criterion: against the fp64 oracle of fused_optim_oracle.py (validated
against torch.optim.AdamW in fp64 by the CPU suite), the native maximum
absolute error in p, m, v after 5 steps is at most 4 x the error of
torch.optim.AdamW run in fp32 on the CPU on the same inputs, plus one fp32 ulp
of the largest magnitude.  Both errors are printed per case (``pytest -s``);
profiles/fused_adamw.txt holds the table measured on an MI355X.
"""
import math
import types

import numpy as np
import pytest
import torch

from fused_optim_oracle import accuracy_report, oracle_adamw, sched_lr, torch_adamw

pytestmark = pytest.mark.gpu

DEV = "cuda"
BETAS = (0.9, 0.999)
EPS = 1e-8
LR = 1e-3


def _nat():
    from distributed_ml_pytorch_amd.ops._ext import native

    return native()


def _raw_arena(n, shadow=True, seed=0):
    """A flat arena of raw tensors (no model): what the kernels see."""
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g)
    a = types.SimpleNamespace(numel=n, device=torch.device(DEV, 0), params=[], slots=[],
                              p32=p.to(DEV), g32=torch.zeros(n, device=DEV),
                              w16=torch.zeros(n, dtype=torch.bfloat16, device=DEV) if shadow
                              else None)
    return a, p


def _core(arena, kind="adamw", mask=None, **kw):
    from distributed_ml_pytorch_amd.parallel.fused_optim import FusedOptimCore

    core = FusedOptimCore(arena, kind, kw.pop("lr", LR), betas=BETAS, eps=EPS, **kw)
    if kind == "adamw":
        core.mask = mask.to(DEV) if mask is not None else None
    return core


def _mask(n, kind):
    nb = n // 64
    if kind is None:
        return None
    if nb <= 4:
        return torch.tensor([1, 0, 1, 0][:nb], dtype=torch.uint8)
    return (torch.rand(nb, generator=torch.Generator().manual_seed(7)) < 0.6).to(torch.uint8)


def _ulps(a, b):
    """max |a - b| in units of the fp32 spacing at the larger magnitude."""
    a = a.detach().float().cpu().numpy()
    b = b.detach().float().cpu().numpy()
    sp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32))
    return float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)) / sp))


# option sets: every switch of the kernel appears on and off
#   clip: None = off, "below" / "above" the bound, "zero" = all-zero gradient
OPTIONS = {
    "plain":       dict(acc=True, shadow=True, mask=True, wd=0.05, clip=None, gs=1.0),
    "nulls_below": dict(acc=False, shadow=False, mask=False, wd=0.0, clip="below", gs=1.0),
    "above_gs":    dict(acc=True, shadow=True, mask=True, wd=0.05, clip="above", gs=0.25),
    "zero_grad":   dict(acc=True, shadow=True, mask=True, wd=0.05, clip="zero", gs=1.0),
}
# one mask block / lanes of one wave under different flags / grid-stride tail with
# an odd block count / sumsq partials at the 1024-block cap / more float4s than
# one trip of the 2048 x 256 grid
SIZES = [64, 256, 64 * 1021, 64 * 20000, 64 * 40000]


@pytest.mark.parametrize("opt", list(OPTIONS))
@pytest.mark.parametrize("n", SIZES)
def test_adamw_kernel_against_oracle(n, opt):
    o = OPTIONS[opt]
    steps, max_norm = 5, (1.0 if o["clip"] else 0.0)
    arena, p0 = _raw_arena(n, o["shadow"])
    mask = _mask(n, True if o["mask"] else None)
    core = _core(arena, mask=mask, weight_decay=o["wd"], grad_scale=o["gs"],
                 max_grad_norm=max_norm)
    assert (core.partials is None) == (o["clip"] is None)      # clipping off: no norm launch
    acc = torch.zeros(n, device=DEV) if o["acc"] else None
    gen = torch.Generator().manual_seed(n + 1)
    target = {None: 1.0, "below": 0.5, "above": 5.0, "zero": 0.0}[o["clip"]]
    grads = [torch.randn(n, generator=gen) * (target / o["gs"] / math.sqrt(n))
             for _ in range(steps)]
    acc_sum = torch.zeros(n, device=DEV)
    gscales, norms = [], []
    for g in grads:
        before = arena.p32.clone()
        arena.g32.copy_(g)
        core.step(arena, acc)
        acc_sum += arena.p32 - before
        h = core.hyper.cpu()
        gscales.append(float(h[2])), norms.append(float(h[5]))
    decay = mask.repeat_interleave(64) if mask is not None else None
    kw = dict(decay=decay, lr=LR, betas=BETAS, eps=EPS, wd=o["wd"], grad_scale=o["gs"],
              max_norm=max_norm)
    ref = oracle_adamw(p0, grads, **kw)
    t32 = torch_adamw(p0, grads, dtype=torch.float32, **kw)
    got = dict(p=arena.p32, m=core.m, v=core.v)
    rows = accuracy_report(got, t32, ref)
    for k, (en, et, bound) in rows.items():
        print(f"adamw n={n} {opt} {k}: native err {en:.3e}  torch-fp32 err {et:.3e}  "
              f"bound {bound:.3e}  ratio {en / et if et else float('nan'):.2f}")
    for k, (en, et, bound) in rows.items():
        assert en <= bound, (k, en, et, bound)
    assert core.t == steps
    # gradient scale: exact wherever no clipping happens
    gs32 = float(np.float32(o["gs"]))
    if o["clip"] in (None, "below", "zero"):
        assert gscales == [gs32] * steps
    else:
        want = [o["gs"] * c for c in ref["clips"]]
        assert max(ref["clips"]) < 1.0
        assert gscales == pytest.approx(want, rel=2e-6)
    if o["clip"] is None:
        assert norms == [0.0] * steps
    else:
        assert norms == pytest.approx(ref["norms"], rel=2e-6, abs=0.0)
    if o["clip"] == "zero":
        # parameters move by decay only; undecayed blocks do not move at all
        assert not core.m.any() and not core.v.any()
        keep = decay.bool()
        assert torch.equal(arena.p32.cpu()[~keep], p0[~keep])
        assert not torch.equal(arena.p32.cpu()[keep], p0[keep])
    if arena.w16 is not None:
        assert torch.equal(arena.w16, arena.p32.bfloat16())
    if acc is not None:
        assert torch.equal(acc, acc_sum)


def test_adamw_without_mask_decays_everything():
    n = 256
    arena, p0 = _raw_arena(n)
    core = _core(arena, mask=None, weight_decay=0.05)
    core.step(arena, None)                       # zero gradient: decay only
    assert not torch.equal(arena.p32.cpu()[64:128], p0[64:128])
    ref = oracle_adamw(p0, [torch.zeros(n)], lr=LR, betas=BETAS, eps=EPS, wd=0.05)
    assert _ulps(arena.p32, ref["p"].float()) <= 1


def test_bindings_refuse_bad_arguments():
    nat = _nat()
    n = 256
    arena, _ = _raw_arena(n)
    core = _core(arena, mask=_mask(n, True))
    z = torch.zeros(n, device=DEV)
    ok = (arena.g32, arena.p32, None, core.m, core.v, arena.w16)
    with pytest.raises(RuntimeError, match="decay mask"):
        nat.adamw_fused_step(*ok, torch.zeros(3, dtype=torch.uint8, device=DEV), core.hyper,
                             0.0, EPS)
    with pytest.raises(RuntimeError, match="hyper block"):
        nat.adamw_fused_step(*ok, core.mask, torch.zeros(4, device=DEV), 0.0, EPS)
    with pytest.raises(RuntimeError, match="elements"):
        nat.adamw_fused_step(arena.g32, arena.p32, None, core.m, z[:128], arena.w16, core.mask,
                             core.hyper, 0.0, EPS)
    with pytest.raises(RuntimeError, match="dtype"):
        nat.asgd_fused_step_dev(arena.g32.double(), arena.p32, None, None, None, core.hyper,
                                0.0, 0.0, 0.0, False)
    with pytest.raises(RuntimeError, match="partials"):
        nat.optim_hyper(core.hyper, arena.g32, torch.zeros(8, device=DEV))
    with pytest.raises(RuntimeError, match="together"):
        nat.optim_hyper(core.hyper, arena.g32, None)


SGD_VARIANTS = [dict(momentum=0.0, nesterov=False, wd=0.0),
                dict(momentum=0.9, nesterov=False, wd=0.0),
                dict(momentum=0.9, nesterov=True, wd=1e-3),
                dict(momentum=0.0, nesterov=False, wd=1e-3)]


@pytest.mark.parametrize("v", SGD_VARIANTS, ids=lambda v: "m{momentum}_n{nesterov:d}_wd{wd}".format(**v))
def test_sgd_dev_is_bitwise_sgd_at_constant_lr(v):
    nat = _nat()
    n, lr = 64 * 1021, 0.05
    a1, _ = _raw_arena(n)
    a2, _ = _raw_arena(n)
    core = _core(a2, "sgd", lr=lr, weight_decay=v["wd"], momentum=v["momentum"],
                 nesterov=v["nesterov"])
    acc1, acc2 = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    mom1 = torch.zeros(n, device=DEV) if v["momentum"] else None
    mom2 = torch.zeros(n, device=DEV) if v["momentum"] else None
    gen = torch.Generator().manual_seed(3)
    for i in range(3):
        g = torch.randn(n, generator=gen).to(DEV)
        damp = 0.1 if i else 0.0
        a1.g32.copy_(g), a2.g32.copy_(g)
        nat.asgd_fused_step(a1.g32, a1.p32, acc1, mom1, a1.w16, lr, v["wd"], v["momentum"],
                            damp, v["nesterov"])
        core.step(a2, acc2, mom2, damp)
    assert float(core.hyper.cpu()[2]) == 1.0 and core.t == 3
    assert torch.equal(a1.p32, a2.p32) and torch.equal(acc1, acc2)
    assert torch.equal(a1.w16, a2.w16)
    if mom1 is not None:
        assert torch.equal(mom1, mom2)


def test_sgd_dev_with_clipping_is_sgd_on_scaled_gradients():
    nat = _nat()
    n, lr, wd, mu = 64 * 1021, 0.05, 1e-3, 0.9
    a1, _ = _raw_arena(n)
    a2, _ = _raw_arena(n)
    core = _core(a2, "sgd", lr=lr, weight_decay=wd, momentum=mu, grad_scale=0.5,
                 max_grad_norm=1.0)
    mom1, mom2 = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    gen = torch.Generator().manual_seed(4)
    for i in range(3):
        g = (torch.randn(n, generator=gen) * 0.1).to(DEV)      # norm ~ 0.5 * 25: clips
        a2.g32.copy_(g)
        core.step(a2, None, mom2, 0.0)
        h = core.hyper.cpu()
        gscale, norm = float(h[2]), float(h[5])
        want = 0.5 * float(g.double().norm())
        assert norm == pytest.approx(want, rel=2e-6)
        assert gscale == pytest.approx(0.5 / (want + 1e-6), rel=2e-6) and gscale < 0.5
        a1.g32.copy_(g * gscale)
        nat.asgd_fused_step(a1.g32, a1.p32, None, mom1, a1.w16, lr, wd, mu, 0.0, False)
        assert _ulps(a1.p32, a2.p32) <= 2 and _ulps(mom1, mom2) <= 2


def test_set_base_lr_reaches_the_device():
    """Host-side schedules (inv_epoch) change the base lr between steps: the next
    device step uses it, and the step count survives the rewrite of the block."""
    nat = _nat()
    n = 64 * 1021
    a1, _ = _raw_arena(n)
    a2, _ = _raw_arena(n)
    core = _core(a2, "sgd", lr=0.1)
    g = torch.randn(n, generator=torch.Generator().manual_seed(5)).to(DEV)
    for lr in (0.1, 0.05, 0.025):
        core.set_base_lr(lr)
        a1.g32.copy_(g), a2.g32.copy_(g)
        nat.asgd_fused_step(a1.g32, a1.p32, None, None, a1.w16, lr, 0.0, 0.0, 0.0, False)
        core.step(a2, None)
        assert core.lr() == float(np.float32(lr))
        assert torch.equal(a1.p32, a2.p32)
    assert core.t == 3


def test_device_schedule_and_bias_corrections():
    nat = _nat()
    from distributed_ml_pytorch_amd.parallel.fused_optim import Schedule

    base, w, n, lo = 3e-3, 4, 10, 1e-5
    arena, _ = _raw_arena(64)
    core = _core(arena, lr=base, schedule=Schedule("warmup_cosine", w, n, lo))
    for t in range(1, 13):
        nat.optim_hyper(core.hyper, None, None)
        h = core.hyper.cpu()
        assert int(h.view(torch.int32)[0]) == t
        lr_t = float(h[1])
        want = sched_lr(base, t, "warmup_cosine", w, n, lo)
        assert abs(lr_t - want) <= 8 * 2.0 ** -24 * base, (t, lr_t, want)
        if t >= n:
            assert lr_t == float(np.float32(lo))
        for got, beta in ((float(h[3]), BETAS[0]), (float(h[4]), BETAS[1])):
            ref = np.float32(1.0 - beta ** t)
            assert abs(got - float(ref)) <= 4 * float(np.spacing(ref)), (t, beta, got, ref)
        assert float(h[2]) == 1.0 and float(h[5]) == 0.0


def _async_opt(seed=0, **kw):
    from distributed_ml_pytorch_amd.models import build_model
    from distributed_ml_pytorch_amd.parallel.asgd import Asynchronous
    from distributed_ml_pytorch_amd.parallel.clients import LocalPSClient
    from distributed_ml_pytorch_amd.parallel.fused_optim import Schedule

    torch.manual_seed(seed)
    model, _, _ = build_model("mlp")
    model = model.to(DEV)
    opt = Asynchronous(model.parameters(), lr=LR, n_push=10 ** 6, n_pull=10 ** 6, model=model,
                       client=LocalPSClient(staleness=0), optimizer="adamw", betas=BETAS,
                       eps=EPS, weight_decay=0.05, max_grad_norm=1.0,
                       schedule=Schedule("warmup_cosine", 3, 10, 1e-5), **kw)
    return model, opt


def _fixed_grads(arena, steps, seed=11):
    """Fixed gradients on the real elements (the padding between parameters never
    receives one in training and is not part of a checkpoint); odd steps clip."""
    n = arena.numel
    used = torch.zeros(n)
    for s in arena.slots:
        used[s.offset:s.offset + s.numel] = 1.0
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(n, generator=gen) * used * ((5.0 if i % 2 else 0.4) / math.sqrt(n)))
            .to(DEV) for i in range(steps)]


def test_graph_replay_is_bitwise_eager_through_a_changing_lr():
    _, eager = _async_opt()
    _, graphed = _async_opt()
    assert torch.equal(eager.arena.p32, graphed.arena.p32)
    grads = _fixed_grads(eager.arena, 12)
    for g in grads:
        eager.arena.g32.copy_(g)
        eager.local_step()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                       # ONE capture
        graphed.local_step()
    lrs = []
    for g in grads:
        graphed.arena.g32.copy_(g)
        graph.replay()
        lrs.append(graphed.core.lr())
    torch.cuda.synchronize()
    assert graphed.core.t == 12                         # the capture itself applied nothing
    for a, b in ((eager.arena.p32, graphed.arena.p32), (eager.core.m, graphed.core.m),
                 (eager.core.v, graphed.core.v), (eager.acc, graphed.acc),
                 (eager.arena.w16, graphed.arena.w16)):
        assert torch.equal(a, b)
    want = [sched_lr(LR, t, "warmup_cosine", 3, 10, 1e-5) for t in range(1, 13)]
    assert lrs == pytest.approx(want, rel=1e-6)
    assert len(set(lrs[:10])) == 10                     # twelve launches, ten distinct rates


def test_checkpoint_roundtrip_bitwise_gpu(tmp_path):
    from distributed_ml_pytorch_amd.utils import checkpoint as ck

    _, full = _async_opt()
    grads = _fixed_grads(full.arena, 6)
    for g in grads:
        full.arena.g32.copy_(g)
        full.local_step()
    m1, o1 = _async_opt()
    for g in grads[:3]:
        o1.arena.g32.copy_(g)
        o1.local_step()
    path = str(tmp_path / "w.pt")
    ck.save_worker_checkpoint(path, m1, o1, 3)
    m2, o2 = _async_opt(seed=99)
    assert ck.load_worker_checkpoint(path, m2, o2) == 3 and o2.core.t == 3
    for g in grads[3:]:
        o2.arena.g32.copy_(g)
        o2.local_step()
    for a, b in ((o2.arena.p32, full.arena.p32), (o2.core.m, full.core.m),
                 (o2.core.v, full.core.v), (o2.acc, full.acc), (o2.arena.w16, full.arena.w16)):
        assert torch.equal(a, b)
    assert o2.core.t == 6 and o2.core.lr() == full.core.lr()


def _worker(mode, **kw):
    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, Worker

    cfg = TrainConfig(model="mlp", batch_size=16, optimizer="adamw", lr_schedule="warmup_cosine",
                      warmup_steps=3, max_steps=12, clip_grad_norm=1.0, mode=mode, ps="local",
                      n_push=1, n_pull=1, evaluate=False, verbose=False, **kw)
    w = Worker(cfg, DistInfo(device=torch.device(DEV, 0)))
    g = torch.Generator().manual_seed(0)
    x = torch.randn(16, *w.input_shape, generator=g)
    y = torch.randint(0, w.num_classes, (16,), generator=g)
    return w, w.prepare(x, y)


@pytest.mark.parametrize("mode", ["asgd", "single"])
def test_worker_captures_once_and_trains(mode):
    w, (x, y) = _worker(mode)
    assert w.enable_graph()
    losses, graphs, lrs = [], [], []
    for _ in range(12):
        loss, _ = w.train_step(x, y)
        losses.append(float(loss.float().item()))
        graphs.append(w.graph)
        lrs.append(w.opt.core.lr())
    w.finish()
    assert graphs[1] is not None and all(g is graphs[1] for g in graphs[1:])   # no re-capture
    assert all(math.isfinite(v) for v in losses), losses
    assert losses[11] < losses[0], losses
    want = [sched_lr(w.cfg.lr, t, "warmup_cosine", 3, 12, 0.0) for t in range(1, 13)]
    assert lrs == pytest.approx(want, rel=1e-6)
    assert w.opt.param_groups[0]["lr"] == w.cfg.lr        # the graph key never changed
    assert w.opt.core.grad_norm() > 0


def test_master_equals_worker_after_each_round():
    """n_push = n_pull = 1, staleness 0 (the round's pull lands in the same step):
    when the push has been applied and before the pulled snapshot overwrites the
    worker, the PS master (old + (p_new - p_old)) and the worker's p_new agree
    to 4 ulp -- one rounding in p_new - p_old, one in the PS add."""
    w, (x, y) = _worker("asgd", staleness=0)
    client = w.opt.client
    worst = []
    land = client.land_due

    def checked_land(step, force=False):
        worst.append(_ulps(client.master, w.arena.p32))
        return land(step, force)

    client.land_due = checked_land
    for _ in range(6):
        w.train_step(x, y)
        assert torch.equal(client.master, w.arena.p32)     # after the landing: the same vector
    client.land_due = land
    w.finish()
    print("master vs worker before landing, ulp:", worst)
    assert len(worst) == 6 and max(worst) <= 4, worst


def _is_copy(name: str) -> bool:
    return name.startswith(("__amd_rocclr_copyBuffer", "Memcpy", "memcpy"))


@pytest.mark.strict_native
@pytest.mark.parametrize("mode", ["asgd", "single"])
def test_new_paths_run_only_native_kernels(mode):
    """One profiled eager step with the stock oracle mode OFF: every device kernel
    is ``dmp::`` except copies -- no ATen elementwise / reduction kernel, in
    particular no ``mul_`` for grad_scale, norm or clip."""
    from torch.profiler import ProfilerActivity, profile

    w, (x, y) = _worker(mode)
    w.train_step(x, y)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        loss, _ = w.train_step(x, y)
        torch.cuda.synchronize()
    w.finish()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert names, "profiler recorded no device work"
    foreign = sorted({n for n in names if "dmp::" not in n and not _is_copy(n)})
    assert not foreign, f"{mode}: non-native device kernels in a training step: {foreign}"
    for k in ("optim_hyper_kernel", "adamw_fused_step_kernel", "sumsq_partial_kernel"):
        assert any(k in n for n in names), (k, names)
    assert math.isfinite(float(loss.float().item()))
