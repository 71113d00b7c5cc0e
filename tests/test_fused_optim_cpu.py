"""AdamW + global-norm clipping + warmup-cosine schedule: the pure-torch CPU path
of parallel/fused_optim.py (the specification the HIP kernels follow) against
an fp64 oracle that is itself validated against torch.optim.AdamW in fp64."""
import math

import pytest
import torch

from distributed_ml_pytorch_amd.models import build_model
from distributed_ml_pytorch_amd.parallel.arena import attach_arena
from distributed_ml_pytorch_amd.parallel.asgd import Asynchronous
from distributed_ml_pytorch_amd.parallel.clients import LocalPSClient
from distributed_ml_pytorch_amd.parallel.ddp import FusedAdamW, FusedSGD
from distributed_ml_pytorch_amd.parallel.fused_optim import FusedOptimCore, Schedule

from fused_optim_oracle import (accuracy_report, oracle_adamw, sched_lr, torch_adamw)

SCHED = dict(kind="warmup_cosine", warmup=3, total=10, lr_min=1e-5)
HP = dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-8, wd=0.05, max_norm=1.0)
STEPS = 10


def _schedule():
    return Schedule("warmup_cosine", SCHED["warmup"], SCHED["total"], SCHED["lr_min"])


def _elem_masks(arena):
    """(used, decay) per arena element, built from the slots (not from the core)."""
    used = torch.zeros(arena.numel, dtype=torch.bool)
    decay = torch.zeros(arena.numel, dtype=torch.bool)
    for p, s in zip(arena.params, arena.slots):
        used[s.offset:s.offset + s.numel] = True
        if p.dim() > 1:
            decay[s.offset:s.offset + s.numel] = True
    return used, decay


def _grads(arena, steps=STEPS, seed=0):
    """Fixed random gradients on the real elements; odd steps are large enough
    to clip at max_norm 1 (norm ~7), even steps are not (norm ~0.4)."""
    used, _ = _elem_masks(arena)
    g = torch.Generator().manual_seed(seed)
    n = float(used.sum())
    out = []
    for i in range(steps):
        target = 7.0 if i % 2 else 0.4
        out.append(torch.randn(arena.numel, generator=g) * used * (target / math.sqrt(n)))
    return out


def _make(which, model_name="mlp", wd=HP["wd"], schedule=True, max_norm=HP["max_norm"], seed=0):
    torch.manual_seed(seed)
    model, _, _ = build_model(model_name)
    kw = dict(betas=HP["betas"], eps=HP["eps"], weight_decay=wd, max_grad_norm=max_norm,
              schedule=_schedule() if schedule else None)
    if which == "async":
        opt = Asynchronous(model.parameters(), lr=HP["lr"], n_push=10 ** 6, n_pull=10 ** 6,
                           model=model, client=LocalPSClient(staleness=0), optimizer="adamw", **kw)
    else:
        arena = attach_arena(model, shadow_dtype=None)
        opt = FusedAdamW(model.parameters(), arena, HP["lr"], model=model, **kw)
    return model, opt


def _run(opt, grads):
    for g in grads:
        opt.arena.g32.copy_(g)
        opt.local_step()


def test_oracle_matches_torch_adamw_fp64():
    g = torch.Generator().manual_seed(1)
    n = 64 * 9
    p0 = torch.randn(n, generator=g, dtype=torch.float64)
    decay = (torch.arange(n) // 64) % 2 == 0
    grads = [torch.randn(n, generator=g, dtype=torch.float64) * (0.3 if i % 2 else 0.01)
             for i in range(STEPS)]
    kw = dict(decay=decay, grad_scale=0.25, sched=SCHED, **HP)
    ref = oracle_adamw(p0, grads, **kw)
    assert min(ref["clips"]) < 1.0 and max(ref["clips"]) == 1.0   # both branches taken
    tt = torch_adamw(p0, grads, dtype=torch.float64, **kw)
    for k in ("p", "m", "v"):
        rel = float((tt[k] - ref[k]).abs().max() / ref[k].abs().max())
        assert rel <= 1e-12, (k, rel)


@pytest.mark.parametrize("which", ["async", "fused"])
def test_cpu_path_matches_oracle(which):
    model, opt = _make(which)
    a = opt.arena
    grads = _grads(a)
    _, decay = _elem_masks(a)
    p0 = a.p32.clone()
    acc_sum = torch.zeros_like(p0)
    lrs, norms = [], []
    for g in grads:
        before = a.p32.clone()
        a.g32.copy_(g)
        opt.local_step()
        acc_sum += a.p32 - before
        lrs.append(opt.core.lr())
        norms.append(opt.core.grad_norm())
    kw = dict(decay=decay, sched=SCHED, **HP)
    ref = oracle_adamw(p0, grads, **kw)
    assert min(ref["clips"]) < 1.0 and max(ref["clips"]) == 1.0
    t32 = torch_adamw(p0, grads, dtype=torch.float32, **kw)
    got = dict(p=a.p32, m=opt.core.m, v=opt.core.v)
    for k, (en, et, bound) in accuracy_report(got, t32, ref).items():
        print(f"{which} {k}: cpu-path err {en:.3e}  torch-fp32 err {et:.3e}  bound {bound:.3e}")
        assert en <= bound, (k, en, et, bound)
    assert opt.core.t == STEPS
    assert lrs == pytest.approx(ref["lrs"], rel=1e-12)
    assert norms == pytest.approx(ref["norms"], rel=1e-5)
    if which == "async":
        # the push accumulator is the sum of the applied updates, decay included
        assert torch.equal(opt.acc, acc_sum)
        assert float((opt.acc.double() - ref["acc"]).abs().max()) <= 1e-6
    # padding never moves
    used, _ = _elem_masks(a)
    assert torch.all(a.p32[~used] == 0)


def test_one_dim_parameters_are_not_decayed():
    _, opt_wd = _make("async", wd=0.05)
    _, opt_0 = _make("async", wd=0.0)
    assert torch.equal(opt_wd.arena.p32, opt_0.arena.p32)
    grads = _grads(opt_wd.arena, steps=3)
    _run(opt_wd, grads)
    _run(opt_0, grads)
    a = opt_wd.arena
    seen = {1: 0, 2: 0}
    for p, s in zip(a.params, a.slots):
        sl = slice(s.offset, s.offset + s.numel)
        same = torch.equal(opt_wd.arena.p32[sl], opt_0.arena.p32[sl])
        assert same == (p.dim() <= 1), (s.shape, same)
        seen[min(p.dim(), 2)] += 1
    assert seen[1] and seen[2]


def test_no_weight_decay_names_are_honoured():
    model, opt_wd = _make("async", model_name="vit_tiny", wd=0.05)
    _, opt_0 = _make("async", model_name="vit_tiny", wd=0.0)
    assert model.no_weight_decay() == {"cls_token", "pos_embed"}
    grads = _grads(opt_wd.arena, steps=2)
    _run(opt_wd, grads)
    _run(opt_0, grads)
    a = opt_wd.arena
    slot = {id(p): s for p, s in zip(a.params, a.slots)}
    named = dict(model.named_parameters())
    for name in ("cls_token", "pos_embed"):
        assert named[name].dim() > 1            # only the name keeps them from decaying
        s = slot[id(named[name])]
        sl = slice(s.offset, s.offset + s.numel)
        assert not opt_wd.core.mask[s.offset // 64:(s.offset + s.numel + 63) // 64].any()
        assert torch.equal(opt_wd.arena.p32[sl], opt_0.arena.p32[sl])
    s = slot[id(named["head.weight"])]
    sl = slice(s.offset, s.offset + s.numel)
    assert opt_wd.core.mask[s.offset // 64:(s.offset + s.numel + 63) // 64].all()
    assert not torch.equal(opt_wd.arena.p32[sl], opt_0.arena.p32[sl])


def test_schedule_closed_form():
    base, w, n, lo = 0.01, 4, 12, 1e-4
    model, _, _ = build_model("mlp")
    arena = attach_arena(model, shadow_dtype=None)
    core = FusedOptimCore(arena, "sgd", base, schedule=Schedule("warmup_cosine", w, n, lo))
    seen = {}
    for t in range(1, n + 6):
        core.step(arena, None)
        seen[t] = core.lr()
    for t in (1, w, w + 1, n, n + 5):
        assert seen[t] == pytest.approx(sched_lr(base, t, "warmup_cosine", w, n, lo), rel=1e-14)
    assert seen[1] == pytest.approx(base / w)
    assert seen[w] == base
    assert seen[w + 1] == pytest.approx(lo + 0.5 * (base - lo) * (1 + math.cos(math.pi / (n - w))))
    assert seen[n] == lo and seen[n + 5] == lo
    assert all(seen[t] > seen[t + 1] for t in range(w, n))
    with pytest.raises(ValueError):
        Schedule("warmup_cosine", 5, 5)


def test_sgd_with_clip_and_schedule_cpu():
    """FusedSGD(max_grad_norm, schedule): torch.optim.SGD on clipped, averaged
    gradients with the scheduled lr (the path asgd_fused_step_dev takes on GPU)."""
    torch.manual_seed(0)
    model, _, _ = build_model("mlp")
    arena = attach_arena(model, shadow_dtype=None)
    opt = FusedSGD(model.parameters(), arena, 0.1, momentum=0.9, weight_decay=1e-3,
                   grad_scale=0.5, max_grad_norm=1.0, schedule=_schedule())
    grads = _grads(arena, steps=4)
    p = arena.p32.double().clone()
    buf = None
    for t, g in enumerate(grads, 1):
        arena.g32.copy_(g)
        opt.local_step()
        norm = 0.5 * float(g.double().norm())
        d = g.double() * (0.5 * min(1.0, 1.0 / (norm + 1e-6))) + 1e-3 * p
        buf = d.clone() if buf is None else 0.9 * buf + d
        p = p - sched_lr(0.1, t, **SCHED) * buf
    assert float((arena.p32.double() - p).abs().max()) <= 1e-6
    assert opt.param_groups[0]["lr"] == 0.1            # the host-side lr stays at the base


def test_checkpoint_roundtrip_bitwise(tmp_path):
    from distributed_ml_pytorch_amd.utils import checkpoint as ck

    model, opt = _make("async")
    grads = _grads(opt.arena, steps=8)
    _run(opt, grads)

    m1, o1 = _make("async")
    _run(o1, grads[:4])
    path = str(tmp_path / "w.pt")
    ck.save_worker_checkpoint(path, m1, o1, 4)
    sd = torch.load(path, weights_only=True)
    assert sd["opt"]["t"] == 4 and sd["opt"]["schedule"]["kind"] == "warmup_cosine"
    assert sd["opt"]["m"] is not None and sd["opt"]["v"] is not None

    m2, o2 = _make("async", seed=123)               # a fresh worker, different init
    assert ck.load_worker_checkpoint(path, m2, o2) == 4
    assert o2.core.t == 4
    _run(o2, grads[4:])
    for a, b in ((o2.arena.p32, opt.arena.p32), (o2.core.m, opt.core.m),
                 (o2.core.v, opt.core.v), (o2.acc, opt.acc)):
        assert torch.equal(a, b)
    assert o2.core.lr() == opt.core.lr()


def test_old_checkpoint_still_loads(tmp_path):
    from distributed_ml_pytorch_amd.utils import checkpoint as ck

    torch.manual_seed(0)
    m, _, _ = build_model("mlp")
    old = Asynchronous(m.parameters(), lr=0.1, n_push=2, n_pull=2, model=m, momentum=0.9,
                       client=LocalPSClient())
    assert old.core is None
    old.acc.normal_()
    path = str(tmp_path / "old.pt")
    ck.save_worker_checkpoint(path, m, old, 7)
    sd = torch.load(path, weights_only=True)
    assert not {"m", "v", "t", "schedule"} & set(sd["opt"])     # the parent's format
    m2, o2 = _make("async", seed=5)
    assert ck.load_worker_checkpoint(path, m2, o2) == 7
    assert torch.equal(o2.acc, old.acc) and o2.core.t == 0
    assert torch.equal(o2.arena.p32, old.arena.p32)
    m3, _, _ = build_model("mlp")                                  # and into plain SGD, as before
    o3 = Asynchronous(m3.parameters(), lr=0.5, n_push=2, n_pull=2, model=m3, momentum=0.9,
                      client=LocalPSClient())
    ck.load_worker_checkpoint(path, m3, o3)
    assert torch.equal(o3.mom, old.mom) and o3.param_groups[0]["lr"] == 0.1


def test_default_options_take_the_existing_path():
    m, _, _ = build_model("mlp")
    opt = Asynchronous(m.parameters(), lr=0.1, n_push=1, n_pull=1, model=m,
                       client=LocalPSClient())
    assert opt.core is None
    m2, _, _ = build_model("mlp")
    assert FusedSGD(m2.parameters(), attach_arena(m2, shadow_dtype=None), 0.1).core is None
    with pytest.raises(ValueError):
        Asynchronous(m.parameters(), lr=0.1, n_push=1, n_pull=1, model=m, optimizer="adam")


def test_cli_flags():
    from distributed_ml_pytorch_amd.cli import build_parser, config_from_args
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig

    cfg = config_from_args(build_parser().parse_args([]))
    assert cfg.optimizer == "sgd" and cfg.lr_schedule == "constant"
    assert cfg.clip_grad_norm == 0.0 and cfg.warmup_steps == 0 and cfg.schedule_steps is None
    d = TrainConfig()
    assert (d.optimizer, d.beta1, d.beta2, d.adam_eps, d.lr_min) == ("sgd", 0.9, 0.999, 1e-8, 0.0)
    cfg = config_from_args(build_parser().parse_args(
        ["--optimizer", "adamw", "--beta1", "0.8", "--beta2", "0.95", "--adam-eps", "1e-6",
         "--clip-grad-norm", "1.5", "--warmup-steps", "7", "--lr-min", "1e-5",
         "--lr-schedule", "warmup_cosine", "--schedule-steps", "90"]))
    assert (cfg.optimizer, cfg.beta1, cfg.beta2, cfg.adam_eps) == ("adamw", 0.8, 0.95, 1e-6)
    assert (cfg.clip_grad_norm, cfg.warmup_steps, cfg.lr_min) == (1.5, 7, 1e-5)
    assert cfg.lr_schedule == "warmup_cosine" and cfg.schedule_steps == 90


def test_worker_cpu_adamw_trains():
    """The trainer wires the options through: a CPU Worker with AdamW + clip +
    warmup-cosine lowers the loss on a fixed batch and reports lr / grad norm."""
    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, Worker

    cfg = TrainConfig(model="mlp", batch_size=16, optimizer="adamw", lr=1e-3, weight_decay=0.05,
                      lr_schedule="warmup_cosine", warmup_steps=3, max_steps=12,
                      clip_grad_norm=1.0, mode="asgd", ps="local", n_push=1, n_pull=1, cuda=False,
                      evaluate=False, verbose=False)
    w = Worker(cfg, DistInfo(device=torch.device("cpu")))
    g = torch.Generator().manual_seed(0)
    x, y = w.prepare(torch.randn(16, *w.input_shape, generator=g),
                     torch.randint(0, w.num_classes, (16,), generator=g))
    losses, lrs = [], []
    for _ in range(12):
        losses.append(float(w.train_step(x, y)[0]))
        lrs.append(w.opt.core.lr())
    w.finish()
    assert all(math.isfinite(v) for v in losses) and losses[-1] < losses[0]
    assert lrs == pytest.approx([sched_lr(1e-3, t, "warmup_cosine", 3, 12, 0.0)
                                 for t in range(1, 13)])
    assert w.opt.core.grad_norm() > 0
    assert w.opt.param_groups[0]["lr"] == 1e-3
