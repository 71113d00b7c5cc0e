"""What the model EMA costs: the fused optimizer passes, the buffer launch and
a whole training step, with EMA off, on at K = 1 and on at K = 32.

Every arm is ONE captured step (optim_hyper + the step kernel, as a Worker's
graph holds it) replayed under its own pair of device events; the arms are
replayed in turn in one process, window after window, and the minimum over the
windows is reported (the least disturbed one).  For K = 32 the replays between
two EMA updates (off-steps) and the updating ones (on-steps) are reported
separately: the hyper block decides on the device which one a replay is.
Needs the GPU.

    python scripts/model_ema_bench.py [--models vit_b16 resnet18] [--windows 5]
                                      [--step-model vit_b16 --step-batch 64]
"""
import argparse
import os
import statistics
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_ml_pytorch_amd.models import build_model                     # noqa: E402
from distributed_ml_pytorch_amd.parallel.arena import ALIGN, attach_arena     # noqa: E402
from distributed_ml_pytorch_amd.parallel.ema import ModelEma                  # noqa: E402
from distributed_ml_pytorch_amd.parallel.fused_optim import FusedOptimCore    # noqa: E402

K = 32
DECAY = 0.9998


def arena_numel(name):
    model, _, _ = build_model(name)
    off = 0
    for p in model.parameters():
        off = (off + p.numel() + ALIGN - 1) // ALIGN * ALIGN
    pad = ALIGN * 840
    return (max(off, ALIGN) + pad - 1) // pad * pad


def raw_arena(n, dev):
    return types.SimpleNamespace(numel=n, device=dev, params=[], slots=[],
                                 p32=torch.randn(n, device=dev),
                                 g32=torch.randn(n, device=dev) * 1e-3,
                                 w16=torch.zeros(n, dtype=torch.bfloat16, device=dev))


def capture(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def replay_ms(graph, count):
    """Time of each of ``count`` replays, every one under its own event pair."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(count)]
    for a, b in ev:
        a.record()
        graph.replay()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def bench_passes(name, kind, windows, dev):
    n = arena_numel(name)
    ns = raw_arena(n, dev)
    acc = torch.zeros(n, device=dev)
    mom = torch.zeros(n, device=dev) if kind == "sgd" else None
    arms = {}
    for label, kw in (("off", {}), ("K=1", dict(ema_decay=DECAY)),
                      (f"K={K}", dict(ema_decay=DECAY, ema_every=K))):
        core = FusedOptimCore(ns, kind, 1e-3, weight_decay=0.05,
                              momentum=0.9 if kind == "sgd" else 0.0, **kw)
        if kind == "adamw":
            core.mask = (torch.rand(n // ALIGN, device=dev) < 0.9).to(torch.uint8)
        arms[label] = (core, capture(lambda c=core: c.step(ns, acc, mom, 0.0)))
    rows = {"off": [], "K=1": [], f"K={K} off-steps": [], f"K={K} on-steps": []}
    for _ in range(windows):
        for label, (core, graph) in arms.items():
            t0 = core.t
            ms = replay_ms(graph, 2 * K)
            if label != f"K={K}":
                rows[label].append(statistics.mean(ms))
                continue
            on = [m for i, m in enumerate(ms) if (t0 + i + 1) % K == 0]
            off = [m for i, m in enumerate(ms) if (t0 + i + 1) % K]
            assert len(on) == 2
            rows[f"K={K} on-steps"].append(statistics.mean(on))
            rows[f"K={K} off-steps"].append(statistics.mean(off))
    print(f"\n{name} arena ({n} elements), {kind}: hyper + step kernel, one replay, "
          f"min [max] over {windows} windows of {2 * K} replays, ms")
    base = min(rows["off"])
    for label, v in rows.items():
        print(f"  {label:16s} {min(v):7.4f} [{max(v):.4f}]   {min(v) / base:5.3f} x off")


def bench_buffers(windows, dev):
    model, _, _ = build_model("resnet50")
    model = model.to(dev)
    arena = attach_arena(model, shadow_dtype=torch.bfloat16, channels_last=True)
    core = FusedOptimCore(arena, "sgd", 1e-3, ema_decay=DECAY)
    avg = ModelEma(model, core)
    core.step(arena, None)                       # publishes D, O of an EMA step
    graph = capture(avg.update_buffers)
    ms = [statistics.mean(replay_ms(graph, 64)) for _ in range(windows)]
    print(f"\nresnet50 buffers: {len(avg.live)} tensors, {avg.flat.numel()} elements, one "
          f"ema_buffers launch: min {min(ms):.4f} [max {max(ms):.4f}] ms")


def bench_step(name, batch, windows, steps, dev):
    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, Worker

    arms = {}
    for label, kw in (("off", {}), ("K=1", dict(model_ema=DECAY)),
                      (f"K={K}", dict(model_ema=DECAY, model_ema_every=K))):
        w = Worker(TrainConfig(model=name, batch_size=batch, mode="single", optimizer="adamw",
                               lr=1e-3, weight_decay=0.05, evaluate=False, verbose=False, **kw),
                   DistInfo(device=dev))
        g = torch.Generator().manual_seed(0)
        x = torch.randn(batch, *w.input_shape, generator=g)
        y = torch.randint(0, w.num_classes, (batch,), generator=g)
        x, y = w.prepare(x, y)
        assert w.enable_graph(True)
        for _ in range(3):
            w.train_step(x, y, keep=False)
        torch.cuda.synchronize()
        assert w.graph is not None
        arms[label] = w
    rows = {k: [] for k in arms}
    for _ in range(windows):
        for label, w in arms.items():
            rows[label].append(statistics.mean(replay_ms(w.graph, steps)))
    print(f"\n{name} batch {batch}, single AdamW, whole captured step, mean of {steps} replays, "
          f"min [max] over {windows} windows, ms")
    base = min(rows["off"])
    for label, v in rows.items():
        print(f"  {label:16s} {min(v):8.4f} [{max(v):.4f}]   {min(v) / base:6.4f} x off")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="*", default=["vit_b16", "resnet18"])
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--step-model", default="vit_b16")
    ap.add_argument("--step-batch", type=int, default=64)
    ap.add_argument("--step-replays", type=int, default=32)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    dev = torch.device("cuda", 0)
    print(torch.cuda.get_device_name(0), flush=True)
    for name in a.models:
        for kind in ("adamw", "sgd"):
            bench_passes(name, kind, a.windows, dev)
            torch.cuda.empty_cache()
    bench_buffers(a.windows, dev)
    if not a.no_step:
        bench_step(a.step_model, a.step_batch, a.windows, a.step_replays, dev)


if __name__ == "__main__":
    main()
