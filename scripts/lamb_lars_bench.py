"""Pass times of the LAMB and LARS steps at real arena sizes, and the training
step of a model with each optimizer.

Passes: for each model's flat arena (real tensor layout, random contents) the
captured step of AdamW, LAMB, SGD with momentum and LARS -- optim_hyper plus the
update launches, with the push accumulator and the bf16 shadow, no EMA, no
clipping -- and a device-to-device copy as the ceiling.  Steps (--steps): the
whole captured training step of --mode single with each optimizer.  Graphs are
replayed in turn, timed with device events, minimum of --rounds windows.  Needs
the GPU.

    python scripts/lamb_lars_bench.py [--models vit_b16 resnet18] [--steps vit_b16:64 resnet18:512]
"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_ml_pytorch_amd.models import build_model                     # noqa: E402
from distributed_ml_pytorch_amd.parallel.arena import FlatArena               # noqa: E402
from distributed_ml_pytorch_amd.parallel.fused_optim import FusedOptimCore    # noqa: E402
from distributed_ml_pytorch_amd.runtime.dist import DistInfo                  # noqa: E402
from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, Worker    # noqa: E402

DEV = torch.device("cuda", 0)
# bytes per parameter each pass must move (acc and shadow on, no EMA)
BYTES = {"copy": 8.0, "adamw": 38.0, "lamb": 24.0 + 26.0, "sgd_mom": 30.0, "lars": 8.0 + 30.0}


def timed(graph, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        graph.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def capture(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def in_turn(graphs, iters, rounds):
    times = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            times[k].append(timed(g, iters))
    return times


def passes(name, iters, rounds):
    model, _, _ = build_model(name)
    arena = FlatArena(list(model.parameters()), device=DEV)
    n = arena.numel
    arena.g32.normal_(std=1e-3)
    acc, mom, dst = (torch.zeros(n, device=DEV) for _ in range(3))
    cores = {k: FusedOptimCore(arena, kind, 1e-3, weight_decay=0.05, momentum=0.9)
             for k, kind in (("adamw", "adamw"), ("lamb", "lamb"), ("sgd_mom", "sgd"),
                             ("lars", "lars"))}
    fns = {"copy": lambda: dst.copy_(arena.p32)}
    for k, c in cores.items():
        fns[k] = (lambda c=c: c.step(arena, acc, mom if c.kind in ("sgd", "lars") else None))
    times = in_turn({k: capture(f) for k, f in fns.items()}, iters, rounds)
    nch = cores["lamb"].chunks.shape[0]
    print(f"\n{name}: arena {n} elements, {len(arena.slots)} tensors, {nch} chunks; "
          f"{rounds} windows x {iters} replays, min [max] ms")
    for k, t in times.items():
        print(f"  {k:8s} {min(t):7.4f} [{max(t):.4f}] ms   {BYTES[k]:5.1f} B/param   "
              f"{n * BYTES[k] / min(t) / 1e9:6.2f} TB/s")
    print(f"  lamb / adamw {min(times['lamb']) / min(times['adamw']):.2f}x   "
          f"lars / sgd_mom {min(times['lars']) / min(times['sgd_mom']):.2f}x")


def steps(name, batch, iters, rounds):
    graphs, keep = {}, []
    for opt in (("adamw", "lamb") if name.startswith("vit") else ("sgd", "lars")):
        cfg = TrainConfig(model=name, batch_size=batch, optimizer=opt, lr=1e-3, momentum=0.9,
                          weight_decay=0.05, mode="single", evaluate=False, verbose=False)
        w = Worker(cfg, DistInfo(device=DEV))
        x, y = w.prepare(torch.randn(batch, *w.input_shape),
                         torch.randint(0, w.num_classes, (batch,)))
        w.enable_graph()
        for _ in range(3):
            w.train_step(x, y)
        torch.cuda.synchronize()
        assert w.graph is not None, "the step was not captured"
        graphs[opt] = w.graph
        keep.append(w)
    times = in_turn(graphs, iters, rounds)
    print(f"\n{name} bs {batch} training step, {rounds} windows x {iters} replays, min [max] ms")
    for k, t in times.items():
        print(f"  {k:6s} {min(t):8.3f} [{max(t):.3f}] ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="*", default=["vit_b16", "resnet18"])
    ap.add_argument("--steps", nargs="*", default=[], metavar="MODEL:BATCH")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    print(torch.cuda.get_device_name(0), flush=True)
    for name in a.models:
        passes(name, a.iters, a.rounds)
        torch.cuda.empty_cache()
    for spec in a.steps:
        name, batch = spec.split(":")
        steps(name, int(batch), max(a.iters // 3, 5), a.rounds)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
