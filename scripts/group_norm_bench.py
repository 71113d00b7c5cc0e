#!/usr/bin/env python
"""GroupNorm + residual + ReLU (csrc/group_norm.hip) at the ResNet-18 CIFAR stage maps
(batch 512) and the ResNet-50 ImageNet maps (batch 128), G = 32: forward and backward
against (a) a same-run device copy of the bytes each pass moves, (b) this tree's
BatchNorm apply / backward pair at the same shape and (c) stock bf16 ``F.group_norm`` +
add + relu in the oracle mode; then the captured ``resnet18_gn`` / ``resnet50_gn`` step
next to the BatchNorm model's in the same process.

Protocol: one captured graph of ``--launches`` launches per arm, the arms replayed in
turn, device events around each replay, minimum of ``--windows`` windows.  Nothing that
clears memory may be recorded into a graph: the BatchNorm arms get persistent slot
buffers (without them the bindings allocate zeroed ones, a memset node), and the stock
arms, whose kernels are not ours to vouch for, are timed eagerly, ``--launches`` calls
between two device events, in turn with the graphs.  Needs a GPU.
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CL = torch.channels_last
SHAPES = [(512, 32, 64), (512, 16, 128), (512, 8, 256), (512, 4, 512),
          (128, 112, 64), (128, 56, 64), (128, 56, 256), (128, 28, 512), (128, 14, 1024),
          (128, 7, 2048)]
G, EPS = 32, 1e-5


def capture(fn, launches):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            fn()
    return g


def eager(fn, launches):
    def run():
        for _ in range(launches):
            fn()
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return run


def time_arms(arms, launches, windows):
    """{name: min us per launch}: captured graphs (eager loops for the ``stock`` arms)
    run in turn."""
    runs = {k: eager(fn, launches) if k.startswith("stock") else capture(fn, launches).replay
            for k, fn in arms.items()}                              # any GPU error ends the run
    best = {k: float("inf") for k in runs}
    for _ in range(windows):
        for k, run in runs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            run()
            b.record()
            b.synchronize()
            best[k] = min(best[k], a.elapsed_time(b) * 1e3 / launches)
    return best


def kernels(args):
    from distributed_ml_pytorch_amd.ops._ext import native
    from distributed_ml_pytorch_amd.ops._policy import stock_allowed
    from distributed_ml_pytorch_amd.ops.conv import bn_slot_buffer

    nat = native()
    print(f"(a) GN + residual + ReLU, G = {G}: {args.launches} launches per graph, min of "
          f"{args.windows} windows.  copy3 / copy5: device copies of 3 / 5 activations' bytes "
          "(forward: x, residual in, y out; backward: x, dy, y in, dx, dres out)")
    for N, HW, C in SHAPES:
        x, r, dy = (torch.randn(N, C, HW, HW, device="cuda").bfloat16().contiguous(memory_format=CL)
                    for _ in range(3))
        gamma, beta = torch.ones(C, device="cuda"), torch.zeros(C, device="cuda")
        dg, db = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
        slab = torch.empty(nat.gn_slab_numel(C), device="cuda")
        y, stats = nat.gn_fwd(x, r, gamma, beta, G, EPS, True)
        own = argparse.Namespace()          # holds the BN arms' persistent zeroed slots
        fs = bn_slot_buffer(own, "f", C, x.device)
        bs = bn_slot_buffer(own, "b", C, x.device)
        by, bstats, _ = nat.bn_fwd(x, r, gamma, beta, rm, rv, 0.1, EPS, True, True, fs)
        act = x.numel() * 2
        src3 = torch.empty(3 * act // 2, dtype=torch.uint8, device="cuda")
        dst3 = torch.empty_like(src3)
        src5 = torch.empty(5 * act // 2, dtype=torch.uint8, device="cuda")
        dst5 = torch.empty_like(src5)
        xg = x.detach().clone().requires_grad_(True)

        def stock_fwd():
            return torch.relu(F.group_norm(x, G, gamma.bfloat16(), beta.bfloat16(), EPS) + r)

        with stock_allowed(True):
            ys = torch.relu(F.group_norm(xg, G, gamma.bfloat16(), beta.bfloat16(), EPS) + r)
            t = time_arms({
                "copy3": lambda: dst3.copy_(src3),
                "gn fwd": lambda: nat.gn_fwd(x, r, gamma, beta, G, EPS, True),
                "bn fwd": lambda: nat.bn_fwd(x, r, gamma, beta, rm, rv, 0.1, EPS, True, True, fs),
                "stock fwd": stock_fwd,
                "copy5": lambda: dst5.copy_(src5),
                "gn bwd": lambda: nat.gn_bwd(x, dy, y, gamma, stats, G, True, True, dg, db, slab),
                "bn bwd": lambda: nat.bn_bwd(x, dy, by, gamma, bstats, dg, db, True, True, bs),
                "stock bwd": lambda: torch.autograd.grad(ys, xg, dy, retain_graph=True),
            }, args.launches, args.windows)
        pf, pb = nat.gn_plan(N, C, HW, HW, G), nat.gn_plan(N, C, HW, HW, G, -1, True)
        print(f"{N}x{HW}x{HW}x{C} ({act / 1e6:.1f} MB; fwd {pf['route']} {pf['slice_channels']} ch x "
              f"{pf['parts']} parts, bwd {pb['route']} {pb['slice_channels']} ch x {pb['parts']} "
              "parts): " + " | ".join(f"{k} {v:7.1f} us" for k, v in t.items()))
        print(f"    gn fwd {3 * act / t['gn fwd'] / 1e6:5.2f} TB/s of its 3 activations (copy3 "
              f"{3 * act / t['copy3'] / 1e6:5.2f}); gn bwd {5 * act / t['gn bwd'] / 1e6:5.2f} TB/s "
              f"of its 5 (copy5 {5 * act / t['copy5'] / 1e6:5.2f})")


def step(args, model, batch):
    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, Worker

    out = {}
    for name in (model, model + "_gn"):
        cfg = TrainConfig(model=name, batch_size=batch, mode="asgd", ps="local", lr=0.01,
                          evaluate=False, verbose=False)
        w = Worker(cfg, DistInfo(device=torch.device("cuda", 0)))
        x, y = w.prepare(torch.randn(batch, *w.input_shape),
                         torch.randint(0, w.num_classes, (batch,)))
        assert w.enable_graph()
        for _ in range(3):
            w.train_step(x, y)
        best = float("inf")
        for _ in range(args.windows):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.steps):
                w.train_step(x, y)
            b.record()
            b.synchronize()
            best = min(best, a.elapsed_time(b) / args.steps)
        w.finish()
        out[name] = best
    print(f"(b) batch {batch} ASGD captured step, min over {args.windows} windows of "
          f"{args.steps} steps: " + " | ".join(f"{k} {v:.3f} ms" for k, v in out.items()))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--no-steps", action="store_true", help="kernel table only")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "group_norm_bench needs a GPU"
    print("group_norm_bench:", torch.cuda.get_device_name(0))
    kernels(a)
    if not a.no_steps:
        step(a, "resnet18", 512)
        step(a, "resnet50", 128)
