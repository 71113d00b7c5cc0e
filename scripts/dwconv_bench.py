#!/usr/bin/env python
"""Depthwise 7x7 conv (csrc/dwconv.hip) at the four ConvNeXt-T stage shapes, batch 128:
forward, data gradient and weight gradient against a same-run device copy (the byte
floor) and stock ``F.conv2d(groups=C)`` bf16 channels-last in the oracle mode, then the
convnext_tiny batch-128 captured step and the depthwise kernels' share of it.

Protocol: one captured graph of ``--launches`` launches per arm, the arms replayed in
turn, device events around each replay, minimum of ``--windows`` windows.  Needs a GPU.
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CL = torch.channels_last
SHAPES = [(56, 96), (28, 192), (14, 384), (7, 768)]


def capture(fn, launches):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            fn()
    return g


def time_arms(arms, launches, windows):
    """{name: min us per launch} of captured graphs replayed in turn."""
    graphs = {k: capture(fn, launches) for k, fn in arms.items()}   # any GPU error ends the run
    best = {k: float("inf") for k in graphs}
    for _ in range(windows):
        for k, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            best[k] = min(best[k], a.elapsed_time(b) * 1e3 / launches)
    return best


def kernels(args):
    from distributed_ml_pytorch_amd.ops._ext import native
    from distributed_ml_pytorch_amd.ops._policy import stock_allowed

    nat, N, K = native(), args.batch, 7
    print(f"(a) depthwise {K}x{K}, batch {N}: {args.launches} launches per graph, min of "
          f"{args.windows} windows; bytes = one read + one write of the activation (forward, "
          "dgrad) or two reads (wgrad)")
    print("expectation (derived): a pass moves 2 x the activation and issues 49 fp32 FMAs per "
          "output; at stage 1 (154 MB, 1.9 G FMAs) the VALU time is about the byte time, so the "
          "native passes should land within about 2x of the copy and near the stock kernels")
    for HW, C in SHAPES:
        x, dy = (torch.randn(N, C, HW, HW, device="cuda").bfloat16().contiguous(memory_format=CL)
                 for _ in range(2))
        w = (torch.randn(C, 1, K, K, device="cuda") * 0.1).bfloat16()
        b = torch.zeros(C, device="cuda")
        dw, db = torch.zeros(C, 1, K, K, device="cuda"), torch.zeros(C, device="cuda")
        slab = torch.empty(nat.dwconv_slab_numel(C, K), device="cuda")
        out = torch.empty_like(x)
        nbytes = 2 * x.numel() * 2
        with stock_allowed(True):
            t = time_arms({
                "copy": lambda: out.copy_(x),
                "fwd": lambda: nat.dwconv_fwd(x, w, b),
                "dgrad": lambda: nat.dwconv_fwd(dy, w, None, True),
                "wgrad": lambda: nat.dwconv_wgrad(dy, x, dw, db, slab),
                "stock fwd": lambda: F.conv2d(x, w, None, 1, K // 2, 1, C),
                "stock dgrad": lambda: torch.ops.aten.convolution_backward(
                    dy, x, w, None, (1, 1), (K // 2,) * 2, (1, 1), False, (0, 0), C,
                    (True, False, False)),
                "stock wgrad": lambda: torch.ops.aten.convolution_backward(
                    dy, x, w, None, (1, 1), (K // 2,) * 2, (1, 1), False, (0, 0), C,
                    (False, True, False)),
            }, args.launches, args.windows)
        plan = nat.dwconv_plan(HW, HW, C, K)
        print(f"{HW}x{HW}x{C} ({nbytes / 1e6:.1f} MB, tile {plan[0]}x{plan[1]}x{plan[2]}): " +
              " | ".join(f"{k} {v:7.1f} us {nbytes / v / 1e6:5.2f} TB/s" for k, v in t.items()))


def step(args):
    from torch.profiler import ProfilerActivity, profile

    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, Worker

    cfg = TrainConfig(model="convnext_tiny", batch_size=args.batch, mode="single",
                      optimizer="adamw", lr=1e-3, drop_path=0.1, evaluate=False, verbose=False)
    w = Worker(cfg, DistInfo(device=torch.device("cuda", 0)))
    x, y = w.prepare(torch.randn(args.batch, *w.input_shape),
                     torch.randint(0, w.num_classes, (args.batch,)))
    w.train_step(x, y)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:      # one eager step
        w.train_step(x, y)
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    dur = lambda e: getattr(e, "device_time", None) or getattr(e, "cuda_time", 0)
    total = sum(dur(e) for e in ev)
    for key in ("dwconv_kernel", "dwconv_wgrad", "layer_scale"):
        part = sum(dur(e) for e in ev if key in e.name)
        print(f"(b) eager step kernel time: {key:20s} {part / 1e3:8.3f} ms of {total / 1e3:.3f} "
              f"({100 * part / max(total, 1):.1f} %)")
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
    print(f"(b) convnext_tiny batch {args.batch} AdamW drop-path 0.1 captured step: min "
          f"{best:.3f} ms / step over {args.windows} windows of {args.steps} steps")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "dwconv_bench needs a GPU"
    print("dwconv_bench:", torch.cuda.get_device_name(0))
    kernels(a)
    step(a)
