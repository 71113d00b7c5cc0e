"""Pass times of the fused optimizer kernels at real arena sizes.

For each model's flat-arena length: a device-to-device copy (the HBM copy
ceiling of the box), asgd_fused_step (plain SGD: g, p, acc in; p, acc, bf16
shadow out), and the AdamW step = sumsq_partial (norm pass) + optim_hyper +
adamw_fused_step, timed with device events in alternating windows.  Rates are
the bytes each pass must move over its time.  Needs the GPU.

    python scripts/fused_adamw_bench.py [--models vit_b16 resnet18] [--iters 50] [--rounds 5]
"""
import argparse
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_ml_pytorch_amd.models import build_model                     # noqa: E402
from distributed_ml_pytorch_amd.ops._ext import native                        # noqa: E402
from distributed_ml_pytorch_amd.parallel.arena import ALIGN                   # noqa: E402
from distributed_ml_pytorch_amd.parallel.fused_optim import FusedOptimCore    # noqa: E402


def arena_numel(name):
    model, _, _ = build_model(name)
    off = 0
    for p in model.parameters():
        off = (off + p.numel() + ALIGN - 1) // ALIGN * ALIGN
    pad = ALIGN * 840
    return (max(off, ALIGN) + pad - 1) // pad * pad, sum(p.numel() for p in model.parameters())


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=["vit_b16", "resnet18"])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    nat = native()
    dev = torch.device("cuda", 0)
    print(torch.cuda.get_device_name(0), flush=True)
    try:
        print(subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True,
                             timeout=30).stdout.strip(), flush=True)
    except (OSError, subprocess.TimeoutExpired):
        print("clocks: rocm-smi not available")
    for name in a.models:
        n, used = arena_numel(name)
        ns = types_arena(n, dev)
        core = FusedOptimCore(ns, "adamw", 1e-3, weight_decay=0.05, max_grad_norm=1.0)
        core.mask = (torch.rand(n // ALIGN, device=dev) < 0.9).to(torch.uint8)
        core_noclip = FusedOptimCore(ns, "adamw", 1e-3, weight_decay=0.05)
        core_noclip.m, core_noclip.v, core_noclip.mask = core.m, core.v, core.mask
        acc = torch.zeros(n, device=dev)
        dst = torch.empty(n, device=dev)
        passes = {
            # name: (callable, bytes per element)
            "copy fp32 (ceiling)": (lambda: dst.copy_(ns.p32), 8.0),
            "asgd_fused_step": (lambda: nat.asgd_fused_step(ns.g32, ns.p32, acc, None, ns.w16,
                                                            1e-3, 0.0, 0.0, 0.0, False), 22.0),
            "sumsq_partial (norm)": (lambda: nat.optim_hyper(core.hyper, ns.g32, core.partials),
                                     4.0),
            "adamw_fused_step + hyper": (lambda: core_noclip.step(ns, acc), 38.0 + 1.0 / 64),
            "adamw + hyper + norm": (lambda: core.step(ns, acc), 42.0 + 1.0 / 64),
        }
        for fn, _ in passes.values():           # warm every pass
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {k: [] for k in passes}
        for _ in range(a.rounds):                # alternating windows
            for k, (fn, _) in passes.items():
                times[k].append(timed(fn, a.iters))
        print(f"\n{name}: arena {n} elements ({used} parameters), {a.rounds} windows x "
              f"{a.iters} launches, median [min-max] ms")
        for k, (_, bpe) in passes.items():
            t = statistics.median(times[k])
            print(f"  {k:28s} {t:7.4f} [{min(times[k]):.4f}-{max(times[k]):.4f}] ms   "
                  f"{bpe:5.1f} B/elem   {n * bpe / t / 1e9:6.2f} TB/s")
        c = statistics.median(times["copy fp32 (ceiling)"])
        for k in ("asgd_fused_step", "adamw_fused_step + hyper", "adamw + hyper + norm"):
            t = statistics.median(times[k])
            print(f"  {k:28s} {passes[k][1] / t / (8.0 / c):5.2f} of the copy ceiling")
        del core, core_noclip, ns, acc, dst
        torch.cuda.empty_cache()


def types_arena(n, dev):
    import types

    return types.SimpleNamespace(numel=n, device=dev, params=[], slots=[],
                                 p32=torch.randn(n, device=dev),
                                 g32=torch.randn(n, device=dev) * 1e-3,
                                 w16=torch.zeros(n, dtype=torch.bfloat16, device=dev))


if __name__ == "__main__":
    main()
