"""Pass times of the push hand-off and the PS apply, bf16 wire against MX8.

For each model's flat-arena length: push_handoff (bf16 out) against
push_handoff_mx8, and ps_apply (bf16 delta; plain and fp32-atomic) against
ps_apply_mx8, in one process on one box.  Every pass is captured as ``--iters``
back-to-back launches in one hipGraph and timed by device events around a
replay (no host launch time in the window), in alternating windows; a
device-to-device copy gives the box's copy rate.  Rates are the bytes each pass
must move over its time: the bf16 passes 10 B per element (4 in, 2 + 4 out /
4 + 2 in, 4 out), the MX8 passes 9.03 (the payload is 1 + 1/32 B per element).
Needs the GPU.

    python scripts/mx8_wire_bench.py [--models vit_b16 resnet18] [--iters 20] [--rounds 7]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_ml_pytorch_amd.ops._ext import native                        # noqa: E402
from distributed_ml_pytorch_amd.parallel import wire8                         # noqa: E402
from fused_adamw_bench import arena_numel                                     # noqa: E402


def graphed(fn, iters):
    """``iters`` launches of ``fn`` as one captured graph -> ms per launch of a replay."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()

    def run():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        g.replay()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / iters

    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=["vit_b16", "resnet18"])
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs the GPU"
    nat = native()
    dev = torch.device("cuda", 0)
    print(torch.cuda.get_device_name(0), flush=True)
    for name in a.models:
        n, used = arena_numel(name)
        nbytes = wire8.layout(n)[2]
        mx = 8.0 + nbytes / n
        # accumulators hold what a push would carry (-lr * gradient sums); a hand-off
        # leaves zeros (bf16) or the residual (MX8) behind: neither kernel's memory
        # traffic depends on the values
        acc16 = torch.randn(n, device=dev) * 1e-3
        acc8 = acc16.clone()
        out16 = torch.empty(n, dtype=torch.bfloat16, device=dev)
        out8 = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        nat.push_handoff_mx8(acc8.clone(), out8)           # a real payload for the applies
        d16 = (torch.randn(n, device=dev) * 1e-3).to(torch.bfloat16)
        shard = torch.randn(n, device=dev)
        dst = torch.empty(n, device=dev)
        passes = {
            # name: (callable, bytes per element)
            "copy fp32 (copy rate)": (lambda: dst.copy_(shard), 8.0),
            "push_handoff bf16": (lambda: nat.push_handoff(acc16, None, out16), 10.0),
            "push_handoff_mx8": (lambda: nat.push_handoff_mx8(acc8, out8), mx),
            "ps_apply bf16": (lambda: nat.ps_apply(shard, d16, None, 1e-3), 10.0),
            "ps_apply_mx8": (lambda: nat.ps_apply_mx8(shard, out8, None, 1e-3), mx),
            "ps_apply bf16 atomic": (lambda: nat.ps_apply(shard, d16, None, 1e-3, True), 10.0),
            "ps_apply_mx8 atomic": (lambda: nat.ps_apply_mx8(shard, out8, None, 1e-3, True), mx),
        }
        runs = {k: graphed(fn, a.iters) for k, (fn, _) in passes.items()}
        times = {k: [] for k in passes}
        for _ in range(a.rounds):                # alternating windows
            for k, run in runs.items():
                times[k].append(run())
        print(f"\n{name}: arena {n} elements ({used} parameters), payload {nbytes} B "
              f"({nbytes / n:.4f} B/elem), {a.rounds} windows x {a.iters} graph-replayed "
              f"launches, median [min-max] ms")
        med = {}
        for k, (_, bpe) in passes.items():
            t = med[k] = statistics.median(times[k])
            spread = (max(times[k]) - min(times[k])) / t
            print(f"  {k:24s} {t:7.4f} [{min(times[k]):.4f}-{max(times[k]):.4f}] ms   "
                  f"spread {100 * spread:4.1f} %   {bpe:5.2f} B/elem   "
                  f"{n * bpe / t / 1e9:6.2f} TB/s")
        for b, m in (("push_handoff bf16", "push_handoff_mx8"), ("ps_apply bf16", "ps_apply_mx8"),
                     ("ps_apply bf16 atomic", "ps_apply_mx8 atomic")):
            print(f"  {m:24s} {med[m] / med[b]:5.3f} x the time of {b}")
        del runs, passes, acc16, acc8, out16, out8, d16, shard, dst
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
