"""Pass times of the push hand-off and the PS apply on every push wire: fp32,
bf16, MX8 and sparse block top-k at K = 8 and K = 32.

For each model's flat-arena length, in one process on one box: every pass is
captured as ``--iters`` back-to-back launches in one hipGraph and timed by device
events around a replay (no host launch time in the window), in alternating
windows (``mx8_wire_bench.graphed``); a device-to-device copy gives the box's
copy rate.

A hand-off consumes its accumulator (fp32 / bf16 leave zeros, MX8 the rounding
residual, top-k everything it did not send -- and a block that keeps being
drained without new gradients runs out of non-zeros after ``3 * 256 / K``
hand-offs, since each take strips 8 of a value's 24 bits).  So every hand-off
launch is preceded, inside the graph, by ``acc.copy_(src)``, the stand-in for the
optimizer steps between two pushes; ``refill alone`` is that copy by itself and
the hand-off column is the pair minus it.  The applies need no refill.

Bytes a pass must move per element: the dense passes read 4 and write their
payload plus 4; the top-k hand-off reads 4 and writes K / 64 (plus the touched
float4s), the top-k applies read K / 64 and touch at most K 32-B sectors per
256 elements.  Needs the GPU.

    python scripts/topk_wire_bench.py [--models vit_b16 resnet18] [--iters 10] [--rounds 7]
"""
import argparse
import os
import statistics
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from distributed_ml_pytorch_amd.ops._ext import native                        # noqa: E402
from distributed_ml_pytorch_amd.parallel import wire8, wire_topk              # noqa: E402
from fused_adamw_bench import arena_numel                                     # noqa: E402
from mx8_wire_bench import graphed                                            # noqa: E402

KS = (8, 32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", nargs="+", default=["vit_b16", "resnet18"])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
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
        nbytes = wire8.layout(n)[2]
        # what a push carries: -lr * gradient sums
        src = torch.randn(n, device=dev) * 1e-3
        acc = src.clone()
        out32 = torch.empty(n, device=dev)
        out16 = torch.empty(n, dtype=torch.bfloat16, device=dev)
        out8 = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        outk = {k: torch.zeros(wire_topk.layout(n, k)[1], dtype=torch.int32, device=dev)
                for k in KS}
        # real payloads for the applies
        nat.push_handoff(src.clone(), out32, None)
        nat.push_handoff(src.clone(), None, out16)
        nat.push_handoff_mx8(src.clone(), out8)
        for k in KS:
            nat.push_handoff_topk(src.clone(), outk[k], k)
        shard = torch.randn(n, device=dev)
        dst = torch.empty(n, device=dev)

        def refilled(fn):
            def both():
                acc.copy_(src)
                fn()
            return both

        handoffs = {
            "push_handoff fp32": (lambda: nat.push_handoff(acc, out32, None), 12.0),
            "push_handoff bf16": (lambda: nat.push_handoff(acc, None, out16), 10.0),
            "push_handoff_mx8": (lambda: nat.push_handoff_mx8(acc, out8), 8.0 + nbytes / n),
        }
        applies = {
            "ps_apply fp32": (lambda: nat.ps_apply(shard, out32, None, 1e-3), 12.0),
            "ps_apply bf16": (lambda: nat.ps_apply(shard, out16, None, 1e-3), 10.0),
            "ps_apply_mx8": (lambda: nat.ps_apply_mx8(shard, out8, None, 1e-3), 8.0 + nbytes / n),
            "ps_apply fp32 atomic": (lambda: nat.ps_apply(shard, out32, None, 1e-3, True), 12.0),
            "ps_apply bf16 atomic": (lambda: nat.ps_apply(shard, out16, None, 1e-3, True), 10.0),
            "ps_apply_mx8 atomic": (lambda: nat.ps_apply_mx8(shard, out8, None, 1e-3, True),
                                    8.0 + nbytes / n),
        }
        for k in KS:
            handoffs[f"push_handoff_topk K={k}"] = (
                lambda k=k: nat.push_handoff_topk(acc, outk[k], k), 4.0 + k / 64)
            applies[f"ps_apply_topk K={k}"] = (
                lambda k=k: nat.ps_apply_topk(shard, outk[k], None, 1e-3, False, None, k), None)
            applies[f"ps_apply_topk K={k} atomic"] = (
                lambda k=k: nat.ps_apply_topk(shard, outk[k], None, 1e-3, True, None, k), None)
        passes = {"copy fp32 (copy rate)": (lambda: dst.copy_(shard), 8.0),
                  "refill alone": (lambda: acc.copy_(src), 8.0)}
        passes.update({k: (refilled(fn), bpe) for k, (fn, bpe) in handoffs.items()})
        passes.update(applies)
        runs = {k: graphed(fn, a.iters) for k, (fn, _) in passes.items()}
        times = {k: [] for k in passes}
        for _ in range(a.rounds):                # alternating windows
            for k, run in runs.items():
                times[k].append(run())
        print(f"\n{name}: arena {n} elements ({used} parameters); payload B/elem: fp32 4, bf16 2, "
              f"MX8 {nbytes / n:.4f}, top-k " +
              ", ".join(f"K={k} {4 * outk[k].numel() / n:.4f}" for k in KS) +
              f"; {a.rounds} windows x {a.iters} graph-replayed launches, median [min-max] ms")
        med = {k: statistics.median(v) for k, v in times.items()}
        refill = med["refill alone"]
        for k, (_, bpe) in passes.items():
            t = med[k]
            spread = (max(times[k]) - min(times[k])) / t
            line = (f"  {k:30s} {t:7.4f} [{min(times[k]):.4f}-{max(times[k]):.4f}] ms   "
                    f"spread {100 * spread:4.1f} %")
            if k in handoffs:
                own = t - refill
                line += (f"   minus refill {own:7.4f} ms   {bpe:5.2f} B/elem   "
                         f"{n * bpe / own / 1e9:6.2f} TB/s")
            elif bpe is not None:
                line += f"   {bpe:5.2f} B/elem   {n * bpe / t / 1e9:6.2f} TB/s"
            print(line)
        for k in KS:
            for b, m in (("push_handoff_mx8", f"push_handoff_topk K={k}"),):
                print(f"  {m:30s} {(med[m] - refill) / (med[b] - refill):5.3f} x the time of {b} "
                      f"(both minus the refill)")
            for b, m in (("ps_apply_mx8", f"ps_apply_topk K={k}"),
                         ("ps_apply_mx8 atomic", f"ps_apply_topk K={k} atomic")):
                print(f"  {m:30s} {med[m] / med[b]:5.3f} x the time of {b}")
        del runs, passes, handoffs, applies, acc, src, out32, out16, out8, outk, shard, dst
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
