"""Pass times of the delay-compensated PS applies and of the reply snapshot.

For each model's flat-arena length, in one process on one box: ps_apply_dc
(plain and fp32-atomic) against ps_apply on every wire (fp32, bf16, MX8), and
ps_snapshot (payload + backup from one read) against the ``copy_`` it replaces
in the reply path.  Every pass is captured as ``--iters`` back-to-back launches
in one hipGraph and timed by device events around a replay (no host launch time
in the window), in alternating windows.  Rates are the bytes each pass must move
over its time: the compensated apply streams the backup as a third operand,
4 B per element more than the plain apply (fp32 wire: 16 against 12); the
atomic forms count the payload, the 4 B added in memory and, compensated, the
shard and backup loads.  Needs the GPU.

    python scripts/delay_comp_bench.py [--models vit_b16 resnet18] [--iters 20] [--rounds 7]
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
from mx8_wire_bench import graphed                                            # noqa: E402

SCALE, C = 1e-3, 0.4


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
        # deltas of the size a push carries; no pass's memory traffic depends on the values
        d32 = torch.randn(n, device=dev) * 1e-3
        d16 = d32.to(torch.bfloat16)
        d8 = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        nat.push_handoff_mx8(d32.clone(), d8)
        shard = torch.randn(n, device=dev)
        bak = shard + 1e-3 * torch.randn(n, device=dev)
        out32 = torch.empty(n, device=dev)
        out16 = torch.empty(n, dtype=torch.bfloat16, device=dev)
        wires = {"fp32": (nat.ps_apply, nat.ps_apply_dc, d32, 4.0),
                 "bf16": (nat.ps_apply, nat.ps_apply_dc, d16, 2.0),
                 "mx8": (nat.ps_apply_mx8, nat.ps_apply_dc_mx8, d8, nbytes / n)}
        passes = {}     # name: (callable, bytes per element)
        pairs = []
        for w, (plain, dc, d, wb) in wires.items():
            for atomic, tag in ((False, ""), (True, " atomic")):
                base, comp = f"ps_apply {w}{tag}", f"ps_apply_dc {w}{tag}"
                passes[base] = (lambda plain=plain, d=d, atomic=atomic:
                                plain(shard, d, None, SCALE, atomic), wb + (4.0 if atomic else 8.0))
                passes[comp] = (lambda dc=dc, d=d, atomic=atomic:
                                dc(shard, d, bak, None, SCALE, C, atomic), wb + 12.0)
                pairs.append((base, comp))
        passes["copy_ fp32 (reply today)"] = (lambda: out32.copy_(shard), 8.0)
        passes["ps_snapshot fp32"] = (lambda: nat.ps_snapshot(shard, out32, None, None), 8.0)
        passes["ps_snapshot fp32+bak"] = (lambda: nat.ps_snapshot(shard, out32, None, bak), 12.0)
        passes["ps_snapshot bf16+bak"] = (lambda: nat.ps_snapshot(shard, None, out16, bak), 10.0)
        runs = {k: graphed(fn, a.iters) for k, (fn, _) in passes.items()}
        times = {k: [] for k in passes}
        for _ in range(a.rounds):                # alternating windows
            for k, run in runs.items():
                times[k].append(run())
        print(f"\n{name}: arena {n} elements ({used} parameters), {a.rounds} windows x "
              f"{a.iters} graph-replayed launches, median [min-max] ms")
        med, rate = {}, {}
        for k, (_, bpe) in passes.items():
            t = med[k] = statistics.median(times[k])
            rate[k] = n * bpe / t / 1e9
            spread = (max(times[k]) - min(times[k])) / t
            print(f"  {k:26s} {t:7.4f} [{min(times[k]):.4f}-{max(times[k]):.4f}] ms   "
                  f"spread {100 * spread:4.1f} %   {bpe:5.2f} B/elem   {rate[k]:6.2f} TB/s")
        for base, comp in pairs:
            print(f"  {comp:26s} {med[comp] / med[base]:5.3f} x the time, "
                  f"{100 * rate[comp] / rate[base]:5.1f} % of the bandwidth of {base}")
        print(f"  {'ps_snapshot fp32+bak':26s} "
              f"{med['ps_snapshot fp32+bak'] / med['copy_ fp32 (reply today)']:5.3f} x the time "
              f"of the copy_ it replaces (12 B/elem against 8)")
        del runs, passes, d32, d16, d8, shard, bak, out32, out16
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
