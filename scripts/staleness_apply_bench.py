"""What the staleness policy "damp" adds to a PS apply (parallel/staleness.py).

Times, at the ResNet-18 arena size on one GPU, the atomic fp32 ``ps_apply`` of
the link path (a) plain, as policy "off" launches it, and (b) damped:
``ps_stale_factor`` + ``ps_apply(factor=slot)``, one extra 1-block launch per
apply.  With ``--other-ext PATH`` (the ``_native*.so`` of another build, e.g. of
the parent commit) the plain apply of that build is timed too, in alternating
fresh processes, so both see the same machine state:

    python scripts/staleness_apply_bench.py --other-ext /path/to/_native.so

Each figure is device-event time over ``--iters`` back-to-back launches on one
stream after a warm-up, per apply, in microseconds.
"""
import argparse
import importlib.util
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _arena_numel() -> int:
    from distributed_ml_pytorch_amd.models import build_model
    from distributed_ml_pytorch_amd.parallel.arena import FlatArena

    model, _, _ = build_model("resnet18", None)
    return FlatArena(list(model.parameters()), device="cpu", shadow_dtype=None,
                     with_grads=False).p32.numel()


def _load(ext: str | None):
    import torch  # noqa: F401  (the extension links against torch's libraries)

    if ext is None:
        from distributed_ml_pytorch_amd.ops._ext import native

        return native()
    spec = importlib.util.spec_from_file_location("_native", ext)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def child(ext: str | None, iters: int, n: int):
    import torch

    nat = _load(ext)
    dev = torch.device("cuda", 0)
    shard = torch.zeros(n, device=dev)
    delta = torch.randn(n, device=dev) * 1e-3
    cnt = torch.zeros(1, dtype=torch.int32, device=dev)

    def timed(fn):
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return 1e3 * a.elapsed_time(b) / iters

    def plain():
        nat.ps_apply(shard, delta, None, 1.0, True)
        nat.ps_count(cnt, 1)

    out = {"plain_us": timed(plain)}
    if ext is None:
        slot = torch.zeros(2, device=dev)
        log = torch.zeros(nat.ps_stale_log_numel(), dtype=torch.int32, device=dev)

        def damped():
            nat.ps_stale_factor(cnt, 0, 1 << 20, slot, log)      # bound never reached: f = 1
            nat.ps_apply(shard, delta, None, 1.0, True, slot)
            nat.ps_count(cnt, 1)

        def factor_only():
            nat.ps_stale_factor(cnt, 0, 1 << 20, slot, log)

        out["damped_us"] = timed(damped)
        out["factor_kernel_us"] = timed(factor_only)
        out["plain_again_us"] = timed(plain)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--other-ext", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--numel", type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child is not None:
        return child(None if a.child == "tree" else a.child, a.iters, a.numel)
    n = _arena_numel()
    arms = ["tree"] + ([a.other_ext] if a.other_ext else [])
    rows = {arm: [] for arm in arms}
    for r in range(a.rounds):
        for arm in arms:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", arm,
                                "--iters", str(a.iters), "--numel", str(n)],
                               capture_output=True, text=True, timeout=300, cwd=ROOT)
            if p.returncode != 0:
                raise SystemExit(f"{arm} failed ({p.returncode}):\n{p.stderr[-2000:]}")
            res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
            rows[arm].append(res)
            print(f"round {r} {'tree ' if arm == 'tree' else 'other'} " +
                  " ".join(f"{k}={v:.2f}" for k, v in res.items()), flush=True)
    print(f"\narena: {n} fp32 elements ({4 * n / 2 ** 20:.1f} MiB), {a.iters} launches per figure, "
          f"{a.rounds} alternating rounds; median [min, max] in us per apply")
    for arm in arms:
        for k in rows[arm][0]:
            v = [r[k] for r in rows[arm]]
            print(f"{'tree ' if arm == 'tree' else 'other'} {k:18s} {statistics.median(v):8.2f} "
                  f"[{min(v):.2f}, {max(v):.2f}]")


if __name__ == "__main__":
    main()
