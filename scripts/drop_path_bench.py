"""What stochastic depth costs, in one process on one GPU:

(a) the draw launch (``csrc/drop_path.hip``): the [24, 64] table of ViT-B/16 at
    batch 64;
(b) one add+LayerNorm forward / backward pair on the ViT-B/16 stream
    (64 x 197 rows of 768), row-scaled at p = 0.1 against the unscaled pair;
(c) the captured ``vit_b16`` training step at batch 64, one arm per
    ``--arms`` rate (default 0 and 0.1), each worker with its own graph.

(a) and (b): every arm is a graph of several launches; (c): the workers' own
captured steps.  The arms are replayed in turn, ``--repeats`` times after a
warm-up, and timed with device events; the minimum and the spread over the
repeats are reported.  ``--skip-kernels`` leaves out (a) and (b) (the A/B of a
``drop_path = 0`` step between two trees runs (c) alone, one process per tree,
in turn).  ``--out FILE`` also writes the report there
(``profiles/drop_path.txt`` holds one).  Needs a GPU: no fallback."""
import argparse
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
os.environ.setdefault("DMP_CONV_TUNE_SEED", os.path.join(ROOT, "tuning", "mi355x_tune_cache.json"))

import torch  # noqa: E402

from distributed_ml_pytorch_amd.ops._ext import native  # noqa: E402
from distributed_ml_pytorch_amd.runtime.dist import DistInfo  # noqa: E402
from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, Worker  # noqa: E402

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, n):
    """Device milliseconds of ``n`` calls of ``fn`` (events around them)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def graph_of(run):
    run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for _ in range(3):
        g.replay()
    return g


def alternate(arms, launches, replays, repeats):
    res = {k: [] for k in arms}
    for _ in range(repeats):
        for name, g in arms.items():
            res[name].append(1e3 * timed(g.replay, replays) / (launches * replays))
    return res


def report(tag, res, base):
    b = min(res[base])
    for name, v in res.items():
        say(f"{tag} {name:12}: min {min(v):8.2f} us, spread {max(v) - min(v):6.2f} "
            f"({min(v) - b:+7.2f} us, x{min(v) / b:.3f} against {base})")


def bench_draw(replays, repeats):
    from distributed_ml_pytorch_amd.ops import functional as DF

    rates = [r for r in DF.drop_path_rates(0.1, 12) for _ in range(2)]
    thr, sc = DF.drop_path_consts(rates, "cuda")
    state = torch.zeros(1, dtype=torch.int64, device="cuda")
    launches = 16

    def run():
        for _ in range(launches):
            DF.drop_path_table(state, thr, sc, 64, 11)

    res = alternate({"draw": graph_of(run)}, launches, replays, repeats)
    say(f"(a) draw of the [24, 64] table, {launches} launches per graph, {replays} replays, "
        f"{repeats} repeats")
    report("(a)", res, "draw")


def bench_pair(replays, repeats):
    from distributed_ml_pytorch_amd.ops.functional import LN_SLOTS

    nat = native()
    B, T, D = 64, 197, 768
    g = torch.Generator().manual_seed(0)
    rn = lambda *s: torch.randn(*s, generator=g).to(torch.bfloat16).cuda()
    x, r, dy, dh = rn(B * T, D), rn(B * T, D), rn(B * T, D), rn(B * T, D)
    gamma, beta = torch.ones(D, device="cuda"), torch.zeros(D, device="cuda")
    dg, db = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
    slots = torch.zeros(LN_SLOTS * 2 * D, device="cuda")
    keep = torch.rand(B, generator=g) >= 0.1
    s = torch.where(keep, torch.tensor(1.0) / torch.tensor(0.9), torch.tensor(0.0)).cuda()
    launches = 4

    def pair(scale):
        def run():
            for _ in range(launches):
                if scale is None:
                    y, mean, rstd, h = nat.layernorm_fwd(x, gamma, beta, 1e-6, r)
                    nat.layernorm_bwd(h, dy, gamma, mean, rstd, dg, db, slots, dh)
                else:
                    y, mean, rstd, h = nat.layernorm_fwd(x, gamma, beta, 1e-6, r, scale, T)
                    nat.layernorm_bwd(h, dy, gamma, mean, rstd, dg, db, slots, dh, scale, T)
        return run

    arms = {"unscaled": graph_of(pair(None)), "scaled": graph_of(pair(s))}
    mb = B * T * D * 2 / 1e6
    say(f"(b) add+LayerNorm forward + backward pair, {B * T} rows of {D} ({mb:.1f} MB per stream; "
        f"{int(keep.sum())} of {B} samples kept), {launches} pairs per graph, {replays} replays, "
        f"{repeats} repeats; the scaled backward writes one more stream")
    report("(b)", alternate(arms, launches, replays, repeats), "unscaled")


def bench_steps(rates, batch, steps, warmup, repeats):
    info = DistInfo(device=torch.device("cuda", 0))
    arms = {}
    for p in rates:
        kw = {"drop_path": p} if p > 0 else {}
        cfg = TrainConfig(model="vit_b16", batch_size=batch, mode="asgd", ps="local", lr=0.01,
                          n_push=10 ** 9, n_pull=10 ** 9, evaluate=False, verbose=False, **kw)
        w = Worker(cfg, info)
        w.enable_graph(True)
        g = torch.Generator().manual_seed(0)
        x, y = w.prepare(torch.randn(batch, *w.input_shape, generator=g),
                         torch.randint(0, w.num_classes, (batch,), generator=g))

        def step(w=w, x=x, y=y):
            w.train_step(x, y, keep=False)

        for _ in range(warmup):
            step()
        x, y = w.static_inputs()          # replayed in place: no input copy in the window

        def step(w=w, x=x, y=y):          # noqa: F811
            w.train_step(x, y, keep=False)

        arms[f"drop_path {p:g}"] = (step, w)
    res = {k: [] for k in arms}
    for _ in range(repeats):
        for name, (step, _) in arms.items():
            res[name].append(timed(step, steps) / steps)
    say(f"(c) vit_b16 batch {batch} captured training step, {steps} steps per window, {repeats} "
        f"windows per arm in turn, device-event time")
    base = next(iter(res))
    b = min(res[base])
    for name, v in res.items():
        say(f"(c) {name:14}: " + " ".join(f"{t:7.3f}" for t in v)
            + f" ms / step (min {min(v):.3f}, spread {max(v) - min(v):.3f}, {min(v) - b:+.3f} ms "
              f"against {base})")
    for _, w in arms.values():
        w.finish()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--arms", default="0,0.1", help="drop path rates of the step arms of (c)")
    ap.add_argument("--skip-kernels", action="store_true", help="leave out (a) and (b)")
    ap.add_argument("--skip-steps", action="store_true", help="leave out (c)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("drop_path_bench.py measures on the GPU; none found")
    say(f"drop_path_bench: {torch.cuda.get_device_name(0)}")
    if not a.skip_kernels:
        bench_draw(a.replays, a.repeats)
        say()
        bench_pair(a.replays, a.repeats)
        say()
    if not a.skip_steps:
        bench_steps([float(p) for p in a.arms.split(",")], a.batch, a.steps, a.warmup, a.repeats)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
