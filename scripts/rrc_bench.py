"""What the random-resized-crop assembler costs, in one process on one GPU, every
arm against the plain crop kernel of the same run:

(a) one launch at 3 x 224 x 224 output, batch 128: the plain assembler
    (``csrc/data.hip``, crop 4 + flip) against ``csrc/data_rrc.hip`` from 224- and
    256-stored datasets, staged and direct form, plain and with Mixup;
(b) the captured ResNet-50 step at batch 128 fed by ``DeviceLoader`` with
    ``crop_flip`` against the step fed by ``rrc_flip`` from 256-stored images.

(a): every arm is a graph of several launches; the arms are replayed in turn,
``--repeats`` times, after a warm-up, and timed with device events; the minimum
and the spread over the repeats are reported.  (b): two workers, each with its
own captured step, timed in turn the same way.  ``--out FILE`` also writes the
report there (``profiles/rrc_assemble.txt`` is that file).  Needs a GPU: no
fallback."""
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
from distributed_ml_pytorch_amd.utils.device_data import (DeviceDataset, DeviceLoader,  # noqa: E402
                                                          RrcConfig, rrc_box_table)

LINES = []
OUT = 224


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


def dataset(n, size, seed=0):
    g = torch.Generator().manual_seed(seed)
    return DeviceDataset(torch.randint(0, 256, (n, 3, size, size), generator=g, dtype=torch.uint8),
                         torch.randint(0, 10, (n,), generator=g), (0.5,) * 3, (0.25,) * 3,
                         device="cuda")


def bench_assembler(n, batch, launches, replays, repeats):
    nat = native()
    sets = {s: dataset(n, s) for s in (224, 256)}
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(1)).to(torch.int32).cuda()
    assert launches * batch <= n
    x = torch.empty((batch, 3, OUT, OUT), dtype=torch.bfloat16, device="cuda",
                    memory_format=torch.channels_last)
    y = torch.empty(batch, dtype=torch.int64, device="cuda")
    y2, lam = torch.empty_like(y), torch.empty(batch, dtype=torch.float32, device="cuda")

    def plain():
        ds = sets[224]
        for k in range(launches):
            nat.batch_assemble(ds.data, ds.labels, ds.lut, perm[k * batch:(k + 1) * batch], batch,
                               x, y, None, 4, True, 7, k)

    def rrc(ds, table, path, mix):
        def run():
            for k in range(launches):
                idx = perm[k * batch:(k + 1) * batch]
                if mix:
                    nat.batch_assemble_rrc_mix(ds.data, ds.labels, ds.lut, idx, batch, table, None,
                                               x, y, y2, lam, None, True, 7, k, 0.3172, 0.3172,
                                               0, 0, 0, 0, path, False)
                else:
                    nat.batch_assemble_rrc(ds.data, ds.labels, ds.lut, idx, batch, table, None, x,
                                           y, None, True, 7, k, path, False)
        return run

    arms = {"plain crop_flip 224": graph_of(plain)}
    for size, ds in sets.items():
        table = rrc_box_table(size, size).cuda()
        for form, path in (("staged", -1), ("direct", 0)):
            arms[f"rrc {size} {form}"] = graph_of(rrc(ds, table, path, False))
        arms[f"rrc {size} staged mixup"] = graph_of(rrc(ds, table, -1, True))
    staged, strip, rows, lds = nat.batch_assemble_rrc_plan(256, 256, 3, OUT, OUT, False)
    say(f"(a) 3x{OUT}x{OUT} output, batch {batch}: {launches} launches per graph, {replays} replays, "
        f"{repeats} repeats; plan of 256 -> {OUT}: staged {staged}, strips of {strip} rows, "
        f"{rows} staged rows, {lds} B of LDS")
    res = {k: [] for k in arms}
    for _ in range(repeats):
        for name, g in arms.items():
            res[name].append(1e3 * timed(g.replay, replays) / (launches * replays))
    base = min(res["plain crop_flip 224"])
    for name, v in res.items():
        say(f"(a) {name:24}: min {min(v):8.2f} us / launch, spread {max(v) - min(v):6.2f} "
            f"({min(v) - base:+7.2f} us, x{min(v) / base:.3f} against the plain kernel)")
    return res


def bench_steps(batch, n, steps, warmup, repeats):
    info = DistInfo(device=torch.device("cuda", 0))
    arms = {}
    for name, size, kw in (("crop_flip", 224, dict(pad=4, flip=True)),
                           ("rrc_flip 256", 256, dict(flip=True, rrc=RrcConfig(), out_hw=(OUT, OUT)))):
        cfg = TrainConfig(model="resnet50", num_classes=1000, batch_size=batch, mode="asgd",
                          ps="local", lr=0.05, evaluate=False, verbose=False, device_data=True,
                          augment="crop_flip")
        w = Worker(cfg, info)
        w.enable_graph(True)
        loader = DeviceLoader(dataset(n, size), batch, shuffle=True, drop_last=True, seed=0, **kw)

        def step(w=w, loader=loader):
            x, y = loader.next(out=w.static_batch_buffers())
            w.train_step(x, y, keep=False)

        for _ in range(warmup):
            step()
        arms[name] = (step, w)
    res = {k: [] for k in arms}
    for _ in range(repeats):
        for name, (step, _) in arms.items():
            res[name].append(timed(step, steps) / steps)
    say(f"(b) resnet50 batch {batch} captured step fed by DeviceLoader, {steps} steps per window, "
        f"{repeats} windows per arm in turn, device-event time (host launch included)")
    b = min(res["crop_flip"])
    for name, v in res.items():
        say(f"(b) {name:14}: " + " ".join(f"{t:7.3f}" for t in v)
            + f" ms / step (min {min(v):.3f}, spread {max(v) - min(v):.3f}, {min(v) - b:+.3f} ms)")
    for _, w in arms.values():
        w.finish()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=6)
    ap.add_argument("--skip-steps", action="store_true", help="leave out (b)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("rrc_bench.py measures on the GPU; none found")
    say(f"rrc_bench: {torch.cuda.get_device_name(0)}")
    res = bench_assembler(1024, 128, 8, a.replays, a.repeats)
    plain, new = min(res["plain crop_flip 224"]), min(res["rrc 256 staged"])
    say(f"expectation from the bytes (the launch writes the same 301 KB per image and reads at "
        f"most the box, so it should land near the plain form): rrc 256 staged {new:.1f} us against "
        f"{plain:.1f} us of the plain kernel in this run, x{new / plain:.3f}")
    say()
    if not a.skip_steps:
        bench_steps(128, 512, a.steps, a.warmup, a.repeats)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
