"""What Mixup / CutMix cost, in one process on one GPU, every arm against the
plain kernel in the same run:

(a) the batch assembler (``csrc/data.hip``), plain against the mixing form in its
    three modes (none, mixup, cutmix), with crop 4 + flip: CIFAR-shaped data at
    batch 512 and 64 (images staged through LDS) and 3 x 224 x 224 at batch 128
    (direct gather, several waves per image);
(b) the fused softmax-cross-entropy (``csrc/xent.hip``), plain against the
    two-target form, bf16 logits [512, 10] and [128, 1000];
(c) the captured ResNet-18 step at batch 512 fed by ``DeviceLoader`` with
    ``crop_flip``, without and with ``--mixup 0.8 --cutmix 1.0``.

(a) and (b): every arm is a graph of several launches; the arms are replayed in
turn, ``--repeats`` times, after a warm-up, and timed with device events; the
minimum and the spread over the repeats are reported.  (c): two workers, each
with its own captured step, timed in turn the same way.  ``--out FILE`` also
writes the report there (``profiles/mix_assemble.txt`` is that file).  Needs a
GPU: no fallback."""
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
                                                          MixConfig, MixParams)

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
    """{name: [us per launch, one per repeat]} of graphs replayed in turn."""
    res = {k: [] for k in arms}
    for _ in range(repeats):
        for name, g in arms.items():
            res[name].append(1e3 * timed(g.replay, replays) / (launches * replays))
    return res


def report(tag, res, base):
    b = min(res[base])
    for name, v in res.items():
        say(f"{tag} {name:14}: min {min(v):8.2f} us / launch, spread {max(v) - min(v):6.2f} "
            f"({min(v) - b:+7.2f} us, x{min(v) / b:.3f} against {base})")


def bench_assembler(shape, n, batch, launches, replays, repeats):
    c, h, w = shape
    g = torch.Generator().manual_seed(0)
    ds = DeviceDataset(torch.randint(0, 256, (n, c, h, w), generator=g, dtype=torch.uint8),
                       torch.randint(0, 10, (n,), generator=g), (0.5,) * c, (0.25,) * c,
                       device="cuda")
    nat = native()
    perm = torch.randperm(n, generator=g).to(torch.int32).cuda()
    assert launches * batch <= n
    x = torch.empty((batch, c, h, w), dtype=torch.bfloat16, device="cuda",
                    memory_format=torch.channels_last)
    y = torch.empty(batch, dtype=torch.int64, device="cuda")
    y2, lam = torch.empty_like(y), torch.empty(batch, dtype=torch.float32, device="cuda")
    box = (h // 4, h // 4 + h // 2, w // 4, w // 4 + w // 2)            # a quarter of the image
    modes = {"mix none": MixParams("none", 1.0, 1.0, (0, 0, 0, 0)),
             "mix mixup": MixParams("mixup", 0.3172, 0.3172, (0, 0, 0, 0)),
             "mix cutmix": MixParams("cutmix", 1.0, 0.75, box)}

    def plain():
        for k in range(launches):
            nat.batch_assemble(ds.data, ds.labels, ds.lut, perm[k * batch:(k + 1) * batch], batch,
                               x, y, None, 4, True, 7, k)

    def mixed(p):
        def run():
            for k in range(launches):
                nat.batch_assemble_mix(ds.data, ds.labels, ds.lut, perm[k * batch:(k + 1) * batch],
                                       batch, x, y, y2, lam, None, 4, True, 7, k, p.pix_lam,
                                       p.label_lam, *p.box)
        return run

    arms = {"plain": graph_of(plain)}
    for name, p in modes.items():
        arms[name] = graph_of(mixed(p))
    form = "staged" if nat.batch_assemble_is_staged(ds.data) else "direct"
    moved = batch * c * h * w * 3 / 1e6
    say(f"(a) {c}x{h}x{w} batch {batch} ({form}; plain moves {moved:.1f} MB: uint8 in, bf16 out), "
        f"{launches} launches per graph, {replays} replays, {repeats} repeats")
    report("(a)", alternate(arms, launches, replays, repeats), "plain")
    del ds


def bench_xent(B, C, launches, replays, repeats):
    nat = native()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, C, generator=g).to(torch.bfloat16).cuda()
    y = torch.randint(0, C, (B,), generator=g).cuda()
    y2 = torch.randint(0, C, (B,), generator=g).cuda()
    lam = torch.rand(B, generator=g).cuda()

    def plain():
        for _ in range(launches):
            nat.softmax_xent(x, y, True, 0.1, -100)

    def mix():
        for _ in range(launches):
            nat.softmax_xent_mix(x, y, y2, lam, True, 0.1, -100)

    arms = {"plain": graph_of(plain), "two-target": graph_of(mix)}
    say(f"(b) softmax-xent bf16 [{B}, {C}], {launches} launches per graph, {replays} replays, "
        f"{repeats} repeats (multi-block shapes: the finalize launch included)")
    report("(b)", alternate(arms, launches, replays, repeats), "plain")


def bench_steps(batch, n, steps, warmup, repeats):
    info = DistInfo(device=torch.device("cuda", 0))
    g = torch.Generator().manual_seed(0)
    ds = DeviceDataset(torch.randint(0, 256, (n, 3, 32, 32), generator=g, dtype=torch.uint8),
                       torch.randint(0, 10, (n,), generator=g), device=info.device)
    arms = {}
    for name, kw in (("crop_flip", {}), ("crop_flip + mix", {"mixup": 0.8, "cutmix": 1.0})):
        cfg = TrainConfig(model="resnet18", batch_size=batch, mode="asgd", ps="local", lr=0.05,
                          evaluate=False, verbose=False, device_data=True, augment="crop_flip", **kw)
        w = Worker(cfg, info)
        w.enable_graph(True)
        mix = MixConfig(0.8, 1.0) if kw else None
        loader = DeviceLoader(ds, batch, shuffle=True, drop_last=True, pad=4, flip=True, seed=0,
                              mix=mix)

        def step(w=w, loader=loader):
            x, y = loader.next(out=w.static_batch_buffers())
            w.train_step(x, y, keep=False, mix=loader.last_mix)

        for _ in range(warmup):
            step()
        arms[name] = (step, w)
    res = {k: [] for k in arms}
    for _ in range(repeats):
        for name, (step, _) in arms.items():
            res[name].append(timed(step, steps) / steps)
    say(f"(c) resnet18 batch {batch} captured step fed by DeviceLoader, {steps} steps per window, "
        f"{repeats} windows per arm in turn, device-event time (host draw and launch included)")
    b = min(res["crop_flip"])
    for name, v in res.items():
        say(f"(c) {name:16}: " + " ".join(f"{t:7.3f}" for t in v)
            + f" ms / step (min {min(v):.3f}, spread {max(v) - min(v):.3f}, {min(v) - b:+.3f} ms)")
    for _, w in arms.values():
        w.finish()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=12)
    ap.add_argument("--skip-steps", action="store_true", help="leave out (c)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mix_bench.py measures on the GPU; none found")
    say(f"mix_bench: {torch.cuda.get_device_name(0)}")
    for shape, n, batch, launches in (((3, 32, 32), 16384, 512, 32), ((3, 32, 32), 16384, 64, 32),
                                      ((3, 224, 224), 1024, 128, 8)):
        bench_assembler(shape, n, batch, launches, a.replays, a.repeats)
        say()
    for B, C in ((512, 10), (128, 1000)):
        bench_xent(B, C, 32, a.replays, a.repeats)
        say()
    if not a.skip_steps:
        bench_steps(512, 50000, a.steps, a.warmup, a.repeats)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
