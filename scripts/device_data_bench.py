"""What feeding the training step costs, three ways, in one process on one GPU
(ResNet-18 on CIFAR-shaped data, the bench batch 512 and the reference batch 64):

(a) host milliseconds per batch of the host path: ``make_loaders`` over the
    fp32-normalised set plus ``Worker.prepare`` (cast, re-layout, upload);
(b) the batch assembler kernel (``csrc/data.hip``) alone, graph-replayed, with
    and without crop + flip, in its staged and its direct form;
(c) milliseconds per step of the captured step fed by ``DeviceBatchPool`` (what
    ``bench.py`` times; repeated, its spread is the yardstick), by the host
    loader, and by ``DeviceLoader`` writing the graph's own inputs.

Every timed window ends in a device synchronise; sclk is sampled over each
window as the bench line reports it.  ``--out FILE`` also writes the report there
(``profiles/device_data.txt`` is that file).  Needs a GPU: no fallback."""
import argparse
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
os.environ.setdefault("DMP_CONV_TUNE_SEED", os.path.join(ROOT, "tuning", "mi355x_tune_cache.json"))

import torch  # noqa: E402
from torch.utils.data import TensorDataset  # noqa: E402

from distributed_ml_pytorch_amd.ops._ext import native  # noqa: E402
from distributed_ml_pytorch_amd.runtime.dist import DistInfo  # noqa: E402
from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, Worker  # noqa: E402
from distributed_ml_pytorch_amd.utils.data import (DeviceBatchPool, make_loaders,  # noqa: E402
                                                   normalize_uint8)
from distributed_ml_pytorch_amd.utils.device_data import DeviceDataset, DeviceLoader  # noqa: E402
from distributed_ml_pytorch_amd.utils.metrics import ClockSampler  # noqa: E402

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


class Window:
    """A timed window: host clock around work that ends in a synchronise, sclk sampled over it."""

    def __init__(self, dev):
        self.clock = ClockSampler(dev.index or 0)

    def __enter__(self):
        torch.cuda.synchronize()
        self.clock.start()
        self.t0 = time.perf_counter()
        return self

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.seconds = time.perf_counter() - self.t0
        r = self.clock.stop()
        self.sclk = r["sclk_mhz_mean"] if r else None


def sclk(w):
    return "sclk n/a" if w.sclk is None else f"sclk {w.sclk:.0f} MHz"


def host_batches(loader, w):
    while True:
        for xb, yb in loader:
            yield w.prepare(xb, yb)


def bench_host_path(w, loader, n):
    it = host_batches(loader, w)
    for _ in range(3):
        next(it)
    with Window(w.device) as win:
        for _ in range(n):
            next(it)
    return win


def bench_kernel(ds, batch, pad, flip, path, launches=32, replays=20):
    """ms per launch of `launches` assembler launches captured in one graph."""
    nat = native()
    perm = torch.randperm(ds.n, generator=torch.Generator().manual_seed(0)).to(torch.int32) \
        .to(ds.device)
    x = torch.empty((batch, *ds.shape), dtype=torch.bfloat16, device=ds.device,
                    memory_format=torch.channels_last)
    y = torch.empty(batch, dtype=torch.int64, device=ds.device)

    def run():
        for k in range(launches):
            nat.batch_assemble(ds.data, ds.labels, ds.lut, perm[k * batch:(k + 1) * batch], batch,
                               x, y, None, pad, flip, 7, k, path)

    run()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    for _ in range(3):
        g.replay()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(replays):
        g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / (launches * replays)


def bench_steps(w, feed, steps, warmup):
    """ms per step of `steps` training steps fed by `feed()` -> (x, y)."""
    for _ in range(warmup):
        w.train_step(*feed(), keep=False)
    with Window(w.device) as win:
        for _ in range(steps):
            w.train_step(*feed(), keep=False)
    return win


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batches", type=int, nargs="+", default=[512, 64])
    ap.add_argument("--n", type=int, default=50000, help="samples (CIFAR-10 train split: 50000)")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3, help="runs of every step arm, interleaved")
    ap.add_argument("--host-batches", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("device_data_bench.py measures on the GPU; none found")
    info = DistInfo(device=torch.device("cuda", 0))
    g = torch.Generator().manual_seed(0)
    xu8 = torch.randint(0, 256, (a.n, 3, 32, 32), generator=g, dtype=torch.uint8)
    yl = torch.randint(0, 10, (a.n,), generator=g)
    t0 = time.perf_counter()
    host_ds = TensorDataset(normalize_uint8(xu8), yl)
    t_norm = time.perf_counter() - t0
    ds = DeviceDataset(xu8, yl, device=info.device)
    say(f"device_data_bench: {torch.cuda.get_device_name(0)}, resnet18, {a.n} CIFAR-shaped samples")
    say(f"host set: fp32 normalised {host_ds.tensors[0].numel() * 4 / 2**20:.0f} MiB "
        f"({t_norm:.2f} s to normalise); device set: uint8 {ds.data.numel() / 2**20:.0f} MiB")
    for batch in a.batches:
        say()
        say(f"== batch {batch} ==")
        cfg = TrainConfig(model="resnet18", batch_size=batch, mode="asgd", ps="local", lr=0.05,
                          evaluate=False, verbose=False)
        w = Worker(cfg, info)
        w.enable_graph(True)
        host_loader, _ = make_loaders(host_ds, host_ds, batch, batch, shuffle_seed=0)
        # (a) the host side alone
        win = bench_host_path(w, host_loader, a.host_batches)
        say(f"(a) host loader + prepare: {1e3 * win.seconds / a.host_batches:8.3f} ms / batch "
            f"({a.host_batches} batches, upload included, {sclk(win)})")
        # (b) the kernel alone
        for pad, flip, what in ((0, False, "no augmentation"), (4, True, "crop 4 + flip")):
            for path, form in ((-1, "staged"), (0, "direct")):
                ms = bench_kernel(ds, batch, pad, flip, path)
                say(f"(b) batch_assemble {form:6} {what:15}: {1e3 * ms:8.2f} us / launch "
                    "(32 launches per graph, 20 replays)")
        # (c) the captured step, fed three ways
        pool = DeviceBatchPool(batch, w.input_shape, w.num_classes, w.device, n_batches=4,
                               dtype=w.compute_dtype, seed=0)
        host_it = host_batches(host_loader, w)
        dev = DeviceLoader(ds, batch, shuffle=True, drop_last=True, pad=4, flip=True, seed=0)
        feeds = {"DeviceBatchPool": pool.next, "host loader": lambda: next(host_it),
                 "DeviceLoader": lambda: dev.next(out=w.static_inputs())}
        w.train_step(*pool.next())           # capture
        res = {k: [] for k in feeds}
        for _ in range(a.repeats):
            for name, feed in feeds.items():
                win = bench_steps(w, feed, a.steps, a.warmup)
                res[name].append((1e3 * win.seconds / a.steps, win.sclk))
        for name, runs in res.items():
            ms = [r[0] for r in runs]
            clk = ", ".join("n/a" if r[1] is None else f"{r[1]:.0f}" for r in runs)
            say(f"(c) step fed by {name:15}: " + " ".join(f"{v:7.3f}" for v in ms)
                + f" ms / step (min {min(ms):.3f}, spread {max(ms) - min(ms):.3f}; sclk MHz {clk})")
        base = [r[0] for r in res["DeviceBatchPool"]]
        d = min(r[0] for r in res["DeviceLoader"]) - min(base)
        say(f"    DeviceLoader - DeviceBatchPool (min over runs): {d:+.3f} ms; "
            f"DeviceBatchPool run-to-run spread {max(base) - min(base):.3f} ms")
        w.finish()
        del w, pool, dev
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
