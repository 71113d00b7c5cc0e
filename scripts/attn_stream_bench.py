"""Time the streaming attention route (csrc/attention_stream.hip), graph-replayed.

(a) streaming against resident at the sizes both take (B 64, H 12, N 197 / 256):
    the price of the online rescale and the tiling;
(b) streaming at B 16, H 12, N 577 / 1025 against the two routes a user had for
    those shapes before it: stock ``F.scaled_dot_product_attention`` on bf16 and
    the ``matmul + native softmax`` oracle route of ``ops.functional.attention``
    (both in the stock oracle mode), each from the qkv rows to d(qkv);
(c) one ``vit_b16_384`` batch-16 training step: ms per step and the share of its
    24 attention calls (12 layers, from the kernel times of (b)).

Every figure is the time of K calls captured in one graph and replayed, device
events around the replays, min over rounds with the arms alternating inside a
round; the spread is max - min over the rounds.  TF/s use the flop count of
scripts/attn_bench.py: 4 B H N^2 64 forward, 2.5x that backward.  sclk is sampled
over each arm's windows.  ``--out FILE`` also writes the report there
(``profiles/attention_stream.txt`` is that file).  Needs a GPU: no fallback."""
import argparse
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
os.environ.setdefault("DMP_CONV_TUNE_SEED", os.path.join(ROOT, "tuning", "mi355x_tune_cache.json"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from distributed_ml_pytorch_amd.ops import functional as DF  # noqa: E402
from distributed_ml_pytorch_amd.ops._ext import native  # noqa: E402
from distributed_ml_pytorch_amd.ops._policy import stock_allowed  # noqa: E402
from distributed_ml_pytorch_amd.utils.metrics import ClockSampler  # noqa: E402

LINES = []
RESIDENT, STREAM = 0, 1


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def capture(fn, calls):
    """`calls` calls of fn in one graph (warmed up on a side stream first)."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(calls):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def time_arms(arms, calls, replays, rounds):
    """arms: name -> fn.  Returns name -> (min us per call, spread us, mean sclk MHz)."""
    graphs = {k: capture(fn, calls) for k, fn in arms.items()}
    us = {k: [] for k in arms}
    clk = {k: [] for k in arms}
    for _ in range(rounds):
        for k, g in graphs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            sampler = ClockSampler(torch.cuda.current_device())
            torch.cuda.synchronize()
            sampler.start()
            a.record()
            for _ in range(replays):
                g.replay()
            b.record()
            b.synchronize()
            r = sampler.stop()
            us[k].append(a.elapsed_time(b) * 1e3 / (calls * replays))
            if r:
                clk[k].append(r["sclk_mhz_mean"])
    return {k: (min(v), max(v) - min(v), sum(clk[k]) / len(clk[k]) if clk[k] else None)
            for k, v in us.items()}


def fmt(name, t, flop):
    us, spread, clk = t
    c = "sclk n/a" if clk is None else f"sclk {clk:.0f} MHz"
    return f"    {name:<34s} {us:9.1f} us  (spread {spread:6.1f})  {flop / us / 1e6:6.0f} TF/s  {c}"


def inputs(B, N, H):
    g = torch.Generator(device="cuda").manual_seed(N)
    qkv = (torch.randn(B, N, 3 * H * 64, device="cuda", generator=g) * 0.5).to(torch.bfloat16)
    dout = torch.randn(B, N, H * 64, device="cuda", generator=g).to(torch.bfloat16)
    return qkv, dout


def native_arms(qkv, dout, H, route, tag):
    nat = native()
    out, lse = nat.attention_fwd(qkv, H, route)
    return {f"{tag} fwd": lambda: nat.attention_fwd(qkv, H, route),
            f"{tag} bwd": lambda: nat.attention_bwd(qkv, out, dout, lse, H, route)}


def stock_arms(qkv, dout, H, kind):
    """fwd and fwd + bwd of a stock route from the qkv rows to d(qkv), as
    ops.functional.attention_qkv reaches it (views in, one reshape out)."""
    B, N, _ = qkv.shape
    x = qkv.clone().requires_grad_(True)

    def fwd(t):
        q, k, v = t.view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4)
        o = F.scaled_dot_product_attention(q, k, v) if kind == "sdpa" else DF.attention(q, k, v)
        return o.transpose(1, 2).reshape(B, N, H * 64)

    def fwd_only():
        with torch.no_grad():
            return fwd(qkv)

    def fwd_bwd():
        return torch.autograd.grad(fwd(x), x, dout)

    return {f"{kind} fwd": fwd_only, f"{kind} fwd+bwd": fwd_bwd}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--calls", type=int, default=8, help="calls per graph")
    ap.add_argument("--replays", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="vit_b16_384 steps (0: skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "attn_stream_bench needs a GPU"
    say(f"# attn_stream_bench: {torch.cuda.get_device_name(0)}, {a.calls} calls per graph, "
        f"{a.replays} replays, min over {a.rounds} rounds (spread = max - min), head dim 64, bf16")
    T = lambda *x: time_arms(*x, a.calls, a.replays, a.rounds)

    say("(a) streaming against resident, B 64, H 12")
    H = 12
    for N in (197, 256):
        qkv, dout = inputs(64, N, H)
        flop = 4.0 * 64 * H * N * N * 64
        t = T({**native_arms(qkv, dout, H, RESIDENT, "resident"),
               **native_arms(qkv, dout, H, STREAM, "streaming")})
        say(f"  N {N}")
        for k in ("resident fwd", "streaming fwd"):
            say(fmt(k, t[k], flop))
        for k in ("resident bwd", "streaming bwd"):
            say(fmt(k, t[k], 2.5 * flop))
        say(f"    streaming / resident: fwd {t['streaming fwd'][0] / t['resident fwd'][0]:.3f}  "
            f"bwd {t['streaming bwd'][0] / t['resident bwd'][0]:.3f}")

    say("(b) streaming against the stock routes, B 16, H 12 (qkv rows -> out, -> d(qkv))")
    kernel_us = {}
    for N in (577, 1025):
        qkv, dout = inputs(16, N, H)
        flop = 4.0 * 16 * H * N * N * 64
        arms = native_arms(qkv, dout, H, STREAM, "streaming")
        with stock_allowed(True):
            arms.update(stock_arms(qkv, dout, H, "sdpa"))
            arms.update(stock_arms(qkv, dout, H, "matmul+softmax"))
            t = T(arms)
        say(f"  N {N}" + ("  (past 1024 keys attention() itself goes to SDPA: the two stock arms "
                          "are the same route)" if N > 1024 else ""))
        ours_f, ours_b = t["streaming fwd"][0], t["streaming bwd"][0]
        kernel_us[N] = ours_f + ours_b
        say(fmt("streaming fwd", t["streaming fwd"], flop))
        say(fmt("streaming bwd", t["streaming bwd"], 2.5 * flop))
        say(f"    {'streaming fwd+bwd (sum)':<34s} {ours_f + ours_b:9.1f} us")
        for kind in ("sdpa", "matmul+softmax"):
            say(fmt(f"{kind} fwd", t[f"{kind} fwd"], flop))
            say(fmt(f"{kind} fwd+bwd", t[f"{kind} fwd+bwd"], 3.5 * flop))
        bf = min(t["sdpa fwd"][0], t["matmul+softmax fwd"][0])
        bb = min(t["sdpa fwd+bwd"][0], t["matmul+softmax fwd+bwd"][0])
        say(f"    streaming / faster stock route: fwd {ours_f / bf:.3f}  "
            f"fwd+bwd {(ours_f + ours_b) / bb:.3f}  (stock sdpa spread: fwd "
            f"{t['sdpa fwd'][1]:.1f} us, fwd+bwd {t['sdpa fwd+bwd'][1]:.1f} us)")

    if a.steps > 0:
        from distributed_ml_pytorch_amd.runtime.dist import DistInfo
        from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, Worker

        say("(c) vit_b16_384, batch 16, ASGD, local PS: one training step")
        cfg = TrainConfig(model="vit_b16_384", batch_size=16, mode="asgd", ps="local", n_push=1,
                          n_pull=1, lr=0.01, evaluate=False, verbose=False)
        w = Worker(cfg, DistInfo(device=torch.device("cuda", 0)))
        g = torch.Generator().manual_seed(0)
        x = torch.randn(16, *w.input_shape, generator=g)
        y = torch.randint(0, w.num_classes, (16,), generator=g)
        x, y = w.prepare(x, y)
        for _ in range(3):
            w.train_step(x, y)
        ms = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.steps):
                w.train_step(x, y)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / a.steps)
        w.finish()
        att = 12 * kernel_us[577] / 1e3
        say(f"    {min(ms):.2f} ms / step (min of 3 x {a.steps} eager steps, spread "
            f"{max(ms) - min(ms):.2f}); attention 12 x (fwd + bwd) = {att:.2f} ms from (b): "
            f"{100 * att / min(ms):.1f} % of the step")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
