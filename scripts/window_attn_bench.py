"""Time the shifted-window attention kernels (csrc/attention_window.hip), graph-replayed.

(a) the four Swin-T stage shapes at batch 128, forward and backward (with the
    bias-table gradient), against a device copy that moves the same bytes (8C
    per token forward, 14C backward) and against the stock route in the oracle
    mode: roll + partition + SDPA with the bias and mask as its additive mask +
    reverse, from the qkv rows to out and to d(qkv);
(b) one captured ``swin_tiny`` batch-128 training step: ms per step and the share
    of its 12 window-attention calls (from the kernel times of (a)).

Expectation, stated before measuring: the forward moves 8C bytes per token (Swin-T
stage 1 at batch 128: 308 MB), so its floor is roughly the device copy of those
bytes; the backward moves about twice that.  The report says confirmed / refuted.

Every figure is the time of K calls captured in one graph and replayed, device
events around the replays, min over rounds with the arms alternating inside a
round; the spread is max - min over the rounds; sclk is sampled over each arm's
windows.  ``--out FILE`` also writes the report there
(``profiles/window_attention.txt`` is that file).  Needs a GPU: no fallback."""
import argparse
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("DMP_CONV_TUNE_SEED", os.path.join(ROOT, "tuning", "mi355x_tune_cache.json"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from attn_stream_bench import LINES, say, time_arms  # noqa: E402
from distributed_ml_pytorch_amd.ops import functional as DF  # noqa: E402
from distributed_ml_pytorch_amd.ops._ext import native  # noqa: E402
from distributed_ml_pytorch_amd.ops._policy import stock_allowed  # noqa: E402

STAGES = ((56, 3, 3, 2), (28, 6, 3, 2), (14, 12, 3, 6), (7, 24, 0, 2))   # map, heads, shift, depth
WS, BATCH = 7, 128


def stock_arms(qkv, dout, table, heads, sh):
    B, Hm, Wm, _ = qkv.shape
    N, C = WS * WS, heads * 32
    bias = table[DF.window_bias_index(WS, qkv.device).reshape(-1)].view(N, N, heads).permute(2, 0, 1)
    mask = bias[None].to(qkv.dtype)
    if sh:
        lab = DF._windows(DF.window_region_labels(Hm, Wm, WS, sh, qkv.device)[None], WS)
        m = (lab[:, :, None] != lab[:, None, :]).to(qkv.dtype) * DF.WINDOW_MASK_VALUE
        mask = (mask + m[:, None]).repeat(B, 1, 1, 1)
    x = qkv.clone().requires_grad_(True)

    def fwd(t):
        r = torch.roll(t, (-sh, -sh), (1, 2)) if sh else t
        q, k, v = DF._windows(r, WS).view(-1, N, 3, heads, 32).permute(2, 0, 3, 1, 4)
        o = F.scaled_dot_product_attention(q, k, v, attn_mask=mask).transpose(1, 2)
        o = o.reshape(B, Hm // WS, Wm // WS, WS, WS, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hm, Wm, C)
        return torch.roll(o, (sh, sh), (1, 2)) if sh else o

    def fwd_only():
        with torch.no_grad():
            return fwd(qkv)

    return {"stock fwd": fwd_only, "stock fwd+bwd": lambda: torch.autograd.grad(fwd(x), x, dout)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--calls", type=int, default=4, help="calls per graph")
    ap.add_argument("--replays", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10, help="swin_tiny steps per window (0: skip)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "window_attn_bench needs a GPU"
    say(f"# window_attn_bench: {torch.cuda.get_device_name(0)}, {a.calls} calls per graph, "
        f"{a.replays} replays, min over {a.rounds} rounds (spread = max - min), window {WS}, "
        f"head dim 32, bf16, batch {BATCH}")
    say("expectation: fwd ~ a device copy moving 8C bytes per token, bwd ~ twice the fwd")
    nat, total_us = native(), 0.0
    for Hm, heads, sh, depth in STAGES:
        C = heads * 32
        g = torch.Generator(device="cuda").manual_seed(Hm)
        qkv = (torch.randn(BATCH, Hm, Hm, 3 * C, device="cuda", generator=g) * 0.5).bfloat16()
        dout = torch.randn(BATCH, Hm, Hm, C, device="cuda", generator=g).bfloat16()
        table = torch.randn((2 * WS - 1) ** 2, heads, device="cuda", generator=g) * 0.02
        dtable = torch.zeros_like(table)
        tok = BATCH * Hm * Hm
        cf, cb = (torch.empty(2, tok * C * n // 4, device="cuda", dtype=torch.int32) for n in (4, 7))
        arms = {"window fwd": lambda: nat.window_attention_fwd(qkv, table, heads, WS, sh),
                "window bwd": lambda: nat.window_attention_bwd(qkv, dout, table, dtable, heads, WS,
                                                               sh),
                "copy 8C": lambda: cf[1].copy_(cf[0]), "copy 14C": lambda: cb[1].copy_(cb[0])}
        with stock_allowed(True):
            arms.update(stock_arms(qkv, dout, table, heads, sh))
            t = time_arms(arms, a.calls, a.replays, a.rounds)
        say(f"  map {Hm} x {Hm}, C {C}, heads {heads}, shift {sh}: fwd moves {8 * C * tok / 1e6:.0f} "
            f"MB, bwd {14 * C * tok / 1e6:.0f} MB")
        for k, nbytes in (("window fwd", 8), ("copy 8C", 8), ("window bwd", 14), ("copy 14C", 14),
                          ("stock fwd", 8), ("stock fwd+bwd", 22)):
            us, spread, clk = t[k]
            c = "sclk n/a" if clk is None else f"sclk {clk:.0f} MHz"
            say(f"    {k:<16s} {us:9.1f} us  (spread {spread:6.1f})  "
                f"{nbytes * C * tok / us / 1e6:6.2f} TB/s of its minimum bytes  {c}")
        f, b = t["window fwd"][0], t["window bwd"][0]
        say(f"    fwd / copy 8C {f / t['copy 8C'][0]:.2f}   bwd / copy 14C {b / t['copy 14C'][0]:.2f}"
            f"   bwd / fwd {b / f:.2f}   window / stock: fwd {f / t['stock fwd'][0]:.3f}  fwd+bwd "
            f"{(f + b) / t['stock fwd+bwd'][0]:.3f}")
        total_us += depth * (f + b)

    if a.steps > 0:
        from distributed_ml_pytorch_amd.runtime.dist import DistInfo
        from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, Worker

        say(f"(b) swin_tiny, batch {BATCH}, ASGD, local PS: one captured training step")
        cfg = TrainConfig(model="swin_tiny", batch_size=BATCH, mode="asgd", ps="local", n_push=1000,
                          n_pull=1000, lr=0.01, evaluate=False, verbose=False)
        w = Worker(cfg, DistInfo(device=torch.device("cuda", 0)))
        g = torch.Generator().manual_seed(0)
        x, y = w.prepare(torch.randn(BATCH, *w.input_shape, generator=g),
                         torch.randint(0, w.num_classes, (BATCH,), generator=g))
        captured = w.enable_graph()
        for _ in range(4):
            w.train_step(x, y)
        ms = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.steps):
                w.train_step(x, y)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1) / a.steps)
        w.finish()
        say(f"    {min(ms):.2f} ms / step (graph {'on' if captured and w.graph is not None else 'OFF'}"
            f", min of 5 x {a.steps} steps, spread {max(ms) - min(ms):.2f}); window attention 12 x "
            f"(fwd + bwd) = {total_us / 1e3:.2f} ms from (a): {100 * total_us / 1e3 / min(ms):.1f} % "
            "of the step")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
