#!/usr/bin/env python
"""Headline benchmark: ResNet-18 Downpour/ASGD training throughput (samples/s, whole node).

BASELINE.json metric: "samples/sec (whole node) ResNet-18 ASGD at 1/2/4/8 MI355X".
Config: ResNet-18 (CIFAR stem, 11,173,962 params, random init), synthetic
CIFAR-10-shaped batches resident in HBM, bf16 compute / fp32 master params,
Downpour SGD with n_push = n_pull = 10 (reference defaults, main.py:146-147).

Topologies (``--ps``):

* ``local``   (N = 1 default): one worker with an in-process PS on the same GPU
  (push = PS apply kernel, pull = snapshot + land): every ASGD operation runs.
* ``sharded`` (N > 1 default): every rank is a worker and owns 1/N of the fp32
  master; push = reduce-scatter of the accumulated deltas + apply, pull =
  all-gather, both on a side HIP stream over RCCL/xGMI, landed with
  staleness <= 1 step.  Simultaneous pushes are AVERAGED by default at N > 1
  (``--delta-scale auto`` = ``mean``): summing them as a central Downpour PS adds
  every worker's delta (``--delta-scale sum``) multiplies the step by N, and at
  N = 8 with lr 0.05 the ResNet-18 time-to-target run collapsed to a uniform
  predictor (loss ln 10, profiles/ttl_n8_delta_scale_r2.txt).
  The collectives make it lock-step at pull time (bounded drift).
* ``sharded_async``: the same 1/N shards, each served by its own PS thread
  (parallel/async_sharded.py): gloo headers, point-to-point payloads on one
  2-rank group per direction (RCCL on GPUs, device-resident shards, every peer
  on its own link stream: parallel/links.py); no collective after start-up, so
  a late rank delays only its own shard's replies.  Its GPU test runs at world
  1 (no peer): the multi-rank link code is exercised by the CPU gloo tests.
* ``central``: the reference topology (/root/reference/Makefile:13-20,
  example/main.py:135-138): rank 0 is the parameter server (fp32 master on its
  GPU, payloads over one RCCL communicator per (PS, worker) pair, each pair on
  its own stream so transfers to different workers overlap, headers on a
  gloo control group), ranks 1..N-1 are workers; pushed deltas are averaged
  over the workers by default (``--delta-scale auto``; ``sum`` = the reference).  Whole-node samples/s counts
  the workers' samples only (the PS GPU trains nothing).

Per-GPU batch is fixed as N grows (weak scaling).

Launch: ``python bench.py --gpus N`` with N > 1 and no launcher environment
starts ``torch.distributed.run`` with N ranks as a CHILD process (this parent
never touches the GPU) and relays rank 0's line; under a launcher
(RANK/WORLD_SIZE set) ``--gpus`` must equal WORLD_SIZE.

Timing: W untimed warmup steps, then exactly K steps bracketed by barrier +
``torch.cuda.synchronize()`` on both sides; the max elapsed over ranks is used.
Rank 0 prints ONE JSON line.

A plain run (``--gpus N --steps K --warmup W``) does only what the headline
figure needs: set-up, warmup, the K timed steps, the line.  Everything else the
benchmark measures runs only with ``--full``: the K steps at the reference's
batch (``--ref-batch``), the time-to-target-loss runs (``--ttl-*``, ASGD and
the sync-DP comparison) and, at N > 1, the reference-topology check
(``--central-check``).  Without ``--full`` those options are ignored.

``--dump-outputs DIR`` writes what the last timed step returned to its caller
(``loss.npy``, ``hits.npy``) and the fp32 master parameters it left behind
(``params.npy``) as float32 arrays; a model above ``_DUMP_MAX_PARAMS`` elements
is sampled at fixed seeded indices (``params_index.npy``).  Weights and batches
are seeded, so two builds given the same arguments see identical inputs.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
# per-shape kernel picks measured offline on MI355X (ops/tuner.py), loaded as a
# READ-ONLY seed (a bench run never rewrites the committed file); set before the
# package is imported
os.environ.setdefault("DMP_CONV_TUNE_SEED", os.path.join(
    os.path.dirname(os.path.abspath(__file__)), "tuning", "mi355x_tune_cache.json"))

METRIC = "samples/sec (whole node) ResNet-18 ASGD at 1/2/4/8 MI355X; time-to-target-loss"


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--model", default="resnet18")
    ap.add_argument("--batch", type=int, default=512,
                    help="per-GPU batch (sweep: profiles/batch_sweep_r1.txt)")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline figure does not need: --ref-batch, the "
                         "time-to-target runs (--ttl-*) and the central check at N > 1; "
                         "without it those options are ignored")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write the last timed step's outputs (loss, "
                         "hits, fp32 master parameters) to DIR/<name>.npy as float32")
    ap.add_argument("--ref-batch", type=int, default=64,
                    help="with --full: also time K steps at the reference's default batch "
                         "(its example/main.py:142); 0 skips")
    ap.add_argument("--mode", default="asgd", choices=["asgd", "sync", "single"])
    ap.add_argument("--ps", default="auto", choices=["auto", "local", "sharded", "sharded_async", "central"])
    ap.add_argument("--delta-scale", default="auto",
                    help="PS push combine: 'sum' (Downpour PS), 'mean' over workers, or x; "
                         "'auto' = mean for the sharded PSs at N > 1 (their pushes are applied "
                         "together), sum for the central PS (the reference, applied one by one)")
    ap.add_argument("--wire-dtype", default="fp32", choices=["fp32", "bf16"],
                    help="push/pull payload dtype (master stays fp32; bf16 deltas are "
                         "reduced in fp32 by the sharded PS)")
    ap.add_argument("--n-push", type=int, default=10)
    ap.add_argument("--n-pull", type=int, default=10)
    ap.add_argument("--staleness", type=int, default=1)
    ap.add_argument("--lr", type=float, default=0.05)
    ap.add_argument("--momentum", type=float, default=0.0)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--bucket-mb", type=float, default=0.0,
                    help="sync mode all-reduce bucket (MB); 0 = measured on the group at start-up")
    ap.add_argument("--graph", type=int, default=1, help="capture fwd+bwd+update in a hipGraph")
    ap.add_argument("--profile-steps", type=int, default=0,
                    help="extra steps after timing, for rocprofv3 windows")
    ap.add_argument("--ttl-target", type=float, default=0.5,
                    help="with --full, after the throughput run: "
                         "train a FRESH model on learnable synthetic "
                         "data until the mean loss of 10 steps <= target and report the "
                         "wall time (the metric's time-to-target-loss half); 0 skips")
    ap.add_argument("--ttl-max-steps", type=int, default=4000)
    ap.add_argument("--ttl-signal", type=float, default=0.1,
                    help="class-template amplitude of the time-to-target images (0.1: ~540 "
                         "steps to training loss 0.5 and held-out accuracy 0.7 at ~650 steps at "
                         "N=1; at 0.05 the training loss fell by memorising the set while the "
                         "held-out accuracy stayed at 0.26: profiles/ttl_heldout_calibration_r4.txt)")
    ap.add_argument("--ttl-batches", type=int, default=128, help="distinct TTL batches (one dataset, all ranks)")
    ap.add_argument("--ttl-heldout-batches", type=int, default=8,
                    help="held-out split of the TTL data: same class templates, disjoint samples "
                         "(its own noise seed), evaluated through the no-grad native path every "
                         "--ttl-eval-every steps as the reference evaluates on its test set "
                         "(/root/reference/example/main.py:83-89,110-131); 0 skips")
    ap.add_argument("--ttl-eval-every", type=int, default=50)
    ap.add_argument("--ttl-plateau-steps", type=int, default=500,
                    help="once the training-loss target is reached, stop waiting for the held-out "
                         "accuracy target after this many steps without a new best held-out "
                         "accuracy (N > 1 on the shared 128-batch set plateaus below 0.7: "
                         "0.65 at N = 2 from step ~1600 to 4000); 0 = wait up to --ttl-max-steps")
    ap.add_argument("--ttl-heldout-acc", type=float, default=0.7,
                    help="held-out accuracy target: ttl_heldout_steps = first evaluation at or above it")
    ap.add_argument("--central-check", type=int, default=-1,
                    help="with --full, before the JSON line, at N>1: "
                         "STEPS of the reference topology (rank 0 "
                         "= PS, pushes / pulls over the per-pair payload communicators, RCCL on "
                         "GPUs) with a one-line report on stderr; -1 = 12 when the timed run "
                         "is not already central, 0 = off")
    ap.add_argument("--central-check-timeout", type=float, default=150.0,
                    help="seconds before a stuck central check ends every rank (exit 0: the "
                         "benchmark line is already out)")
    ap.add_argument("--ttl-compare-sync", type=int, default=1,
                    help="also measure time-to-target of sync all-reduce DP at the same N")
    a = ap.parse_args(argv)
    if not a.full:
        # a plain run times the headline steps only
        a.ref_batch, a.ttl_target, a.central_check = 0, 0.0, 0
    return a


# ----------------------------------------------------------------------- spawn
def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _spawn(a, argv) -> int:
    """Start N ranks under torch.distributed.run as a child process.  Nothing in
    this parent initialises the GPU (no torch.cuda call), so the children own it."""
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", "4")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.abspath(__file__), *argv]
    return subprocess.run(cmd, env=env).returncode


# -------------------------------------------------------------------- helpers
class _Ctx:
    """Groups and roles of one benchmark process."""

    def __init__(self, a, info):
        import torch.distributed as dist

        self.info = info
        self.world = info.world_size
        self.cpu_group = None
        self.worker_group = None
        self.ps_groups = None
        self.central = a.mode == "asgd" and a.ps == "central"
        if info.is_distributed:
            # host-side result exchange + stop decisions never ride on RCCL
            self.cpu_group = dist.new_group(backend="gloo") if info.backend != "gloo" else None
            if self.central:
                from distributed_ml_pytorch_amd.parallel.server import make_ps_groups

                payload = "rccl" if info.backend == "nccl" else "gloo"
                self.ps_groups = make_ps_groups(0, payload)
                self.worker_group = dist.new_group(list(range(1, self.world)))
        self.is_ps = self.central and info.rank == 0
        self.n_workers = self.world - 1 if self.central else self.world

    def worker_barrier(self):
        import torch.distributed as dist

        if not self.info.is_distributed:
            return
        if self.info.backend == "nccl":
            dist.barrier(group=self.worker_group, device_ids=[self.info.device.index])
        else:
            dist.barrier(group=self.worker_group)

    def host_reduce(self, vals, op="max"):
        """Element-wise MAX (or SUM) of a float list over every rank, on the CPU."""
        import torch
        import torch.distributed as dist

        t = torch.tensor(vals, dtype=torch.float64)
        if self.info.is_distributed:
            dist.all_reduce(t, op=dist.ReduceOp.MAX if op == "max" else dist.ReduceOp.SUM,
                            group=self.cpu_group)
        return t.tolist()

    def gather(self, obj):
        """Every rank's ``obj`` (host side), in rank order."""
        import torch.distributed as dist

        if not self.info.is_distributed:
            return [obj]
        out = [None] * self.world
        dist.all_gather_object(out, obj, group=self.cpu_group)
        return out

    def worker_mean(self, t):
        """Mean of a device scalar over the workers (a TTL stop decision)."""
        import torch.distributed as dist

        if self.info.is_distributed and self.n_workers > 1:
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.worker_group)
            t /= self.n_workers
        return t


def _sync():
    import torch

    if torch.cuda.is_available():
        torch.cuda.synchronize()


def _serve(a, cfg, ctx, sessions: int):
    """Rank 0 of the central topology: one PS run per worker session."""
    from distributed_ml_pytorch_amd.runtime.trainer import run_server

    stats = None
    for _ in range(sessions):
        st = run_server(cfg, ctx.info, ctx.ps_groups)
        stats = stats or st      # the throughput session's counts
    return stats


def _timed_steps(w, pool, steps, warmup, ctx, clock=None):
    """Returns (elapsed s, last loss, last hits); ``clock`` (utils.metrics.ClockSampler)
    samples sclk / power over exactly the timed window."""
    trace = os.environ.get("DMP_BENCH_LOSSES") == "1"
    seen = []
    for _ in range(warmup):
        x, y = pool.next()
        loss, _ = w.train_step(x, y)
        if trace:
            seen.append(loss)
    ctx.worker_barrier()
    _sync()
    w.timer.reset()
    if clock is not None:
        clock.start()
    t0 = time.perf_counter()
    for _ in range(steps):
        x, y = pool.next()
        loss, hits = w.train_step(x, y, keep=trace)   # untraced: only the last step's are read
        if trace:
            seen.append(loss)
    _sync()
    ctx.worker_barrier()
    elapsed = time.perf_counter() - t0
    if clock is not None:     # stopped outside the timed window
        w.clock_reading = clock.stop()
    if trace:
        print("[trace] losses " + " ".join(f"{float(v.float()):.3g}" for v in seen)
              + f" |p| {w.param_norm():.4f}", file=sys.stderr, flush=True)
    return elapsed, loss, hits


_DUMP_MAX_PARAMS = 12 * 2 ** 20     # 48 MB of float32: the whole dump stays under 64 MB


def _dump_outputs(path, w, loss, hits):
    """What the last timed step handed back (loss, hits) and the fp32 master
    parameters it left, as ``path/<name>.npy`` in float32.  A model with more than
    ``_DUMP_MAX_PARAMS`` parameters is sampled at fixed (seeded, sorted) indices,
    stored beside the sample as ``params_index.npy``."""
    import numpy as np
    import torch

    os.makedirs(path, exist_ok=True)
    flat = w.arena.p32.detach().reshape(-1)
    if flat.numel() > _DUMP_MAX_PARAMS:
        g = torch.Generator().manual_seed(0)
        idx = torch.randint(0, flat.numel(), (_DUMP_MAX_PARAMS // 4,), generator=g).sort().values
        np.save(os.path.join(path, "params_index.npy"), idx.numpy().astype(np.float64))
        flat = flat[idx.to(flat.device)]
    np.save(os.path.join(path, "params.npy"), flat.float().cpu().numpy())
    np.save(os.path.join(path, "loss.npy"), loss.detach().float().reshape(-1).cpu().numpy())
    np.save(os.path.join(path, "hits.npy"), hits.detach().float().reshape(-1).cpu().numpy())


def time_to_target(a, cfg, ctx, mode=None):
    """Wall time for a freshly initialised model (same engine, same config) to
    bring the mean training loss over 10 steps down to ``--ttl-target`` on
    class-template synthetic images (learnable, unlike the noise batches of the
    throughput run).  Includes graph capture and the first (tuning) step."""
    from dataclasses import replace

    import torch

    from distributed_ml_pytorch_amd.runtime.trainer import Worker
    from distributed_ml_pytorch_amd.utils.data import ttl_pools

    info = ctx.info
    cfg = replace(cfg, mode=mode or cfg.mode, seed=1000)
    torch.manual_seed(1000 + info.rank)
    w = Worker(cfg, info, ctx.ps_groups)
    w.enable_graph(bool(a.graph))
    # one fixed dataset of --ttl-batches batches for every N (seed shared by all
    # ranks), each worker starting at its own offset into it: with per-rank
    # datasets, N workers saw N x the distinct samples and the training loss fell
    # later simply because there was less to memorise (sync DP at N = 8 took
    # 2200 steps against 970 at N = 1 in the 8-rank rehearsal).  The held-out
    # split (same templates, disjoint samples) is what generalisation is scored on.
    pool, held = ttl_pools(a.batch, w.input_shape, w.num_classes, w.device, a.ttl_batches,
                           a.ttl_heldout_batches, dtype=w.compute_dtype, signal=a.ttl_signal)
    widx = info.rank - 1 if ctx.central else info.rank
    pool.i = (widx * a.ttl_batches // max(1, ctx.n_workers)) % a.ttl_batches
    if held is not None:
        # tune the no-grad kernels for the eval shapes before the clock starts
        w.evaluate(zip(held.x[:1], held.y[:1]))
    ctx.worker_barrier()
    _sync()
    t0 = time.perf_counter()
    steps, reached, window = 0, False, []
    t_train, train_steps = None, 0
    h_reached, h_steps, h_time, h_last = held is None, None, None, (None, None)
    h_best, h_best_step, plateau = -1.0, 0, False
    eval_s = 0.0
    while steps < a.ttl_max_steps:
        x, y = pool.next()
        loss, _ = w.train_step(x, y)
        window.append(loss.detach().float())
        steps += 1
        if steps % 10 == 0:
            # every worker takes the same stop decision, or the ones that keep
            # training would block in a push the others never join
            m = ctx.worker_mean(torch.stack(window).mean().reshape(1))
            window.clear()
            if steps % 200 == 0 and info.rank == 0:   # progress for long (multi-rank) runs
                print(f"[ttl] {mode or cfg.mode} step {steps} mean loss {float(m.item()):.4f}"
                      + (f" held-out loss {h_last[0]:.4f} acc {h_last[1]:.4f}"
                         if h_last[0] is not None else ""), file=sys.stderr, flush=True)
            if not reached and float(m.item()) <= a.ttl_target:
                reached = True
                _sync()
                # training time only: the held-out evaluations are reported apart
                t_train, train_steps = time.perf_counter() - t0 - eval_s, steps
        if held is not None and steps % a.ttl_eval_every == 0:
            # the reference's periodic test-set evaluation (main.py:83-89): the
            # native no-grad forward over the whole held-out split, BN in eval mode
            te = time.perf_counter()
            hl, ha = w.evaluate(zip(held.x, held.y))
            hv = ctx.worker_mean(torch.tensor([hl, ha], dtype=torch.float64,
                                              device=w.device)).tolist()
            h_last = (hv[0], hv[1])
            eval_s += time.perf_counter() - te
            if not h_reached and h_last[1] >= a.ttl_heldout_acc:
                # training time only, like time_to_target_s (evaluations excluded)
                h_reached, h_steps, h_time = True, steps, time.perf_counter() - t0 - eval_s
            if h_last[1] > h_best + 1e-3:
                h_best, h_best_step = h_last[1], steps
            # (worker-mean values: every rank takes the same decision)
            plateau = (reached and not h_reached and a.ttl_plateau_steps > 0
                       and steps - h_best_step >= a.ttl_plateau_steps)
        if reached and (h_reached or plateau):
            break
    _sync()
    t = time.perf_counter() - t0
    w.finish()
    out = {"time_to_target_s": round(t_train if reached else t, 3),
           "ttl_steps": train_steps if reached else steps, "ttl_reached": reached}
    if held is not None:
        out.update({"ttl_heldout_loss": None if h_last[0] is None else round(h_last[0], 4),
                    "ttl_heldout_acc": None if h_last[1] is None else round(h_last[1], 4),
                    "ttl_heldout_steps": h_steps, "ttl_heldout_reached": bool(h_reached),
                    "ttl_heldout_s": None if h_time is None else round(h_time, 3),
                    "ttl_heldout_best_acc": round(h_best, 4) if h_best >= 0 else None,
                    "ttl_heldout_plateau_stop": bool(plateau),
                    "ttl_eval_s": round(eval_s, 3)})
    return out


def _central_check(a, cfg, ctx, steps: int, line=None):
    """The reference's own topology (/root/reference/example/main.py:135-165: one
    PS process, every other rank a Downpour worker) run for ``steps`` worker steps
    after the timed runs: the (PS, worker) payload communicators -- RCCL pairs on
    GPUs -- carry real pushes and pulls, and rank 0 reports what moved.  Runs BEFORE rank 0 prints its line and returns the report that goes into
    it (``central_check``); a watchdog ends a stuck check: rank 0 prints the
    measured line with ``central_check.ok = false`` and every rank exits 3."""
    import threading
    from dataclasses import replace

    from distributed_ml_pytorch_amd.parallel.server import make_ps_groups
    from distributed_ml_pytorch_amd.runtime.dist import preflight
    from distributed_ml_pytorch_amd.runtime.trainer import Worker, run_server
    from distributed_ml_pytorch_amd.utils.data import DeviceBatchPool

    info = ctx.info

    def _expire():
        # a hang in the pair communicators or the PS loop is a FAILURE: rank 0
        # still prints the measured line (with the failed check in it), and every
        # rank exits non-zero
        print(f"[central-check] rank {info.rank}: no result after "
              f"{a.central_check_timeout:.0f} s, exiting", file=sys.stderr, flush=True)
        if info.rank == 0 and line is not None:
            line["central_check"] = {"ok": False, "timeout_s": a.central_check_timeout}
            print(json.dumps(line), flush=True)
        os._exit(3)

    dog = threading.Timer(a.central_check_timeout, _expire)
    dog.daemon = True
    dog.start()
    t0 = time.perf_counter()
    payload = "rccl" if info.backend == "nccl" else "gloo"
    groups = make_ps_groups(0, payload)
    pf = preflight(info, ctx.cpu_group, groups[1], 0)
    ccfg = replace(cfg, ps="central", delta_scale="sum", n_push=2, n_pull=2, seed=2000)
    mine = None
    if info.rank == 0:
        st = run_server(ccfg, info, groups)
        mine = {k: st[k] for k in ("version", "counts", "bytes_in", "bytes_out",
                                   "staleness_max") if k in st}
    else:
        w = Worker(ccfg, info, groups)
        w.enable_graph(bool(a.graph))
        pool = DeviceBatchPool(a.batch, w.input_shape, w.num_classes, w.device, n_batches=2,
                               dtype=w.compute_dtype, seed=info.rank + 50)
        t1 = time.perf_counter()
        for _ in range(steps):
            x, y = pool.next()
            loss, _ = w.train_step(x, y)
        lv = float(loss.float().item())
        ms = 1e3 * (time.perf_counter() - t1) / steps
        st = w.opt.client.stats() if hasattr(w.opt, "client") else {}
        mine = {"rank": info.rank, "ms_per_step": round(ms, 3), "loss": round(lv, 4),
                "hip_graph": bool(getattr(w, "use_graph", False) and w.graph is not None),
                "pushes": st.get("pushes"), "pulls": st.get("pulls")}
        w.finish()
        del w
    got = ctx.gather(mine)
    dog.cancel()
    if info.rank == 0:
        ps, workers = got[0], got[1:]
        ok = all(r is not None and r["loss"] == r["loss"] for r in workers) and \
            int(ps.get("version", 0)) > 0
        rep = {"ok": ok, "payload": payload, "steps": steps, "pairs_pinged": pf["pairs_pinged"],
               "rccl_ranks": pf["rccl_ranks"], "seconds": round(time.perf_counter() - t0, 2),
               "ps": ps, "workers": workers}
        print("[central-check] " + json.dumps(rep), file=sys.stderr, flush=True)
        return rep
    return None


def run(a):
    import torch

    from distributed_ml_pytorch_amd.runtime.dist import init_distributed, shutdown
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, Worker
    from distributed_ml_pytorch_amd.utils.data import DeviceBatchPool

    from distributed_ml_pytorch_amd.runtime.dist import apply_hw_queue_policy

    # every multi-rank topology (sharded workers, PS ranks, sync DP, and the
    # central check that follows the line) runs several HIP streams per process:
    # one queue policy for all of them, set before the first torch.cuda call
    hw_queues = apply_hw_queue_policy(int(os.environ.get("WORLD_SIZE", "1")))
    cuda = torch.cuda.is_available()
    info = init_distributed(use_cuda=cuda)
    world = info.world_size
    if a.mode == "asgd" and a.ps == "auto":
        a.ps = "sharded" if world > 1 else "local"
    if a.delta_scale == "auto":
        # the sharded PSs apply the W simultaneous pushes together ('sum' collapsed
        # the N=8 TTL run, profiles/ttl_n8_delta_scale_r2.txt); the central PS
        # applies each push as it arrives, as the reference's Downpour PS does
        a.delta_scale = "mean" if (a.mode == "asgd" and a.ps in ("sharded", "sharded_async")
                                   and world > 1) else "sum"
    if a.mode == "asgd" and a.ps == "local" and world > 1:
        raise SystemExit("--ps local is the 1-GPU in-process PS; with N > 1 use sharded/central")
    if a.mode == "asgd" and a.ps == "central" and world < 2:
        raise SystemExit("--ps central needs >= 2 ranks (rank 0 = PS, ranks 1.. = workers)")
    ctx = _Ctx(a, info)
    from distributed_ml_pytorch_amd.runtime.dist import preflight

    # observed, not configured: the ranks a collective reached, distinct devices,
    # every (PS, worker) payload communicator answering (raises on a mismatch)
    pf = preflight(info, ctx.cpu_group, ctx.ps_groups[1] if ctx.ps_groups else None, 0)
    cfg = TrainConfig(model=a.model, batch_size=a.batch, lr=a.lr, momentum=a.momentum,
                      n_push=a.n_push, n_pull=a.n_pull, staleness=a.staleness, mode=a.mode,
                      ps=a.ps if a.mode == "asgd" else "local", dtype=a.dtype, cuda=True,
                      evaluate=False, verbose=False, bucket_mb=a.bucket_mb,
                      delta_scale=a.delta_scale, payload="auto", wire_dtype=a.wire_dtype)
    res = {}
    ps_stats = None
    if ctx.is_ps:
        ps_stats = _serve(a, cfg, ctx, 2 if a.ttl_target > 0 else 1)
        elapsed = ref_elapsed = 0.0
        final_loss = 0.0
        graphed = False
        in_shape = None
        dev_name = str(info.device)
    else:
        w = Worker(cfg, info, ctx.ps_groups)
        graphed = w.enable_graph(bool(a.graph))
        pool = DeviceBatchPool(a.batch, w.input_shape, w.num_classes, w.device, n_batches=4,
                               dtype=w.compute_dtype, seed=info.rank)
        from distributed_ml_pytorch_amd.utils.metrics import ClockSampler

        clock = ClockSampler(w.device.index or 0) if w.device.type == "cuda" else None
        elapsed, loss, hits = _timed_steps(w, pool, a.steps, a.warmup, ctx, clock)
        if a.dump_outputs and info.rank == (1 if ctx.central else 0):
            _dump_outputs(a.dump_outputs, w, loss, hits)     # the first worker's
        res["gpu_clock"] = getattr(w, "clock_reading", None)
        final_loss = float(loss.float().item())
        graphed = bool(getattr(w, "use_graph", False) and w.graph is not None)
        res["phases_host_ms"] = {k: v["mean_ms"] for k, v in w.timer.summary().items()}
        for _ in range(a.profile_steps):
            x, y = pool.next()
            w.train_step(x, y)
        ref_elapsed = 0.0
        if a.ref_batch:
            pool64 = DeviceBatchPool(a.ref_batch, w.input_shape, w.num_classes, w.device,
                                     n_batches=4, dtype=w.compute_dtype, seed=info.rank + 7)
            ref_elapsed, _, _ = _timed_steps(w, pool64, a.steps, max(a.warmup, 3), ctx)
        _sync()
        in_shape = tuple(w.input_shape)
        dev_name = str(w.device)
        if hasattr(w.opt, "client"):
            res["comm"] = {k: v for k, v in w.opt.client.stats().items() if "device_ms" in k}
        if w.ddp is not None:
            # the all-reduce bucket this node measured for itself (parallel/ddp.py)
            res["bucket"] = {"bucket_mb": w.ddp.bucket_mb, "buckets": w.ddp.num_buckets,
                             "calibration_mb_ms_busbw": w.ddp.calibration}
        w.finish()
        del w
    ttl = ttl_sync = None
    if a.ttl_target > 0:
        ttl = time_to_target(a, cfg, ctx) if not ctx.is_ps else None
        if a.ttl_compare_sync and not ctx.central and a.mode == "asgd":
            ttl_sync = time_to_target(a, cfg, ctx, mode="sync")
    # -------- reduce over ranks (host side; the PS contributes zeros) --------
    ttl_vals = [ttl["time_to_target_s"], ttl["ttl_steps"], float(ttl["ttl_reached"])] \
        if ttl else [0.0, 0.0, 0.0]
    # held-out fields are already worker means (identical on every worker); the
    # MAX brings them to rank 0 (the PS contributes -1 = "not a worker")
    held_keys = ("ttl_heldout_loss", "ttl_heldout_acc", "ttl_heldout_steps",
                 "ttl_heldout_reached", "ttl_heldout_s", "ttl_eval_s", "ttl_heldout_best_acc",
                 "ttl_heldout_plateau_stop")
    held_vals = [-1.0 if not ttl or ttl.get(k) is None else float(ttl[k]) for k in held_keys]
    red = ctx.host_reduce([elapsed, -elapsed if elapsed else -1e30, ref_elapsed, final_loss,
                           *ttl_vals, *held_vals])
    elapsed, min_elapsed, ref_elapsed, final_loss = red[0], -red[1], red[2], red[3]
    if ttl is not None or ctx.is_ps:
        ttl = {"time_to_target_s": round(red[4], 3), "ttl_steps": int(red[5]),
               "ttl_reached": bool(red[6])} if a.ttl_target > 0 else None
        if ttl is not None and a.ttl_heldout_batches > 0:
            hv = dict(zip(held_keys, red[7:7 + len(held_keys)]))
            ttl.update({
                "ttl_heldout_loss": None if hv["ttl_heldout_loss"] < 0 else round(hv["ttl_heldout_loss"], 4),
                "ttl_heldout_acc": None if hv["ttl_heldout_acc"] < 0 else round(hv["ttl_heldout_acc"], 4),
                "ttl_heldout_steps": None if hv["ttl_heldout_steps"] < 0 else int(hv["ttl_heldout_steps"]),
                "ttl_heldout_reached": hv["ttl_heldout_reached"] > 0,
                "ttl_heldout_s": None if hv["ttl_heldout_s"] < 0 else round(hv["ttl_heldout_s"], 3),
                "ttl_eval_s": max(0.0, round(hv["ttl_eval_s"], 3)),
                "ttl_heldout_best_acc": (None if hv["ttl_heldout_best_acc"] < 0
                                         else round(hv["ttl_heldout_best_acc"], 4)),
                "ttl_heldout_plateau_stop": hv["ttl_heldout_plateau_stop"] > 0,
                "ttl_heldout_target_acc": a.ttl_heldout_acc})
    if ctx.is_ps:
        shape_src = ctx.host_reduce([0.0, 0.0, 0.0])      # matched by workers below
    else:
        shape_src = ctx.host_reduce(list(map(float, in_shape)))
    in_shape = tuple(int(v) for v in shape_src)
    # per-rank worker facts (graph capture, host phases, device comm spans) gathered
    # onto rank 0: in the central topology rank 0 is the PS and trains nothing
    mine = None if ctx.is_ps else {"rank": info.rank, "hip_graph": bool(graphed),
                                   "bucket": res.get("bucket"),
                                   "phases_host_ms": res.get("phases_host_ms"),
                                   "comm": res.get("comm"), "gpu_clock": res.get("gpu_clock")}
    ranks = ctx.gather(mine)
    out = None
    if info.rank == 0:
        nw = ctx.n_workers
        global_batch = a.batch * nw
        value = global_batch * a.steps / elapsed
        par = {"asgd": f"asgd-{a.ps}-ps x{world}", "sync": f"dp{world}",
               "single": "single"}[a.mode]
        if ctx.central:
            par = f"asgd-central-ps 1ps+{nw}w"
        on_gpu = cuda
        workers = [r for r in ranks if r is not None]
        graphed = bool(workers) and all(r["hip_graph"] for r in workers)
        out = {
            "metric": METRIC,
            "value": round(value, 2),
            "unit": "samples/s",
            "n_gpus": world,
            "steps": a.steps,
            "warmup": a.warmup,
            "ms_per_step": round(1e3 * elapsed / a.steps, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": a.dtype if on_gpu else "fp32 (CPU run: no bf16 compute)",
            "data": ("synthetic ({} images, random labels, {}); random-init weights".format(
                "x".join(map(str, in_shape)), "HBM-resident" if on_gpu else "host memory")),
            "config": {"model": (f"{a.model} ({'CIFAR' if in_shape[-1] <= 64 else 'ImageNet'} stem)"
                                 if a.model.startswith("resnet") else a.model),
                       "global_batch": global_batch, "per_gpu_batch": a.batch,
                       "seq_len": None, "image": "x".join(map(str, in_shape)),
                       "parallelism": par, "n_push": a.n_push, "n_pull": a.n_pull,
                       "staleness": a.staleness, "lr": a.lr,
                       "push_combine": a.delta_scale,
                       "hip_graph": bool(graphed), "master_dtype": "fp32",
                       "wire_dtype": a.wire_dtype},
            "world_size": world,
            "backend": info.backend,
            "rccl_ranks": pf["rccl_ranks"],
            "preflight": {k: pf[k] for k in ("ranks_observed", "devices_distinct",
                                             "pairs_pinged") if k in pf},
            "workers": nw,
            "device": dev_name if on_gpu else "cpu",
            "ms_per_step_fastest_rank": round(1e3 * min_elapsed / a.steps, 4),
            "final_loss": round(final_loss, 4),
        }
        # host phases / comm spans of the first WORKER (rank 0, or rank 1 when
        # rank 0 is the central PS), plus the per-worker graph flags
        first = workers[0] if workers else {}
        if first.get("phases_host_ms"):
            out["phases_host_ms"] = first["phases_host_ms"]
        if first.get("bucket"):
            out["sync_dp_bucket"] = first["bucket"]
        if first.get("comm"):
            out["comm_first_worker"] = first["comm"]
            out["comm_first_worker_rank"] = first["rank"]
        # sclk / socket power sampled over the timed window (amdsmi), so box
        # variance shows up beside the number; None where amdsmi is unavailable
        out["gpu_clock_timed_window"] = first.get("gpu_clock")
        out["gpu_max_hw_queues"] = hw_queues
        if len(workers) > 1:
            clocks = [r["gpu_clock"]["sclk_mhz_mean"] for r in workers if r.get("gpu_clock")]
            if clocks:
                out["sclk_mhz_mean_min_over_workers"] = min(clocks)
            out["worker_hip_graph"] = [bool(r["hip_graph"]) for r in workers]
        if a.ref_batch and ref_elapsed > 0:
            out["reference_batch"] = {
                "per_gpu_batch": a.ref_batch, "global_batch": a.ref_batch * nw,
                "ms_per_step": round(1e3 * ref_elapsed / a.steps, 4),
                "value": round(a.ref_batch * nw * a.steps / ref_elapsed, 2)}
        if ps_stats:
            out["ps"] = {k: ps_stats[k] for k in ("version", "counts", "staleness_mean",
                                                  "staleness_max", "bytes_in", "bytes_out")
                         if k in ps_stats}
        if ttl is not None:
            out.update(ttl)
            out.update({"ttl_target_loss": a.ttl_target,
                        "ttl_data": f"synthetic class-template images (signal {a.ttl_signal} "
                                    f"+ N(0,1) noise), one dataset of {a.ttl_batches} "
                                    "batches shared by all workers (per-worker offsets); "
                                    f"held-out split of {a.ttl_heldout_batches} batches from the "
                                    "same templates with disjoint samples, evaluated every "
                                    f"{a.ttl_eval_every} steps"})
        if ttl_sync is not None:
            out["ttl_sync_dp"] = ttl_sync
    steps = a.central_check if a.central_check >= 0 else (12 if not ctx.central else 0)
    check_ok = True
    if steps > 0 and world > 1 and a.mode == "asgd":
        rep = _central_check(a, cfg, ctx, steps, out)
        if info.rank == 0:
            out["central_check"] = rep
            check_ok = bool(rep and rep["ok"])
    if info.rank == 0:
        print(json.dumps(out), flush=True)
    shutdown()
    if not check_ok:
        sys.exit(3)          # the line is out, but the reference-topology check failed
    shutdown()


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    a = parse(argv)
    launched = "RANK" in os.environ and "WORLD_SIZE" in os.environ
    if not launched and a.gpus > 1:
        sys.exit(_spawn(a, argv))
    if launched and int(os.environ["WORLD_SIZE"]) != a.gpus:
        raise SystemExit(f"bench.py --gpus {a.gpus} but the launcher started "
                         f"WORLD_SIZE={os.environ['WORLD_SIZE']} ranks")
    run(a)


if __name__ == "__main__":
    main()
