"""Training driver: the reference's ``example/main.py`` loop as a reusable engine.

Roles and loop follow /root/reference/example/main.py:31-138 (rank 0 = PS in
the central topology, workers train with ``Asynchronous``; ``--no-distributed``
= plain SGD), plus the modes BASELINE.json asks for:

* ``mode="asgd"``   Downpour SGD; ``ps`` = ``central`` (reference star,
  gloo or RCCL payloads), ``sharded`` (PS co-located on every GPU, collective
  push/pull), ``sharded_async`` (one PS thread per shard, point-to-point
  push/pull, no rank waits for another: parallel/async_sharded.py) or
  ``local`` (in-process PS, 1 device);
* ``mode="sync"``   bucketed all-reduce data parallel;
* ``mode="single"`` plain SGD, no communication.

Per step: zero the flat grad arena (one memset) -> bf16 channels-last forward
through the native layers -> fused softmax-xent -> backward (native kernels
write fp32 weight grads straight into the arena) -> [bucket sync] -> fused
optimizer kernel (+ push/pull).  No host sync per step: the loss is kept on
device and only read at log points.
"""
from __future__ import annotations

import logging
import math
import os
import time
from dataclasses import asdict, dataclass, field

import torch
import torch.distributed as dist

from ..models import build_model, is_vit
from ..ops.eval_fold import fold_session
from ..ops.functional import softmax_cross_entropy, softmax_cross_entropy_mix, unit_grad
from ..parallel.arena import attach_arena
from ..parallel.asgd import Asynchronous
from ..parallel.async_sharded import AsyncShardedPSClient
from ..parallel.clients import (MX8_FLAVOURS, GlooPSClient, LocalPSClient, RcclPSClient,
                                ShardedPSClient, SharedPSClient, check_push_wire)
from ..parallel.ddp import BucketedAllReduce, FusedAdamW, FusedSGD
from ..parallel.fused_optim import Schedule, check_ema_options
from ..parallel.server import ParameterServer, make_ps_groups
from ..parallel.staleness import check_policy
from ..utils import checkpoint as ckpt
from ..utils.data import get_datasets, make_loaders
from ..utils.device_data import (AUGMENTS, MAX_PAD, DeviceLoader, MixConfig, check_mix_config,
                                 get_device_datasets)
from ..utils.metrics import IterationLog, StepTimer, Throughput, classification_report
from .determinism import enable_determinism
from .dist import DistInfo, preflight

_LOG = logging.getLogger(__name__)


class DivergenceError(RuntimeError):
    """Training produced non-finite parameters (the log-interval watchdog)."""


@dataclass
class TrainConfig:
    model: str = "alexnet"
    num_classes: int | None = None
    dataset: str = "synthetic"
    data_dir: str = "./data"
    n_train: int = 50000
    n_test: int = 10000
    batch_size: int = 64
    test_batch_size: int = 10000
    epochs: int = 20
    max_steps: int | None = None
    lr: float = 0.008
    momentum: float = 0.0
    weight_decay: float = 0.0
    lr_schedule: str = "constant"     # "inv_epoch": the reference's LambdaLR(1/(epoch+1)), per
                                      # epoch on the host; "warmup_cosine": per step on the device
    optimizer: str = "sgd"            # sgd | adamw (parallel/fused_optim.py)
    beta1: float = 0.9
    beta2: float = 0.999
    adam_eps: float = 1e-8
    clip_grad_norm: float = 0.0       # global-norm gradient clipping; 0 = off
    warmup_steps: int = 0             # warmup_cosine: linear warm-up updates
    lr_min: float = 0.0               # warmup_cosine: floor reached at schedule_steps
    schedule_steps: int | None = None  # warmup_cosine length; None: max_steps, else all epochs
    n_push: int = 10
    n_pull: int = 10
    staleness: int = 1
    pull_mode: str = "overwrite"
    wire_dtype: str = "fp32"
    push_wire: str = "same"           # same | mx8 (parallel/wire8.py) | topk (wire_topk.py);
                                      # mx8 and topk: local and central PS only
    push_topk: int = 8                # K of push_wire topk: entries per 256-element block, 1..32
    mode: str = "asgd"                # asgd | sync | single
    ps: str = "central"               # central | sharded | sharded_async | local
    payload: str = "auto"             # central PS payload transport: gloo | rccl | auto
    dtype: str = "bf16"               # compute dtype on GPU (CPU always fp32)
    cuda: bool = True
    log_interval: int = 100
    evaluate: bool = True
    seed: int = 0
    log_dir: str = "log"
    checkpoint: str | None = None
    checkpoint_every: int = 0
    resume: str | None = None         # base path: workers read <base>.worker<rank>.pt, the PS <base>
    ps_resume: str | None = None      # explicit PS checkpoint (overrides <base> for the PS)
    delta_scale: str = "sum"          # PS push combine: "sum" (Downpour PS semantics) | "mean" | float
    ps_worker_timeout: float = 0.0    # central PS: drop a worker silent this long (0 = never)
    stale_bound: int = 0              # S of the version-based staleness bound (parallel/staleness.py)
    stale_policy: str = "off"         # off | damp | block (central and sharded_async PS only)
    delay_comp: float = 0.0           # lambda of delay compensation (DC-ASGD); 0 = off
    bucket_mb: float = 0.0            # sync-DP all-reduce bucket; <= 0: measured (ddp.py)
    label_smoothing: float = 0.0
    divergence_check: bool = True     # halt on non-finite parameters at each log interval
    deterministic: bool = False       # bitwise-reproducible debug mode (runtime/determinism.py)
    device_data: bool = False         # dataset resident on the device as uint8, batches assembled
                                      # by one native kernel per step (utils/device_data.py)
    augment: str = "none"             # none | crop | flip | crop_flip (device_data only)
    crop_pad: int = 4                 # zero padding of the random crop
    mixup: float = 0.0                # Mixup alpha, 0 = off (device_data only)
    cutmix: float = 0.0               # CutMix alpha, 0 = off (device_data only)
    mix_prob: float = 1.0             # probability that a batch is mixed at all
    mix_switch_prob: float = 0.5      # with both on: probability of CutMix over Mixup
    drop_path: float = 0.0            # stochastic depth rate of the last ViT block; 0 = off
    model_ema: float = 0.0            # decay of the model EMA (parallel/ema.py); 0 = off
    model_ema_every: int = 1          # EMA update every K optimizer steps
    model_ema_warmup: bool = False    # decay min(d, (1 + u) / (10 + u)) at EMA update u
    verbose: bool = True
    extra: dict = field(default_factory=dict)


def _dtype(name: str) -> torch.dtype:
    return {"bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "fp32": torch.float32,
            "float32": torch.float32, "fp16": torch.float16}[name]


class Worker:
    """One training process: model + arena + optimizer + step function."""

    def __init__(self, cfg: TrainConfig, info: DistInfo, ps_groups=None, client=None):
        """``client``: an explicit PS client for ``mode='asgd'`` (e.g. a
        :class:`~..parallel.clients.SharedPSClient` of the virtual-worker runner)."""
        self.cfg = cfg
        self.info = info
        check_stale_config(cfg, info)
        check_push_wire_config(cfg, client)
        check_delay_comp_config(cfg, info, client)
        check_device_data_config(cfg, info)
        check_drop_path_config(cfg)
        check_model_ema_config(cfg)
        if cfg.deterministic:
            cfg = self.cfg = enable_determinism(cfg)
        torch.manual_seed(cfg.seed + info.rank)
        self.device = info.device if (cfg.cuda and info.device.type == "cuda") else \
            torch.device("cpu")
        self.compute_dtype = _dtype(cfg.dtype) if self.device.type == "cuda" else torch.float32
        if self.device.type == "cuda" and self.compute_dtype != torch.bfloat16:
            from ..ops._policy import is_allowed

            if not is_allowed():
                # the native kernels are bf16-compute (fp32 masters / accumulation);
                # an fp32 GPU run would train entirely on MIOpen / hipBLASLt / ATen
                raise ValueError(
                    f"--dtype {cfg.dtype} on the GPU: every native gfx950 kernel computes "
                    "in bf16 (fp32 master weights and accumulation), so this would train "
                    "entirely on stock MIOpen / hipBLASLt / ATen kernels.  Use --dtype bf16, "
                    "or --deterministic for the explicit fp32 stock-kernel oracle mode.")
        # (the model draws its drop-path seed from torch's generator, seeded per rank above)
        model, shape, nc = build_model(cfg.model, cfg.num_classes, drop_path=cfg.drop_path)
        self.input_shape, self.num_classes = shape, nc
        self.model = model.to(self.device)
        shadow = self.compute_dtype if self.compute_dtype != torch.float32 else None
        self.arena = attach_arena(self.model, shadow_dtype=shadow,
                                  channels_last=True)
        self.ddp = None
        self.timer = StepTimer()
        self.step_idx = 0
        # resume the parameters BEFORE the optimizer exists: its PS client seeds the
        # master (local / sharded) or the central PS from the live parameters
        resume = _worker_resume_path(cfg.resume, info.rank) if cfg.resume else None
        if cfg.resume and info.is_distributed and not (cfg.mode == "asgd" and cfg.ps == "central"):
            # every rank of a collective topology must take the same decision: the
            # sharded clients restore through a collective, so one rank starting
            # fresh while the others resume would hang them (central-PS workers
            # resume independently: a fresh one adopts the PS params at its pull)
            _agree_on_resume(resume is not None, info)
        if resume:
            self.step_idx = ckpt.load_worker_model(resume, self.model)
        params = list(self.model.parameters())
        if cfg.lr_schedule not in ("constant", "inv_epoch", "warmup_cosine"):
            raise ValueError(f"unknown lr_schedule {cfg.lr_schedule!r}")
        if cfg.optimizer not in ("sgd", "adamw"):
            raise ValueError(f"unknown optimizer {cfg.optimizer!r}; 'sgd' or 'adamw'")
        # extra optimizer arguments: empty with the defaults, so the plain SGD
        # constructors (and their by-value kernel) are reached exactly as before
        okw = {}
        if cfg.clip_grad_norm > 0:
            okw["max_grad_norm"] = cfg.clip_grad_norm
        if cfg.lr_schedule == "warmup_cosine":
            total = cfg.schedule_steps or cfg.max_steps or \
                cfg.epochs * max(1, cfg.n_train // cfg.batch_size)
            okw["schedule"] = Schedule("warmup_cosine", cfg.warmup_steps, total, cfg.lr_min)
        sgd_kw = {}
        if cfg.model_ema > 0:
            okw.update(ema_decay=cfg.model_ema, ema_every=cfg.model_ema_every,
                       ema_warmup=cfg.model_ema_warmup)
            sgd_kw["model"] = self.model       # FusedSGD: the buffers that are averaged
        adam = dict(betas=(cfg.beta1, cfg.beta2), eps=cfg.adam_eps)
        if cfg.mode == "asgd":
            client = client if client is not None else self._make_client(ps_groups)
            if cfg.optimizer == "adamw":
                okw.update(optimizer="adamw", **adam)
            if cfg.push_wire != "same":      # an explicit client takes the configured wire too
                okw["push_wire"] = cfg.push_wire
                okw["push_topk"] = cfg.push_topk
            self.opt = Asynchronous(params, lr=cfg.lr, n_push=cfg.n_push, n_pull=cfg.n_pull,
                                    model=self.model, client=client, momentum=cfg.momentum,
                                    weight_decay=cfg.weight_decay, **okw)
        elif cfg.mode == "sync":
            world = dist.get_world_size() if info.is_distributed else 1
            if info.is_distributed:
                dist.broadcast(self.arena.p32, 0)
                self.arena.refresh_shadow()
            self.ddp = BucketedAllReduce(self.arena, bucket_mb=cfg.bucket_mb)
            if cfg.optimizer == "adamw":
                self.opt = FusedAdamW(params, self.arena, cfg.lr, weight_decay=cfg.weight_decay,
                                      grad_scale=1.0 / world, model=self.model, **adam, **okw)
            else:
                self.opt = FusedSGD(params, self.arena, cfg.lr, cfg.momentum,
                                    weight_decay=cfg.weight_decay, grad_scale=1.0 / world, **okw,
                                    **sgd_kw)
        elif cfg.mode == "single":
            if cfg.optimizer == "adamw":
                self.opt = FusedAdamW(params, self.arena, cfg.lr, weight_decay=cfg.weight_decay,
                                      model=self.model, **adam, **okw)
            else:
                self.opt = FusedSGD(params, self.arena, cfg.lr, cfg.momentum,
                                    weight_decay=cfg.weight_decay, **okw, **sgd_kw)
        else:
            raise ValueError(f"unknown mode {cfg.mode!r}")
        if isinstance(self.opt, Asynchronous):
            self.opt.timer = self.timer
        if resume:
            ckpt.load_worker_optimizer(resume, self.opt)

    def _make_client(self, ps_groups):
        cfg, info = self.cfg, self.info
        kw = dict(staleness=cfg.staleness, pull_mode=cfg.pull_mode,
                  wire_dtype=_dtype(cfg.wire_dtype), push_wire=cfg.push_wire,
                  push_topk=cfg.push_topk)
        if cfg.ps == "local" or not info.is_distributed:
            return LocalPSClient(**kw)
        if cfg.ps == "sharded":
            return ShardedPSClient(delta_scale=cfg.delta_scale, **kw)
        if cfg.ps == "sharded_async":
            return AsyncShardedPSClient(delta_scale=cfg.delta_scale,
                                        stale_bound=cfg.stale_bound,
                                        stale_policy=cfg.stale_policy, **kw)
        if cfg.ps == "central":
            ctrl, pairs = ps_groups if ps_groups is not None else (None, {})
            if pairs and self.device.type == "cuda" and _payload(cfg, info) == "rccl":
                return RcclPSClient(0, ctrl, pairs[info.rank], **kw)
            return GlooPSClient(ps_rank=0, group=ctrl, **kw)
        raise ValueError(f"unknown ps kind {cfg.ps!r}")

    # --------------------------------------------------------------- stepping
    def prepare(self, x, y):
        x = x.to(self.device, non_blocking=True)
        if self.device.type == "cuda":
            x = x.to(self.compute_dtype)
            if x.dim() == 4:
                x = x.contiguous(memory_format=torch.channels_last)
        return x, y.to(self.device, non_blocking=True)

    # ------------------------------------------------------------ hipGraph path
    def enable_graph(self, enabled: bool = True):
        """Replay forward+backward+fused update as ONE captured hipGraph per step.

        The push/pull/land half of the ASGD step (which depends on the step
        index) stays eager between replays.  Sync DP is captured whole: the
        bucket all-reduces that the grad-ready hooks launch during backward
        (RCCL on the comm stream, ordered by events) and the wait before the
        update are part of the graph.  Gloo collectives cannot be captured:
        sync DP over gloo stays eager.
        """
        can = self.device.type == "cuda"
        if self.ddp is not None and self.info.is_distributed:
            # gloo collectives cannot be captured; RCCL ones can, OPT-IN
            # (DMP_GRAPH_SYNC=1): eager sync DP pays the host launch of every
            # dispatch (~350 per ResNet-50 step, profiles/sync_dp_capture_ab_r4.txt),
            # but that A/B ran at world 1 and a captured multi-rank all-reduce has
            # not been replayed on a multi-GPU node yet, so multi-rank sync DP
            # steps eagerly by default.  With capture on, a capture that fails on
            # ANY rank makes every rank step eagerly (_capture_agreed).
            can = can and self.info.backend == "nccl" and \
                os.environ.get("DMP_GRAPH_SYNC", "0") == "1"
        self.use_graph = bool(enabled) and can
        self.graph = None
        return self.use_graph

    @property
    def mixes(self) -> bool:
        """Whether the training batches carry two targets (Mixup / CutMix)."""
        return self.cfg.mixup > 0 or self.cfg.cutmix > 0

    def _need_mix(self, mix):
        if mix is None:
            raise ValueError("this run mixes (--mixup / --cutmix): train_step needs "
                             "mix=(y2, lam) of the batch")
        return mix

    def _loss(self, logits, y, mix):
        if not self.mixes:
            return softmax_cross_entropy(logits, y, self.cfg.label_smoothing)
        y2, lam = self._need_mix(mix)
        return softmax_cross_entropy_mix(logits, y, y2, lam, self.cfg.label_smoothing)

    def _graph_body(self):
        self.opt.zero_grad()
        logits = self.model(self._gx)
        loss, hits = self._loss(logits, self._gy, (self._gy2, self._glam))
        loss.backward(unit_grad(loss))
        if self.ddp is not None:
            self.ddp.synchronize()
        self.opt.local_step()
        return loss.detach(), hits

    def _capture(self, x, y, mix=None):
        """Run this step eagerly on a side stream (tunes kernels, warms the
        allocator and libraries), then capture the step body for later replays."""
        self._gx = x.detach().clone()
        self._gy = y.detach().clone()
        self._gy2 = self._glam = None
        if self.mixes:
            y2, lam = self._need_mix(mix)
            self._gy2, self._glam = y2.detach().clone(), lam.detach().clone()
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            loss, hits = self._graph_body()
            self.opt.comm_step()
            self.step_idx += 1
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        err = None
        try:
            # thread_local: RCCL's watchdog thread queries events while we capture
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self._gloss, self._ghits = self._graph_body()
        except RuntimeError as e:     # e.g. a collective backend that cannot be captured
            err = str(e)
            if self.ddp is not None:
                self.ddp.reset()
        # sync DP: every rank replays or every rank steps eagerly -- a rank whose
        # capture failed must not run a different launch path from its peers
        # (capture records the collectives, it does not run them, so this
        # agreement all-reduce is the first collective after the eager step)
        if self.ddp is not None and self.info.is_distributed and \
                not self._capture_agreed(err is None):
            err = err or "a peer rank's capture failed"
            self.ddp.reset()
        if err is not None:
            print(f"[trainer] hipGraph capture failed ({err}); stepping eagerly", flush=True)
            self.use_graph = False
            self.graph = None
            return loss.clone(), hits.clone()
        self.graph = g
        self._graph_key = self._make_graph_key(x)
        return loss.clone(), hits.clone()

    def _make_graph_key(self, x):
        """A by-value lr is baked into the captured update kernel, so it keys the
        graph; with the device-resident hyper block (``opt.core``) the kernels
        read lr from memory and the graph survives any learning rate."""
        lr = None if getattr(self.opt, "core", None) is not None else \
            self.opt.param_groups[0]["lr"]
        return (tuple(x.shape), x.dtype, lr)

    def _capture_agreed(self, ok: bool) -> bool:
        """MIN-all-reduce of the local capture verdict over the sync-DP group."""
        import torch.distributed as dist

        flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=self.device)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN, group=self.ddp.group)
        return bool(flag.item())

    def static_inputs(self):
        """The captured step's own input buffers ``(x, y)``, or ``None`` while no
        graph is captured.  A batch written into them (utils/device_data.py) and
        handed to :meth:`train_step` as these very tensors is replayed in place,
        with no copy."""
        if getattr(self, "use_graph", False) and self.graph is not None:
            return self._gx, self._gy
        return None

    def static_mix_inputs(self):
        """The captured step's own ``(y2, lam)`` buffers of a mixing run, next to
        :meth:`static_inputs`; ``None`` while no graph is captured or without mixing."""
        if getattr(self, "use_graph", False) and self.graph is not None and self.mixes:
            return self._gy2, self._glam
        return None

    def static_batch_buffers(self):
        """What a :class:`DeviceLoader` writes the next batch into: ``(x, y)``, or
        ``(x, y, y2, lam)`` in a mixing run; ``None`` while no graph is captured."""
        xy = self.static_inputs()
        if xy is None or not self.mixes:
            return xy
        return (*xy, *self.static_mix_inputs())

    def _graph_step(self, x, y, keep: bool = True, mix=None):
        key = self._make_graph_key(x)
        if self.graph is None or key != self._graph_key:
            return self._capture(x, y, mix)
        with self.timer.time("compute_launch"):
            if x is not self._gx:
                self._gx.copy_(x, non_blocking=True)
            if y is not self._gy:
                self._gy.copy_(y, non_blocking=True)
            if self.mixes:
                y2, lam = self._need_mix(mix)
                if y2 is not self._gy2:
                    self._gy2.copy_(y2, non_blocking=True)
                if lam is not self._glam:
                    self._glam.copy_(lam, non_blocking=True)
            self.graph.replay()
        self.opt.comm_step()
        self.step_idx += 1
        # the captured outputs are overwritten by the next replay: copies unless
        # the caller reads them before the next step (``keep=False``)
        if not keep:
            return self._gloss, self._ghits
        return self._gloss.clone(), self._ghits.clone()

    def param_norm(self) -> float:
        """L2 norm of the flat fp32 master parameters: one native reduction over
        the arena on GPU (csrc/optim.hip sumsq_partial_kernel), the divergence
        watchdog's probe -- a NaN / inf anywhere in the model shows up here."""
        flat = self.arena.p32
        if flat.is_cuda:
            from ..ops._ext import native

            return math.sqrt(float(native().sumsq(flat)))
        return float(flat.double().norm())

    def train_step(self, x, y, keep: bool = True, mix=None):
        """One fwd+bwd+update. Returns (loss, hits) as device tensors (no sync).
        ``keep=False``: with hipGraph replay the returned tensors are the graph's
        own outputs, valid until the next step (no per-step copy kernels).
        ``mix``: ``(y2, lam)`` of a mixed batch (utils/device_data.py), required
        when the config mixes: the loss is the two-target cross-entropy."""
        if getattr(self, "use_graph", False):
            return self._graph_step(x, y, keep, mix)
        with self.timer.time("compute_launch"):
            self.opt.zero_grad()
            logits = self.model(x)
            loss, hits = self._loss(logits, y, mix)
            loss.backward(unit_grad(loss))
        if self.ddp is not None:
            with self.timer.time("allreduce_wait"):
                self.ddp.synchronize()
        if isinstance(self.opt, Asynchronous):
            self.opt.local_step()
            self.opt.comm_step()
        else:
            with self.timer.time("update"):
                self.opt.step()
        self.step_idx += 1
        return loss.detach(), hits

    @torch.no_grad()
    def evaluate(self, loader, max_batches: int | None = None, per_class: bool = False,
                 ema: bool = False):
        """Mean loss and accuracy over ALL test batches (reference used the last batch
        only, main.py:127); restores train mode afterwards (D6).

        ``ema``: evaluate the averaged model (``--model-ema``): parameters and
        buffers are exchanged with their averages for the pass and back afterwards.

        ``per_class``: also return the [C, C] confusion matrix (rows = true class),
        from which :func:`~..utils.metrics.classification_report` prints the
        reference's verbose per-class precision/recall/F1 table (main.py:127-131).
        """
        if ema:
            avg = getattr(self.opt, "ema", None)
            if avg is None:
                raise ValueError("evaluate(ema=True) needs a run with model_ema > 0")
            with avg.applied():
                return self.evaluate(loader, max_batches, per_class)
        was = self.model.training
        self.model.eval()
        tot_loss = torch.zeros((), device=self.device)
        tot_hits = torch.zeros((), device=self.device, dtype=torch.int64)
        c = self.num_classes
        conf = torch.zeros(c * c, device=self.device, dtype=torch.int64) if per_class else None
        n = 0
        nb = 0
        with fold_session():                 # eval BatchNorms folded into their convs once
            for xb, yb in loader:
                xb, yb = self.prepare(xb, yb)
                out = self.model(xb)
                loss, hits = softmax_cross_entropy(out, yb)
                tot_loss += loss.float() * yb.numel()
                tot_hits += hits.to(torch.int64)
                if conf is not None:
                    pred = out.float().argmax(1)
                    # rows with an ignored / out-of-range label are skipped, as the
                    # loss kernel skips them (bincount rejects negative indices)
                    ok = (yb >= 0) & (yb < c)
                    conf += torch.bincount((yb * c + pred)[ok], minlength=c * c)
                n += yb.numel()
                nb += 1
                if max_batches and nb >= max_batches:
                    break
        self.model.train(was)
        if n == 0:
            res = (float("nan"), float("nan"))
        else:
            res = ((tot_loss / n).item(), tot_hits.item() / n)
        if per_class:
            return (*res, conf.view(c, c).cpu())
        return res

    def set_lr(self, lr: float):
        for g in self.opt.param_groups:
            g["lr"] = lr
        core = getattr(self.opt, "core", None)
        if core is not None:          # between steps, never inside a capture
            core.set_base_lr(lr)

    def finish(self):
        if isinstance(self.opt, Asynchronous):
            self.opt.finish()


def check_stale_config(cfg: TrainConfig, info: DistInfo):
    """The staleness bound is enforced by a PS that serves workers one by one
    (central, sharded_async).  Asking for it anywhere else is an error at
    start-up, never silently ignored."""
    check_policy(cfg.stale_policy, cfg.stale_bound)
    if cfg.stale_policy == "off":
        return
    enforced = cfg.mode == "asgd" and info.is_distributed and \
        cfg.ps in ("central", "sharded_async")
    if not enforced:
        what = f"--mode {cfg.mode}" if cfg.mode != "asgd" else (
            f"--ps {cfg.ps}" if info.is_distributed else "a single-process run (local PS)")
        raise ValueError(
            f"--stale-policy {cfg.stale_policy} cannot be enforced with {what}: only the "
            "central PS and --ps sharded_async serve pulls and applies per worker "
            "(the local PS has one worker, the collective sharded PS is lock-step)")


def check_device_data_config(cfg: TrainConfig, info: DistInfo):
    """Augmentation exists in the device-resident data path only, and that path
    writes bf16 batches on a GPU: anything else is an error at start-up."""
    if cfg.augment not in AUGMENTS:
        raise ValueError(f"unknown --augment {cfg.augment!r}; one of {sorted(AUGMENTS)}")
    if cfg.augment != "none" and not cfg.device_data:
        raise ValueError(f"--augment {cfg.augment} needs --device-data: the host loader applies "
                         "no augmentation (random crop and flip run in the batch assembler)")
    check_mix_config(cfg.mixup, cfg.cutmix, cfg.mix_prob, cfg.mix_switch_prob)
    if (cfg.mixup > 0 or cfg.cutmix > 0) and not cfg.device_data:
        raise ValueError("--mixup / --cutmix need --device-data: the host loader mixes nothing "
                         "(both samples are blended in the batch assembler)")
    if not cfg.device_data:
        return
    if not 0 <= cfg.crop_pad <= MAX_PAD:
        raise ValueError(f"--crop-pad must be in 0..{MAX_PAD}, got {cfg.crop_pad}")
    on_gpu = cfg.cuda and info.device.type == "cuda"
    if on_gpu and (cfg.deterministic or _dtype(cfg.dtype) != torch.bfloat16):
        raise ValueError("--device-data on the GPU assembles bf16 batches: it cannot feed "
                         f"--dtype {cfg.dtype}{' --deterministic' if cfg.deterministic else ''} "
                         "(fp32 compute); use --dtype bf16 or the host loader")


def check_drop_path_config(cfg: TrainConfig):
    """Stochastic depth lives in the ViT's fused residual adds: a rate outside
    [0, 1), or a model without them, is an error at start-up."""
    if not 0.0 <= cfg.drop_path < 1.0:
        raise ValueError(f"--drop-path must be in [0, 1), got {cfg.drop_path}")
    if cfg.drop_path > 0 and not is_vit(cfg.model):
        raise ValueError(f"--drop-path {cfg.drop_path} with --model {cfg.model}: stochastic depth "
                         "exists for the ViT models only (the ResNets' residual add lives in "
                         "the BatchNorm kernels)")


def check_model_ema_config(cfg: TrainConfig):
    """Model EMA options: decay in [0, 1), interval >= 1, and neither the interval
    nor the decay warm-up without a decay -- an error at start-up."""
    try:
        check_ema_options(cfg.model_ema, cfg.model_ema_every, cfg.model_ema_warmup)
    except ValueError as e:
        raise ValueError(f"--model-ema / --model-ema-every / --model-ema-warmup: {e}") from None


def make_device_loaders(cfg: TrainConfig, info: DistInfo, w: "Worker"):
    """Train and test :class:`DeviceLoader` of a run with ``device_data``: the
    train loader augments and mixes as configured and shards as the host path does
    (sync DP by rank, every other mode the whole set in the rank's own order); the
    test loader serves the test set in order, unaugmented and unmixed."""
    tr, te, source = get_device_datasets(cfg.dataset, cfg.data_dir, w.input_shape, w.num_classes,
                                         cfg.n_train, cfg.n_test, cfg.seed, w.device)
    crop, flip = AUGMENTS[cfg.augment]
    shard = cfg.mode == "sync" and info.is_distributed
    mix = MixConfig(cfg.mixup, cfg.cutmix, cfg.mix_prob, cfg.mix_switch_prob) \
        if cfg.mixup > 0 or cfg.cutmix > 0 else None
    train = DeviceLoader(tr, cfg.batch_size, shuffle=True, drop_last=True,
                         pad=cfg.crop_pad if crop else 0, flip=flip, seed=cfg.seed + info.rank,
                         rank=info.rank if shard else 0, world=info.world_size if shard else 1,
                         out_dtype=w.compute_dtype, mix=mix)
    test = DeviceLoader(te, cfg.test_batch_size, shuffle=False, drop_last=False,
                        out_dtype=w.compute_dtype)
    return train, test, source + "+device"


def delay_comp_coefficient(cfg: TrainConfig) -> float:
    """``c = lambda / (lr * n_push)``: what the servers take.  A push carries
    ``d = -lr * sum(g_i)`` of ``n_push`` steps; DC-ASGD's ``lambda * g*g`` becomes
    ``c * d*d`` per unit of ``d`` (``(sum g)^2 ~ n^2 gbar^2`` against ``sum(g^2) ~
    n gbar^2``).  Formed once from the base learning rate: under a decaying
    schedule the compensation shrinks with ``lr_t / lr_0``."""
    return cfg.delay_comp / (cfg.lr * cfg.n_push) if cfg.delay_comp else 0.0


def check_delay_comp_config(cfg: TrainConfig, info: DistInfo, client=None):
    """Delay compensation corrects a stale push at a PS that hands every worker
    its own snapshot: the central PS, and the shared PS of the virtual workers
    (``client``).  Anywhere else, and with an update that is not proportional to
    the gradient (AdamW), asking for it is an error at start-up.  SGD with
    momentum passes: its delta is a running mean of gradients, for which
    ``lambda * g*g`` is an approximation."""
    lam = cfg.delay_comp
    if not (0.0 <= lam < float("inf")):
        raise ValueError(f"--delay-comp must be finite and >= 0, got {lam!r}")
    if lam == 0:
        return
    what = None
    if cfg.mode != "asgd":
        what = (f"--mode {cfg.mode}", "there is no parameter server and no stale push")
    elif cfg.optimizer == "adamw":
        what = ("--optimizer adamw", "its update is not proportional to the gradient, so "
                "lambda * g*g is no stand-in for the curvature seen by the pushed delta")
    elif client is not None and not isinstance(client, SharedPSClient):
        what = (type(client).__name__, "this client's server keeps no per-worker backup")
    elif client is None and (cfg.ps != "central" or not info.is_distributed):
        flavour = f"--ps {cfg.ps}" if info.is_distributed else \
            "--ps local (a single-process run)"
        what = (flavour, "a single worker or a lock-step collective has no stale push to "
                "correct, and the sharded_async shard servers do not compensate")
    if what:
        raise ValueError(f"--delay-comp {lam} is not supported with {what[0]}: {what[1]} "
                         "(delay compensation runs on the central PS and the virtual workers)")
    if not cfg.lr > 0 or cfg.n_push < 1:
        raise ValueError("--delay-comp needs lr > 0 and n_push >= 1 (c = lambda / (lr n_push))")


def check_push_wire_config(cfg: TrainConfig, client=None):
    """The 8-bit and the sparse top-k push wire exist where one worker's push
    reaches one server: the local PS and the central PS.  Anywhere else they are
    an error at start-up."""
    if check_push_wire(cfg.push_wire, cfg.push_topk) == "same":
        return
    what = None
    if cfg.mode != "asgd":
        what = f"--mode {cfg.mode}"
    elif client is not None and not client.supports_mx8:
        what = f"{type(client).__name__} (virtual workers)"
    elif client is None and cfg.ps in ("sharded", "sharded_async"):
        what = f"--ps {cfg.ps}"
    if what:
        name = "8-bit" if cfg.push_wire == "mx8" else "sparse"
        raise ValueError(f"--push-wire {cfg.push_wire} is not supported with {what}: the {name} "
                         f"push wire runs on {MX8_FLAVOURS}")


def _payload(cfg: TrainConfig, info: DistInfo) -> str:
    if cfg.payload != "auto":
        return cfg.payload
    return "rccl" if info.backend == "nccl" else "gloo"


def run_server(cfg: TrainConfig, info: DistInfo, ps_groups):
    """Rank 0 in the central topology (reference main.py:135-138)."""
    ctrl, pairs = ps_groups
    model, _, _ = build_model(cfg.model, cfg.num_classes)
    payload = _payload(cfg, info)
    server = ParameterServer(model=model, control_group=ctrl, pair_groups=pairs,
                             payload=payload,
                             device=info.device if payload == "rccl" else "cpu",
                             checkpoint_path=cfg.checkpoint,
                             checkpoint_every=cfg.checkpoint_every,
                             worker_timeout=cfg.ps_worker_timeout or None,
                             delta_scale=cfg.delta_scale, stale_bound=cfg.stale_bound,
                             stale_policy=cfg.stale_policy,
                             delay_comp=delay_comp_coefficient(cfg),
                             push_topk=cfg.push_topk if cfg.push_wire == "topk" else 0)
    ps_path = _ps_resume_path(cfg)
    if ps_path:
        server.load_checkpoint(ps_path)
    elif cfg.ps_resume:
        raise FileNotFoundError(f"--ps-resume {cfg.ps_resume}: no parameter-server checkpoint")
    stats = server.run()
    if cfg.verbose:
        print(f"[ps] finished: {stats}", flush=True)
    return stats


def run_training(cfg: TrainConfig, info: DistInfo):
    """Entry point for every rank. Returns a result dict (worker) or PS stats."""
    check_stale_config(cfg, info)
    check_push_wire_config(cfg)
    check_delay_comp_config(cfg, info)
    check_device_data_config(cfg, info)
    check_drop_path_config(cfg)
    check_model_ema_config(cfg)
    ps_groups = None
    central = cfg.mode == "asgd" and cfg.ps == "central" and info.is_distributed
    if central:
        ps_groups = make_ps_groups(0, _payload(cfg, info))
    # start-up checks every rank joins: ranks reached by a collective, distinct
    # devices on RCCL, every (PS, worker) payload communicator answering
    pf = preflight(info, None, ps_groups[1] if ps_groups else None, 0)
    if cfg.verbose and info.rank == 0 and info.is_distributed:
        print(f"[preflight] {pf}", flush=True)
    if central and info.rank == 0:
        return {"role": "ps", "preflight": pf, **run_server(cfg, info, ps_groups)}
    w = Worker(cfg, info, ps_groups)
    if cfg.device_data:
        # the dataset lives on the device; the step replays as a graph whose input
        # buffers the loader's kernel writes in place
        train_loader, test_loader, source = make_device_loaders(cfg, info, w)
        w.enable_graph(True)
    else:
        tr, te, source = get_datasets(cfg.dataset, cfg.data_dir, w.input_shape, w.num_classes,
                                      cfg.n_train, cfg.n_test, seed=cfg.seed)
        # every worker sees the full dataset in its own shuffle order (reference has no
        # DistributedSampler, main.py:27); sync-DP shards by rank instead.
        if cfg.mode == "sync" and info.is_distributed:
            idx = list(range(info.rank, len(tr), info.world_size))
            tr = torch.utils.data.Subset(tr, idx)
        train_loader, test_loader = make_loaders(tr, te, cfg.batch_size, cfg.test_batch_size,
                                                 shuffle_seed=cfg.seed + info.rank)
    core = getattr(w.opt, "core", None)
    if core is not None and cfg.lr_schedule == "warmup_cosine" and \
            not (cfg.schedule_steps or cfg.max_steps) and core.t == 0:
        core.set_total_steps(max(cfg.epochs * len(train_loader), cfg.warmup_steps + 1))
    log = IterationLog()
    log_phases = bool(cfg.log_interval)
    meter = Throughput(sync_cuda=w.device.type == "cuda")
    base_lr = cfg.lr
    done = False
    t_start = time.perf_counter()
    for epoch in range(cfg.epochs):
        if cfg.lr_schedule == "inv_epoch":
            w.set_lr(base_lr / (epoch + 1))
        if cfg.verbose and info.rank <= 1:
            print(f"Training for epoch {epoch}", flush=True)
        batches = train_loader.iter_into(w.static_batch_buffers) if cfg.device_data \
            else train_loader
        for i, (xb, yb) in enumerate(batches):
            if not cfg.device_data:
                xb, yb = w.prepare(xb, yb)
            loss, hits = w.train_step(xb, yb, mix=train_loader.last_mix if w.mixes else None)
            meter.add(yb.numel())
            row = log.append(epoch, i, loss)
            if cfg.log_interval and i % cfg.log_interval == 0 and i > 0:
                row["samples_per_sec"] = meter.rate()
                row["param_norm"] = w.param_norm()
                if core is not None:      # the only read-back of the hyper block
                    row["lr"], row["grad_norm"] = core.lr(), core.grad_norm()
                if cfg.divergence_check and not math.isfinite(row["param_norm"]):
                    raise DivergenceError(
                        f"rank {info.rank}: non-finite parameters at epoch {epoch} iteration {i} "
                        f"(loss {float(loss):.4g}); lower --lr or pass --no-divergence-check")
                if cfg.evaluate:
                    row["test_loss"], row["test_accuracy"] = w.evaluate(test_loader)
                    if cfg.model_ema > 0:
                        row["ema_test_loss"], row["ema_test_accuracy"] = \
                            w.evaluate(test_loader, ema=True)
                log.flush_pending()
                if cfg.verbose:
                    print("Timestamp: {timestamp} | Iteration: {iteration:6} | "
                          "Loss: {training_loss:6.4f} | Test Loss: {tl} | Test Accuracy: {ta} | "
                          "samples/s: {sps:.1f}".format(
                              tl=_fmt(row.get("test_loss")), ta=_fmt(row.get("test_accuracy")),
                              sps=row["samples_per_sec"], **row), flush=True)
            if cfg.checkpoint and cfg.checkpoint_every and w.step_idx % cfg.checkpoint_every == 0:
                ckpt.save_worker_checkpoint(_worker_ckpt(cfg, info), w.model, w.opt, w.step_idx)
            if log_phases and i % cfg.log_interval == 0 and i > 0:
                row.update({f"{k}_ms": v["mean_ms"] for k, v in w.timer.summary().items()})
            if cfg.max_steps and w.step_idx >= cfg.max_steps:
                done = True
                break
        if cfg.evaluate and not done:
            vl, va, conf = w.evaluate(test_loader, per_class=True)
            if cfg.verbose:
                print(f"epoch {epoch}: lr {w.opt.param_groups[0]['lr']:.5g} "
                      f"test loss {vl:.4f} test accuracy {va:.4f}", flush=True)
                # the reference's verbose eval prints sklearn's per-class report
                # (/root/reference/example/main.py:127-131)
                print(classification_report(conf), flush=True)
            if cfg.model_ema > 0 and cfg.verbose:      # only ever printed: no pass without it
                el, ea = w.evaluate(test_loader, ema=True)
                print(f"epoch {epoch}: model EMA test loss {el:.4f} test accuracy {ea:.4f}",
                      flush=True)
        if done:
            break
    w.finish()
    elapsed = time.perf_counter() - t_start
    final = w.evaluate(test_loader) if cfg.evaluate else (float("nan"), float("nan"))
    final_ema = w.evaluate(test_loader, ema=True) if cfg.evaluate and cfg.model_ema > 0 else None
    if cfg.checkpoint:
        ckpt.save_worker_checkpoint(_worker_ckpt(cfg, info), w.model, w.opt, w.step_idx)
    from ..utils.metrics import log_path

    path = log_path(cfg.mode == "single" and not info.is_distributed,
                    w.device.type == "cuda", info.rank, cfg.log_dir)
    log.to_csv(path)
    res = {"role": "worker", "rank": info.rank, "steps": w.step_idx, "elapsed_s": elapsed,
           "samples_per_sec": meter.rate(), "test_loss": final[0], "test_accuracy": final[1],
           "data": source, "log": path, "preflight": pf}
    if final_ema is not None:
        res["ema_test_loss"], res["ema_test_accuracy"] = final_ema
    if isinstance(w.opt, Asynchronous):
        res.update(w.opt.stats())
    res["phases"] = w.timer.summary()
    if cfg.verbose:
        print(f"[worker {info.rank}] {res}", flush=True)
    return res


def _worker_ckpt(cfg, info):
    return ckpt.worker_checkpoint_path(cfg.checkpoint, info.rank)


def _agree_on_resume(have: bool, info: DistInfo):
    """Collective check that every rank found (or did not find) its worker
    checkpoint; raises on disagreement instead of hanging in the restore."""
    dev = info.device if info.backend == "nccl" else torch.device("cpu")
    t = torch.tensor([1.0 if have else 0.0, 0.0 if have else 1.0], device=dev)
    dist.all_reduce(t)
    n_have, n_miss = int(round(float(t[0]))), int(round(float(t[1])))
    if n_have and n_miss:
        raise RuntimeError(
            f"resume: {n_have} rank(s) found their worker checkpoint and {n_miss} did not "
            f"(this is rank {info.rank}, {'found' if have else 'missing'}): the sharded / "
            "sync topologies restore collectively; supply every <base>.worker<r>.pt or none")


def _worker_resume_path(base: str, rank: int) -> str | None:
    """``<base>.worker<rank>.pt`` if present, else ``base`` when it is itself a worker
    checkpoint, else ``None`` (e.g. only a PS checkpoint: the worker starts fresh
    and adopts the PS parameters at its first pull)."""
    cand = ckpt.worker_checkpoint_path(base, rank)
    if os.path.exists(cand):
        return cand
    if os.path.exists(base) and ckpt.checkpoint_kind(base) == "worker":
        return base
    return None


def _ps_resume_path(cfg) -> str | None:
    for p in (cfg.ps_resume, cfg.resume):
        if p and os.path.exists(p) and ckpt.checkpoint_kind(p) == "ps":
            return p
    return None


def _fmt(v):
    return "   n/a" if v is None or (isinstance(v, float) and math.isnan(v)) else f"{v:6.4f}"


def config_dict(cfg: TrainConfig) -> dict:
    return asdict(cfg)
