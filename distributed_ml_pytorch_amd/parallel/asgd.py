"""Downpour / asynchronous SGD optimizer (reference C1 + C8).

Worker side of DistBelief Downpour SGD, re-implemented from the behaviour of
/root/reference/asgd/optim/Asynchronous.py:20-71:

* every ``n_pull`` steps request the PS parameters (:48-49),
* accumulate ``-lr * grad`` into a push accumulator (:54-55),
* every ``n_push`` steps send the accumulator to the PS and zero it (:58-60),
* always apply the local SGD step ``p -= lr * grad`` (:63-68).

What is different by design:

* one fused HIP kernel over the flat arena does accumulate + local step +
  bf16 shadow refresh (no per-step ravel ``torch.cat``, no per-tensor loop);
* the accumulator lives on the parameters' device (D4);
* a pulled snapshot is landed at a step boundary by the optimizer itself,
  never written into live parameters by a listener thread (D13), and at most
  ``staleness`` steps after it was requested (bounded staleness);
* ``super().__init__`` is called correctly (D2) and ``DownpourSGD`` is exported
  (D1).
"""
from __future__ import annotations

import torch
import torch.distributed as dist
from torch.optim.optimizer import required

from .arena import attach_arena, get_arena
from .clients import GlooPSClient, LocalPSClient, PSClient, check_push_wire
from .ema import ModelEma
from .fused_optim import (KINDS, ArenaOptimizer, FusedOptimCore, check_ema_options,
                          sgd_by_value)


def default_client(**kw) -> PSClient:
    """The reference's implicit choice: rank 0 is the PS over gloo, else local."""
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        return GlooPSClient(ps_rank=0, **kw)
    return LocalPSClient(**kw)


class Asynchronous(ArenaOptimizer):
    has_client = True

    def __init__(self, params, lr=required, n_push=required, n_pull=required, model=required, *,
                 client: PSClient | None = None, staleness: int = 1, momentum: float = 0.0,
                 dampening: float = 0.0, nesterov: bool = False, weight_decay: float = 0.0,
                 pull_mode: str = "overwrite", wire_dtype: torch.dtype = torch.float32,
                 shadow_dtype: torch.dtype | None | str = "auto", optimizer: str = "sgd",
                 betas=(0.9, 0.999), eps: float = 1e-8, max_grad_norm: float = 0.0,
                 schedule=None, push_wire: str = "same", push_topk: int = 8,
                 ema_decay: float = 0.0, ema_every: int = 1, ema_warmup: bool = False,
                 trust_coef: float = 0.001, lars_eps: float = 0.0):
        """``optimizer``: ``"sgd"``, ``"adamw"``, ``"lamb"`` or ``"lars"`` (the
        layer-wise adaptive kinds of :mod:`.fused_optim`; ``momentum`` serves LARS,
        which takes neither ``nesterov`` nor ``dampening``).

        ``ema_decay > 0``: an exponential moving average of the parameters and the
        floating-point buffers is kept by the update pass (:mod:`.fused_optim`,
        :mod:`.ema`; ``self.ema.applied()`` evaluates with it).  A pull landing is no
        EMA event: the average sees the landed values at its next update.

        ``push_wire="mx8"``: pushes travel as block-scaled 8-bit payloads
        (:mod:`.wire8`) and the accumulator keeps the quantisation residual, so
        nothing is lost, only delayed to the next push.  ``push_wire="topk"``:
        a push carries the ``push_topk`` (1..32) largest entries of every
        256-element block (:mod:`.wire_topk`); everything else stays in the
        accumulator for a later push.  Local and central PS clients only;
        ``"same"`` (default) pushes in ``wire_dtype``."""
        if lr is required or n_push is required or n_pull is required or model is required:
            raise TypeError("Asynchronous needs lr, n_push, n_pull and model")
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if int(n_push) < 1 or int(n_pull) < 1:
            raise ValueError("n_push and n_pull must be >= 1")
        if optimizer not in KINDS:
            raise ValueError(f"unknown optimizer {optimizer!r}; one of {KINDS}")
        if optimizer == "lars" and (nesterov or dampening):
            raise ValueError("optimizer 'lars' takes neither nesterov nor dampening")
        check_ema_options(ema_decay, ema_every, ema_warmup)
        arena = get_arena(model)
        if arena is None:
            dev = next(model.parameters()).device
            if shadow_dtype == "auto":
                shadow_dtype = torch.bfloat16 if dev.type == "cuda" else None
            arena = attach_arena(model, shadow_dtype=shadow_dtype)
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, nesterov=nesterov,
                        weight_decay=weight_decay)
        super().__init__(params, defaults, arena,
                         mom=bool(momentum and optimizer == "sgd") or optimizer == "lars")
        self.model = model
        self.n_push = int(n_push)
        self.n_pull = int(n_pull)
        mine = {id(p) for g in self.param_groups for p in g["params"]}
        if mine != {id(p) for p in arena.params}:
            raise ValueError("Asynchronous must be given exactly model.parameters() "
                             "(the push/pull vector is the whole model, as in the reference)")
        self.acc = torch.zeros(arena.numel, dtype=torch.float32, device=arena.device)
        # AdamW, clipping, a per-step schedule or a model EMA: the update reads lr
        # and the gradient scale from a device-resident hyper block
        # (fused_optim.py); plain constant-lr SGD keeps the by-value kernel
        if optimizer != "sgd" or max_grad_norm > 0 or schedule is not None or ema_decay > 0:
            trust = dict(trust_coef=trust_coef, lars_eps=lars_eps) if optimizer == "lars" else {}
            self.core = FusedOptimCore(arena, optimizer, lr, betas=betas, eps=eps,
                                       weight_decay=weight_decay, momentum=momentum,
                                       nesterov=nesterov, max_grad_norm=max_grad_norm,
                                       schedule=schedule, model=model, ema_decay=ema_decay,
                                       ema_every=ema_every, ema_warmup=ema_warmup, **trust)
        self.idx = 0
        self.timer = _NO_TIMER      # a utils.metrics.StepTimer when the trainer wires one
        if client is None:
            client = default_client(staleness=staleness, pull_mode=pull_mode,
                                    wire_dtype=wire_dtype, push_wire=push_wire,
                                    push_topk=push_topk)
        elif check_push_wire(push_wire, push_topk) != "same":
            client.push_wire = push_wire       # an explicit client takes the optimizer's knob
            client.push_topk = int(push_topk)
        self.client = client
        self.client.attach(self)
        self.client.init()
        # the average starts from the parameters as the PS client left them
        if ema_decay > 0:
            self.core.reset_ema()
            self.ema = ModelEma(model, self.core, self.client)

    # reference-visible attributes -----------------------------------------
    @property
    def accumulated_gradients(self) -> torch.Tensor:
        return self.acc

    def _update(self, g):
        """Fused accumulate + SGD (or the core's kind), the push accumulator included."""
        damp = self._first_step_dampening(g)
        if self.core is not None:
            return self._core_step(self.acc, self.mom, damp)
        sgd_by_value(self.arena, self.acc, self.mom, g["lr"], g["weight_decay"], g["momentum"],
                     damp, g["nesterov"])

    @torch.no_grad()
    def comm_step(self):
        """Host-scheduled half: push / pull / land on the reference cadence."""
        t = self.timer
        if self.idx % self.n_push == 0:
            with t.time("push"):
                self.client.push(self.idx)
        if self.idx % self.n_pull == 0:
            with t.time("pull_issue"):
                self.client.request_pull(self.idx)
        with t.time("land"):
            self.client.land_due(self.idx)
        self.idx += 1

    def finish(self):
        """Land outstanding pulls, flush sends, tell the PS we are done."""
        self.client.finish()

    def stats(self) -> dict:
        return {"steps": self.idx, **self.client.stats()}


class _NoTimer:
    class _Ctx:
        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

    _ctx = _Ctx()

    def time(self, name):
        return self._ctx


_NO_TIMER = _NoTimer()


# The reference's package exports this name (asgd/optim/__init__.py:1) while its
# class body is called Asynchronous (Asynchronous.py:40): both names, one class.
DownpourSGD = Asynchronous
