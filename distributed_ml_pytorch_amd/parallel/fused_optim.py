"""Optimizer core shared by the fused optimizers: AdamW / SGD over the flat
arena with global-norm gradient clipping and a per-step learning-rate schedule.

Everything that changes from step to step -- the step count ``t``, the
effective ``lr_t``, the gradient scale ``grad_scale * clip``, Adam's bias
corrections -- lives in a small device buffer (the *hyper block* of
``csrc/optim.hip``) that one single-block kernel advances on the step's stream.
No per-step host value enters a kernel argument, so a captured step graph is
captured once and replays through a changing learning rate, and nothing here
synchronises with the host (``lr()`` / ``grad_norm()`` read back; call them at
log intervals only).

One step (the CPU path below is the readable specification; the GPU path is
``optim_hyper`` + ``adamw_fused_step`` / ``asgd_fused_step_dev``)::

    norm   = grad_scale * ||g||_2                      (only with clipping on)
    clip   = min(1, max_grad_norm / (norm + 1e-6))     (torch clip_grad_norm_)
    gscale = grad_scale * clip
    t     += 1
    lr_t   = schedule(t)
    g'     = gscale * g
    AdamW:  m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g'^2
            p = p (1 - lr_t wd decay) - lr_t / (1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
    SGD:    torch.optim.SGD on g' (weight decay, momentum, nesterov) with lr_t
    acc   += p_new - p_old      (the Downpour push carries the applied update)

``decay`` is 0 for parameters with ``dim() <= 1`` (biases, norm scales and
shifts) and for the names a model lists in ``no_weight_decay()``; AdamW's
decoupled weight decay skips them.  It is held as one ``uint8`` per 64-element
arena block (every parameter starts on such a boundary, ``arena.ALIGN``).

Model EMA (``ema_decay > 0``; evaluation through :mod:`.ema`): a flat fp32
buffer ``e`` of the arena's length, a copy of ``p32`` when the optimizer is
built, averaged in the same pass after the parameter update of step ``t``::

    t % K != 0:  e untouched                       (K = ema_every)
    u   = t / K                                    (EMA update index, 1-based)
    d_u = min(decay, (1 + u) / (10 + u))  with ema_warmup, else decay    (fp64)
    D, O = fp32(d_u), fp32(1 - d_u)                (the difference in fp64)
    e   = fl32(fl32(D * e) + fl32(O * p_new))      (three roundings, no FMA)

timm's form: it carries about one ulp of rounding noise per update and never
stalls.  ``decay`` enters as its fp32 rounding, as ``base_lr`` does.  A pull
landing (``Asynchronous``) changes ``p32`` between two steps and is no EMA
event: the average sees the landed values at its next update.
"""
from __future__ import annotations

import logging
import math
from dataclasses import asdict, dataclass

import torch

from .arena import ALIGN, FlatArena

_LOG = logging.getLogger(__name__)

# hyper-block words (csrc/optim.hip enum HyperWord)
H_STEP, H_LR, H_GSCALE, H_BC1, H_BC2, H_NORM, H_KIND, H_BASE_LR, H_LR_MIN, H_WARMUP, H_TOTAL, \
    H_BETA1, H_BETA2, H_MAX_NORM, H_GRAD_SCALE, H_OMB1, H_OMB2, H_EMA_D, H_EMA_O, H_EMA_U, \
    H_EMA_DECAY, H_EMA_EVERY, H_EMA_WARM = range(23)
HYPER_WORDS = 24
_KINDS = {"constant": 0, "warmup_cosine": 1}
_PARTIALS = 1024            # launch_sumsq_partial's block cap


def _f32(x: float) -> float:
    """``x`` rounded to fp32, as a Python float."""
    return float(torch.tensor(x, dtype=torch.float32))


def check_ema_options(decay: float, every: int = 1, warmup: bool = False) -> float:
    """Validate the model-EMA options -> the decay as its fp32 rounding.
    ``decay`` in [0, 1) (0 = off), ``every >= 1``; ``every`` / ``warmup`` without a
    decay are an error, never silently ignored."""
    if not (isinstance(decay, (int, float)) and 0.0 <= decay < 1.0):
        raise ValueError(f"model EMA decay must be in [0, 1), got {decay!r}")
    if int(every) != every or every < 1:
        raise ValueError(f"model EMA interval (every) must be an integer >= 1, got {every!r}")
    d32 = _f32(decay)
    if d32 >= 1.0:
        raise ValueError(f"model EMA decay {decay!r} rounds to 1 in fp32: the average would "
                         "never move")
    if decay == 0 and (every != 1 or warmup):
        raise ValueError("model EMA interval / warmup given without a decay (model EMA is off)")
    return d32


def ema_coeffs(decay: float, every: int, warmup: bool, t: int):
    """``(u, D, O)`` of optimizer step ``t`` (1-based): the EMA update index and
    the two published fp32 scalars; ``D = 1, O = 0`` on a step without an update."""
    u = t // every
    if t % every:
        return u, 1.0, 0.0
    d = _f32(decay)
    if warmup:
        d = min(d, (1 + u) / (10 + u))
    return u, _f32(d), _f32(1.0 - d)


@dataclass(frozen=True)
class Schedule:
    """Per-step learning-rate schedule evaluated on the device.

    ``warmup_cosine``: linear from ``base_lr / warmup_steps`` to ``base_lr`` over
    the first ``warmup_steps`` updates, half a cosine down to ``lr_min`` at
    update ``total_steps``, ``lr_min`` from there on."""
    kind: str = "constant"
    warmup_steps: int = 0
    total_steps: int = 0
    lr_min: float = 0.0

    def __post_init__(self):
        if self.kind not in _KINDS:
            raise ValueError(f"unknown schedule {self.kind!r}; one of {sorted(_KINDS)}")
        if self.warmup_steps < 0:
            raise ValueError("warmup_steps must be >= 0")
        if self.kind == "warmup_cosine" and self.total_steps <= self.warmup_steps:
            raise ValueError(f"warmup_cosine needs total_steps ({self.total_steps}) > "
                             f"warmup_steps ({self.warmup_steps})")

    def lr_at(self, base_lr: float, t: int) -> float:
        """Closed form of the learning rate of update ``t`` (1-based)."""
        if self.kind == "constant":
            return base_lr
        w, n = self.warmup_steps, self.total_steps
        if t <= w:
            return base_lr * t / w
        if t >= n:
            return self.lr_min
        return self.lr_min + 0.5 * (base_lr - self.lr_min) * (
            1.0 + math.cos(math.pi * (t - w) / (n - w)))


def make_schedule(s) -> Schedule:
    if s is None:
        return Schedule()
    if isinstance(s, Schedule):
        return s
    if isinstance(s, str):
        return Schedule(kind=s)
    return Schedule(**dict(s))


def decay_mask(arena: FlatArena, model: torch.nn.Module | None = None) -> torch.Tensor:
    """``uint8 [arena.numel / 64]``: 1 where AdamW's weight decay applies."""
    skip = set()
    if model is not None and hasattr(model, "no_weight_decay"):
        named = dict(model.named_parameters())
        for name in model.no_weight_decay():
            if name not in named:
                raise KeyError(f"no_weight_decay() names {name!r}, which is not a parameter")
            skip.add(id(named[name]))
    mask = torch.zeros(arena.numel // ALIGN, dtype=torch.uint8)
    for p, s in zip(arena.params, arena.slots):
        if p.dim() <= 1 or id(p) in skip:
            continue
        mask[s.offset // ALIGN:(s.offset + s.numel + ALIGN - 1) // ALIGN] = 1
    return mask


def sync_base_lr(core: "FusedOptimCore", lr: float):
    """Adopt a ``param_groups`` lr the host changed (``inv_epoch``, user code).
    A captured step never gets here with a new value: the base lr of a device
    schedule is constant, and ``Worker.set_lr`` updates the core between steps."""
    if lr != core.base_lr:
        if core.native is not None and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("the base learning rate changed inside a graph capture; call "
                               "core.set_base_lr() between steps")
        core.set_base_lr(lr)


class FusedOptimCore:
    """Owns the hyper block, the norm partials, ``m`` / ``v`` and the decay mask
    of one optimizer over one arena; ``step`` applies one update."""

    def __init__(self, arena: FlatArena, kind: str = "adamw", lr: float = 1e-3, *,
                 betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0,
                 momentum: float = 0.0, nesterov: bool = False, grad_scale: float = 1.0,
                 max_grad_norm: float = 0.0, schedule=None,
                 model: torch.nn.Module | None = None, ema_decay: float = 0.0,
                 ema_every: int = 1, ema_warmup: bool = False):
        if kind not in ("sgd", "adamw"):
            raise ValueError(f"unknown optimizer {kind!r}; 'sgd' or 'adamw'")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"betas must be in [0, 1): {betas}")
        if eps < 0.0 or max_grad_norm < 0.0 or lr < 0.0:
            raise ValueError("lr, eps and max_grad_norm must be >= 0")
        if arena.numel % ALIGN:
            raise ValueError("arena length must be a multiple of 64")
        self.arena = arena
        self.kind = kind
        self.base_lr = float(lr)
        self.betas = (float(betas[0]), float(betas[1]))
        self.eps = float(eps)
        self.weight_decay = float(weight_decay)
        self.momentum = float(momentum)
        self.nesterov = bool(nesterov)
        self.grad_scale = float(grad_scale)
        self.max_grad_norm = float(max_grad_norm)
        self.schedule = make_schedule(schedule)
        self.ema_decay = check_ema_options(ema_decay, ema_every, ema_warmup)
        self.ema_every = int(ema_every)
        self.ema_warmup = bool(ema_warmup)
        dev = arena.device
        self.native = None
        if dev.type == "cuda":
            from ..ops._ext import native

            self.native = native()
            assert self.native.optim_hyper_words() == HYPER_WORDS
        self.m = self.v = self.mask = None
        if kind == "adamw":
            self.m = torch.zeros(arena.numel, dtype=torch.float32, device=dev)
            self.v = torch.zeros(arena.numel, dtype=torch.float32, device=dev)
            self.mask = decay_mask(arena, model).to(dev)
        self.partials = None
        if self.native is not None and self.max_grad_norm > 0:
            self.partials = torch.zeros(_PARTIALS, dtype=torch.float32, device=dev)
        # host copy of the per-step values: THE state on the CPU path, the values
        # the hyper block is (re)written from on the GPU
        self._t = 0
        self._lr_t = self.schedule.lr_at(self.base_lr, 1)
        self._norm = 0.0
        self.hyper = None
        if self.native is not None:
            self._write_hyper()
        # model EMA: a copy of the parameters as they are now (an optimizer whose
        # PS client re-seeds them afterwards calls reset_ema() again)
        self.ema = None
        self._ema_last = (1.0, 0.0)         # (D, O) of the last step, CPU path
        if self.ema_decay > 0:
            self.ema = torch.empty(arena.numel, dtype=torch.float32, device=dev)
            self.reset_ema()

    # -------------------------------------------------------------- model EMA
    @torch.no_grad()
    def reset_ema(self):
        """``e <- p32`` (construction, and a resume whose checkpoint holds no EMA)."""
        if self.ema is not None:
            self.ema.copy_(self.arena.p32)

    @property
    def ema_updates(self) -> int:
        """EMA updates applied so far (a device read-back on the GPU)."""
        if self.ema is None:
            return 0
        if self.hyper is None:
            return self._t // self.ema_every
        return int(self._read_hyper().view(torch.int32)[H_EMA_U])

    def ema_last(self):
        """``(D, O)`` of the last step (CPU path; the kernels read the hyper block)."""
        return self._ema_last

    # ------------------------------------------------------------ hyper block
    def _write_hyper(self):
        """(Re)build the whole block from the host-side description (construction,
        checkpoint load, a new base lr / schedule length): one small H2D copy."""
        h = torch.zeros(HYPER_WORDS, dtype=torch.float32)
        hi = h.view(torch.int32)
        b1, b2 = self.betas if self.kind == "adamw" else (0.0, 0.0)
        t = self._t
        hi[H_STEP] = t
        h[H_LR] = self._lr_t
        h[H_GSCALE] = self.grad_scale
        h[H_BC1] = 1.0 - b1 ** t if t else 1.0
        h[H_BC2] = 1.0 - b2 ** t if t else 1.0
        h[H_NORM] = self._norm
        hi[H_KIND] = _KINDS[self.schedule.kind]
        h[H_BASE_LR] = self.base_lr
        h[H_LR_MIN] = self.schedule.lr_min
        hi[H_WARMUP] = self.schedule.warmup_steps
        hi[H_TOTAL] = self.schedule.total_steps
        h[H_BETA1], h[H_BETA2] = b1, b2
        h[H_MAX_NORM] = self.max_grad_norm
        h[H_GRAD_SCALE] = self.grad_scale
        h[H_OMB1], h[H_OMB2] = 1.0 - b1, 1.0 - b2
        if self.ema_decay > 0:
            # between steps: "no update" until the next step publishes its own
            h[H_EMA_D], h[H_EMA_O] = 1.0, 0.0
            hi[H_EMA_U] = t // self.ema_every
            h[H_EMA_DECAY] = self.ema_decay
            hi[H_EMA_EVERY] = self.ema_every
            hi[H_EMA_WARM] = int(self.ema_warmup)
        if self.hyper is None:
            self.hyper = h.to(self.arena.device)
        else:
            self.hyper.copy_(h)

    def _read_hyper(self) -> torch.Tensor:
        return self.hyper.cpu()

    @property
    def t(self) -> int:
        """Updates applied so far (a device read-back on the GPU)."""
        if self.hyper is None:
            return self._t
        return int(self._read_hyper().view(torch.int32)[H_STEP])

    def lr(self) -> float:
        """Learning rate of the last update (before the first: of the first)."""
        if self.hyper is None:
            return self._lr_t
        return float(self._read_hyper()[H_LR])

    def grad_norm(self) -> float:
        """``grad_scale * ||g||`` of the last update; 0 with clipping off."""
        if self.hyper is None:
            return self._norm
        return float(self._read_hyper()[H_NORM])

    def _resync(self, t: int | None = None):
        self._t = self.t if t is None else int(t)
        self._lr_t = self.schedule.lr_at(self.base_lr, max(self._t, 1))
        if self.hyper is not None:
            self._norm = self.grad_norm() if t is None else 0.0
            self._write_hyper()

    def set_base_lr(self, lr: float):
        """New base learning rate (host-side schedules such as ``inv_epoch``).
        Not for use inside a graph capture: it copies to the device."""
        self.base_lr = float(lr)
        self._resync()

    def set_total_steps(self, total_steps: int):
        self.schedule = Schedule(self.schedule.kind, self.schedule.warmup_steps, int(total_steps),
                                 self.schedule.lr_min)
        self._resync()

    # ------------------------------------------------------------------- step
    @torch.no_grad()
    def step(self, arena: FlatArena | None = None, acc: torch.Tensor | None = None,
             mom: torch.Tensor | None = None, dampening: float = 0.0):
        """One update of ``arena.p32`` from ``arena.g32`` (+ bf16 shadow, + ``acc``).
        ``mom`` / ``dampening``: the SGD momentum buffer and this step's dampening."""
        a = arena if arena is not None else self.arena
        if self.native is not None:
            clip = self.partials is not None
            self.native.optim_hyper(self.hyper, a.g32 if clip else None, self.partials)
            if self.kind == "adamw":
                self.native.adamw_fused_step(a.g32, a.p32, acc, self.m, self.v, a.w16, self.mask,
                                             self.hyper, self.weight_decay, self.eps, self.ema)
            else:
                self.native.asgd_fused_step_dev(a.g32, a.p32, acc, mom, a.w16, self.hyper,
                                                self.weight_decay, self.momentum, dampening,
                                                self.nesterov, self.ema)
            return
        g = a.g32
        clipc = 1.0
        if self.max_grad_norm > 0:
            self._norm = self.grad_scale * float(g.norm())
            c = self.max_grad_norm / (self._norm + 1e-6)
            clipc = c if (c < 1.0 or c != c) else 1.0
        gscale = self.grad_scale * clipc
        self._t += 1
        t = self._t
        lr = self._lr_t = self.schedule.lr_at(self.base_lr, t)
        gs = g * gscale if gscale != 1.0 else g
        p = a.p32
        if self.kind == "adamw":
            b1, b2 = self.betas
            self.m.mul_(b1).add_(gs, alpha=1.0 - b1)
            self.v.mul_(b2).addcmul_(gs, gs, value=1.0 - b2)
            denom = self.v.sqrt().div_(math.sqrt(1.0 - b2 ** t)).add_(self.eps)
            keep = 1.0 - lr * self.weight_decay * self._decay_elems()
            new = p * keep - (lr / (1.0 - b1 ** t)) * (self.m / denom)
        else:
            d = gs
            if self.weight_decay:
                d = d + self.weight_decay * p
            if mom is not None:
                mom.mul_(self.momentum).add_(d, alpha=1.0 - dampening)
                d = d + self.momentum * mom if self.nesterov else mom
            new = p - lr * d
        if acc is not None:
            acc.add_(new - p)
        p.copy_(new)
        if a.w16 is not None:
            a.w16.copy_(p)
        if self.ema is not None:
            _, D, O = ema_coeffs(self.ema_decay, self.ema_every, self.ema_warmup, t)
            self._ema_last = (D, O)
            if O != 0.0:
                self.ema.copy_(self.ema.mul(D).add(p.mul(O)))

    def _decay_elems(self) -> torch.Tensor:
        if getattr(self, "_decay_f", None) is None:
            self._decay_f = self.mask.to(torch.float32).repeat_interleave(ALIGN)
        return self._decay_f

    # ------------------------------------------------------------- checkpoint
    def state_dict(self) -> dict:
        sd = {"kind": self.kind, "t": self.t, "base_lr": self.base_lr,
              "schedule": asdict(self.schedule),
              "m": self.m.detach().cpu() if self.m is not None else None,
              "v": self.v.detach().cpu() if self.v is not None else None}
        if self.ema is not None:      # a run without EMA writes the keys it always wrote
            sd.update(ema=self.ema.detach().cpu(), ema_updates=self.ema_updates)
        return sd

    def load_state_dict(self, sd: dict):
        if sd.get("kind", self.kind) != self.kind:
            raise ValueError(f"checkpoint holds {sd['kind']!r} state, this optimizer is "
                             f"{self.kind!r}")
        with torch.no_grad():
            for name in ("m", "v"):
                if sd.get(name) is not None and getattr(self, name) is not None:
                    getattr(self, name).copy_(sd[name])
        if sd.get("schedule"):
            self.schedule = make_schedule(sd["schedule"])
        self.base_lr = float(sd.get("base_lr", self.base_lr))
        self._resync(int(sd.get("t", 0)))
        self._ema_last = (1.0, 0.0)
        # EMA state of a checkpoint is ignored with EMA off; a checkpoint without
        # it starts the average from the parameters that were just loaded
        if self.ema is not None:
            e = sd.get("ema")
            if e is not None and e.numel() == self.ema.numel():
                with torch.no_grad():
                    self.ema.copy_(e)
                if int(sd.get("ema_updates", 0)) != self._t // self.ema_every:
                    _LOG.warning("model EMA: the checkpoint counts %s EMA updates, step %d at "
                                 "interval %d gives %d; continuing with the latter",
                                 sd.get("ema_updates"), self._t, self.ema_every,
                                 self._t // self.ema_every)
            else:
                _LOG.warning("model EMA: the checkpoint holds no EMA of this arena; starting "
                             "the average from the loaded parameters")
                self.reset_ema()
