"""Model EMA: the part outside the optimizer pass, and evaluation on the average.

The exponential moving average of the parameters lives in the optimizer core
(:class:`~.fused_optim.FusedOptimCore`, ``core.ema``): the fused step kernels
update it from the new parameters they already hold, with the step's ``D`` /
``O`` scalars from the device-resident hyper block.  :class:`ModelEma` adds

* the model's floating-point buffers (BatchNorm running mean and variance, which
  are no part of the arena), averaged with the same ``D``, ``O`` and formula, as
  timm and torchvision do, by one ``ema_buffers`` launch over a device table
  right after the step (so a captured step captures it).  Integer buffers
  (``num_batches_tracked``, ``drop_path_step``) stay the live model's;
* :meth:`applied`, a context manager that exchanges parameters and buffers with
  their averages in place (``arena_swap``: the bf16 shadow is rewritten in the
  same pass), bumps the arena so that the transposed / padded weight shadows and
  the eval BatchNorm fold rebuild, and exchanges back on exit.  Two exchanges
  restore every bit.  No second model, no second arena.

A pull landing changes ``p32`` between two steps and is not an EMA event: the
average sees the landed values at its next update.  The parameter server keeps
no average, and the virtual workers (runtime/virtual.py) have none either.
"""
from __future__ import annotations

import contextlib
import logging

import torch

_LOG = logging.getLogger(__name__)


class ModelEma:
    def __init__(self, model: torch.nn.Module | None, core, client=None):
        """``core``: the optimizer core that owns the parameter average (EMA on).
        ``model`` None: parameters only.  ``client``: the optimizer's PS client,
        if any; :meth:`applied` refuses to run while it is in a compute half."""
        if core is None or core.ema is None:
            raise ValueError("ModelEma needs an optimizer core with ema_decay > 0")
        self.core = core
        self.arena = core.arena
        self.client = client
        self.names, self.live = [], []
        for name, b in (model.named_buffers() if model is not None else ()):
            if not b.is_floating_point():
                continue
            if b.dtype != torch.float32 or not b.is_contiguous() or b.device != core.ema.device:
                raise ValueError(f"model EMA averages contiguous fp32 buffers on the parameters' "
                                 f"device; {name} is {b.dtype} on {b.device}")
            self.names.append(name)
            self.live.append(b)
        dev = core.ema.device
        self.offsets, off = [], 0
        for b in self.live:
            self.offsets.append(off)
            off += b.numel()
        self.flat = torch.zeros(off, dtype=torch.float32, device=dev)
        self.table = None
        self._applied = False
        self.reset_buffers()
        if core.native is not None and self.live:
            self._ptrs = [b.data_ptr() for b in self.live]
            rows = [[p, o, b.numel()] for p, b, o in zip(self._ptrs, self.live, self.offsets)]
            self.table = torch.tensor(rows, dtype=torch.int64).to(dev)

    # ------------------------------------------------------------------ state
    def _views(self):
        return [self.flat[o:o + b.numel()].view(b.shape) for b, o in zip(self.live, self.offsets)]

    @torch.no_grad()
    def reset_buffers(self):
        """``EMA buffers <- live buffers`` (construction, a resume without EMA state)."""
        for b, v in zip(self.live, self._views()):
            v.copy_(b)

    def _check_table(self):
        # the table holds raw addresses: a buffer that was re-allocated since
        # (model.to(), an assignment) must fail here, not on the device.  Checked
        # at every exchange and when a step is captured, not on every eager step
        for name, b, ptr in zip(self.names, self.live, self._ptrs):
            if b.data_ptr() != ptr:
                raise RuntimeError(f"model EMA: buffer {name} moved since the EMA was built")

    # ------------------------------------------------------------------ update
    @torch.no_grad()
    def update_buffers(self):
        """Average the buffers with the ``D`` / ``O`` of the step ``core`` just
        applied.  Call right after ``core.step`` on the same stream."""
        if not self.live:
            return
        if self.table is not None:
            if torch.cuda.is_current_stream_capturing():
                self._check_table()       # a graph bakes the addresses in: check once, here
            self.core.native.ema_buffers(self.table, self.flat, self.core.hyper, 0)
            return
        D, O = self.core.ema_last()
        if O != 0.0:
            for b, v in zip(self.live, self._views()):
                v.copy_(v.mul(D).add(b.mul(O)))

    # -------------------------------------------------------------------- swap
    @torch.no_grad()
    def _exchange(self):
        a, e = self.arena, self.core.ema
        if self.core.native is not None:
            self.core.native.arena_swap(a.p32, e, a.w16)
            if self.table is not None:
                self._check_table()
                self.core.native.ema_buffers(self.table, self.flat, self.core.hyper, 1)
        else:
            tmp = a.p32.clone()
            a.p32.copy_(e)
            e.copy_(tmp)
            if a.w16 is not None:
                a.w16.copy_(a.p32)
            for b, v in zip(self.live, self._views()):
                tmp = b.clone()
                b.copy_(v)
                v.copy_(tmp)
        a.bump()

    @contextlib.contextmanager
    def applied(self):
        """Inside: the model computes with the averaged parameters and buffers.
        Not inside a graph capture (a replay would exchange again) and not between
        ``zero_grad`` and ``local_step`` of an asynchronous optimizer."""
        if self.core.native is not None and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ModelEma.applied() inside a graph capture")
        if self.client is not None and getattr(self.client, "in_compute", False):
            raise RuntimeError("ModelEma.applied() inside the compute half of a step "
                               "(between zero_grad and local_step)")
        if self._applied:
            raise RuntimeError("ModelEma.applied() is already active")
        self._exchange()
        self._applied = True
        try:
            yield self
        finally:
            self._exchange()
            self._applied = False

    # -------------------------------------------------------------- checkpoint
    def state_dict(self) -> dict:
        return {"names": list(self.names), "buffers": self.flat.detach().cpu()}

    def load_state_dict(self, sd: dict | None):
        """EMA buffers of a checkpoint; one without them (or of another model)
        re-initialises them from the live buffers, which were just loaded."""
        if sd and list(sd.get("names", ())) == self.names and \
                sd["buffers"].numel() == self.flat.numel():
            with torch.no_grad():
                self.flat.copy_(sd["buffers"])
            return
        if self.live:
            _LOG.warning("model EMA: the checkpoint holds no EMA of this model's buffers; "
                         "starting their average from the loaded buffers")
        self.reset_buffers()
