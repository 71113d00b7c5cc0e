"""Where a native backward puts a parameter's fp32 gradient.

A parameter that lives in a ``parallel.arena.FlatArena`` (``p._dmp_arena``
set) has ``p.grad`` as a view of the arena's flat grad buffer: the kernel
accumulates straight into it and autograd gets ``None`` for that input (no
per-parameter grad tensor, no AccumulateGrad copy).  Once the kernel
is enqueued the arena is told the gradient is final through
``p._dmp_grad_ready`` (sync-DP launches its bucket all-reduces from that call).
Any other parameter gets a zeroed temporary that is reshaped, cast and
returned to autograd.  This module is the only place in ``ops`` that knows the
rule; it is pure torch and works on CPU tensors.

A parameter that does not need a gradient gets neither a write nor a notify,
arena or not: a frozen arena parameter's slot stays untouched (the fused
optimizer would otherwise apply whatever a backward accumulated there).
"""
from __future__ import annotations

import torch

CL = torch.channels_last


def notify(*ps):
    """Tell the arena that each parameter's gradient is final."""
    for p in ps:
        cb = getattr(p, "_dmp_grad_ready", None) if p is not None else None
        if cb is not None:
            cb(p)


class GradSink:
    """The buffer a backward kernel accumulates parameter ``p``'s gradient into.

    ``layout`` is what the kernel needs of an arena grad view (else a temporary):

    * ``"any"``: ``p.grad`` as it is;
    * ``"cl"``: 4-D and channels-last contiguous; the temporary is channels-last
      zeros of ``p.shape``;
    * ``"rows"``: a GEMM output -- a channels-last 4-D grad as its
      ``[CO, R*S*CI]`` view (same storage), a contiguous grad as it is; the
      temporary of a 4-D parameter is ``[CO, R*S*CI]``, folded back by ``done``.

    ``dtype`` is the temporary's (None: the parameter's own).  ``buf`` is None
    when no gradient is needed; ``arena`` says ``buf`` aliases ``p.grad``;
    ``hooked`` that a ready callback waits for it.
    """

    def __init__(self, p, needed, layout="any", dtype=torch.float32):
        self.p, self.buf, self.arena = p, None, False
        if p is None or not needed:
            return
        g = p.grad if getattr(p, "_dmp_arena", False) else None
        if g is not None and layout != "any":
            cl = g.dim() == 4 and g.is_contiguous(memory_format=CL)
            if layout == "rows" and cl:
                g = g.permute(0, 2, 3, 1).reshape(g.shape[0], -1)
            elif not (cl if layout == "cl" else g.is_contiguous()):
                g = None
        if g is not None:
            self.buf, self.arena = g, True
            return
        shape = (p.shape[0], p[0].numel()) if layout == "rows" and p.dim() == 4 else p.shape
        fmt = CL if layout == "cl" and p.dim() == 4 else torch.contiguous_format
        self.buf = torch.empty(shape, dtype=dtype or p.dtype, device=p.device,
                               memory_format=fmt).zero_()

    @property
    def hooked(self) -> bool:
        return self.arena and getattr(self.p, "_dmp_grad_ready", None) is not None

    def done(self):
        """Call once the kernels writing ``buf`` are enqueued: the gradient to
        return to autograd (None when it went into the arena, or is not needed)."""
        if self.buf is None:
            return None
        if self.arena:
            notify(self.p)
            return None
        g, p = self.buf, self.p
        if g.shape != p.shape:          # "rows" of a conv weight: (r, s, ci) columns
            g = g.view(p.shape[0], p.shape[2], p.shape[3], p.shape[1]).permute(0, 3, 1, 2)
        return g.to(p.dtype)
