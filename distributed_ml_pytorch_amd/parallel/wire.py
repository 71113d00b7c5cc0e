"""The wire formats of a push, as codecs: fp32, bf16, MX8 (:mod:`.wire8`) and
sparse block top-k (:mod:`.wire_topk`).

Every client and server asks a codec how a push accumulator becomes a payload
(``handoff``), how large the payload of ``n`` elements is and what its header
says (``payload_shape``, ``header``), and how a payload lands in an fp32 master
(``apply``; ``apply_dc`` with delay compensation, :func:`dc_delta`).  On the GPU
these are the native kernels (``csrc/optim.hip``: one wire reader per dense
format, a scatter for top-k); on the CPU the torch expressions below, which the
kernels match bit for bit (``tests/test_wire_codec_gpu.py``,
``tests/test_wire_topk_gpu.py``).  The codecs hold
no state: :data:`FP32`, :data:`BF16`, :data:`MX8` and the one :func:`topk` codec
per K are shared by everyone.
"""
from __future__ import annotations

import torch

from . import messaging as M
from . import wire8, wire_topk


def _native():
    from ..ops._ext import native

    return native()


def _f32(x) -> torch.Tensor:
    """``x`` rounded to fp32 once, as a 0-dim CPU tensor (nothing below depends on
    how torch promotes a Python scalar)."""
    if torch.is_tensor(x):
        return x.reshape(-1)[0].to(device="cpu", dtype=torch.float32)
    return torch.tensor(x, dtype=torch.float32)


def dc_delta(d: torch.Tensor, master: torch.Tensor, bak: torch.Tensor, c) -> torch.Tensor:
    """The delay-compensated delta of DC-ASGD (Zheng et al., ICML 2017), the
    specification of the ``ps_apply_dc`` kernels::

        e = d - c * d*d * (master - bak)

    ``bak``: the parameters the pushing worker computed ``d`` from; ``c`` =
    ``lambda / (lr * n_push)``.  All fp32, one separately rounded torch operation
    per line; the kernels run the same operations in the same order with
    contraction off and give the same bits."""
    c = _f32(c)
    t = master - bak
    q = d * d
    r = q * t
    u = c * r
    return d - u


def _apply_dc_cpu(master: torch.Tensor, bak: torch.Tensor, d: torch.Tensor, scale, c, factor):
    """``master += sc * dc_delta(d)`` as two more separately rounded operations;
    ``sc = fp32(scale) * fp32(factor)``.  No ``add_(alpha=)``: that is free to fuse."""
    sc = _f32(scale)
    if factor is not None:
        sc = sc * _f32(factor)
    p = sc * dc_delta(d, master, bak[: master.numel()], c)
    master.copy_(master + p)


class _Dense:
    """One fp32 / bf16 element per element."""

    def __init__(self, dtype: torch.dtype):
        self.dtype = self.header = dtype        # payload dtype = the header's dtype field

    def payload_shape(self, n: int):
        """``(nelem, alloc, dtype)``: elements on the wire, elements of the buffer
        they land in (the apply kernels take whole float4 items), torch dtype."""
        return n, n + (-n) % 4, self.dtype

    def new_payload(self, n: int, device) -> torch.Tensor:
        return torch.empty(n, dtype=self.dtype, device=device)

    def handoff(self, acc: torch.Tensor, buf: torch.Tensor):
        """``buf = acc`` in the wire's dtype, ``acc = 0``."""
        if acc.is_cuda:
            outs = (buf, None) if self.dtype == torch.float32 else (None, buf)
            _native().push_handoff(acc, *outs)
        else:
            buf.copy_(acc)
            acc.zero_()

    def decode(self, payload: torch.Tensor, n: int) -> torch.Tensor:
        return payload[:n].to(torch.float32)

    def apply(self, master: torch.Tensor, payload: torch.Tensor, scale: float,
              atomic: bool = False, factor=None):
        """``master += scale [* factor] * payload``; ``atomic`` and ``factor``
        (a device slot of ``ps_stale_factor``) exist on the GPU only."""
        if master.is_cuda:
            _native().ps_apply(master, payload, None, scale, atomic, factor)
        else:
            master.add_(self.decode(payload, master.numel()), alpha=scale)

    def apply_dc(self, master: torch.Tensor, bak: torch.Tensor, payload: torch.Tensor,
                 scale: float, c: float, atomic: bool = False, factor=None):
        """The delay-compensated apply: ``master += scale [* factor] *
        dc_delta(payload, master, bak, c)``.  GPU: ``ps_apply_dc`` (``factor`` a
        device slot); CPU: ``decode`` plus the specification (``factor`` a number)."""
        if master.is_cuda:
            _native().ps_apply_dc(master, payload, bak, None, scale, c, atomic, factor)
        else:
            _apply_dc_cpu(master, bak, self.decode(payload, master.numel()), scale, c, factor)


class _MX8:
    """Block-scaled 8-bit payload: ``wire8.layout(n)`` bytes for ``n`` elements."""

    dtype = torch.uint8
    header = M.MX8

    def payload_shape(self, n: int):
        nbytes = wire8.layout(n)[2]         # no padding of its own
        return nbytes, nbytes, torch.uint8

    def new_payload(self, n: int, device) -> torch.Tensor:
        # zeroed once: the layout's pad bytes are never written again
        buf = torch.empty(wire8.layout(n)[2], dtype=torch.uint8, device=device)
        if buf.is_cuda:
            _native().zero_(buf)
        else:
            buf.zero_()
        return buf

    def handoff(self, acc: torch.Tensor, buf: torch.Tensor):
        """``buf = quantise(acc)``, ``acc = residual``: the rounding error of this
        push stays in the accumulator and travels with the next one."""
        if acc.is_cuda:
            _native().push_handoff_mx8(acc, buf)
        else:
            payload, resid = wire8.quantize(acc)
            buf.copy_(payload)
            acc.copy_(resid)

    def decode(self, payload: torch.Tensor, n: int) -> torch.Tensor:
        return wire8.dequantize(payload, n)

    def apply(self, master: torch.Tensor, payload: torch.Tensor, scale: float,
              atomic: bool = False, factor=None):
        if master.is_cuda:
            _native().ps_apply_mx8(master, payload, None, scale, atomic, factor)
        else:
            master.add_(self.decode(payload, master.numel()), alpha=scale)

    def apply_dc(self, master: torch.Tensor, bak: torch.Tensor, payload: torch.Tensor,
                 scale: float, c: float, atomic: bool = False, factor=None):
        if master.is_cuda:
            _native().ps_apply_dc_mx8(master, payload, bak, None, scale, c, atomic, factor)
        else:
            _apply_dc_cpu(master, bak, self.decode(payload, master.numel()), scale, c, factor)


class TopK:
    """Sparse block top-k payload (:mod:`.wire_topk`): ``k`` int32 words for every
    256 elements.  One instance per K (:func:`topk`).  ``k=None`` is the reader of
    an ``int32`` payload tensor whose K is not known beforehand: it consumes a
    payload at the K its size gives (``numel / nblk``; a size that does not
    divide is an error) and produces none."""

    dtype = torch.int32

    def __init__(self, k: int | None):
        self.k = None if k is None else wire_topk.check_k(k)

    @property
    def header(self):
        return M.topk(self._mine("header"))

    def _mine(self, what: str) -> int:
        if self.k is None:
            raise ValueError(f"wire.TopK.{what}: the reader of a top-k payload has no K of its "
                             "own; take the codec of a K (wire.topk(k))")
        return self.k

    def _k(self, payload: torch.Tensor, n: int) -> int:
        """K of ``payload`` for ``n`` elements; it must be this codec's when it has one."""
        if payload.dtype != torch.int32:
            raise ValueError(f"wire.TopK: a top-k payload is int32 words, got {payload.dtype}")
        k = wire_topk.k_of(payload.numel(), n)
        if self.k is not None and k != self.k:
            raise ValueError(f"wire.TopK: a payload at K = {k} reached the codec of K = {self.k}")
        return k

    def payload_shape(self, n: int):
        nwords = wire_topk.layout(n, self._mine("payload_shape"))[1]    # no padding of its own
        return nwords, nwords, torch.int32

    def new_payload(self, n: int, device) -> torch.Tensor:
        # zeroed once (an all-zero payload is the empty one); every hand-off rewrites all of it
        buf = torch.empty(self.payload_shape(n)[0], dtype=torch.int32, device=device)
        if buf.is_cuda:
            _native().zero_(buf)
        else:
            buf.zero_()
        return buf

    def handoff(self, acc: torch.Tensor, buf: torch.Tensor):
        """``buf = sparsify(acc)``, ``acc = residual``: what this push does not send
        stays in the accumulator and travels with a later one."""
        k = self._mine("handoff")
        if acc.is_cuda:
            _native().push_handoff_topk(acc, buf, k)
        else:
            payload, resid = wire_topk.sparsify(acc, k)
            buf.copy_(payload)
            acc.copy_(resid)

    def decode(self, payload: torch.Tensor, n: int) -> torch.Tensor:
        return wire_topk.densify(payload, n, self._k(payload, n))

    def apply(self, master: torch.Tensor, payload: torch.Tensor, scale: float,
              atomic: bool = False, factor=None):
        """``master[addr] += scale [* factor] * value`` for every word of the payload;
        every other element keeps its bits.  CPU: the product and the sum are two
        separately rounded torch operations, what the kernels compute."""
        k = self._k(payload, master.numel())
        if master.is_cuda:
            _native().ps_apply_topk(master, payload, None, scale, atomic, factor, k)
        else:
            at, val = wire_topk.entries(payload, master.numel(), k)
            sc = _f32(scale)
            if factor is not None:
                sc = sc * _f32(factor)
            p = sc * val
            master[at] = master[at] + p

    def apply_dc(self, master: torch.Tensor, bak: torch.Tensor, payload: torch.Tensor,
                 scale: float, c: float, atomic: bool = False, factor=None):
        """The delay-compensated apply on the touched elements, against ``bak[addr]``."""
        k = self._k(payload, master.numel())
        if master.is_cuda:
            _native().ps_apply_dc_topk(master, payload, bak, None, scale, c, atomic, factor, k)
        else:
            at, val = wire_topk.entries(payload, master.numel(), k)
            s = master[at]
            _apply_dc_cpu(s, bak[at], val, scale, c, factor)
            master[at] = s


FP32, BF16, MX8 = _Dense(torch.float32), _Dense(torch.bfloat16), _MX8()
_CODECS = {torch.float32: FP32, torch.bfloat16: BF16, M.MX8: MX8, torch.uint8: MX8}
_TOPK_READER = TopK(None)       # of an int32 payload tensor; the dtype alone names no wire


def topk(k: int) -> TopK:
    """The codec of the top-k wire at ``k`` slots per block (one shared instance per K)."""
    key = M.topk(k)
    if key not in _CODECS:
        _CODECS[key] = TopK(k)
    return _CODECS[key]


def codec(what):
    """The codec of a torch dtype, of a header's dtype field (:data:`.messaging.MX8`
    and the :func:`.messaging.topk` values included) or of a payload tensor
    (``uint8`` bytes are an MX8 payload, ``int32`` words a top-k payload)."""
    if torch.is_tensor(what) and what.dtype == torch.int32:
        return _TOPK_READER
    key = what.dtype if torch.is_tensor(what) else what
    if key == torch.float16 and key not in _CODECS:
        _CODECS[key] = _Dense(key)      # a CPU-only wire: the dense expressions in fp16
    if M.topk_k(key):
        return topk(M.topk_k(key))
    return _CODECS[key]


def copy_as(master: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """A copy of the master in ``dtype`` (``.to()`` of the same dtype would alias it)."""
    return master.clone() if master.dtype == dtype else master.to(dtype)


def warm_applies(master: torch.Tensor, codecs, scale: float, with_factor: bool,
                 atomic_only: bool, bak: torch.Tensor | None = None, dc: float = 0.0):
    """Launch every apply kernel a server may need once, on the current stream,
    before any transfer.  HIP loads a kernel's code object at its first launch,
    and that load waited for the work in flight: the first apply stalled every
    other link until the first receive had landed (tests/test_links_gpu.py).
    An all-zero payload leaves the master unchanged (MX8: codes 0 at scale
    2^-127 add +0; top-k: every slot is empty).  ``with_factor``: the damped forms too (policy "damp").
    ``bak`` (one worker's backup) and ``dc``: the server compensates delays, so
    the compensated forms are launched as well, for the same reason -- their
    first launch must not happen during a transfer either (a zero delta gives a
    zero compensated delta whatever the backup holds)."""
    factors = (None, torch.ones(2, device=master.device)) if with_factor else (None,)
    for c in codecs:
        _, alloc, dtype = c.payload_shape(master.numel())
        z = torch.zeros(alloc, dtype=dtype, device=master.device)
        for factor in factors:
            for atomic in ((True,) if atomic_only else (False, True)):
                c.apply(master, z, scale, atomic, factor)
                if bak is not None:
                    c.apply_dc(master, bak, z, scale, dc, atomic, factor)
