"""Sparse block top-k push wire with error feedback (``push_wire="topk"``).

The readable specification of the payload: pure torch, CPU.  The HIP kernels
(``csrc/optim.hip``: ``push_handoff_topk``, ``ps_apply_topk``,
``ps_apply_dc_topk``) produce and consume the same words bit for bit; the CPU
clients and servers use these functions directly.  Each push sends the ``K``
largest entries of every 256-element block of the accumulator and leaves the
rest (and the rounding error of what it sent) to ride into the next push
(Aji & Heafield 2017; Lin et al. 2018; Stich et al. 2018).  A fixed-rate
format: the payload size is known at start-up, nothing is counted or compacted.

**Blocks and K.**  A block is 256 consecutive elements of the flat accumulator;
a short last block is treated as if zero-padded.  ``K`` is in 1..32 (default 8).

**Payload.**  One ``torch.int32`` tensor of ``ceil(n / 256) * K`` words, K slots
per block in block order.  A word is ``(bf16_bits(v) << 16) | idx``: ``idx`` in
[0, 256) is the element's offset in its block, bits 8..15 are zero, and
``bf16_bits`` is torch's ``float32 -> bfloat16`` conversion (round to nearest
even, Inf stays Inf; every NaN is sent as the one quiet NaN ``0x7fc0``, which
torch's scalar conversion gives -- its vectorised one gives other NaN bits).

**Selection.**  The key of an element is its magnitude bits, ``bits(x) &
0x7fffffff``, compared as an unsigned integer: a total order that needs no
float compare, in which non-finite values sort first, NaN above Inf.  A larger
key wins, equal keys go to the lower index, and slot ``r`` of a block holds the
element of rank ``r``.  Elements with key 0 (+-0) are never selected, and
neither are the elements at or past ``n`` in the tail block.

**Empty slots.**  A block with fewer than K non-zero elements fills its
remaining slots with the word ``0``.

**Residual (error feedback).**  A selected element leaves ``x - float(bf16(x))``
in the accumulator.  This is exact in fp32 by the argument in
:mod:`.wire8`'s docstring: the sent value is ``x`` rounded to fewer bits, a
multiple of ``x``'s ulp between 0 and ``2 x``.  A selected non-finite element
leaves 0: the poison reaches the master as on the fp32 wire and does not stay
behind.  (A finite ``|x|`` above bf16's largest value is sent as Inf and leaves
``x - Inf``: it was about to overflow, and the next push carries the rest of
the poison.)  Unselected elements are untouched, bits included.

**Consumers skip zero values.**  Every consumer ignores a word whose value half
is +-0, ``(word & 0x7fff0000) == 0``.  This covers empty slots, and a selected
fp32 subnormal that rounds to bf16 zero (its residual is then ``x`` itself,
which is consistent).  The rule is what keeps an empty slot (``idx`` 0) from
colliding with a real entry at offset 0 of the same block.

**Consumers ignore out-of-range addresses.**  Every consumer ignores a word
whose address ``block * 256 + idx`` is ``>= n`` (``idx`` is the low 8 bits; a
consumer does not look at bits 8..15).  A payload arrives off a wire, and a
malformed one must not write outside the shard.  Addresses within one
well-formed payload are distinct; a payload with duplicate addresses is
malformed, and only an accumulating consumer (the atomic apply) defines it.

On the CPU the selection is a descending sort of ``key * 256 + (255 - idx)``:
these sort keys are unique, so the result does not depend on how
``torch.topk`` breaks ties.
"""
from __future__ import annotations

import torch

BLOCK = 256
K_MAX = 32
K_DEFAULT = 8


def check_k(k) -> int:
    if isinstance(k, bool) or int(k) != k or not 1 <= int(k) <= K_MAX:
        raise ValueError(f"push_topk must be an integer in 1..{K_MAX}, got {k!r}")
    return int(k)


def layout(n: int, k: int):
    """``(nblk, nwords)``: blocks of ``n`` elements and int32 words of their payload."""
    n, k = int(n), check_k(k)
    if n < 0:
        raise ValueError("wire_topk.layout: negative element count")
    nblk = (n + BLOCK - 1) // BLOCK
    return nblk, nblk * k


def k_of(nwords: int, n: int) -> int:
    """The K of a payload of ``nwords`` words for ``n`` elements; a size that is
    not ``ceil(n / 256) * K`` for a K in 1..32 is an error, never a guess."""
    nblk = (int(n) + BLOCK - 1) // BLOCK
    k, rem = divmod(int(nwords), nblk) if nblk else (0, 1)
    if rem or not 1 <= k <= K_MAX:
        raise ValueError(f"wire_topk: {nwords} payload words are no whole K in 1..{K_MAX} "
                         f"slots for each of the {nblk} blocks of {n} elements")
    return k


def sparsify(acc: torch.Tensor, k: int):
    """``acc`` (fp32, any shape, CPU) -> ``(payload int32 [nblk * k], residual fp32 [n])``."""
    x = acc.detach().reshape(-1).to(torch.float32).contiguous()
    n = x.numel()
    nblk, nwords = layout(n, k)
    if n == 0:
        return torch.zeros(0, dtype=torch.int32), x.clone()
    xb = torch.zeros(nblk * BLOCK, dtype=torch.float32)
    xb[:n] = x                                       # the padding has key 0: never selected
    xb = xb.view(nblk, BLOCK)
    key = (xb.view(torch.int32) & 0x7FFFFFFF).to(torch.int64)
    idx = torch.arange(BLOCK, dtype=torch.int64)
    top = torch.topk(key * BLOCK + (BLOCK - 1 - idx), k, dim=1, largest=True, sorted=True).values
    sel = (top >> 8) > 0
    at = BLOCK - 1 - (top & 0xFF)
    v = torch.gather(xb, 1, at)
    sent = v.to(torch.bfloat16)
    half = sent.view(torch.int16).to(torch.int64) & 0xFFFF
    # one NaN on the wire: torch's vectorised and scalar conversions differ in its bits
    half = torch.where(torch.isnan(v), torch.full_like(half, 0x7FC0), half)
    word = (half << 16) | at
    word = torch.where(word >= 2 ** 31, word - 2 ** 32, word)      # as a two's-complement int32
    payload = torch.where(sel, word, torch.zeros_like(word)).to(torch.int32)
    left = torch.where(torch.isfinite(v), v - sent.to(torch.float32), torch.zeros_like(v))
    resid = xb.clone()
    rows = torch.arange(nblk, dtype=torch.int64).unsqueeze(1).expand_as(at)
    resid[rows[sel], at[sel]] = left[sel]
    return payload.reshape(-1), resid.reshape(-1)[:n].clone()


def entries(payload: torch.Tensor, n: int, k: int):
    """``(addr int64, value fp32)`` of the words a consumer applies: both skip
    rules taken (zero value, address ``>= n``).  ``ValueError`` on a wrong dtype
    or size."""
    n = int(n)
    nblk, nwords = layout(n, k)
    payload = payload.detach().reshape(-1)
    if payload.dtype != torch.int32 or payload.numel() != nwords:
        raise ValueError(f"wire_topk: a payload of {n} elements at K = {k} is {nwords} int32 "
                         f"words, got {payload.numel()} of {payload.dtype}")
    payload = payload.cpu()
    block = torch.arange(nblk, dtype=torch.int64).repeat_interleave(int(k))
    addr = block * BLOCK + (payload & 0xFF).to(torch.int64)
    keep = ((payload & 0x7FFF0000) != 0) & (addr < n)
    val = (payload & -65536).view(torch.float32)                  # the bf16 value, widened
    return addr[keep], val[keep]


def densify(payload: torch.Tensor, n: int, k: int) -> torch.Tensor:
    """The fp32 values a payload of ``n`` elements carries, zero where it is silent."""
    addr, val = entries(payload, n, k)
    out = torch.zeros(int(n), dtype=torch.float32)
    out[addr] = val
    return out
