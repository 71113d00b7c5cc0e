"""Block-scaled 8-bit push wire (OCP MXFP8: E4M3 codes, one E8M0 scale per 32).

The readable specification of the ``push_wire="mx8"`` payload: pure torch, CPU.
The HIP kernels (``csrc/optim.hip``: ``push_handoff_mx8``, ``ps_apply_mx8``)
produce and consume the same bytes bit for bit; the CPU clients and servers
use these functions directly.

Payload of ``n`` elements, one ``uint8`` tensor (:func:`layout`)::

    [0, n)                        E4M3 (``e4m3fn``) code bytes
    [scales_off, + ceil(n / 32))  E8M0 scale bytes, scales_off = n rounded up to 16
    total padded to a multiple of 4 (pad bytes are zero)

Per block of 32 consecutive elements (a short last block as if zero-padded):

* ``sb = clamp(E(amax) - 8, 0, 254)`` with ``E(amax)`` the biased fp32 exponent
  field of the block's largest magnitude: the scale is ``2^(sb - 127)``, the OCP
  MX rule with E4M3's ``emax = 8``;
* ``code = e4m3fn(clamp(x * 2^-(sb - 127), -448, 448))``, round to nearest even.
  The clamp is part of the format: the largest magnitude scales into
  [256, 512) and E4M3 ends at 448 (``torch.float8_e4m3fn`` gives NaN above it);
* ``residual = x - dequant(code, sb)`` stays in the push accumulator (error
  feedback: the next push carries it).  This subtraction is EXACT in fp32 (the
  tests rely on it): the dequantised value is ``x`` rounded to fewer bits at a
  coarser quantum, so it is a multiple of ``x``'s ulp, lies between 0 and
  ``2 x``, and the difference is a multiple of that ulp no larger than ``|x|``.
  A value in the saturating band (scaled magnitude in (448, 512)) leaves a
  remainder below 64 quanta (``64 * 2^(sb - 127)``); everything else at most
  half a unit of its E4M3 binade (``2^-10`` quanta in the subnormal range);
* an all-zero block has ``sb = 0`` and codes 0;
* a block holding a non-finite value is sent as ``sb = 0xFF`` (E8M0 NaN) with
  codes 0: it dequantises to NaN in every element and its residual is 0, so a
  diverged worker poisons the master exactly as it does on the fp32 wire.

All scaling goes through ``ldexp``: ``2^-127`` is an fp32 subnormal, and a
constructed reciprocal would depend on the denormal mode.
"""
from __future__ import annotations

import torch

BLOCK = 32
E4M3_MAX = 448.0
SCALE_NAN = 0xFF


def layout(n: int):
    """``(codes_off, scales_off, nbytes)`` of the payload of ``n`` elements."""
    n = int(n)
    if n < 0:
        raise ValueError("wire8.layout: negative element count")
    nblk = (n + BLOCK - 1) // BLOCK
    scales_off = (n + 15) // 16 * 16
    nbytes = (scales_off + nblk + 3) // 4 * 4
    return 0, scales_off, nbytes


def _blocks(flat: torch.Tensor, n: int) -> torch.Tensor:
    nblk = (n + BLOCK - 1) // BLOCK
    if nblk * BLOCK == n:
        return flat.reshape(nblk, BLOCK)
    pad = torch.zeros(nblk * BLOCK, dtype=flat.dtype)
    pad[:n] = flat
    return pad.view(nblk, BLOCK)


def quantize(acc: torch.Tensor):
    """``acc`` (fp32, any shape, CPU) -> ``(payload uint8, residual fp32 [n])``."""
    x = acc.detach().reshape(-1).to(torch.float32).contiguous()
    n = x.numel()
    _, so, nbytes = layout(n)
    payload = torch.zeros(nbytes, dtype=torch.uint8)
    if n == 0:
        return payload, x.clone()
    xb = _blocks(x, n)
    mag = xb.contiguous().view(torch.int32) & 0x7FFFFFFF
    e = mag.max(dim=1).values >> 23                  # biased exponent of the block amax
    bad = (e == 255).unsqueeze(1)                    # inf / NaN somewhere in the block
    sb = (e - 8).clamp(0, 254)
    down = (127 - sb).unsqueeze(1)                   # x * 2^-(sb - 127)
    scaled = torch.ldexp(torch.where(bad, torch.zeros_like(xb), xb), down)
    codes = scaled.clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)
    deq = torch.ldexp(codes.to(torch.float32), -down)
    resid = torch.where(bad, torch.zeros_like(xb), xb - deq)
    sb = torch.where(bad.squeeze(1), torch.full_like(sb, SCALE_NAN), sb)
    payload[:n] = codes.view(torch.uint8).reshape(-1)[:n]
    payload[so: so + sb.numel()] = sb.to(torch.uint8)
    return payload, resid.reshape(-1)[:n].clone()


def dequantize(payload: torch.Tensor, n: int) -> torch.Tensor:
    """The fp32 values a payload of ``n`` elements carries."""
    n = int(n)
    _, so, nbytes = layout(n)
    payload = payload.detach().reshape(-1)
    if payload.dtype != torch.uint8 or payload.numel() != nbytes:
        raise ValueError(f"wire8.dequantize: a payload of {n} elements is {nbytes} uint8 bytes, "
                         f"got {payload.numel()} of {payload.dtype}")
    payload = payload.cpu()
    if n == 0:
        return torch.zeros(0, dtype=torch.float32)
    nblk = (n + BLOCK - 1) // BLOCK
    codes = _blocks(payload[:n].view(torch.float8_e4m3fn).to(torch.float32), n)
    sb = payload[so: so + nblk].to(torch.int32).unsqueeze(1)
    val = torch.ldexp(codes, sb - 127)
    val = torch.where(sb == SCALE_NAN, torch.full_like(val, float("nan")), val)
    return val.reshape(-1)[:n].clone()
