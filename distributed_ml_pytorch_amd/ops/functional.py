"""Autograd-level ops over the gfx950 kernels.

GPU tensors run the hand-written HIP kernels (``_native``); CPU tensors run
the PyTorch formulation of the same math, which doubles as the test oracle.

Where each backward puts its parameter gradients (the arena's flat grad buffer
or a returned tensor) is decided by :class:`._grads.GradSink`.
"""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F
from torch.autograd import Function

from ._ext import native
from ._grads import GradSink, notify
from ._policy import stock_gpu

CL = torch.channels_last


# ----------------------------------------------------- ReLU-mask hand-offs
# A layer with a fused ReLU (conv / linear epilogue) masks its incoming gradient
# by relu'(y) in its backward.  When the gradient's producer already applied
# that mask -- a max-pool over the non-negative ReLU output (a window whose max
# is <= 0 passes no gradient), or a Linear whose data-gradient epilogue masks
# by its own ReLU'd input (EPI_DRELU) -- it registers the gradient tensor
# here, dropout's backward forwards the registration, and the layer skips its
# mask pass.  The mark is an attribute of the tensor OBJECT holding its version
# counter at marking time: a gradient that autograd accumulated or copied is a
# different object, and one that autograd's InputBuffer accumulated a second
# consumer's gradient into IN PLACE has a bumped version -- both are masked as
# usual (masking twice is a no-op anyway, skipping a needed mask is not).
def mark_relu_masked(t):
    if t is not None:
        t._dmp_relu_masked_ver = t._version
    return t


def is_relu_masked(t) -> bool:
    return t is not None and getattr(t, "_dmp_relu_masked_ver", None) == t._version


# ------------------------------------------------ deferred residual-gradient mask
# The backward of a BatchNorm + residual + ReLU (bn2 of a BasicBlock) owes its
# residual input dres = dY * relu'(.): an activation-sized write (67 MB at the
# ResNet-18 bs512 stage 1) that the residual's consumer reads straight back.  When
# the block marks the residual as consumed ONLY by that BatchNorm
# (``mark_residual_only``) and it was produced by a consumer that understands the
# hand-off -- the alias output of a native conv (its dgrad adds the gradient in
# the epilogue) or a native BatchNorm (its backward reduce / apply mask dY) --
# the BN backward skips dres and passes dY itself with its 1-bit ReLU mask
# attached; the consumer applies the mask where it reads the gradient
# (csrc/conv.hip ConvArgs::addmask, or bn.hip's mode-3 kernels).  Any other
# path materialises the masked tensor first (``resolve_deferred``).
_BN_DEFER_RES = os.environ.get("DMP_BN_DEFER_RES", "1") != "0"
# hand-offs by outcome (diagnostics / tests): made, masked inside a native
# consumer kernel, materialised by apply_bitmask
DEFER_RES_STATS = {"deferred": 0, "native": 0, "materialized": 0}


def mark_residual_only(t):
    """Declare that ``t`` is consumed only as a BatchNorm residual (single use)."""
    if t is not None:
        t._dmp_residual_only = True
    return t


def defer_tag(t, mask):
    t._dmp_defer_mask = (mask, t._version)
    return t


def deferred_mask(t):
    """The ReLU bit mask still owed by gradient ``t`` (None: ``t`` is final)."""
    tag = getattr(t, "_dmp_defer_mask", None) if t is not None else None
    if tag is None:
        return None
    if tag[1] != t._version:
        # single use was declared: nothing may accumulate into the hand-off
        raise RuntimeError("deferred residual gradient was modified in place")
    return tag[0]


def apply_bitmask(t, mask):
    """``t * bit`` of the [pixels, C/8] uint8 ReLU mask (channels_last NCHW ``t``)."""
    DEFER_RES_STATS["materialized"] += 1
    N, C, H, W = t.shape
    rows = t.permute(0, 2, 3, 1).contiguous().view(-1, 8)
    shifts = torch.arange(8, dtype=torch.uint8, device=t.device)
    keep = ((mask.view(-1, 1) >> shifts) & 1).bool()
    out = torch.where(keep, rows, torch.zeros((), dtype=t.dtype, device=t.device))
    return out.view(N, H, W, C).permute(0, 3, 1, 2)


def apply_bitmask_rows(t, mask):
    """``apply_bitmask`` for a dense row-major [M, N] (N % 8 == 0) operand."""
    DEFER_RES_STATS["materialized"] += 1
    rows = t.contiguous().view(-1, 8)
    shifts = torch.arange(8, dtype=torch.uint8, device=t.device)
    keep = ((mask.view(-1, 1) >> shifts) & 1).bool()
    return torch.where(keep, rows, torch.zeros((), dtype=t.dtype, device=t.device)).view(t.shape)


def resolve_deferred(t):
    m = deferred_mask(t)
    return t if m is None else apply_bitmask(t, m)


def nonneg(t) -> bool:
    """``t`` is known >= 0 (the output of a fused ReLU, or a dropout of one)."""
    return bool(getattr(t, "_dmp_nonneg", False))


def set_nonneg(t, flag: bool = True):
    if flag and t is not None:
        t._dmp_nonneg = True
    return t


# --------------------------------------------------------------- shadow weight
class _ShadowWeight(Function):
    """Use the arena's bf16 shadow of an fp32 master parameter in compute.

    Forward returns the pre-cast bf16 shadow (refreshed by the fused optimizer
    kernel each step, so no per-step cast).  Backward folds the bf16 weight
    gradient into the fp32 master grad in place.
    """

    @staticmethod
    def forward(ctx, p, w16):
        ctx.p = p
        return w16.view_as(w16)

    @staticmethod
    def backward(ctx, g):
        p = ctx.p
        if p.grad is None:
            return g.to(p.dtype), None
        p.grad.add_(g)
        notify(p)
        return None, None


def compute_weight(p: torch.Tensor | None, dtype: torch.dtype):
    if p is None:
        return None
    if p.dtype == dtype:
        return p
    w16 = getattr(p, "_dmp_w16", None)
    if w16 is not None and dtype == w16.dtype and p.requires_grad and torch.is_grad_enabled():
        return _ShadowWeight.apply(p, w16)
    if w16 is not None and dtype == w16.dtype:
        return w16
    return p.to(dtype)


# --------------------------------------------------------------- cross entropy
_UNIT = {}          # device -> persistent fp32 scalar 1.0 (the loss's seed gradient)


def unit_grad(like: torch.Tensor) -> torch.Tensor:
    """A persistent ``1.0`` to seed ``loss.backward(unit_grad(loss))`` with: the
    cross-entropy backward recognises it (by storage) and hands back its
    precomputed dlogits untouched -- no ones-fill, cast and multiply kernels per
    step (autograd's default seed is a fresh ``ones_like``)."""
    key = (like.device, like.dtype)
    u = _UNIT.get(key)
    if u is None:
        u = torch.ones((), dtype=like.dtype, device=like.device)
        _UNIT[key] = u
    return u


def _is_unit(g) -> bool:
    u = _UNIT.get((g.device, g.dtype))
    return u is not None and g.data_ptr() == u.data_ptr() and g.dim() == 0


class _SoftmaxXent(Function):
    @staticmethod
    def forward(ctx, logits, labels, smoothing, ignore_index):
        ctx.set_materialize_grads(False)
        loss, hits, dlogits = native().softmax_xent(logits.contiguous(), labels.contiguous(), True,
                                                    float(smoothing), int(ignore_index))
        ctx.save_for_backward(dlogits)
        ctx.mark_non_differentiable(hits)
        return loss, hits

    @staticmethod
    def backward(ctx, gloss, ghits):
        (dlogits,) = ctx.saved_tensors
        if gloss is None:
            return None, None, None, None
        if _is_unit(gloss):
            return dlogits, None, None, None
        return dlogits * gloss.to(dlogits.dtype), None, None, None


def softmax_cross_entropy(logits, labels, label_smoothing: float = 0.0, ignore_index: int = -100):
    """Mean cross-entropy; returns ``(loss, hits)`` with hits = #top-1 correct.

    Reference: ``F.cross_entropy`` + ``torch.max`` at /root/reference/example/main.py:71,75.
    """
    if logits.is_cuda:
        return _SoftmaxXent.apply(logits, labels, label_smoothing, ignore_index)
    loss = F.cross_entropy(logits.float(), labels, label_smoothing=label_smoothing,
                           ignore_index=ignore_index)
    with torch.no_grad():
        valid = labels != ignore_index
        hits = ((logits.argmax(1) == labels) & valid).sum().to(torch.int32)
    return loss, hits


class _SoftmaxXentMix(Function):
    @staticmethod
    def forward(ctx, logits, labels, labels2, lam, smoothing, ignore_index):
        ctx.set_materialize_grads(False)
        loss, hits, dlogits = native().softmax_xent_mix(
            logits.contiguous(), labels.contiguous(), labels2.contiguous(), lam.contiguous(), True,
            float(smoothing), int(ignore_index))
        ctx.save_for_backward(dlogits)
        ctx.mark_non_differentiable(hits)
        return loss, hits

    @staticmethod
    def backward(ctx, gloss, ghits):
        (dlogits,) = ctx.saved_tensors
        if gloss is None:
            return (None,) * 6
        if _is_unit(gloss):
            return (dlogits,) + (None,) * 5
        return (dlogits * gloss.to(dlogits.dtype),) + (None,) * 5


def softmax_cross_entropy_mix(logits, y, y2, lam, label_smoothing: float = 0.0,
                              ignore_index: int = -100):
    """Mean two-target cross-entropy of the mixed batches (Mixup / CutMix,
    utils/device_data.py); returns ``(loss, hits)``.  Per row::

        loss_r = (1 - eps) (lam_r (lse - x_y) + (1 - lam_r) (lse - x_y2)) + eps (lse - mean x)

    with ``lam`` float32 [B].  A row is valid iff both labels are (not
    ``ignore_index``, inside ``[0, C)``); invalid rows add no loss, no gradient
    and no hit and are left out of the mean.  A target of weight exactly 0 is not
    formed.  Hits compare the argmax with ``y`` where ``lam >= 0.5``, else ``y2``.
    At ``lam == 1`` everywhere this is :func:`softmax_cross_entropy` bit for bit."""
    if logits.is_cuda:
        return _SoftmaxXentMix.apply(logits, y, y2, lam, label_smoothing, ignore_index)
    x = logits.float()
    c = x.shape[1]
    ok1 = (y != ignore_index) & (y >= 0) & (y < c)
    ok2 = (y2 != ignore_index) & (y2 >= 0) & (y2 < c)
    valid = ok1 & ok2
    t1 = torch.where(valid, y, torch.full_like(y, ignore_index))
    t2 = torch.where(valid, y2, torch.full_like(y2, ignore_index))
    lam = lam.to(x.dtype)
    wl = 1 - lam
    # label_smoothing is applied once, outside the two target terms
    nll1 = F.cross_entropy(x, t1, ignore_index=ignore_index, reduction="none")
    nll2 = F.cross_entropy(x, t2, ignore_index=ignore_index, reduction="none")
    zero = torch.zeros_like(nll1)
    rows = torch.where(lam != 0, lam * nll1, zero) + torch.where(wl != 0, wl * nll2, zero)
    if label_smoothing > 0:
        smooth = torch.logsumexp(x, 1) - x.mean(1)
        rows = (1 - label_smoothing) * rows + label_smoothing * smooth
    rows = torch.where(valid, rows, zero)
    loss = rows.sum() / valid.sum().clamp(min=1).to(x.dtype)
    with torch.no_grad():
        tgt = torch.where(lam >= 0.5, y, y2)
        hits = ((logits.argmax(1) == tgt) & valid).sum().to(torch.int32)
    return loss, hits


# ------------------------------------------------------------------ batchnorm
# (running the backward reduce inside the consuming conv's dgrad epilogue was
# tried and measured a loss: profiles/bn_bwd_fusion_r2.txt)
_BN_BITMASK = os.environ.get("DMP_BN_BITMASK", "1") != "0"   # backward passes by path (diagnostics)
# BatchNorm finalize folded into the apply passes (csrc/bn.hip fold kernels): no
# separate finalize launch per BN and direction.  Slot hygiene: the forward apply
# zeroes the layer's backward slots and the backward apply the forward slot sums
# it read, so a buffer left holding sums (an unpaired pass) is flagged
# dirty (``mark_slots``) and zeroed by the next producer (``ops.conv.bn_slot_buffer``) or
# backward before it accumulates again.
_BN_FOLD = os.environ.get("DMP_BN_FOLD", "1") != "0"
# data_ptrs of slot buffers holding sums nobody will zero (keyed by storage, not
# by Python object: a buffer comes back from an autograd Function as a new
# wrapper of the same storage)
_SLOTS_DIRTY: set = set()


def mark_slots(buf, dirty: bool):
    if dirty:
        _SLOTS_DIRTY.add(buf.data_ptr())
    else:
        _SLOTS_DIRTY.discard(buf.data_ptr())


def clean_slots(buf):
    """Zero ``buf`` if it holds leftover sums (see ``_BN_FOLD``)."""
    if buf.data_ptr() in _SLOTS_DIRTY:
        if buf.is_cuda:
            native().zero_(buf)      # native fill kernel, not an ATen memset
        else:
            buf.zero_()
        _SLOTS_DIRTY.discard(buf.data_ptr())
    return buf


def _fresh_slots(buf, C, device):
    if buf is None:
        return torch.zeros(2 * 64 * C + 4, dtype=torch.float32, device=device)
    return clean_slots(buf)


class _BNAct(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, residual, running_mean, running_var, training, momentum, eps,
                relu, part=None, slots=None, stem=None):
        res_handoff = residual is not None and bool(
            getattr(residual, "_dmp_residual_only", False)
            and (getattr(residual, "_dmp_bn_out", False) or getattr(residual, "_dmp_conv_alias", False)))
        if x.dim() == 4:
            x = x.contiguous(memory_format=CL)
            if residual is not None:
                residual = residual.contiguous(memory_format=CL)
        # BN + residual + ReLU: the backward's ReLU mask depends on the residual;
        # keep it as 1 bit per element (written by the apply) instead of y
        want_mask = bool(relu and residual is not None and _BN_BITMASK)
        ctx.fold = bool(_BN_FOLD and training and x.is_cuda)
        ctx.fpart = None
        if ctx.fold:
            C = x.shape[1]
            bslots = slots[1] if slots is not None else None
            src = part if part is not None else _fresh_slots(
                slots[0] if slots is not None else None, C, x.device)
            y, stats, mask = native().bn_fwd_fold(
                x, src, part is not None, residual, gamma, beta, running_mean, running_var,
                float(momentum), float(eps), bool(relu), want_mask, bslots)
            mark_slots(src, True)          # read here, zeroed by the backward apply
            if bslots is not None:
                mark_slots(bslots, False)  # zeroed by this apply
            ctx.fpart = src
        elif part is not None and training:
            if slots is not None:          # sums a folded pass left behind (mode switch)
                clean_slots(slots[1])
            # statistics already reduced per block by the producing conv's epilogue
            C = x.shape[1]
            y, stats, mask = native().bn_fwd_from_partials(
                x, part, (part.numel() - 4) // (2 * C), residual, gamma, beta, running_mean,
                running_var, float(momentum), float(eps), bool(relu), want_mask)
        else:
            if slots is not None and training:
                clean_slots(slots[0])
                clean_slots(slots[1])
            y, stats, mask = native().bn_fwd(x, residual, gamma, beta, running_mean, running_var,
                                             float(momentum), float(eps), bool(training),
                                             bool(relu), slots[0] if slots is not None else None,
                                             want_mask)
        ctx.bslots = slots[1] if slots is not None else None
        ctx.relu = relu
        ctx.training = bool(training)      # False: running statistics, dx = k1 * dz
        ctx.has_res = residual is not None
        # dres handed over unmasked with the bit mask (see deferred residual mask)
        ctx.defer_res = bool(_BN_DEFER_RES and ctx.fold and res_handoff and mask is not None
                             and x.dim() == 4)
        y._dmp_bn_out = True
        ctx.gamma, ctx.beta = gamma, beta
        # one-pass stem backward: folded training BN + ReLU, no residual, 4-D input
        # straight from the MFMA stem conv
        ctx.stem = stem if (ctx.fold and relu and residual is None and x.dim() == 4
                            and ctx.fpart is part and part is not None) else None
        # the backward re-derives the ReLU mask from x and the folded scale/shift
        # unless a residual entered the forward (then the bit mask, or y)
        ctx.save_for_backward(x, y if (relu and residual is not None and mask is None) else None,
                              stats, mask)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, stats, mask = ctx.saved_tensors
        gamma, beta = ctx.gamma, ctx.beta
        # a residual hand-off from the BatchNorm this one feeds: ReLU-free folded
        # passes take the owed mask as their own (mode 3); others materialise it
        in_mask = deferred_mask(dy)
        if in_mask is not None and not (ctx.fold and not ctx.relu and not ctx.has_res):
            dy, in_mask = apply_bitmask(dy, in_mask), None
        sg = GradSink(gamma, ctx.needs_input_grad[1], dtype=None)
        sb = GradSink(beta, ctx.needs_input_grad[2], dtype=None)
        dg, db = sg.buf, sb.buf
        stem = ctx.stem
        if stem is not None and in_mask is None:
            # dgamma, dbeta and the stem conv's weight gradient from one pass over
            # dy and x; no dx (the stem's input is data).  The conv's backward finds
            # its weight sink in the hand-off and launches nothing.
            dy = dy.contiguous(memory_format=CL)
            sw = GradSink(stem.master, stem.master is not None and stem.master.requires_grad,
                          "cl")
            native().stem3_bn_bwd(dy, x, stem.x, stats, gamma, dg, db, sw.buf, stem.scratch,
                                  ctx.fpart)
            mark_slots(ctx.fpart, False)       # zeroed by the finalize kernel
            ctx.fpart = None
            return (stem.give(dy, sw), sg.done(), sb.done(), None, None, None, None, None, None,
                    None, None, None, None)
        if ctx.fold:
            if x.dim() == 4:
                dy = dy.contiguous(memory_format=CL)
            else:
                dy = dy.contiguous()
            bs = _fresh_slots(ctx.bslots, x.shape[1], x.device)
            if in_mask is not None:
                DEFER_RES_STATS["native"] += 1
                dx, dres = native().bn_bwd_fold(x, dy, None, gamma, stats, dg, db, True, False,
                                                bs, in_mask, ctx.fpart)
            else:
                dx, dres = native().bn_bwd_fold(x, dy, y, gamma, stats, dg, db, ctx.relu,
                                                ctx.has_res and not ctx.defer_res, bs, mask,
                                                ctx.fpart)
                if ctx.defer_res:
                    dres = defer_tag(dy, mask)
                    DEFER_RES_STATS["deferred"] += 1
            mark_slots(bs, True)
            mark_slots(ctx.fpart, False)
            ctx.fpart = None
        else:
            if x.dim() == 4:
                dy = dy.contiguous(memory_format=CL)
            else:
                dy = dy.contiguous()
            if ctx.bslots is not None:
                # an eval-mode backward after a folded training step: the sums that
                # step's backward left here would be added to dgamma / dbeta
                clean_slots(ctx.bslots)
            dx, dres = native().bn_bwd(x, dy, y, gamma, stats, dg, db, ctx.relu, ctx.has_res,
                                       ctx.bslots, mask, ctx.training)
        return (dx, sg.done(), sb.done(), (dres if ctx.has_res else None), None, None, None, None,
                None, None, None, None, None)


def batch_norm_act(x, weight, bias, running_mean, running_var, training: bool, momentum: float,
                   eps: float, relu: bool = False, residual=None, slots=None):
    """``relu?(batch_norm(x) [+ residual])`` in one fused kernel pair (NHWC bf16 on GPU).

    ``slots``: optional persistent (forward, backward) BN slot-sum buffers of the
    layer (see ``ops.conv.bn_slot_buffer``); fresh zeroed ones when None.

    With ``training=False`` the running statistics normalise and the input
    gradient is ``gamma * invstd * dz`` (they do not depend on ``x``).

    Numeric domain of the native path: two-moment fp32 batch statistics,
    ``var = max(Q/M - mean^2, 0)``, tested up to ``|mean|/sigma = 64``.  Measured
    relative ``invstd`` error (MI355X, bf16 ``randn + offset``): 3e-5 at 16, 6e-4
    at 64 (9.4e-4 at worst), 5e-3 at 256; for a nearly constant channel,
    ``bf16(randn + 1024)``, the variance cancels and ``invstd`` is off by 0.2 to
    0.7 of its value (finite: the clamp).  See the header of ``csrc/bn.hip``.
    """
    if x.is_cuda and x.dtype == torch.bfloat16 and x.shape[1] % 8 == 0 and x.shape[1] <= 2048:
        if not training and (running_mean is None or running_var is None):
            training = True
        part = getattr(x, "_dmp_bn_part", None) if training else None
        # the MFMA stem conv's output (ops.conv.StemHandoff): BN + ReLU backward and
        # the conv's weight gradient run as one pass
        stem = getattr(x, "_dmp_stem", None) if (training and relu and residual is None
                                                   and part is not None) else None
        return _BNAct.apply(x, weight, bias, residual, running_mean, running_var, training,
                            momentum, eps, relu, part, slots, stem)
    if x.is_cuda and x.dtype == torch.bfloat16:
        raise RuntimeError(
            f"batch_norm_act: unsupported bf16 GPU input (C={x.shape[1]}); "
            "the native kernel needs C % 8 == 0 and C <= 2048")
    # CPU, or an fp32 GPU run in the explicit oracle mode (``--deterministic``:
    # every op on PyTorch's fp32 kernels, same model / optimizer / PS)
    stock_gpu("batch_norm", x)
    w = weight.to(x.dtype) if weight is not None else None
    b = bias.to(x.dtype) if bias is not None else None
    y = F.batch_norm(x, running_mean, running_var, w, b, training, momentum, eps)
    if residual is not None:
        y = y + residual
    return F.relu(y) if relu else y


# -------------------------------------------------------------------- pooling
class _GAP(Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous(memory_format=CL)
        ctx.hw = (x.shape[2], x.shape[3])
        return native().gap_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        return native().gap_bwd(dy.contiguous(), ctx.hw[0], ctx.hw[1])


def global_avg_pool(x):
    """[N,C,H,W] -> [N,C] mean over H,W."""
    if x.is_cuda and x.dtype == torch.bfloat16 and x.shape[1] % 8 == 0:
        return _GAP.apply(x)
    stock_gpu("global_avg_pool", x)
    return x.mean(dim=(2, 3))


class _MaxPool(Function):
    @staticmethod
    def forward(ctx, x, k, s, p, nchw_out=False, relu_in=False):
        x = x.contiguous(memory_format=CL)
        # relu_in: x >= 0 (a fused-ReLU output): a window whose max is <= 0 (all
        # zeros) records "no tap", so the backward is relu'-masked already
        y, idx = native().maxpool_fwd(x, k, s, p, nchw_out, relu_in)
        ctx.save_for_backward(idx)
        ctx.meta = (x.shape[2], x.shape[3], k, s, p)
        ctx.relu_in = relu_in
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        H, W, k, s, p = ctx.meta
        dx = native().maxpool_bwd(dy, idx, H, W, k, s, p)
        if ctx.relu_in:
            mark_relu_masked(dx)
        return dx, None, None, None, None, None


def max_pool2d(x, kernel_size: int, stride: int | None = None, padding: int = 0,
               nchw_out: bool = False):
    """Max pool (floor mode): native NHWC kernel for bf16 GPU input (any channel
    count, window <= 15, stride, padding <= window/2), PyTorch otherwise.
    ``nchw_out``: write the output NCHW-contiguous (a pool that feeds a flatten
    in the reference's (c, h, w) order: no layout copy either way)."""
    stride = kernel_size if stride is None else stride
    if (x.is_cuda and x.dtype == torch.bfloat16 and x.dim() == 4
            and 1 <= kernel_size <= 15 and stride >= 1 and 0 <= 2 * padding <= kernel_size
            and x.shape[2] + 2 * padding >= kernel_size
            and x.shape[3] + 2 * padding >= kernel_size):
        y = _MaxPool.apply(x, int(kernel_size), int(stride), int(padding), bool(nchw_out),
                           nonneg(x))
        return set_nonneg(y, nonneg(x))
    stock_gpu("max_pool2d", x)
    return F.max_pool2d(x, kernel_size, stride, padding)


# BatchNorm + ReLU + max pool in one kernel each way (csrc/bn.hip: the pool reads
# the raw conv output and applies the BN itself; the BN backward gathers its dz
# from the pooled gradient): the ImageNet ResNet stem.  DMP_BN_POOL_FUSE=0: the
# unfused BN apply + max pool pair.
_BN_POOL_FUSE = os.environ.get("DMP_BN_POOL_FUSE", "1") != "0"


class _BNReLUPool(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum, eps, k, s, p, part,
                slots):
        x = x.contiguous(memory_format=CL)
        C = x.shape[1]
        bslots = slots[1] if slots is not None else None
        src = part if part is not None else _fresh_slots(
            slots[0] if slots is not None else None, C, x.device)
        y, idx, stats, xm = native().bn_relu_maxpool_fwd(
            x, src, part is not None, gamma, beta, running_mean, running_var, float(momentum),
            float(eps), bslots, k, s, p)
        mark_slots(src, True)              # read here, zeroed by the backward apply
        if bslots is not None:
            mark_slots(bslots, False)      # zeroed by this apply
        ctx.fpart, ctx.bslots, ctx.meta = src, bslots, (k, s, p)
        ctx.gamma, ctx.beta = gamma, beta
        ctx.save_for_backward(x, idx, stats, xm)
        return y

    @staticmethod
    def backward(ctx, dp):
        x, idx, stats, xm = ctx.saved_tensors
        gamma, beta = ctx.gamma, ctx.beta
        sg = GradSink(gamma, ctx.needs_input_grad[1], dtype=None)
        sb = GradSink(beta, ctx.needs_input_grad[2], dtype=None)
        bs = _fresh_slots(ctx.bslots, x.shape[1], x.device)
        k, s, p = ctx.meta
        dx = native().maxpool_bn_bwd(x, dp, idx, xm, gamma, stats, sg.buf, sb.buf, bs, ctx.fpart,
                                     k, s, p)
        mark_slots(bs, True)
        mark_slots(ctx.fpart, False)
        ctx.fpart = None
        return dx, sg.done(), sb.done(), None, None, None, None, None, None, None, None, None


def bn_relu_maxpool_ok(x, bn, k: int, s: int, p: int) -> bool:
    """The fused training path applies: a bf16 GPU NHWC activation feeding a
    ReLU BatchNorm in batch-statistics mode, then a 3x3/s2/p1 max pool."""
    return bool(_BN_POOL_FUSE and _BN_FOLD and x.is_cuda
                and x.dtype == torch.bfloat16 and x.dim() == 4 and bn.training
                and getattr(bn, "relu", False) and 2 * x.numel() < 2 ** 31
                and native().bn_maxpool_supported(x.shape[1], k, s, p))


def bn_relu_maxpool(x, bn, k: int, s: int, p: int):
    """``max_pool2d(relu(bn(x)), k, s, p)`` in one fused kernel pair (see
    ``bn_relu_maxpool_ok``); ``bn`` is an ``ops.layers.BatchNorm2d``."""
    part = getattr(x, "_dmp_bn_part", None)
    y = _BNReLUPool.apply(
        x, bn.weight, bn.bias, bn.running_mean if bn.track_running_stats else None,
        bn.running_var if bn.track_running_stats else None,
        0.1 if bn.momentum is None else bn.momentum, bn.eps, int(k), int(s), int(p), part,
        bn._slots(x))
    return set_nonneg(y)


# ----------------------------------------------------------------------- ReLU
class _ReLU(Function):
    """Standalone ReLU (where no producing GEMM / conv epilogue can take it):
    forward and backward on the native mask kernel (csrc/im2col.hip)."""

    @staticmethod
    def forward(ctx, x):
        y = native().relu_bwd(x, x)          # x > 0 ? x : 0
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        return native().relu_bwd(dy, y)


def relu(x):
    if x.is_cuda and x.dtype == torch.bfloat16:
        return _ReLU.apply(x)
    stock_gpu("relu", x)
    return F.relu(x)


# -------------------------------------------------------------------- dropout
class _Dropout(Function):
    @staticmethod
    def forward(ctx, x, p, seed, offset, mode):
        # the kernel advances the layer's device-side Philox offset itself (last
        # block, arrival ticket): a captured hipGraph replay draws a fresh mask
        y, mask = native().dropout_fwd(x, float(p), int(seed), offset, int(mode))
        ctx.save_for_backward(mask)
        ctx.p, ctx.mode = p, mode
        # the dense format the mask was drawn in (element-wise: memory order);
        # the backward brings dy to it, however the gradient arrives
        ctx.cl = x.dim() == 4 and x.is_contiguous(memory_format=CL) and not x.is_contiguous()
        return y

    @staticmethod
    def backward(ctx, dy):
        (mask,) = ctx.saved_tensors
        dx = native().dropout_bwd(dy, mask, float(ctx.p), int(ctx.mode), ctx.cl)
        if is_relu_masked(dy):
            mark_relu_masked(dx)       # a positive scaling keeps the mask valid
        return dx, None, None, None, None


def dropout(x, p: float, training: bool, channelwise: bool = False, state=None, seed: int = 0):
    """Dropout (``channelwise``: Dropout2d, one draw per (n, c) plane).

    GPU: Philox4x32-10 kernel (``csrc/dropout.hip``) keyed by ``seed`` and the
    device int64 ``state`` = [offset, ticket] (the kernel advances the offset).
    Reference: ``nn.Dropout2d`` / ``F.dropout`` in LeNet
    (/root/reference/example/models.py:10,17,20).
    """
    if not training or p == 0.0:
        return x
    if x.is_cuda and x.dtype in (torch.bfloat16, torch.float32) and state is not None:
        mode = 0
        if channelwise:
            if x.dim() == 4 and x.is_contiguous(memory_format=CL) and not x.is_contiguous():
                mode = 2
            else:
                x = x.contiguous()
                mode = 1
        return set_nonneg(_Dropout.apply(x, p, seed, state, mode), nonneg(x))
    stock_gpu("dropout", x)
    if channelwise:
        return F.dropout2d(x, p, True)
    return F.dropout(x, p, True)


# ----------------------------------------------------------------- layernorm
def _ln_backward(ctx, dy, dh, gi, rscale=None):
    """``(dx, dgamma, dbeta)`` of the LayerNorm Functions: ``dh`` is the
    residual stream's own gradient (added inside the kernel), ``gi`` gamma's
    position among the forward inputs (beta follows it).  With ``rscale`` (the
    row-scaled add) ``dx`` is the pair ``(dx, dr)``."""
    x, mean, rstd = ctx.saved_tensors[:3]
    gamma = ctx.gamma
    sg = GradSink(gamma, ctx.needs_input_grad[gi])
    sb = GradSink(ctx.beta, ctx.needs_input_grad[gi + 1])
    g32 = gamma.detach() if gamma is not None else None
    if dh is not None and dh.dtype != x.dtype:
        dh = dh.to(x.dtype)
    if rscale is None:
        dx = native().layernorm_bwd(x, dy.to(x.dtype), g32, mean, rstd, sg.buf, sb.buf, ctx.slots,
                                    dh)
    else:
        dx = native().layernorm_bwd(x, dy.to(x.dtype), g32, mean, rstd, sg.buf, sb.buf, ctx.slots,
                                    dh, rscale, x.numel() // x.shape[-1] // rscale.numel())
    return dx, sg.done(), sb.done()


class _LayerNorm(Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, eps, slots=None):
        x = x.contiguous()
        g32 = gamma.detach() if gamma is not None else None
        b32 = beta.detach() if beta is not None else None
        y, mean, rstd = native().layernorm_fwd(x, g32, b32, float(eps))
        ctx.save_for_backward(x, mean, rstd)
        ctx.gamma, ctx.beta, ctx.slots = gamma, beta, slots
        return y

    @staticmethod
    def backward(ctx, dy):
        return (*_ln_backward(ctx, dy, None, 1), None, None)


class _AddLayerNorm(Function):
    """h = x + r; y = LayerNorm(h) in one native pass (pre-norm transformer
    residual add fused into the next LayerNorm).  Backward: dh_total = dh +
    LN_bwd(dy) formed inside the LayerNorm-backward kernel; x and r both get it."""

    @staticmethod
    def forward(ctx, x, r, gamma, beta, eps, slots=None):
        ctx.set_materialize_grads(False)
        x = x.contiguous()
        g32 = gamma.detach() if gamma is not None else None
        b32 = beta.detach() if beta is not None else None
        y, mean, rstd, h = native().layernorm_fwd(x, g32, b32, float(eps), r.contiguous())
        ctx.save_for_backward(h, mean, rstd)
        ctx.gamma, ctx.beta, ctx.slots = gamma, beta, slots
        return h, y

    @staticmethod
    def backward(ctx, dh, dy):
        if dy is None:
            return dh, dh, None, None, None, None
        dx, dg, db = _ln_backward(ctx, dy, dh, 2)
        return dx, dx, dg, db, None, None


class _AddLayerNormScaled(Function):
    """:class:`_AddLayerNorm` with the add scaled per sample (stochastic depth):
    ``h = x + r * rscale[sample]`` inside the forward kernel, and the backward
    kernel writes ``r``'s gradient ``dh_total * rscale[sample]`` next to ``dx``.
    ``rscale`` is the forward's own table row, saved with it."""

    @staticmethod
    def forward(ctx, x, r, gamma, beta, eps, slots, rscale):
        ctx.set_materialize_grads(False)
        x = x.contiguous()
        g32 = gamma.detach() if gamma is not None else None
        b32 = beta.detach() if beta is not None else None
        tokens = x.numel() // x.shape[-1] // rscale.numel()
        y, mean, rstd, h = native().layernorm_fwd(x, g32, b32, float(eps), r.contiguous(), rscale,
                                                  tokens)
        ctx.save_for_backward(h, mean, rstd, rscale)
        ctx.gamma, ctx.beta, ctx.slots = gamma, beta, slots
        return h, y

    @staticmethod
    def backward(ctx, dh, dy):
        rscale = ctx.saved_tensors[3]
        if dy is None:
            if dh is None:
                return (None,) * 7
            return dh, native().drop_path_rows(dh, rscale), None, None, None, None, None
        (dx, dr), dg, db = _ln_backward(ctx, dy, dh, 2, rscale)
        return dx, dr, dg, db, None, None, None


class _LayerNormStream(Function):
    """``(h, LayerNorm(h))`` for a residual stream ``h`` that is also read by the
    next residual add: ``h`` comes back as a view, so autograd sees ONE consumer
    and the LayerNorm-backward kernel forms ``dh_total = dh + LN_bwd(dy)``
    itself (two consumers would have autograd sum the gradients with an ATen add
    over the whole stream -- the first ViT block's 19 MB add)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, slots=None):
        ctx.set_materialize_grads(False)
        x = x.contiguous()
        g32 = gamma.detach() if gamma is not None else None
        b32 = beta.detach() if beta is not None else None
        y, mean, rstd = native().layernorm_fwd(x, g32, b32, float(eps))
        ctx.save_for_backward(x, mean, rstd)
        ctx.gamma, ctx.beta, ctx.slots = gamma, beta, slots
        return x.view_as(x), y

    @staticmethod
    def backward(ctx, dh, dy):
        if dy is None:
            return dh, None, None, None, None
        return (*_ln_backward(ctx, dy, dh, 1), None, None)


def stream_layer_norm(x, weight, bias, eps: float, slots=None):
    """``(x, LayerNorm(x))`` where the caller keeps using ``x`` (pre-norm
    residual stream): the returned ``x`` carries the stream's gradient into the
    LayerNorm backward kernel (native bf16 path); plain ``(x, layer_norm(x))``
    elsewhere."""
    if (x.is_cuda and x.dtype == torch.bfloat16 and layernorm_supported(x.shape[-1])
            and (weight is None or weight.dtype == torch.float32)
            and (bias is None or bias.dtype == torch.float32)):
        return _LayerNormStream.apply(x, weight, bias, eps, slots)
    return x, layer_norm(x, weight, bias, eps, slots)


LN_SLOTS = 32   # csrc/transformer.hip kLnSlots


def layernorm_supported(D: int) -> bool:
    """Mirror of csrc/transformer.hip layernorm_supported: D % 8 == 0 and at most 8
    16-B chunks per lane with the widest power-of-two lane group dividing D/8."""
    if D <= 0 or D % 8:
        return False
    nch, lr = D // 8, 64
    while lr > 1 and nch % lr:
        lr //= 2
    return nch // lr <= 8


def add_layer_norm(x, r, weight, bias, eps: float, slots=None, rscale=None):
    """``h = x + r`` and ``LayerNorm(h)`` -> ``(h, y)``: one native pass for bf16 GPU
    rows (``csrc/transformer.hip``), add + :func:`layer_norm` otherwise.

    ``rscale`` (float32 ``[B]``, a row of :func:`drop_path_table`): stochastic
    depth, ``h = x + r * rscale[sample]`` with the product and the sum rounded
    separately in fp32; a sample whose scale is 0 keeps ``x`` bit for bit and
    ``r`` is not read for it."""
    if (x.is_cuda and x.dtype == torch.bfloat16 and r.dtype == torch.bfloat16
            and x.shape == r.shape and layernorm_supported(x.shape[-1])
            and (weight is None or weight.dtype == torch.float32)
            and (bias is None or bias.dtype == torch.float32)):
        if rscale is not None:
            return _AddLayerNormScaled.apply(x, r, weight, bias, eps, slots, rscale)
        return _AddLayerNorm.apply(x, r, weight, bias, eps, slots)
    if rscale is None:
        h = x + r
    elif x.is_cuda and x.dtype == torch.bfloat16:
        h = x + drop_path(r, rscale)      # a D the fused kernel refuses: native scaling
    else:
        h = scaled_add(x, r, rscale)
    return h, layer_norm(h, weight, bias, eps, slots)


# ----------------------------------------------------------- stochastic depth
# Per-sample drop path (Huang et al. 2016; timm's ``drop_path``) on the residual
# branches of the ViT.  One table per training forward, ``S[j][b]`` = the scale
# sample ``b`` applies to branch ``j``: ``1 / (1 - p_j)`` when kept, 0 when
# dropped.  The draw of (b, j) at step ``t`` is word ``b & 3`` of
# ``philox4x32_10(ctr=(b >> 2, j, t, "drop"), key=(seed_lo, seed_hi))``, kept
# when it is ``>= min(int(p_j * 2^32), 0xFFFFFFFF)``: a pure function of
# (seed, step, branch, sample), the same bits from the kernel
# (``csrc/drop_path.hip``) and from the torch form below.
DROP_DOMAIN = 0x64726F70        # "drop": counter word 3 (0x64617461 "data" is the data stream's)


def drop_path_rates(drop_path: float, depth: int) -> list:
    """Rate of each of ``depth`` blocks: the linear ramp ``drop_path * i /
    (depth - 1)`` (timm's ``linspace(0, drop_path, depth)``); one block gets
    ``drop_path`` itself."""
    p = float(drop_path)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"drop path rate must be in [0, 1), got {drop_path}")
    if depth < 1:
        raise ValueError(f"depth must be >= 1, got {depth}")
    if depth == 1:
        return [p]
    return [p * i / (depth - 1) for i in range(depth)]


def drop_path_consts(rates, device=None):
    """``(thresholds int64, scales float32)`` of the branches with drop rates
    ``rates``: keep iff the draw ``>= thresholds[j]``; ``scales[j] = float32(1) /
    float32(1 - p_j)`` (exactly 1 at ``p_j == 0``, where every draw is kept)."""
    for p in rates:
        if not 0.0 <= p < 1.0:
            raise ValueError(f"drop path rate must be in [0, 1), got {p}")
    thr = torch.tensor([min(int(float(p) * 4294967296.0), 0xFFFFFFFF) for p in rates],
                       dtype=torch.int64)
    keep = torch.tensor([1.0 - float(p) for p in rates], dtype=torch.float32)
    scales = torch.ones_like(keep) / keep
    return thr.to(device), scales.to(device)


def drop_path_table(state, thresholds, scales, batch: int, seed: int):
    """The ``[branches, batch]`` float32 scale table of step ``state[0]`` (a
    device-side int64 counter, advanced by 1): one native launch on the GPU, the
    same draws in torch on the CPU."""
    if state.is_cuda:
        return native().drop_path_draw(state, thresholds, scales, int(batch), int(seed))
    from ..utils.device_data import philox4x32_10

    t = int(state[0]) & 0xFFFFFFFF
    nb = scales.numel()
    b = torch.arange(batch, dtype=torch.int64)
    j = torch.arange(nb, dtype=torch.int64)[:, None]
    z = torch.zeros(nb, batch, dtype=torch.int64)
    words = philox4x32_10((z + (b >> 2), z + j, z + t, z + DROP_DOMAIN),
                          (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    word = torch.stack(words, 0).gather(0, (z + (b & 3))[None])[0]
    keep = word >= thresholds.to(torch.int64)[:, None]
    state[0] += 1
    return torch.where(keep, scales[:, None].expand(nb, batch),
                       torch.zeros((), dtype=torch.float32))


def _sample_scale(rscale, like):
    return rscale.view(-1, *([1] * (like.dim() - 1)))


def scaled_add(x, r, rscale):
    """The specification of the row-scaled add in torch: ``x + r * s`` per sample,
    fp32 product and sum rounded separately, one rounding to ``x``'s dtype; a
    dropped sample (``s == 0``) is ``x`` itself and takes nothing from ``r``."""
    stock_gpu("drop_path (scaled add)", x)
    s = _sample_scale(rscale, x)
    h = (x.float() + r.float() * s).to(x.dtype)
    return torch.where(s != 0, h, x)


class _DropPath(Function):
    @staticmethod
    def forward(ctx, x, rscale):
        ctx.save_for_backward(rscale)
        return native().drop_path_rows(x, rscale)

    @staticmethod
    def backward(ctx, dy):
        (rscale,) = ctx.saved_tensors
        return native().drop_path_rows(dy, rscale), None


def drop_path(x, rscale):
    """``x * rscale[sample]`` (float32 ``[B]`` scales of :func:`drop_path_table`) for
    a residual branch that is added outside the fused add+LayerNorm: the native
    row kernel for bf16 GPU input, torch otherwise."""
    if rscale is None:
        return x
    if (x.is_cuda and x.dtype == torch.bfloat16 and x.shape[0] == rscale.numel()
            and (x.numel() // x.shape[0]) % 8 == 0):
        return _DropPath.apply(x, rscale)
    stock_gpu("drop_path", x)
    return (x.float() * _sample_scale(rscale, x)).to(x.dtype)


def layer_norm(x, weight, bias, eps: float, slots=None):
    """LayerNorm over the last dim: native row kernel for bf16 GPU input with fp32
    affine params (``csrc/transformer.hip``), PyTorch otherwise.  ``slots``: the
    layer's persistent zeroed ``[LN_SLOTS * 2 * D]`` fp32 param-grad slot buffer."""
    if (x.is_cuda and x.dtype == torch.bfloat16 and layernorm_supported(x.shape[-1])
            and (weight is None or weight.dtype == torch.float32)
            and (bias is None or bias.dtype == torch.float32)):
        return _LayerNorm.apply(x, weight, bias, eps, slots)
    stock_gpu("layer_norm", x)
    w = compute_weight(weight, x.dtype)
    b = compute_weight(bias, x.dtype)
    return F.layer_norm(x, (x.shape[-1],), w, b, eps)


# ---------------------------------------------------------------------- GELU
class _GELU(Function):
    @staticmethod
    def forward(ctx, x):
        x = x.contiguous()
        ctx.save_for_backward(x)
        return native().gelu_fwd(x)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        return native().gelu_bwd(x, dy)


def gelu(x):
    """tanh-approximate GELU (native bf16 kernel on GPU)."""
    if x.is_cuda and x.dtype == torch.bfloat16 and x.numel() % 8 == 0:
        return _GELU.apply(x)
    stock_gpu("gelu", x)
    return F.gelu(x, approximate="tanh")


# ------------------------------------------------------- token-row select
class _TokenRow(Function):
    """``h[:, tok]`` as a strided view (the native GEMM reads its rows in place,
    row stride N * D: no gather copy); backward = one native pass writing the
    [B, N, D] stream gradient (zeros but the selected rows) instead of ATen's
    zero fill + slice copy."""

    @staticmethod
    def forward(ctx, h, tok):
        ctx.n, ctx.tok = h.shape[1], int(tok)
        return h.select(1, int(tok))

    @staticmethod
    def backward(ctx, g):
        return native().token_row_scatter(g.contiguous(), ctx.n, ctx.tok), None


def token_row(h, tok: int = 0):
    """Row ``tok`` of every sample of a ``[B, N, D]`` token stream (the ViT class
    token feeding the head, /root/reference has no ViT: BASELINE.json config #5)."""
    if h.is_cuda and h.dtype == torch.bfloat16 and h.dim() == 3 and h.shape[-1] % 8 == 0:
        return _TokenRow.apply(h, tok)
    stock_gpu("token_row", h)
    return h[:, tok].contiguous()


# ------------------------------------------------------- ViT token assembly
class _VitEmbed(Function):
    """``cat([cls.expand(B), tok], 1) + pos`` in one native pass; the backward
    copies the token gradient and adds the batch sums into the fp32 gradients of
    ``cls`` / ``pos`` (their arena views) -- no concat, broadcast add, expand-sum
    or per-parameter cast kernels."""

    @staticmethod
    def forward(ctx, tok, cls, pos, cls16, pos16):
        ctx.params = (cls, pos)
        ctx.tok_grad = tok.requires_grad
        return native().vit_embed_fwd(tok, cls16, pos16)

    @staticmethod
    def backward(ctx, dh):
        cls, pos = ctx.params
        sc = GradSink(cls, ctx.needs_input_grad[1])
        sp = GradSink(pos, ctx.needs_input_grad[2])
        dtok = native().vit_embed_bwd(dh, sp.buf, sc.buf, ctx.tok_grad)
        return dtok if ctx.tok_grad else None, sc.done(), sp.done(), None, None


def vit_embed(tok, cls, pos):
    """``cat([cls.expand(B, 1, D), tok], 1) + pos`` (ViT class token + position
    embedding): native kernel pair for bf16 GPU tokens, PyTorch otherwise."""
    if tok.is_cuda and tok.dtype == torch.bfloat16 and tok.shape[-1] % 8 == 0:
        def shadow(p):
            w16 = getattr(p, "_dmp_w16", None)
            return w16 if w16 is not None and w16.dtype == tok.dtype else p.detach().to(tok.dtype)

        cls16, pos16 = shadow(cls), shadow(pos)
        if torch.is_grad_enabled() and (tok.requires_grad or cls.requires_grad
                                        or pos.requires_grad):
            return _VitEmbed.apply(tok, cls, pos, cls16, pos16)
        return native().vit_embed_fwd(tok, cls16, pos16)
    c = compute_weight(cls, tok.dtype).expand(tok.shape[0], -1, -1)
    stock_gpu("vit_embed", tok)
    return torch.cat([c, tok], dim=1) + compute_weight(pos, tok.dtype)


# ------------------------------------------------------------------ attention
class _ScaledSoftmax(Function):
    @staticmethod
    def forward(ctx, s, scale):
        p = native().softmax_fwd(s.contiguous(), float(scale))
        ctx.save_for_backward(p)
        ctx.scale = scale
        return p

    @staticmethod
    def backward(ctx, dp):
        (p,) = ctx.saved_tensors
        return native().softmax_bwd(p, dp, float(ctx.scale)), None


# most tokens the fused attention takes (csrc/attn_plan.h: resident kernels up to
# 256, streaming kernels up to 4096)
ATTENTION_MAX_TOKENS = 4096


def attention_route() -> int:
    """Route request of the fused attention bindings: -1 automatic (resident up
    to 256 tokens, streaming above); ``DMP_ATTN_STREAM=1`` forces the streaming
    kernels at every token count (A/Bs of the two routes at <= 256 tokens)."""
    return 1 if os.environ.get("DMP_ATTN_STREAM", "0") == "1" else -1


class _FusedQKVAttention(Function):
    @staticmethod
    def forward(ctx, qkv, heads, route=-1):
        qkv = qkv.contiguous()
        out, lse = native().attention_fwd(qkv, int(heads), int(route))
        ctx.save_for_backward(qkv, out, lse)
        ctx.heads = int(heads)
        ctx.route = int(route)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, out, lse = ctx.saved_tensors
        return native().attention_bwd(qkv, out, dout, lse, ctx.heads, ctx.route), None, None


def fused_attention_supported(qkv, heads: int) -> bool:
    if not (qkv.is_cuda and qkv.dtype == torch.bfloat16 and qkv.dim() == 3):
        return False
    D = qkv.shape[-1] // 3
    return (qkv.shape[-1] % 3 == 0 and D % heads == 0 and D // heads == 64
            and 1 <= qkv.shape[1] <= ATTENTION_MAX_TOKENS)


def attention_qkv(qkv, heads: int):
    """Multi-head self-attention straight from the qkv projection rows.

    ``qkv``: [B, N, 3*D] (= [B, N, 3, heads, D/heads]); returns [B, N, D] (the
    proj Linear's input rows).  On GPU (head dim 64, bf16, N <= 4096) this is a
    fused MFMA kernel set: up to 256 tokens the resident kernels of
    ``csrc/attention.hip`` (a head's keys and values staged once), above them
    the streaming kernels of ``csrc/attention_stream.hip`` (key / query tiles
    through LDS, online softmax).  Scores never leave the chip and the backward
    writes d(qkv) in place of the qkv layout (no permute copies, zero fills or
    gradient adds).  Elsewhere: SDPA.
    """
    B, N, three_d = qkv.shape
    D = three_d // 3
    if fused_attention_supported(qkv, heads):
        return _FusedQKVAttention.apply(qkv, heads, attention_route())
    q, k, v = qkv.view(B, N, 3, heads, D // heads).permute(2, 0, 3, 1, 4)
    o = attention(q, k, v)
    return o.transpose(1, 2).reshape(B, N, D)


def attention(q, k, v):
    """softmax(q k^T / sqrt(d)) v over [B, H, N, d]: the geometries the fused
    kernels do not take (head dim != 64, more than 4096 tokens, fp32).

    The two batched GEMMs are library GEMMs (hipBLASLt via ``torch.matmul``), so
    on the GPU this runs only in the explicit stock oracle mode (``ops._policy``);
    the scaled row softmax and its backward are native kernels.
    """
    scale = q.shape[-1] ** -0.5
    stock_gpu("attention (torch.matmul / SDPA)", q,
              reason=f"head dim {q.shape[-1]}, {k.shape[-2]} tokens, {q.dtype}: the fused "
                     f"kernels take head dim 64, <= {ATTENTION_MAX_TOKENS} tokens, bf16")
    if q.is_cuda and q.dtype == torch.bfloat16 and k.shape[-2] <= 1024:
        s = torch.matmul(q, k.transpose(-1, -2))
        p = _ScaledSoftmax.apply(s, scale)
        return torch.matmul(p, v)
    return F.scaled_dot_product_attention(q, k, v)
