"""Independent oracles of the Mixup / CutMix path (``utils/device_data.py``,
``csrc/data.hip``, ``csrc/xent.hip``):

* the mixed batch in NumPy: both views from ``data_oracle.assemble_np``, the
  blend in ``np.float32`` operations (each rounded on its own) and a bit-level
  round-to-nearest-even to bf16;
* the two-target loss and its gradient in fp64 from
  ``F.cross_entropy(..., reduction="none")``, with ``lam`` converted exactly;
* an fp32 emulation of the two-target loss in the kernels' operation order, which
  bounds what fp32 arithmetic alone costs against the fp64 oracle.

Shares no code with the implementation under test."""
import numpy as np
import torch
import torch.nn.functional as F

import data_oracle as do

# name: (C, H, W, N, pad, flip, norm, index): the shapes of test_device_data_gpu.CASES
# (tests/test_mix_cpu.py asserts that they are the same)
MNIST = ((0.1307,), (0.3081,))
HALF = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
CASES = {
    "cifar": (3, 32, 32, 64, 4, True, HALF, [0, 63, 5, 5, 17, 63, 0, 31, 8, 9, 10, 11, 62, 1, 5, 40]),
    "mnist": (1, 28, 28, 12, 2, False, MNIST, [11, 0, 3, 3, 7]),
    "odd_5x7": (3, 5, 7, 9, 3, False, HALF, [8, 0, 4]),
    "imagenet": (3, 224, 224, 4, 0, True, HALF, [3, 0]),
    "rgba_3x5": (4, 3, 5, 6, 16, True, ((0.4, 0.5, 0.6, 0.7), (0.2, 0.3, 0.4, 0.5)), [5, 0, 2, 2]),
}
STAGED = ("cifar", "mnist")
SMALL = ("cifar", "mnist", "odd_5x7", "rgba_3x5")
SEED = (0xABCD << 32) | 0x1234
PIX_LAMS = (1.0, 0.0, 0.5, 0.3172, 1e-8)


def f32(v) -> float:
    """The float32 nearest to ``v``, as a Python float."""
    return float(np.float32(v))


def boxes(h, w):
    """Empty, whole image, one pixel, touching each edge, and (for C = 3) boxes that
    start and end mid-way through an 8-value store group: x0 = 1 is value 3 of
    group 0, x1 = 4 ends at value 12, inside group 1."""
    out = {"empty": (0, 0, 0, 0), "whole": (0, h, 0, w), "pixel": (h // 2, h // 2 + 1, w // 2, w // 2 + 1),
           "top": (0, max(1, h // 3), 1, w), "bottom": (h - 1, h, 0, w - 1),
           "left": (1, h, 0, max(1, w // 3)), "right": (0, h - 1, w - 1, w),
           "midgroup": (0, h, 1, min(4, w))}
    return out


def bf16_bits_rne(x32: np.ndarray) -> np.ndarray:
    """float32 array -> bf16 bit patterns, round to nearest even, on the integers."""
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)
    return r.astype(np.uint16)


def bits_to_f32(b: np.ndarray) -> np.ndarray:
    return (b.astype(np.uint32) << np.uint32(16)).view(np.float32)


def mix_np(images_u8, labels, lut_bits, index, pix_lam, label_lam, box, pad, flip, seed, epoch):
    """The mixed batch: x bits uint16 [B, C, H, W], y, y2 int64 [B], lam float32 [B],
    draws int64 [B, 3]."""
    a, y, d = do.assemble_np(images_u8, labels, lut_bits, index, pad, flip, seed, epoch)
    count = len(index)
    out = np.empty_like(a)
    y2 = np.empty_like(y)
    lam = np.float32(pix_lam)
    wl = np.float32(np.float32(1.0) - lam)
    y0, y1, x0, x1 = box
    for b in range(count):
        p = a[count - 1 - b]
        y2[b] = y[count - 1 - b]
        if float(lam) == 1.0:
            row = a[b].copy()
        else:
            t1 = (bits_to_f32(a[b]) * lam).astype(np.float32)
            t2 = (bits_to_f32(p) * wl).astype(np.float32)
            row = bf16_bits_rne((t1 + t2).astype(np.float32))
        row[:, y0:y1, x0:x1] = p[:, y0:y1, x0:x1]
        out[b] = row
    return out, y, y2, np.full(count, np.float32(label_lam), dtype=np.float32), d


# ------------------------------------------------------------------- the loss
def _ok(y, c, ignore_index):
    return (y != ignore_index) & (y >= 0) & (y < c)


def xent_mix_ref(logits, y, y2, lam, smoothing=0.0, ignore_index=-100, gloss=1.0):
    """fp64 two-target loss -> (loss, dlogits * gloss).  Rows with either label
    ignored or out of range drop out; no valid row at all: loss 0, gradient 0."""
    x = logits.detach().cpu().double().requires_grad_(True)
    y, y2 = y.detach().cpu(), y2.detach().cpu()
    lam = lam.detach().cpu().double()              # exact: every float32 is a double
    c = x.shape[1]
    valid = _ok(y, c, ignore_index) & _ok(y2, c, ignore_index)
    t1 = torch.where(valid, y, torch.zeros_like(y))
    t2 = torch.where(valid, y2, torch.zeros_like(y2))
    n1 = F.cross_entropy(x, t1, reduction="none")
    n2 = F.cross_entropy(x, t2, reduction="none")
    zero = torch.zeros_like(n1)
    rows = torch.where(lam != 0, lam * n1, zero) + torch.where(lam != 1, (1 - lam) * n2, zero)
    if smoothing > 0:
        rows = (1 - smoothing) * rows + smoothing * (torch.logsumexp(x, 1) - x.mean(1))
    rows = torch.where(valid, rows, zero)
    loss = rows.sum() / max(int(valid.sum()), 1)
    (loss * gloss).backward()
    return loss.detach(), x.grad


def xent_mix_hits_ref(logits, y, y2, lam, ignore_index=-100):
    """Top-1 hits against the heavier target, NumPy's argmax (first maximum)."""
    x = logits.detach().cpu().double().numpy()
    y, y2 = y.detach().cpu().numpy(), y2.detach().cpu().numpy()
    c = x.shape[1]
    valid = _ok(y, c, ignore_index) & _ok(y2, c, ignore_index)
    tgt = np.where(lam.detach().cpu().numpy() >= np.float32(0.5), y, y2)
    return int(((np.argmax(x, axis=1) == tgt) & valid).sum())


def xent_mix_emulated(logits, y, y2, lam, smoothing=0.0, ignore_index=-100, gloss=1.0):
    """The two-target loss and gradient in fp32, in the kernels' operation order
    (max-shift, sum of exponentials, ``lam * (lse - x_y) + (1 - lam) * (lse - x_y2)``,
    ``(p - eps / C - (1 - eps) * weight) * grad_scale``), the gradient rounded to
    the logits' dtype as the kernels store it."""
    x = logits.detach().cpu().float()
    y, y2 = y.detach().cpu(), y2.detach().cpu()
    lam = lam.detach().cpu().float()
    b, c = x.shape
    valid = _ok(y, c, ignore_index) & _ok(y2, c, ignore_index)
    t1 = torch.where(valid, y, torch.zeros_like(y))
    t2 = torch.where(valid, y2, torch.zeros_like(y2))
    m = x.max(1, keepdim=True).values
    e = torch.exp(x - m)
    s = e.sum(1, keepdim=True)
    lse = (m + torch.log(s)).squeeze(1)
    wl = 1 - lam
    d1 = lse - x.gather(1, t1[:, None]).squeeze(1)
    d2 = lse - x.gather(1, t2[:, None]).squeeze(1)
    zero = torch.zeros_like(d1)
    nll = torch.where(lam != 0, lam * d1, zero) + torch.where(wl != 0, wl * d2, zero)
    eps = float(smoothing)
    rows = (1 - eps) * nll
    if eps > 0:
        rows = rows + eps * (lse - x.sum(1) / c)
    rows = torch.where(valid, rows, zero)
    nvalid = max(int(valid.sum()), 1)
    loss = rows.sum() / nvalid
    w = torch.zeros_like(x)
    w.scatter_add_(1, t1[:, None], lam[:, None])
    w.scatter_add_(1, t2[:, None], wl[:, None])
    g = (e / s - eps / c - (1 - eps) * w) * (1.0 / nvalid)
    g = torch.where(valid[:, None], g, torch.zeros_like(g)).to(logits.dtype)
    g = (g * torch.tensor(gloss).to(logits.dtype)) if gloss != 1.0 else g
    return loss.double(), g


def xent_mix_inputs(B, C, dtype, seed):
    """Logits, two label vectors and per-row weights random in [0, 1] with rows
    forced to exactly 0, 1 and 0.5, and rows with y == y2."""
    g = torch.Generator().manual_seed(seed * 977 + 31 * C + B)
    x = torch.randn(B, C, generator=g).to(dtype)
    y = torch.randint(0, C, (B,), generator=g)
    y2 = torch.randint(0, C, (B,), generator=g)
    lam = torch.rand(B, generator=g)
    lam[0], lam[1], lam[2] = 0.0, 1.0, 0.5
    y2[3] = y[3]
    if B > 8:
        lam[B - 1], lam[B - 2] = 1.0, 0.0
        y2[B - 3] = y[B - 3]
    return x, y, y2, lam
