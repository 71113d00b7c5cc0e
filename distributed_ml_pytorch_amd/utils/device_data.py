"""Device-resident datasets and their crop / flip batch assembler.

The dataset stays on the device as uint8 NHWC images.  One launch per step
(``csrc/data.hip``) gathers a shuffled batch and writes normalised bf16 NHWC
images and int64 labels straight into the training step's input buffers,
through an optional per-sample random crop (zero padding, as torchvision's
``RandomCrop(H, padding=pad)``) and horizontal flip.  No host tensor, no
host-to-device copy and no cast kernel is on the step path.

This file is the readable definition, the CPU implementation and the oracle of
that kernel (the role ``parallel/wire8.py`` plays for the MX8 wire).

**Normalisation** is a ``[C, 256]`` bf16 look-up table,
``normalize_uint8(arange(256), mean, std).to(bfloat16)`` per channel, built on
the CPU: the kernel does no floating-point arithmetic and its output equals
``normalize_uint8(x).to(bfloat16)`` by construction.

**Randomness** is counter-based Philox4x32-10 (the rounds of
``csrc/dropout.hip``).  For the sample with dataset index ``i``::

    r  = philox4x32_10(ctr=(i, epoch, 0, 0x64617461), key=(seed & 0xffffffff, seed >> 32))
    dy = (r.x * (2 pad + 1)) >> 32        dx = (r.y * (2 pad + 1)) >> 32
    f  = r.z >> 31 if flip else 0

so a sample's augmentation is a pure function of (seed, epoch, dataset index):
the same across runs, batch sizes, positions in the batch and resumes.  Crop,
then flip: output pixel ``(h, w)`` reads source row ``h + dy - pad`` and column
``(W - 1 - w if f else w) + dx - pad``; a coordinate outside the image reads the
byte 0 *before* normalisation (black padding, normalised like any pixel).  An
index outside ``[0, N)`` reads nothing: its image is all padding and its label
is -100, the ``ignore_index`` of ``softmax_cross_entropy``.

**Mixup and CutMix** (Zhang et al. 2018, Yun et al. 2019) build a training image
from two samples inside the same launch.  One draw per batch, on the host
(:func:`mix_draw`), a pure function of (seed, epoch, batch number in the epoch)
from a CPU generator of its own, so a resumed run mixes as the uninterrupted one
did and the epoch's order does not move::

    apply = u0 < prob
    mode  = cutmix if cutmix_alpha > 0 and (mixup_alpha == 0 or u1 < switch_prob) else mixup
    lam   = g1 / (g1 + g2),  g1, g2 ~ Gamma(alpha, 1) in fp64        # Beta(alpha, alpha)
    mixup:  pix_lam = label_lam = float32(lam), no box
    cutmix: r = sqrt(1 - lam), ch = int(H r), cw = int(W r), cy ~ randint(H), cx ~ randint(W)
            y0, y1 = clamp(cy - ch // 2, 0, H), clamp(cy + ch // 2, 0, H)   (x likewise)
            pix_lam = 1, label_lam = float32(1 - (y1 - y0)(x1 - x0) / (H W))

The **view** of a sample is the image defined above (its own crop, flip and
normalisation).  The partner of batch row ``b`` is row ``count - 1 - b`` (the
middle row of an odd batch pairs with itself).  With ``a`` row b's view and ``p``
its partner's, output pixel ``(h, w)`` -- output coordinates, after each
sample's own crop and flip -- is ``p`` inside the box ``y0 <= h < y1, x0 <= w <
x1``, else ``a`` when ``pix_lam == 1``, else::

    bf16_rne(fl32(fl32(a * lam) + fl32(p * fl32(1 - lam))))     lam = float32(pix_lam)

four fp32 operations each rounded on its own (no fused multiply-add), so the
kernel and ``(a.float() * lam + p.float() * (1 - lam)).to(bfloat16)`` agree bit
for bit.  The step receives ``y`` (row b's label), ``y2`` (the partner's) and
``lam = label_lam`` per row for the two-target loss
(``ops.functional.softmax_cross_entropy_mix``).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import NamedTuple

import torch

from .data import (CIFAR_MEAN, CIFAR_STD, SyntheticImages, normalize_uint8, read_cifar10_binary,
                   read_mnist_idx)

MAX_CHANNELS = 4            # the kernel's LDS look-up table is [4][256]
MAX_PAD = 16
IGNORE_LABEL = -100
DOMAIN = 0x64617461         # "data": counter word 3, apart from every dropout stream
DEVICE_MARGIN_BYTES = 1 << 30   # free device memory a resident dataset must leave
MNIST_MEAN, MNIST_STD = (0.1307,), (0.3081,)
SYNTH_MEAN, SYNTH_STD = 128.0 / 255.0, 32.0 / 255.0
AUGMENTS = {"none": (False, False), "crop": (True, False), "flip": (False, True),
            "crop_flip": (True, True)}

MIX_DOMAIN = 0x6D697875     # "mixu": the mix generator's seed, apart from epoch_order's

_M32 = 0xFFFFFFFF


# ---------------------------------------------------------------------- Philox
def _mul32(m: int, x: torch.Tensor):
    """(hi, lo) 32-bit halves of ``m * x`` for a constant ``m`` < 2^32 and int64
    ``x`` in [0, 2^32), in int64 arithmetic that never exceeds 2^49."""
    a = m * (x >> 16)
    b = m * (x & 0xFFFF)
    t = a + (b >> 16)
    return t >> 16, ((t & 0xFFFF) << 16) | (b & 0xFFFF)


def philox4x32_10(ctr, key):
    """Philox4x32-10 on int64 tensors holding 32-bit words: ``ctr`` four, ``key``
    two (broadcastable).  Returns the four output words."""
    M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
    c0, c1, c2, c3 = (torch.as_tensor(c, dtype=torch.int64) & _M32 for c in ctr)
    k0, k1 = (torch.as_tensor(k, dtype=torch.int64) & _M32 for k in key)
    for _ in range(10):
        hi0, lo0 = _mul32(M0, c0)
        hi1, lo1 = _mul32(M1, c2)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + W0) & _M32, (k1 + W1) & _M32
    return c0, c1, c2, c3


def sample_draws(index: torch.Tensor, pad: int, flip: bool, seed: int, epoch: int):
    """``(dy, dx, f)`` int64 tensors for the dataset indices ``index``."""
    i = index.to("cpu", torch.int64) & _M32
    z = torch.zeros_like(i)
    r = philox4x32_10((i, z + (epoch & _M32), z, z + DOMAIN), (seed & _M32, (seed >> 32) & _M32))
    span = 2 * pad + 1
    dy, dx = (r[0] * span) >> 32, (r[1] * span) >> 32
    f = (r[2] >> 31) if flip else z
    return dy, dx, f


def _check_args(pad: int, seed: int, epoch: int):
    if not 0 <= pad <= MAX_PAD:
        raise ValueError(f"crop padding must be in 0..{MAX_PAD}, got {pad}")
    if not 0 <= seed < (1 << 64):
        raise ValueError(f"seed must be in [0, 2^64), got {seed}")
    if not 0 <= epoch <= _M32:
        raise ValueError(f"epoch must be in [0, 2^32), got {epoch}")


# --------------------------------------------------------------------- dataset
def build_lut(channels: int, mean, std) -> torch.Tensor:
    """``[C, 256]`` bf16: the normalised value of every byte, per channel."""
    v = torch.arange(256, dtype=torch.uint8).view(256, 1, 1, 1).expand(256, channels, 1, 1)
    return normalize_uint8(v, mean, std).to(torch.bfloat16).view(256, channels).t().contiguous()


class DeviceDataset:
    """``images_u8`` [N, C, H, W] uint8 (as the readers return it) kept on
    ``device`` as dense [N, H, W, C] uint8, int64 labels and the bf16 LUT."""

    def __init__(self, images_u8: torch.Tensor, labels: torch.Tensor, mean=CIFAR_MEAN,
                 std=CIFAR_STD, device="cpu"):
        if images_u8.dtype != torch.uint8 or images_u8.dim() != 4:
            raise ValueError("DeviceDataset takes uint8 images [N, C, H, W], got "
                             f"{images_u8.dtype} {tuple(images_u8.shape)}")
        n, c, h, w = images_u8.shape
        if not 1 <= c <= MAX_CHANNELS:
            raise ValueError(f"DeviceDataset takes 1..{MAX_CHANNELS} channels, got {c}")
        if len(mean) < c or len(std) < c:
            raise ValueError(f"mean / std need {c} entries")
        if labels.shape != (n,):
            raise ValueError(f"labels must be [{n}], got {tuple(labels.shape)}")
        nbytes = n * h * w * c
        if n >= (1 << 31) or nbytes >= (1 << 31) or h < 1 or w < 1:
            # the guard of csrc/geom_guard.h (dataset_ok): 32-bit byte offsets
            raise ValueError(f"a device-resident dataset must stay under 2 GiB of uint8 "
                             f"(N*H*W*C = {nbytes}) and 2^31 samples")
        self.device = torch.device(device)
        if self.device.type == "cuda":
            free, _ = torch.cuda.mem_get_info(self.device)
            need = nbytes + 8 * n
            if need + DEVICE_MARGIN_BYTES > free:
                raise MemoryError(
                    f"the dataset needs {need / 2**20:.0f} MiB on {self.device} and must leave "
                    f"{DEVICE_MARGIN_BYTES / 2**20:.0f} MiB free, but only {free / 2**20:.0f} MiB "
                    "are free; use the host loader (drop --device-data) or a smaller --n-train")
        self.n, self.channels, self.height, self.width = n, c, h, w
        self.mean, self.std = tuple(mean[:c]), tuple(std[:c])
        self.data = images_u8.permute(0, 2, 3, 1).contiguous().to(self.device)
        self.labels = labels.to(torch.int64).contiguous().to(self.device)
        self.lut = build_lut(c, mean, std).to(self.device)

    def __len__(self):
        return self.n

    @property
    def shape(self):
        return (self.channels, self.height, self.width)


def quantize_synthetic(x: torch.Tensor) -> torch.Tensor:
    """``u = clamp(round(32 x + 128), 0, 255)``: with mean 128/255 and std 32/255
    the normalised byte is the original ``x`` up to quantisation."""
    return torch.clamp(torch.round(32.0 * x + 128.0), 0, 255).to(torch.uint8)


def get_device_datasets(name: str, data_dir: str, input_shape, num_classes: int, n_train: int,
                        n_test: int, seed: int, device):
    """The device-resident form of :func:`..utils.data.get_datasets`: returns
    ``(train, test, source)`` with the same sources and the same normalisation."""
    name = name.lower()
    readers = {"cifar10": (read_cifar10_binary, CIFAR_MEAN, CIFAR_STD),
               "mnist": (read_mnist_idx, MNIST_MEAN, MNIST_STD)}
    if name in readers:
        read, mean, std = readers[name]
        try:
            xtr, ytr = read(data_dir, True)
            xte, yte = read(data_dir, False)
            return (DeviceDataset(xtr, ytr, mean, std, device),
                    DeviceDataset(xte, yte, mean, std, device), name)
        except FileNotFoundError:
            name = "synthetic"
    if name != "synthetic":
        raise ValueError(f"unknown dataset {name!r}")
    c = input_shape[0]
    if len(input_shape) != 3 or not 1 <= c <= MAX_CHANNELS:
        raise ValueError(f"--device-data needs image inputs [C<={MAX_CHANNELS}, H, W], "
                         f"got {tuple(input_shape)}")
    out = []
    for n, s in ((n_train, seed), (n_test, seed + 1)):
        if n * int(input_shape[0]) * int(input_shape[1]) * int(input_shape[2]) >= (1 << 31):
            raise ValueError(f"{n} synthetic images of {tuple(input_shape)} exceed the 2 GiB of a "
                             "device-resident dataset; lower --n-train / --n-test")
        src = SyntheticImages(n, input_shape, num_classes, seed=s)
        out.append(DeviceDataset(quantize_synthetic(src.x), src.y, (SYNTH_MEAN,) * c,
                                 (SYNTH_STD,) * c, device))
    return out[0], out[1], "synthetic"


# ------------------------------------------------------------------- assembler
def assemble_reference(ds: DeviceDataset, index: torch.Tensor, pad: int = 0, flip: bool = False,
                       seed: int = 0, epoch: int = 0):
    """The definition of a batch (module docstring), in torch on the CPU.

    Returns ``x`` bf16 [B, C, H, W] with channels-last strides, ``y`` int64 [B]
    and ``draws`` int8 [B, 3] holding ``(dy, dx, f)`` per sample."""
    _check_args(pad, seed, epoch)
    index = index.to("cpu", torch.int64).reshape(-1)
    if index.numel() and (int(index.min()) < -(1 << 31) or int(index.max()) >= (1 << 31)):
        raise ValueError("dataset indices must fit int32")
    n, c, h, w = ds.n, ds.channels, ds.height, ds.width
    data, labels, lut = ds.data.cpu(), ds.labels.cpu(), ds.lut.cpu()
    dy, dx, f = sample_draws(index, pad, flip, seed, epoch)
    valid = (index >= 0) & (index < n)
    safe = torch.where(valid, index, torch.zeros_like(index))
    hh = torch.arange(h).view(1, h, 1)
    ww = torch.arange(w).view(1, 1, w)
    f3 = f.view(-1, 1, 1)
    sh = hh + (dy.view(-1, 1, 1) - pad)                                     # [B, H, 1]
    sw = torch.where(f3 != 0, w - 1 - ww, ww) + (dx.view(-1, 1, 1) - pad)   # [B, 1, W]
    inside = valid.view(-1, 1, 1) & (sh >= 0) & (sh < h) & (sw >= 0) & (sw < w)   # [B, H, W]
    flat = (sh.clamp(0, h - 1) * w + sw.clamp(0, w - 1)).view(len(index), h * w)
    src = data.view(n, h * w, c)[safe.view(-1, 1), flat]                    # [B, H*W, C]
    byte = torch.where(inside.view(-1, h * w, 1), src, torch.zeros_like(src)).to(torch.int64)
    x = lut[torch.arange(c).view(1, 1, c), byte].view(len(index), h, w, c).permute(0, 3, 1, 2)
    y = torch.where(valid, labels[safe], torch.full_like(safe, IGNORE_LABEL))
    draws = torch.stack([dy, dx, f], 1).to(torch.int8)
    return x, y, draws


def assemble(ds: DeviceDataset, index: torch.Tensor, count: int, out_x: torch.Tensor,
             out_y: torch.Tensor, draws=None, pad: int = 0, flip: bool = False, seed: int = 0,
             epoch: int = 0):
    """Write the batch of ``index[:count]`` into rows ``[0, count)`` of ``out_x`` /
    ``out_y`` (and ``draws``): the native kernel on a GPU dataset -- a missing
    extension is an error -- and :func:`assemble_reference` on a CPU one."""
    _check_args(pad, seed, epoch)
    if ds.device.type == "cuda":
        from ..ops._ext import native

        native().batch_assemble(ds.data, ds.labels, ds.lut, index, count, out_x, out_y, draws,
                                pad, flip, seed, epoch)
        return
    x, y, d = assemble_reference(ds, index[:count], pad, flip, seed, epoch)
    out_x[:count].copy_(x)
    out_y[:count].copy_(y)
    if draws is not None:
        draws[:count].copy_(d)


# ---------------------------------------------------------------- mixup / cutmix
@dataclass(frozen=True)
class MixConfig:
    """Mixup / CutMix of the training batches (module docstring)."""
    mixup_alpha: float = 0.0
    cutmix_alpha: float = 0.0
    prob: float = 1.0
    switch_prob: float = 0.5

    def __post_init__(self):
        check_mix_config(self.mixup_alpha, self.cutmix_alpha, self.prob, self.switch_prob)


class MixParams(NamedTuple):
    mode: str               # none | mixup | cutmix
    pix_lam: float          # a float32 value: weight of row b's own view outside the box
    label_lam: float        # a float32 value: weight of row b's own label
    box: tuple              # (y0, y1, x0, x1) in output coordinates; empty: (0, 0, 0, 0)


NO_MIX = MixParams("none", 1.0, 1.0, (0, 0, 0, 0))


def check_mix_config(mixup_alpha, cutmix_alpha, prob, switch_prob):
    for name, a in (("mixup", mixup_alpha), ("cutmix", cutmix_alpha)):
        if not (math.isfinite(a) and a >= 0):
            raise ValueError(f"the {name} alpha must be >= 0, got {a}")
    for name, q in (("mix probability", prob), ("mix switch probability", switch_prob)):
        if not 0 <= q <= 1:
            raise ValueError(f"the {name} must be in [0, 1], got {q}")


def _f32(v: float) -> float:
    return float(torch.tensor(v, dtype=torch.float64).to(torch.float32))


def mix_generator(seed: int, epoch: int, batch_no: int) -> torch.Generator:
    """The CPU generator of one batch's mix draw: seeded by (seed, epoch, batch
    number) and a domain constant, never the generator of ``epoch_order``."""
    s = (seed * 0x9E3779B97F4A7C15 + epoch * 0xC2B2AE3D27D4EB4F + batch_no * 0x165667B19E3779F9
         + MIX_DOMAIN) & ((1 << 63) - 1)
    return torch.Generator().manual_seed(s)


def beta_draw(alpha: float, g: torch.Generator, n: int = 1) -> torch.Tensor:
    """``n`` fp64 draws of Beta(alpha, alpha) as ``g1 / (g1 + g2)`` of two gamma draws."""
    gam = torch._standard_gamma(torch.full((2, n), float(alpha), dtype=torch.float64), generator=g)
    return gam[0] / (gam[0] + gam[1])


def mix_draw(seed: int, epoch: int, batch_no: int, H: int, W: int, mixup_alpha: float = 0.0,
             cutmix_alpha: float = 0.0, prob: float = 1.0, switch_prob: float = 0.5) -> MixParams:
    """The mix of one batch (module docstring): timm's mode rule and ``rand_bbox``."""
    check_mix_config(mixup_alpha, cutmix_alpha, prob, switch_prob)
    g = mix_generator(seed, epoch, batch_no)
    u0, u1 = torch.rand(2, generator=g, dtype=torch.float64).tolist()
    if not (u0 < prob and (mixup_alpha > 0 or cutmix_alpha > 0)):
        return NO_MIX
    cut = cutmix_alpha > 0 and (mixup_alpha == 0 or u1 < switch_prob)
    lam = float(beta_draw(cutmix_alpha if cut else mixup_alpha, g)[0])
    if not 0.0 <= lam <= 1.0:           # both gamma draws underflowed to 0
        return NO_MIX
    if not cut:
        return MixParams("mixup", _f32(lam), _f32(lam), (0, 0, 0, 0))
    r = math.sqrt(1.0 - lam)
    ch, cw = int(H * r), int(W * r)
    cy = int(torch.randint(H, (1,), generator=g))
    cx = int(torch.randint(W, (1,), generator=g))
    y0, y1 = min(max(cy - ch // 2, 0), H), min(max(cy + ch // 2, 0), H)
    x0, x1 = min(max(cx - cw // 2, 0), W), min(max(cx + cw // 2, 0), W)
    return MixParams("cutmix", 1.0, _f32(1.0 - (y1 - y0) * (x1 - x0) / (H * W)), (y0, y1, x0, x1))


def _check_mix_params(params: MixParams, h: int, w: int):
    y0, y1, x0, x1 = params.box
    ok = 0 <= y0 <= y1 <= h and 0 <= x0 <= x1 <= w and 0 <= params.pix_lam <= 1 and \
        0 <= params.label_lam <= 1          # the guard of csrc/geom_guard.h (mix_ok)
    if not ok:
        raise ValueError(f"mix parameters out of range for a {h} x {w} image: {params}")


def assemble_mix_reference(ds: DeviceDataset, index: torch.Tensor, params: MixParams,
                           pad: int = 0, flip: bool = False, seed: int = 0, epoch: int = 0):
    """The definition of a mixed batch (module docstring), in torch on the CPU.

    Returns ``x`` bf16 [B, C, H, W], ``y`` and ``y2`` int64 [B] (row b's and its
    partner's label), ``lam`` float32 [B] (``label_lam``) and row b's ``draws``."""
    _check_mix_params(params, ds.height, ds.width)
    a, y, draws = assemble_reference(ds, index, pad, flip, seed, epoch)
    p, y2 = a.flip(0), y.flip(0)                 # row count - 1 - b
    y0, y1, x0, x1 = params.box
    if params.pix_lam == 1:
        x = a
    else:
        lam = torch.tensor(params.pix_lam, dtype=torch.float32)
        x = (a.float() * lam + p.float() * (1 - lam)).to(torch.bfloat16)
    box = torch.zeros((ds.height, ds.width), dtype=torch.bool)
    box[y0:y1, x0:x1] = True
    x = torch.where(box, p, x)
    lam_rows = torch.full((len(y),), params.label_lam, dtype=torch.float32)
    return x, y, y2, lam_rows, draws


def assemble_mix(ds: DeviceDataset, index: torch.Tensor, count: int, out_x: torch.Tensor,
                 out_y: torch.Tensor, out_y2: torch.Tensor, out_lam: torch.Tensor, draws=None,
                 params: MixParams = NO_MIX, pad: int = 0, flip: bool = False, seed: int = 0,
                 epoch: int = 0, path: int = -1):
    """:func:`assemble` with the mix ``params``: also writes rows ``[0, count)`` of
    ``out_y2`` and ``out_lam``.  The native kernel on a GPU dataset -- a missing
    extension is an error -- and :func:`assemble_mix_reference` on a CPU one."""
    _check_args(pad, seed, epoch)
    _check_mix_params(params, ds.height, ds.width)
    if ds.device.type == "cuda":
        from ..ops._ext import native

        native().batch_assemble_mix(ds.data, ds.labels, ds.lut, index, count, out_x, out_y, out_y2,
                                    out_lam, draws, pad, flip, seed, epoch, params.pix_lam,
                                    params.label_lam, *params.box, path)
        return
    x, y, y2, lam, d = assemble_mix_reference(ds, index[:count], params, pad, flip, seed, epoch)
    out_x[:count].copy_(x)
    out_y[:count].copy_(y)
    out_y2[:count].copy_(y2)
    out_lam[:count].copy_(lam)
    if draws is not None:
        draws[:count].copy_(d)


class DeviceLoader:
    """Batches of a :class:`DeviceDataset`, iterable once per epoch.

    Per epoch one ``torch.randperm`` over this rank's shard (the samples ``rank,
    rank + world, ...``) from a CPU generator seeded by ``(seed, epoch)`` is
    uploaded as int32; a step hands the assembler a view of it, so no host
    tensor is created per step.  ``shuffle=False`` (evaluation) serves the shard
    in order, the last, shorter batch at its true length.  ``out_dtype``: what a
    CPU loader casts its batches to (a CPU run computes in fp32); a GPU loader
    writes bf16 only.

    ``mix``: a :class:`MixConfig` sends every batch through :func:`assemble_mix`
    with the draw of ``(seed, epoch, batch number)`` -- the unmixed batches too,
    with ``lam = 1``.  ``next`` still returns ``(x, y)``; the partner labels and
    the weights of that batch are ``last_mix = (y2, lam)``, written into the
    third and fourth buffer of ``out`` when it has them."""

    def __init__(self, ds: DeviceDataset, batch: int, shuffle: bool = True,
                 drop_last: bool = True, pad: int = 0, flip: bool = False, seed: int = 0,
                 rank: int = 0, world: int = 1, out_dtype: torch.dtype = torch.bfloat16,
                 mix: MixConfig | None = None):
        if batch < 1:
            raise ValueError(f"batch must be >= 1, got {batch}")
        if not 0 <= rank < world:
            raise ValueError(f"rank {rank} outside world {world}")
        _check_args(pad, seed, 0)
        if ds.device.type == "cuda" and out_dtype != torch.bfloat16:
            raise ValueError("a GPU DeviceLoader writes bf16 batches only")
        self.ds, self.batch, self.shuffle, self.drop_last = ds, batch, shuffle, drop_last
        self.pad, self.flip, self.seed, self.out_dtype = pad, flip, seed, out_dtype
        self.mix = mix
        self.last_mix = None        # (y2, lam) of the batch next() returned last
        self.last_params = None     # its MixParams
        self.shard = torch.arange(rank, ds.n, world, dtype=torch.int64)
        self.epoch = 0              # the epoch the next start_epoch() opens
        self._perm = None           # this epoch's order, int32 on the dataset's device
        self._cur_epoch = 0
        self._pos = 0

    def __len__(self):
        n = len(self.shard)
        return n // self.batch if self.drop_last else (n + self.batch - 1) // self.batch

    def epoch_order(self, epoch: int) -> torch.Tensor:
        """The shard's dataset indices in the order epoch ``epoch`` visits them (CPU, int64)."""
        if not self.shuffle:
            return self.shard
        g = torch.Generator().manual_seed((self.seed * 0x9E3779B1 + epoch) & ((1 << 63) - 1))
        return self.shard[torch.randperm(len(self.shard), generator=g)]

    def start_epoch(self, epoch: int | None = None):
        """Open epoch ``epoch`` (default: the one after the last opened)."""
        e = self.epoch if epoch is None else epoch
        if self._perm is None or self.shuffle or self._perm.device != self.ds.device:
            self._perm = self.epoch_order(e).to(torch.int32).to(self.ds.device)
        self._cur_epoch, self._pos, self.epoch = e, 0, e + 1

    def remaining(self) -> int:
        """Batches left in the open epoch."""
        if self._perm is None:
            return 0
        left = len(self.shard) - self._pos
        return left // self.batch if self.drop_last else (left + self.batch - 1) // self.batch

    def next(self, out=None):
        """The next batch ``(x, y)``; opens a new epoch when the last is used up.
        ``out``: ``(x, y)`` buffers of at least the batch's length to write into
        (the step graph's static inputs); they are returned themselves when the
        batch fills them."""
        if self.remaining() == 0:
            self.start_epoch()
            if self.remaining() == 0:
                raise ValueError("the shard holds less than one batch")
        ds = self.ds
        count = min(self.batch, len(self.shard) - self._pos)
        index = self._perm[self._pos:self._pos + count]
        batch_no = self._pos // self.batch
        self._pos += count
        if self.mix is not None:
            return self._next_mixed(index, count, batch_no, out)
        if out is not None:
            x, y = out
        else:
            x = torch.empty((count, ds.channels, ds.height, ds.width), dtype=torch.bfloat16,
                            device=ds.device, memory_format=torch.channels_last)
            y = torch.empty(count, dtype=torch.int64, device=ds.device)
        assemble(ds, index, count, x, y, None, self.pad, self.flip, self.seed, self._cur_epoch)
        if x.shape[0] != count:
            x, y = x[:count], y[:count]
        if x.dtype != self.out_dtype:
            x = x.to(self.out_dtype)
        return x, y

    def _next_mixed(self, index, count, batch_no, out):
        ds, m = self.ds, self.mix
        out = tuple(out) if out is not None else ()
        if len(out) >= 2:
            x, y = out[:2]
        else:
            x = torch.empty((count, ds.channels, ds.height, ds.width), dtype=torch.bfloat16,
                            device=ds.device, memory_format=torch.channels_last)
            y = torch.empty(count, dtype=torch.int64, device=ds.device)
        if len(out) >= 4:
            y2, lam = out[2:4]
        else:
            y2 = torch.empty(x.shape[0], dtype=torch.int64, device=ds.device)
            lam = torch.empty(x.shape[0], dtype=torch.float32, device=ds.device)
        params = mix_draw(self.seed, self._cur_epoch, batch_no, ds.height, ds.width,
                          m.mixup_alpha, m.cutmix_alpha, m.prob, m.switch_prob)
        assemble_mix(ds, index, count, x, y, y2, lam, None, params, self.pad, self.flip, self.seed,
                     self._cur_epoch)
        if x.shape[0] != count:
            x, y, y2, lam = x[:count], y[:count], y2[:count], lam[:count]
        if x.dtype != self.out_dtype:
            x = x.to(self.out_dtype)
        self.last_mix, self.last_params = (y2, lam), params
        return x, y

    def iter_into(self, provider=None):
        """One epoch of batches; ``provider()`` returns the ``(x, y)`` buffers the
        next batch is written into (``(x, y, y2, lam)`` for a mixing loader), or
        ``None`` for fresh tensors."""
        self.start_epoch()
        while self.remaining():
            yield self.next(provider() if provider is not None else None)

    def __iter__(self):
        return self.iter_into(None)
