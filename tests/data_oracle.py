"""Independent NumPy oracle of the device-data batch assembler
(``utils/device_data.py``, ``csrc/data.hip``): a Philox4x32-10 written from the
published definition on Python integers and uint64 arrays, and a literal
``pad -> slice -> flip -> LUT`` assembler, one sample at a time.  Shares no code
with the implementation under test."""
import numpy as np
import torch

PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
]


def philox_np(ctr, key):
    """ctr: 4 uint64 arrays of 32-bit words, key: 2 Python ints.  10 rounds."""
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    mask, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
    c = [np.asarray(v, dtype=np.uint64) & mask for v in ctr]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = m0 * c[0]          # < 2^64: exact in uint64
        p1 = m1 * c[2]
        c = [(p1 >> sh) ^ c[1] ^ np.uint64(k0), p1 & mask, (p0 >> sh) ^ c[3] ^ np.uint64(k1),
             p0 & mask]
        k0 = (k0 + 0x9E3779B9) & 0xFFFFFFFF
        k1 = (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c


def draws_np(index, pad, flip, seed, epoch):
    """[B, 3] int64 (dy, dx, f) of the dataset indices ``index``."""
    i = np.asarray(index, dtype=np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    z = np.zeros_like(i)
    r = philox_np((i, z + np.uint64(epoch), z, z + np.uint64(0x64617461)),
                  (seed & 0xFFFFFFFF, seed >> 32))
    span = np.uint64(2 * pad + 1)
    dy = (r[0] * span) >> np.uint64(32)
    dx = (r[1] * span) >> np.uint64(32)
    f = (r[2] >> np.uint64(31)) if flip else z
    return np.stack([dy, dx, f], 1).astype(np.int64)


def assemble_np(images_u8, labels, lut_bits, index, pad, flip, seed, epoch):
    """images_u8 [N, C, H, W] uint8, lut_bits [C, 256] uint16 (bf16 bit patterns).

    Returns x bits uint16 [B, C, H, W], y int64 [B], draws int64 [B, 3]."""
    images_u8, labels = np.asarray(images_u8), np.asarray(labels)
    n, c, h, w = images_u8.shape
    d = draws_np(index, pad, flip, seed, epoch)
    x = np.zeros((len(index), c, h, w), dtype=np.uint16)
    y = np.zeros(len(index), dtype=np.int64)
    for b, i in enumerate(np.asarray(index, dtype=np.int64)):
        dy, dx, f = (int(v) for v in d[b])
        if 0 <= i < n:
            img, y[b] = images_u8[i], labels[i]
        else:
            img, y[b] = np.zeros((c, h, w), np.uint8), -100
        padded = np.pad(img, ((0, 0), (pad, pad), (pad, pad)))      # black, before normalising
        crop = padded[:, dy:dy + h, dx:dx + w]
        if f:
            crop = crop[:, :, ::-1]
        for ch in range(c):
            x[b, ch] = lut_bits[ch][crop[ch]]
    return x, y, d


def bits(t: torch.Tensor) -> np.ndarray:
    """bf16 tensor (any strides) -> uint16 bit patterns in logical order."""
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def random_dataset(n, c, h, w, seed, classes=10):
    """uint8 images [N, C, H, W] and int64 labels, every byte value present."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (n, c, h, w), generator=g, dtype=torch.uint8)
    y = torch.randint(0, classes, (n,), generator=g)
    return x, y


def write_fake_cifar(root, per_file=8, seed=0):
    """CIFAR-10 binary batches of ``per_file`` random records each under ``root``."""
    rng = np.random.default_rng(seed)
    for name in [f"data_batch_{i}.bin" for i in range(1, 6)] + ["test_batch.bin"]:
        rec = np.zeros((per_file, 3073), dtype=np.uint8)
        rec[:, 0] = rng.integers(0, 10, per_file)
        rec[:, 1:] = rng.integers(0, 256, (per_file, 3072))
        rec.tofile(root / name)
