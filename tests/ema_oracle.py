"""Model-EMA oracle in NumPy, independent of torch: the (u, D, O) sequence of
parallel/fused_optim.py in float64 and the three-rounding update in float32.

    t % K != 0:  no update (D = 1, O = 0)
    u   = t / K
    d_u = min(decay32, (1 + u) / (10 + u))  with warmup, else decay32   (float64)
    D, O = float32(d_u), float32(1 - d_u)    (the difference in float64)
    e   = fl32(fl32(D * e) + fl32(O * p))

NumPy float32 arithmetic rounds every operation on its own: ``D * e`` and
``O * p`` are float32 arrays before they are added, so nothing contracts.
"""
import numpy as np


def coeffs(decay, every, warmup, t):
    """(u, D, O) of optimizer step t (1-based); D and O as np.float32."""
    u = t // every
    if t % every:
        return u, np.float32(1.0), np.float32(0.0)
    d = np.float64(np.float32(decay))
    if warmup:
        d = min(d, np.float64(1 + u) / np.float64(10 + u))
    return u, np.float32(d), np.float32(np.float64(1.0) - d)


def update(e, p, D, O):
    """One EMA update of float32 arrays (returns a new array); O == 0: untouched."""
    e = np.asarray(e, dtype=np.float32)
    p = np.asarray(p, dtype=np.float32)
    if O == 0:
        return e.copy()
    a = (np.float32(D) * e).astype(np.float32)
    b = (np.float32(O) * p).astype(np.float32)
    return (a + b).astype(np.float32)


def replay(e0, ps, decay, every, warmup, t0=0):
    """EMA after the parameter read-backs ``ps`` of steps t0+1, t0+2, ..."""
    e = np.asarray(e0, dtype=np.float32).copy()
    for i, p in enumerate(ps):
        _, D, O = coeffs(decay, every, warmup, t0 + i + 1)
        e = update(e, p, D, O)
    return e


def to_np(t):
    return t.detach().cpu().numpy()
