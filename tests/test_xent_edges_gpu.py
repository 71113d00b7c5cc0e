"""csrc/xent.hip: every launch path of launch_xent_t, bf16 and fp32, against
fp64 F.cross_entropy -- ignore_index and out-of-range labels, forced argmax
ties, wide-range logits, -inf logits, all rows ignored, a non-unit incoming
gradient.  The top-1 reference is NumPy's argmax on the CPU (first occurrence
of the maximum is documented there)."""
import numpy as np
import pytest
import torch

import kernel_oracles as ko

pytestmark = pytest.mark.gpu

# one (B, C) per launch path
PATHS = [("narrow", 70, 10), ("single_cached", 5, 1000), ("single_uncached", 9, 1500),
         ("multi_cached", 40, 1024), ("multi_uncached", 17, 1025)]
DTYPES = [torch.bfloat16, torch.float32]
# loss: rtol = atol; gradient: row_abs over the [B, C] rows
LOSS_TOL = {torch.bfloat16: 2e-2, torch.float32: 1e-5}
GRAD_TOL = {torch.bfloat16: 2e-2, torch.float32: 1e-5}

path_dtype = pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
path_shape = pytest.mark.parametrize("path,B,C", PATHS, ids=[p[0] for p in PATHS])


def test_paths_are_the_ones_named():
    """The (B, C) above against launch_xent_t's dispatch rule."""
    def path(B, C):
        if C <= 32 and B <= (1 << 16):
            return "narrow"
        cached = "cached" if C <= 1024 else "uncached"
        single = B * C <= (1 << 14) or (B <= 16 and C > 1024)
        return ("single_" if single else "multi_") + cached

    assert [path(B, C) for _, B, C in PATHS] == [p[0] for p in PATHS]


def _logits(B, C, dtype, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(seed * 131 + C)
    return (torch.randn(B, C, generator=g) * scale + shift).to(dtype)


def _labels(B, C, seed):
    return torch.randint(0, C, (B,), generator=torch.Generator().manual_seed(seed * 17 + B))


def _run(x, y, smoothing=0.0, ignore_index=-100, gloss=1.0):
    from distributed_ml_pytorch_amd.ops.functional import softmax_cross_entropy

    xd = x.cuda().requires_grad_(True)
    loss, hits = softmax_cross_entropy(xd, y.cuda(), smoothing, ignore_index)
    (loss * gloss).backward()
    assert loss.dtype == torch.float32 and xd.grad.dtype == x.dtype
    return loss.detach().cpu().double(), int(hits.item()), xd.grad.cpu()


def _loss_close(loss, ref, dtype):
    """bf16: rtol = atol = 2e-2; fp32: 1e-5 relative."""
    tol = LOSS_TOL[dtype]
    torch.testing.assert_close(loss, ref, rtol=tol, atol=tol if dtype == torch.bfloat16 else 0.0)


def _check(x, y, smoothing=0.0, ignore_index=-100, gloss=1.0):
    loss, hits, grad = _run(x, y, smoothing, ignore_index, gloss)
    loss_ref, grad_ref = ko.xent_ref(x, y, smoothing, ignore_index, gloss)
    e_grad = ko.row_abs(grad, grad_ref)
    print(f"loss {float(loss):.6f} ref {float(loss_ref):.6f}  grad row_abs {e_grad:.2e}")
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad.float()).all())
    _loss_close(loss, loss_ref, x.dtype)
    assert e_grad <= GRAD_TOL[x.dtype], e_grad
    assert hits == ko.xent_hits_ref(x, y, ignore_index)
    return grad


@path_dtype
@path_shape
@pytest.mark.parametrize("ignore_index", [-100, 3])
def test_xent_ignore_index(path, B, C, dtype, ignore_index):
    """A third of the rows ignored, one label out of range (treated as ignored)."""
    x, y = _logits(B, C, dtype, 1), _labels(B, C, 1)
    y[::3] = ignore_index
    y[1] = C + 3
    grad = _check(x, y, ignore_index=ignore_index)
    dead = (y == ignore_index) | (y >= C)
    assert int(dead.sum()) > B // 3 and float(grad[dead].float().abs().max()) == 0.0


@path_dtype
@path_shape
def test_xent_forced_ties(path, B, C, dtype):
    """Every row holds its maximum twice, at j1 < j2 in different lanes and
    different 64-chunks -- on odd rows j2 sits in the LOWER lane, so the
    cross-lane fold must compare indices, not lanes.  First max wins: only the
    rows labelled j1 are hits."""
    x = _logits(B, C, dtype, 2).clamp_(max=4.0)
    if C <= 32:
        pairs = [(2, 7), (4, 5)]
    else:
        pairs = [(5, 64 * ((C - 1) // 64 - 1) + 37), (40, 67)]
    y = torch.empty(B, dtype=torch.int64)
    n_first = 0
    for r in range(B):
        j1, j2 = pairs[r % 2]
        assert j1 < j2 < C
        x[r, j1] = x[r, j2] = 8.0
        first = (r // 2) % 2 == 0
        y[r] = j1 if first else j2
        n_first += first
    assert 0 < n_first < B
    assert bool((np.argmax(x.double().numpy(), 1) == np.array([pairs[r % 2][0] for r in range(B)])).all())
    loss, hits, grad = _run(x, y)
    assert hits == n_first == ko.xent_hits_ref(x, y)
    loss_ref, grad_ref = ko.xent_ref(x, y)
    _loss_close(loss, loss_ref, dtype)
    assert ko.row_abs(grad, grad_ref) <= GRAD_TOL[dtype]


@path_dtype
@path_shape
def test_xent_wide_range(path, B, C, dtype):
    """fp32 logits randn * 1e3 + 1e4, bf16 logits randn * 60: the max-subtraction
    and the shifted sums carry the whole result."""
    if dtype == torch.float32:
        x = _logits(B, C, dtype, 3, 1e3, 1e4)
    else:
        x = _logits(B, C, dtype, 3, 60.0)
    _check(x, _labels(B, C, 3))


@path_dtype
@path_shape
def test_xent_neg_inf_logits(path, B, C, dtype):
    """-inf at non-label classes.  label_smoothing = 0: the loss is finite and
    matches (the smoothing term eps * (lse - mean(x)) must not be formed at eps = 0:
    0 * inf); smoothing 0.1: +inf on both sides."""
    x, y = _logits(B, C, dtype, 4), _labels(B, C, 4)
    for r in range(B):
        for j in ((int(y[r]) + 1) % C, (int(y[r]) + C // 2) % C, (r * 7) % C):
            if j != int(y[r]):
                x[r, j] = float("-inf")
    x[0, 0] = float("-inf") if int(y[0]) != 0 else x[0, 0]     # a leading -inf (narrow: m = v[0])
    loss, hits, grad = _run(x, y)
    loss_ref, grad_ref = ko.xent_ref(x, y)
    assert bool(torch.isfinite(loss_ref)) and bool(torch.isfinite(grad_ref).all())
    assert bool(torch.isfinite(loss)), float(loss)
    assert bool(torch.isfinite(grad.float()).all())
    _loss_close(loss, loss_ref, dtype)
    assert ko.row_abs(grad, grad_ref) <= GRAD_TOL[dtype]
    assert float(grad[torch.isinf(x)].float().abs().max()) == 0.0
    assert hits == ko.xent_hits_ref(x, y)

    loss_s, _, grad_s = _run(x, y, smoothing=0.1)
    loss_ref_s, _ = ko.xent_ref(x, y, smoothing=0.1)
    assert float(loss_ref_s) == float("inf") and float(loss_s) == float("inf")
    assert bool(torch.isfinite(grad_s.float()).all())


@path_dtype
@path_shape
def test_xent_all_rows_ignored(path, B, C, dtype):
    """The kernel divides by max(#valid, 1): loss == 0 and a zero gradient.
    F.cross_entropy returns NaN here (0 / 0); the difference is deliberate -- a
    batch without a single valid label must not poison the parameters."""
    x = _logits(B, C, dtype, 5)
    y = torch.full((B,), -100, dtype=torch.int64)
    y[B // 2] = C           # out of range counts as ignored too
    loss, hits, grad = _run(x, y)
    assert float(loss) == 0.0 and hits == 0
    assert float(grad.float().abs().max()) == 0.0
    y[B // 2] = -100
    assert bool(torch.isnan(torch.nn.functional.cross_entropy(x.double(), y)))


@path_dtype
@path_shape
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
def test_xent_non_unit_incoming_gradient(path, B, C, dtype, smoothing):
    _check(_logits(B, C, dtype, 6), _labels(B, C, 6), smoothing=smoothing, gloss=0.37)
