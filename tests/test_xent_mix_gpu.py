"""The two-target form of csrc/xent.hip (``softmax_cross_entropy_mix``): every
launch path of launch_xent_t, bf16 and fp32, against the fp64 oracle of
``mix_oracle.py`` with the thresholds ``test_xent_edges_gpu`` uses for the plain
kernel (the two-target loss is a convex combination of the same per-row
quantities; ``test_mix_cpu`` bounds the fp32 arithmetic at a third of them), the
edge rows, and the identity with the plain kernel at ``lam = 1``."""
import numpy as np
import pytest
import torch

import kernel_oracles as ko
import mix_oracle as mo
from test_xent_edges_gpu import DTYPES, GRAD_TOL, LOSS_TOL, PATHS

pytestmark = pytest.mark.gpu

path_dtype = pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f32"])
path_shape = pytest.mark.parametrize("path,B,C", PATHS, ids=[p[0] for p in PATHS])


def _run(x, y, y2, lam, smoothing=0.0, ignore_index=-100, gloss=1.0):
    from distributed_ml_pytorch_amd.ops.functional import softmax_cross_entropy_mix

    xd = x.cuda().requires_grad_(True)
    loss, hits = softmax_cross_entropy_mix(xd, y.cuda(), y2.cuda(), lam.cuda(), smoothing,
                                           ignore_index)
    (loss * gloss).backward()
    assert loss.dtype == torch.float32 and xd.grad.dtype == x.dtype
    return loss.detach().cpu().double(), int(hits.item()), xd.grad.cpu()


def _loss_close(loss, ref, dtype):
    """bf16: rtol = atol = 2e-2; fp32: 1e-5 relative."""
    tol = LOSS_TOL[dtype]
    torch.testing.assert_close(loss, ref, rtol=tol, atol=tol if dtype == torch.bfloat16 else 0.0)


def _check(x, y, y2, lam, smoothing=0.0, ignore_index=-100, gloss=1.0):
    loss, hits, grad = _run(x, y, y2, lam, smoothing, ignore_index, gloss)
    loss_ref, grad_ref = mo.xent_mix_ref(x, y, y2, lam, smoothing, ignore_index, gloss)
    e_grad = ko.row_abs(grad, grad_ref)
    print(f"loss {float(loss):.6f} ref {float(loss_ref):.6f}  grad row_abs {e_grad:.2e}")
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(grad.float()).all())
    _loss_close(loss, loss_ref, x.dtype)
    assert e_grad <= GRAD_TOL[x.dtype], e_grad
    assert hits == mo.xent_mix_hits_ref(x, y, y2, lam, ignore_index)
    return grad


@path_dtype
@path_shape
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
def test_xent_mix_against_fp64(path, B, C, dtype, smoothing):
    """Random weights with rows at exactly 0, 1 and 0.5, rows with y == y2, a
    non-unit incoming gradient."""
    x, y, y2, lam = mo.xent_mix_inputs(B, C, dtype, 1)
    assert float(lam[0]) == 0.0 and float(lam[1]) == 1.0 and float(lam[2]) == 0.5
    assert int(y[3]) == int(y2[3])
    _check(x, y, y2, lam, smoothing=smoothing, gloss=0.37)
    _check(x, y, y2, lam, smoothing=smoothing)


@path_dtype
@path_shape
@pytest.mark.parametrize("ignore_index", [-100, 3])
def test_xent_mix_ignored_through_either_label(path, B, C, dtype, ignore_index):
    """Rows dropped through y, through y2, and by a label out of range in either
    slot: no loss, no gradient, no hit, left out of the mean."""
    x, y, y2, lam = mo.xent_mix_inputs(B, C, dtype, 2)
    y[::5] = ignore_index
    y2[1::5] = ignore_index
    y[2], y2[B - 2] = C + 3, -7
    grad = _check(x, y, y2, lam, ignore_index=ignore_index)
    dead = (y == ignore_index) | (y2 == ignore_index) | (y >= C) | (y2 < 0) | (y < 0) | (y2 >= C)
    assert B // 3 <= int(dead.sum()) < B and float(grad[dead].float().abs().max()) == 0.0
    assert float(grad[~dead].float().abs().max()) > 0.0


@path_dtype
@path_shape
def test_xent_mix_forced_ties_and_the_heavier_target(path, B, C, dtype):
    """Every row holds its maximum twice, at j1 < j2 (the pairs of
    test_xent_edges_gpu); the targets are (j1, j2) or (j2, j1) and lam falls on
    both sides of 0.5 and on it.  First max wins, lam >= 0.5 picks y."""
    x = mo.xent_mix_inputs(B, C, dtype, 3)[0].clamp_(max=4.0)
    pairs = [(2, 7), (4, 5)] if C <= 32 else [(5, 64 * ((C - 1) // 64 - 1) + 37), (40, 67)]
    y, y2 = torch.empty(B, dtype=torch.int64), torch.empty(B, dtype=torch.int64)
    lam = torch.empty(B)
    want = 0
    for r in range(B):
        j1, j2 = pairs[r % 2]
        x[r, j1] = x[r, j2] = 8.0
        swap = (r // 2) % 2 == 1
        y[r], y2[r] = (j2, j1) if swap else (j1, j2)
        lam[r] = (0.5, 0.75, 0.25, 0.4999)[(r // 4) % 4]
        want += int((y[r] if float(lam[r]) >= 0.5 else y2[r]) == j1)
    assert 0 < want < B
    assert bool((np.argmax(x.double().numpy(), 1) == np.array([pairs[r % 2][0] for r in range(B)])).all())
    loss, hits, grad = _run(x, y, y2, lam)
    assert hits == want == mo.xent_mix_hits_ref(x, y, y2, lam)
    loss_ref, grad_ref = mo.xent_mix_ref(x, y, y2, lam)
    _loss_close(loss, loss_ref, dtype)
    assert ko.row_abs(grad, grad_ref) <= GRAD_TOL[dtype]


@path_dtype
@path_shape
def test_xent_mix_neg_inf_logits(path, B, C, dtype):
    """-inf at classes that are no target, and on rows 0 and 1 at the target whose
    weight is exactly 0: the term is not formed (0 * inf), the loss is finite."""
    x, y, y2, lam = mo.xent_mix_inputs(B, C, dtype, 4)
    y2[0], y[1] = (int(y[0]) + 1) % C, (int(y2[1]) + 1) % C
    lam[0], lam[1] = 1.0, 0.0
    for r in range(B):
        for j in ((int(y[r]) + 2) % C, (int(y[r]) + C // 2) % C, (r * 7) % C):
            if j != int(y[r]) and j != int(y2[r]):
                x[r, j] = float("-inf")
    x[0, y2[0]] = x[1, y[1]] = float("-inf")
    loss, hits, grad = _run(x, y, y2, lam)
    loss_ref, grad_ref = mo.xent_mix_ref(x, y, y2, lam)
    assert bool(torch.isfinite(loss_ref)) and bool(torch.isfinite(grad_ref).all())
    assert bool(torch.isfinite(loss)), float(loss)
    assert bool(torch.isfinite(grad.float()).all())
    _loss_close(loss, loss_ref, dtype)
    assert ko.row_abs(grad, grad_ref) <= GRAD_TOL[dtype]
    assert float(grad[torch.isinf(x)].float().abs().max()) == 0.0
    assert hits == mo.xent_mix_hits_ref(x, y, y2, lam)


@path_dtype
@path_shape
def test_xent_mix_all_rows_ignored(path, B, C, dtype):
    x, y, y2, lam = mo.xent_mix_inputs(B, C, dtype, 5)
    y[::2] = -100
    y2[1::2] = -100
    y2[0] = C                                   # out of range next to an ignored label
    loss, hits, grad = _run(x, y, y2, lam)
    assert float(loss) == 0.0 and hits == 0
    assert float(grad.float().abs().max()) == 0.0


@path_dtype
@path_shape
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
def test_xent_mix_at_weight_one_is_the_plain_kernel(path, B, C, dtype, smoothing):
    """lam = 1 and y2 valid: loss, hits and dlogits of the plain kernel, bit for
    bit, ignored rows and a non-unit incoming gradient included."""
    from distributed_ml_pytorch_amd.ops.functional import softmax_cross_entropy

    x, y, y2, _ = mo.xent_mix_inputs(B, C, dtype, 6)
    y[::5] = -100
    for gloss in (1.0, 0.37):
        xd = x.cuda().requires_grad_(True)
        want, want_hits = softmax_cross_entropy(xd, y.cuda(), smoothing)
        (want * gloss).backward()
        xm = x.cuda().requires_grad_(True)
        from distributed_ml_pytorch_amd.ops.functional import softmax_cross_entropy_mix

        loss, hits = softmax_cross_entropy_mix(xm, y.cuda(), y2.cuda(), torch.ones(B, device="cuda"),
                                               smoothing)
        (loss * gloss).backward()
        assert torch.equal(loss, want) and torch.equal(hits, want_hits)
        assert torch.equal(xm.grad, xd.grad)
        assert float(xm.grad.float().abs().max()) > 0.0


def test_binding_rejections():
    from distributed_ml_pytorch_amd.ops._ext import native

    nat = native()
    x = torch.zeros((4, 10), dtype=torch.bfloat16, device="cuda")
    y = torch.zeros(4, dtype=torch.int64, device="cuda")
    lam = torch.ones(4, device="cuda")
    nat.softmax_xent_mix(x, y, y, lam, True, 0.0, -100)
    with pytest.raises(RuntimeError, match="labels2"):
        nat.softmax_xent_mix(x, y, y.to(torch.int32), lam, True, 0.0, -100)
    with pytest.raises(RuntimeError, match="labels2"):
        nat.softmax_xent_mix(x, y, y[:3], lam, True, 0.0, -100)
    with pytest.raises(RuntimeError, match="lam"):
        nat.softmax_xent_mix(x, y, y, lam.double(), True, 0.0, -100)
    with pytest.raises(RuntimeError, match="lam"):
        nat.softmax_xent_mix(x, y, y, lam.cpu(), True, 0.0, -100)
