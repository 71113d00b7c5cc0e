"""Mixup / CutMix on the CPU: ``assemble_mix_reference`` against the NumPy oracle
(``mix_oracle.py``) bit for bit, its identities, the per-batch draw, the
two-target loss against fp64, and a CPU training run end to end."""
import csv
import math

import numpy as np
import pytest
import torch

import data_oracle as do
import mix_oracle as mo
from distributed_ml_pytorch_amd.utils import device_data as dd

SEED = mo.SEED


def _dataset(name, seed=21):
    c, h, w, n, pad, flip, norm, index = mo.CASES[name]
    x, y = do.random_dataset(n, c, h, w, seed)
    return x, y, dd.DeviceDataset(x, y, *norm, device="cpu"), pad, flip, index


def _oracle(x, y, ds, index, params, pad, flip, epoch):
    return mo.mix_np(x.numpy(), y.numpy(), do.bits(ds.lut), index, params.pix_lam,
                     params.label_lam, params.box, pad, flip, SEED, epoch)


def _assert_is_oracle(got, want):
    gx, gy, gy2, glam, gd = got
    wx, wy, wy2, wlam, wd = want
    assert gx.dtype == torch.bfloat16 and gy.dtype == gy2.dtype == torch.int64
    assert glam.dtype == torch.float32 and gd.dtype == torch.int8
    assert np.array_equal(do.bits(gx), wx), "x differs from the NumPy oracle"
    assert np.array_equal(gy.numpy(), wy) and np.array_equal(gy2.numpy(), wy2)
    assert np.array_equal(glam.numpy(), wlam) and np.array_equal(gd.numpy().astype(np.int64), wd)


def test_cases_are_those_of_the_plain_assembler_tests():
    import test_device_data_gpu as gpu_tests
    assert mo.CASES == gpu_tests.CASES and mo.STAGED == gpu_tests.STAGED and mo.SEED == gpu_tests.SEED


# ------------------------------------------------------- reference vs oracle
@pytest.mark.parametrize("name", mo.SMALL)
@pytest.mark.parametrize("pix_lam", mo.PIX_LAMS)
def test_reference_equals_oracle_over_the_blend_weights(name, pix_lam):
    """Even and odd count, every pix_lam, no box and a box on top of the blend."""
    x, y, ds, pad, flip, index = _dataset(name)
    h, w = ds.height, ds.width
    for idx in (index, index[:-1] if len(index) > 1 else index):
        for box in ((0, 0, 0, 0), mo.boxes(h, w)["midgroup"]):
            p = dd.MixParams("mixup", mo.f32(pix_lam), mo.f32(0.25), box)
            t = torch.tensor(idx)
            _assert_is_oracle(dd.assemble_mix_reference(ds, t, p, pad, flip, SEED, 3),
                              _oracle(x, y, ds, idx, p, pad, flip, 3))


@pytest.mark.parametrize("name", mo.SMALL)
def test_reference_equals_oracle_over_the_boxes(name):
    x, y, ds, pad, flip, index = _dataset(name)
    area = ds.height * ds.width
    for idx in (index, index[:-1] if len(index) > 1 else index):
        for bname, box in mo.boxes(ds.height, ds.width).items():
            lab = mo.f32(1 - (box[1] - box[0]) * (box[3] - box[2]) / area)
            p = dd.MixParams("cutmix", 1.0, lab, box)
            _assert_is_oracle(dd.assemble_mix_reference(ds, torch.tensor(idx), p, pad, flip, SEED, 0),
                              _oracle(x, y, ds, idx, p, pad, flip, 0))


def test_blend_expression_is_exact_at_weight_one_and_equal_operands():
    """What the definition relies on: ``a * lam + p * (1 - lam)`` in fp32 returns
    ``a`` at lam = 1 and at a == p for every bf16 LUT value and tested weight."""
    a = dd.build_lut(3, (0.4, 0.5, 0.6), (0.2, 0.3, 0.4)).reshape(-1)
    one = torch.tensor(1.0, dtype=torch.float32)
    assert torch.equal((a.float() * one + a.flip(0).float() * (1 - one)).to(torch.bfloat16), a)
    for v in mo.PIX_LAMS:
        lam = torch.tensor(v, dtype=torch.float32)
        assert torch.equal((a.float() * lam + a.float() * (1 - lam)).to(torch.bfloat16), a), v


# ------------------------------------------------------------------ identities
@pytest.mark.parametrize("name", mo.SMALL)
def test_mode_none_is_the_plain_batch(name):
    _, _, ds, pad, flip, index = _dataset(name)
    t = torch.tensor(index)
    x, y, y2, lam, d = dd.assemble_mix_reference(ds, t, dd.NO_MIX, pad, flip, SEED, 1)
    px, py, pd = dd.assemble_reference(ds, t, pad, flip, SEED, 1)
    assert torch.equal(x, px) and torch.equal(y, py) and torch.equal(d, pd)
    assert torch.equal(y2, py.flip(0)) and torch.equal(lam, torch.ones(len(index)))
    assert [int(v) for v in y2] == [int(py[len(index) - 1 - b]) for b in range(len(index))]


@pytest.mark.parametrize("name", mo.SMALL)
def test_weight_zero_and_whole_image_box_give_the_partner(name):
    _, _, ds, pad, flip, index = _dataset(name)
    t = torch.tensor(index)
    px, py, _ = dd.assemble_reference(ds, t, pad, flip, SEED, 2)
    for p in (dd.MixParams("mixup", 0.0, 0.0, (0, 0, 0, 0)),
              dd.MixParams("cutmix", 1.0, 0.0, (0, ds.height, 0, ds.width))):
        x, y, y2, lam, _ = dd.assemble_mix_reference(ds, t, p, pad, flip, SEED, 2)
        for b in range(len(index)):
            assert torch.equal(x[b], px[len(index) - 1 - b]), (p.mode, b)
        assert torch.equal(y, py) and torch.equal(y2, py.flip(0)) and float(lam.max()) == 0.0


def test_out_of_range_index_as_row_and_as_partner():
    x, y, ds, _, _, _ = _dataset("odd_5x7")
    index = [2, 9, -1, 8, 1 << 20, 4]              # partners: 4 <-> 2^20, 9 <-> 8... by position
    pad_img = ds.lut[:, 0].view(3, 1, 1).expand(3, 5, 7)
    t = torch.tensor(index)
    none = dd.assemble_mix_reference(ds, t, dd.NO_MIX, 2, True, SEED, 0)
    assert none[1].tolist()[1:3] == [-100, -100] and none[1].tolist()[4] == -100
    assert none[2].tolist() == none[1].tolist()[::-1]
    assert torch.equal(none[0][1], pad_img) and torch.equal(none[0][4], pad_img)
    swap = dd.assemble_mix_reference(ds, t, dd.MixParams("mixup", 0.0, 0.0, (0, 0, 0, 0)), 2, True,
                                     SEED, 0)
    assert torch.equal(swap[0][0], none[0][5]) and torch.equal(swap[0][3], pad_img)   # partner -1
    assert torch.equal(swap[0][1], pad_img)                                         # partner 2^20
    for p in (dd.MixParams("mixup", mo.f32(0.3172), mo.f32(0.3172), (0, 0, 0, 0)),
              dd.MixParams("cutmix", 1.0, mo.f32(0.5), (1, 4, 2, 6))):
        _assert_is_oracle(dd.assemble_mix_reference(ds, t, p, 2, True, SEED, 0),
                          _oracle(x, y, ds, index, p, 2, True, 0))


def test_assemble_mix_writes_only_the_first_count_rows():
    _, _, ds, pad, flip, index = _dataset("odd_5x7")
    rows, count = 5, 3
    out_x = torch.full((rows, 3, 5, 7), -7.0, dtype=torch.bfloat16)
    out_y, out_y2 = torch.full((rows,), 42), torch.full((rows,), 43)
    out_lam, draws = torch.full((rows,), 9.0), torch.full((rows, 3), 99, dtype=torch.int8)
    p = dd.MixParams("mixup", mo.f32(0.5), mo.f32(0.5), (0, 0, 0, 0))
    dd.assemble_mix(ds, torch.tensor(index + [1, 2]), count, out_x, out_y, out_y2, out_lam, draws, p,
                    pad, flip, SEED, 0)
    want = dd.assemble_mix_reference(ds, torch.tensor(index), p, pad, flip, SEED, 0)
    for g, w in zip((out_x, out_y, out_y2, out_lam, draws), want):
        assert torch.equal(g[:count], w)
    assert bool((out_x[count:] == -7).all()) and out_y[count:].tolist() == [42, 42]
    assert out_y2[count:].tolist() == [43, 43] and out_lam[count:].tolist() == [9.0, 9.0]
    assert bool((draws[count:] == 99).all())
    with pytest.raises(ValueError, match="mix parameters"):
        dd.assemble_mix(ds, torch.tensor(index), count, out_x, out_y, out_y2, out_lam, None,
                        dd.MixParams("cutmix", 1.0, 1.0, (0, 6, 0, 7)))
    with pytest.raises(ValueError, match="mix parameters"):
        dd.assemble_mix(ds, torch.tensor(index), count, out_x, out_y, out_y2, out_lam, None,
                        dd.MixParams("mixup", float("nan"), 1.0, (0, 0, 0, 0)))


# ------------------------------------------------------------------------ draw
MIX = dict(mixup_alpha=0.8, cutmix_alpha=1.0, prob=0.9, switch_prob=0.5)


def test_draw_is_a_function_of_seed_epoch_and_batch():
    base = dd.mix_draw(7, 2, 5, 32, 32, 0.8, 0.0)
    assert base == dd.mix_draw(7, 2, 5, 32, 32, 0.8, 0.0) and base.mode == "mixup"
    for other in ((8, 2, 5), (7, 3, 5), (7, 2, 6)):
        assert dd.mix_draw(*other, 32, 32, 0.8, 0.0) != base, other
    assert dd.mix_draw(7, 2, 5, 32, 32, 0.0, 0.0) == dd.NO_MIX
    assert dd.mix_draw(7, 2, 5, 32, 32, 0.8, 1.0, prob=0.0) == dd.NO_MIX
    assert dd.mix_draw(7, 2, 5, 32, 32, 0.0, 1.0).mode == "cutmix"
    assert dd.mix_draw(7, 2, 5, 32, 32, 0.8, 1.0, switch_prob=0.0).mode == "mixup"
    assert dd.mix_draw(7, 2, 5, 32, 32, 0.8, 1.0, switch_prob=1.0).mode == "cutmix"


def test_epoch_order_has_not_moved():
    """The order of an epoch is what it was before mixing existed: the literal
    permutations, the formula, and no draw of a mixing loader touches it."""
    x, y = do.random_dataset(16, 3, 8, 8, 0)
    ds = dd.DeviceDataset(x, y, device="cpu")
    plain = dd.DeviceLoader(ds, 4, seed=5)
    mixed = dd.DeviceLoader(ds, 4, seed=5, mix=dd.MixConfig(**MIX))
    assert plain.epoch_order(0).tolist() == EPOCH_ORDER_SEED5[0]
    assert plain.epoch_order(3).tolist() == EPOCH_ORDER_SEED5[3]
    for e in (0, 3):
        g = torch.Generator().manual_seed((5 * 0x9E3779B1 + e) & ((1 << 63) - 1))
        assert plain.epoch_order(e).tolist() == torch.randperm(16, generator=g).tolist()
    for e in range(2):
        order, seen = plain.epoch_order(e), 0
        for k, ((px, py), (mx, my)) in enumerate(zip(plain, mixed)):
            seen += 1
            assert torch.equal(py, my) and torch.equal(py, y[order[4 * k:4 * k + 4]])
            y2, lam = mixed.last_mix
            assert torch.equal(y2, py.flip(0))
            want = dd.mix_draw(5, e, k, 8, 8, **MIX)
            assert mixed.last_params == want and torch.equal(lam, torch.full((4,), want.label_lam))
            if want.mode == "none":
                assert torch.equal(px, mx)
        assert seen == 4
    assert plain.last_mix is None


# computed once from DeviceLoader.epoch_order before the mix draw was added
EPOCH_ORDER_SEED5 = {
    0: [14, 10, 2, 0, 15, 4, 3, 9, 7, 1, 12, 13, 8, 6, 11, 5],
    3: [7, 9, 2, 3, 6, 8, 14, 11, 10, 0, 5, 15, 4, 13, 1, 12],
}


def test_draws_over_256_batches():
    modes, H, W = {}, 32, 24
    for k in range(256):
        p = dd.mix_draw(SEED, 1, k, H, W, **MIX)
        modes[p.mode] = modes.get(p.mode, 0) + 1
        y0, y1, x0, x1 = p.box
        assert 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W              # guard::mix_ok
        assert 0.0 <= p.pix_lam <= 1.0 and 0.0 <= p.label_lam <= 1.0
        assert p.pix_lam == mo.f32(p.pix_lam) and p.label_lam == mo.f32(p.label_lam)
        if p.mode == "none":
            assert p == dd.NO_MIX
        elif p.mode == "mixup":
            assert p.box == (0, 0, 0, 0) and p.pix_lam == p.label_lam
        else:
            assert p.pix_lam == 1.0
            assert p.label_lam == float(np.float32(1 - (y1 - y0) * (x1 - x0) / (H * W)))
    print(modes)
    assert set(modes) == {"none", "mixup", "cutmix"} and min(modes.values()) >= 8, modes


def test_beta_draws_have_the_mean_of_the_distribution():
    """Beta(0.8, 0.8): mean 0.5, standard deviation 0.31; over 4096 draws the
    standard error is 0.005, the bound 0.03 six of them."""
    v = dd.beta_draw(0.8, torch.Generator().manual_seed(1234), 4096)
    assert v.dtype == torch.float64 and v.shape == (4096,)
    assert float(v.min()) >= 0.0 and float(v.max()) <= 1.0
    print(float(v.mean()), float(v.std()))
    assert abs(float(v.mean()) - 0.5) <= 0.03
    again = dd.beta_draw(0.8, torch.Generator().manual_seed(1234), 4096)
    assert torch.equal(v, again)
    # the per-batch draw is the same construction
    lams = [dd.mix_draw(3, 0, k, 8, 8, 0.8, 0.0).pix_lam for k in range(4096)]
    assert abs(float(np.mean(lams)) - 0.5) <= 0.03


# ------------------------------------------------------------- loss on the CPU
def _cpu_loss(x, y, y2, lam, smoothing=0.0, gloss=1.0):
    from distributed_ml_pytorch_amd.ops.functional import softmax_cross_entropy_mix

    xr = x.clone().requires_grad_(True)
    loss, hits = softmax_cross_entropy_mix(xr, y, y2, lam, smoothing)
    (loss * gloss).backward()
    return loss.detach().double(), int(hits), xr.grad


@pytest.mark.parametrize("B,C", [(70, 10), (9, 1000), (17, 1025)])
@pytest.mark.parametrize("smoothing", [0.0, 0.1])
def test_cpu_loss_against_fp64(B, C, smoothing):
    import kernel_oracles as ko

    x, y, y2, lam = mo.xent_mix_inputs(B, C, torch.float32, 1)
    y[4], y2[5] = -100, C + 2                         # dropped through either slot
    loss, hits, grad = _cpu_loss(x, y, y2, lam, smoothing, 0.37)
    ref, gref = mo.xent_mix_ref(x, y, y2, lam, smoothing, gloss=0.37)
    torch.testing.assert_close(loss, ref, rtol=1e-5, atol=0.0)
    assert ko.row_abs(grad, gref) <= 1e-5
    assert hits == mo.xent_mix_hits_ref(x, y, y2, lam)
    assert float(grad[4].abs().max()) == 0.0 and float(grad[5].abs().max()) == 0.0


def test_cpu_loss_at_weight_one_is_the_plain_loss():
    from distributed_ml_pytorch_amd.ops.functional import softmax_cross_entropy

    for B, C in ((70, 10), (33, 1000)):
        x, y, y2, _ = mo.xent_mix_inputs(B, C, torch.float32, 2)
        y[::5] = -100
        xr = x.clone().requires_grad_(True)
        want, want_hits = softmax_cross_entropy(xr, y)
        want.backward()
        loss, hits, grad = _cpu_loss(x, y, y2, torch.ones(B))
        assert float(loss) == float(want.detach()) and hits == int(want_hits)
        assert torch.equal(grad, xr.grad)


def test_cpu_loss_ignored_rows_and_zero_weight_targets():
    x, y, y2, lam = mo.xent_mix_inputs(12, 10, torch.float32, 3)
    keep = torch.ones(12, dtype=torch.bool)
    y[2], y2[7], y[9] = -100, -100, 10
    keep[[2, 7, 9]] = False
    full = _cpu_loss(x, y, y2, lam)
    part = _cpu_loss(x[keep], y[keep], y2[keep], lam[keep])
    torch.testing.assert_close(full[0], part[0], rtol=1e-6, atol=0.0)
    assert full[1] == part[1] and float(full[2][~keep].abs().max()) == 0.0
    torch.testing.assert_close(full[2][keep], part[2], rtol=1e-6, atol=1e-9)
    # -inf at a target of weight exactly 0: the loss stays finite
    x2 = x.clone()
    lam2 = lam.clone()
    lam2[0], lam2[1] = 1.0, 0.0
    y2[0] = (int(y[0]) + 1) % 10
    y[1] = (int(y2[1]) + 1) % 10
    x2[0, y2[0]] = x2[1, y[1]] = float("-inf")
    loss, _, grad = _cpu_loss(x2, y, y2, lam2)
    ref, gref = mo.xent_mix_ref(x2, y, y2, lam2)
    assert math.isfinite(float(loss)) and bool(torch.isfinite(grad).all())
    torch.testing.assert_close(loss, ref, rtol=1e-5, atol=0.0)
    # every row dropped: loss 0, gradient 0
    loss, hits, grad = _cpu_loss(x, torch.full((12,), -100), y2, lam)
    assert float(loss) == 0.0 and hits == 0 and float(grad.abs().max()) == 0.0


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_fp32_arithmetic_costs_a_third_of_the_gpu_thresholds_at_most(dtype):
    """The thresholds of tests/test_xent_mix_gpu.py are those of the plain kernel
    (test_xent_edges_gpu): the two-target loss is a convex combination of the
    same per-row quantities.  An fp32 emulation in the kernels' operation order,
    against the fp64 oracle at the shapes of that file, stays within a third of
    each (the project's 3x rule)."""
    import kernel_oracles as ko

    import test_xent_edges_gpu as edges
    for _, B, C in edges.PATHS:
        for smoothing in (0.0, 0.1):
            x, y, y2, lam = mo.xent_mix_inputs(B, C, dtype, 1)
            loss, grad = mo.xent_mix_emulated(x, y, y2, lam, smoothing)
            ref, gref = mo.xent_mix_ref(x, y, y2, lam, smoothing)
            e_loss = abs(float(loss) - float(ref))
            e_grad = ko.row_abs(grad, gref)
            tol_l, tol_g = edges.LOSS_TOL[dtype], edges.GRAD_TOL[dtype]
            bound = tol_l * abs(float(ref)) + (tol_l if dtype == torch.bfloat16 else 0.0)
            print(f"B {B} C {C} eps {smoothing}: loss err {e_loss:.2e} of {bound:.2e}, "
                  f"grad row_abs {e_grad:.2e} of {tol_g:.0e}")
            assert e_loss <= bound / 3 and e_grad <= tol_g / 3


# ------------------------------------------------------------------ end to end
def test_training_with_mixup_and_cutmix_on_the_cpu(tmp_path):
    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, run_training

    do.write_fake_cifar(tmp_path, per_file=8)
    cfg = TrainConfig(model="lenet", dataset="cifar10", data_dir=str(tmp_path), batch_size=8,
                      test_batch_size=5, epochs=1, mode="single", cuda=False, lr=0.01,
                      log_interval=2, device_data=True, augment="crop_flip", mixup=0.8, cutmix=1.0,
                      label_smoothing=0.1, verbose=False, log_dir=str(tmp_path / "log"))
    res = run_training(cfg, DistInfo(device=torch.device("cpu")))
    assert res["data"] == "cifar10+device" and res["steps"] == 5
    assert np.isfinite(res["test_loss"]) and 0.0 <= res["test_accuracy"] <= 1.0
    with open(res["log"]) as f:
        losses = [float(r["training_loss"]) for r in csv.DictReader(f)]
    assert len(losses) == 5 and all(math.isfinite(v) and v > 0 for v in losses), losses


def test_mix_configuration_errors(tmp_path):
    from distributed_ml_pytorch_amd.cli import build_parser, config_from_args
    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, run_training

    info = DistInfo(device=torch.device("cpu"))

    def run(**kw):
        run_training(TrainConfig(model="mlp", mode="single", cuda=False, verbose=False,
                                 log_dir=str(tmp_path), **kw), info)

    with pytest.raises(ValueError, match="--device-data"):
        run(mixup=0.8)
    with pytest.raises(ValueError, match="--device-data"):
        run(cutmix=1.0)
    with pytest.raises(ValueError, match="alpha"):
        run(device_data=True, mixup=-0.1)
    with pytest.raises(ValueError, match="alpha"):
        run(device_data=True, cutmix=-1.0)
    with pytest.raises(ValueError, match="probability"):
        run(device_data=True, mixup=0.8, mix_prob=1.5)
    with pytest.raises(ValueError, match="probability"):
        run(device_data=True, mixup=0.8, cutmix=1.0, mix_switch_prob=-0.2)
    a = build_parser().parse_args(["--no-distributed", "--device-data", "--mixup", "0.8", "--cutmix",
                                   "1.0", "--mix-prob", "0.9", "--mix-switch-prob", "0.25"])
    cfg = config_from_args(a)
    assert (cfg.mixup, cfg.cutmix, cfg.mix_prob, cfg.mix_switch_prob) == (0.8, 1.0, 0.9, 0.25)
    cfg = config_from_args(build_parser().parse_args(["--no-distributed"]))
    assert (cfg.mixup, cfg.cutmix, cfg.mix_prob, cfg.mix_switch_prob) == (0.0, 0.0, 1.0, 0.5)
