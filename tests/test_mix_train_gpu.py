"""Training with Mixup / CutMix on the GPU: the device loader's mixing assembler
feeding the captured step's four input buffers, the two-target loss inside the
graph, and both against the plain path and the CPU loss."""
import math

import pytest
import torch

import data_oracle as do
from distributed_ml_pytorch_amd.utils import device_data as dd
from distributed_ml_pytorch_amd.utils.data import CIFAR_MEAN, CIFAR_STD, read_cifar10_binary
from test_xent_edges_gpu import LOSS_TOL

pytestmark = pytest.mark.gpu


def _is_copy(name: str) -> bool:
    return name.startswith(("__amd_rocclr_copyBuffer", "Memcpy", "memcpy"))


def _kernels(prof):
    return [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def _setup(tmp_path, per_file, **kw):
    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import (TrainConfig, Worker,
                                                            make_device_loaders)

    info = DistInfo(device=torch.device("cuda", 0))
    cfg = TrainConfig(dataset="cifar10", data_dir=str(tmp_path), batch_size=32, mode="single",
                      lr=0.01, evaluate=False, verbose=False, device_data=True, **kw)
    w = Worker(cfg, info)
    train, test, source = make_device_loaders(cfg, info, w)
    assert source == "cifar10+device" and len(train) == 5 * per_file // 32
    assert test.mix is None and (train.mix is not None) == w.mixes     # evaluation never mixes
    return w, train, test


@pytest.mark.strict_native
def test_mixed_training_fed_by_the_device_loader_runs_only_native_kernels(tmp_path):
    """ResNet-18, batch 32, crop + flip, Mixup 0.8 + CutMix 1.0, graph-replayed:
    a replayed step -- mixing assembly and two-target loss included -- is dmp::
    kernels only, with no copy of any kind, in the graph's own four buffers."""
    from torch.profiler import ProfilerActivity, profile

    do.write_fake_cifar(tmp_path, per_file=32)
    w, train, test = _setup(tmp_path, 32, model="resnet18", augment="crop_flip", mixup=0.8,
                            cutmix=1.0)
    assert w.enable_graph(True)
    assert w.static_inputs() is None and w.static_mix_inputs() is None
    losses, modes = [], []
    batches = train.iter_into(w.static_batch_buffers)
    for _ in range(3):                                   # step 1 captures, 2 and 3 replay
        x, y = next(batches)
        losses.append(w.train_step(x, y, keep=False, mix=train.last_mix)[0].clone())
        modes.append(train.last_params.mode)
    gx, gy = w.static_inputs()
    gy2, glam = w.static_mix_inputs()
    assert x is gx and y is gy and train.last_mix[0] is gy2 and train.last_mix[1] is glam
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        x, y = next(batches)                             # a step inside the epoch
        loss, _ = w.train_step(x, y, keep=False, mix=train.last_mix)
        torch.cuda.synchronize()
    assert x is gx and y is gy and train.last_mix[0] is gy2 and train.last_mix[1] is glam
    assert w.graph is not None
    assert torch.equal(gy2, gy.flip(0))
    assert torch.equal(glam, torch.full_like(glam, train.last_params.label_lam))
    losses.append(loss.clone())
    modes.append(train.last_params.mode)
    for x, y in train:                                   # the next epoch, fresh tensors: copied in
        losses.append(w.train_step(x, y, keep=False, mix=train.last_mix)[0].clone())
        modes.append(train.last_params.mode)
    names = _kernels(prof)
    assert any("batch_assemble_mix" in n for n in names), names
    assert any("xent_mix" in n for n in names), names
    assert sum("dmp::" in n for n in names) >= 20, names   # the replayed graph's kernels are seen
    foreign = sorted({n for n in names if "dmp::" not in n})
    assert not foreign, f"not dmp:: kernels in a mixed device-fed replayed step: {foreign}"
    assert not [n for n in names if _is_copy(n)]
    assert len(losses) == 9 and set(modes) <= {"mixup", "cutmix"}, modes
    assert all(math.isfinite(float(v.float())) and float(v.float()) > 0 for v in losses), losses
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        vl, va = w.evaluate(test)                        # unchanged: unmixed batches, the plain loss
        torch.cuda.synchronize()
    assert math.isfinite(vl) and 0.0 <= va <= 1.0
    names = _kernels(prof)
    assert any("softmax_xent" in n for n in names), names
    assert not [n for n in names if "xent_mix" in n or "batch_assemble_mix" in n], names
    with pytest.raises(ValueError, match="mix="):
        w.train_step(gx, gy, keep=False)                 # a mixing run without the second target
    w.finish()


def test_mixing_configured_but_never_applied_is_the_plain_step_bit_for_bit(tmp_path):
    """mixup 0.8 with mix_prob 0: every batch goes through the mixing assembler
    and the two-target loss with lam = 1, and the first step has the loss and the
    hits of the same step of a run without mixing.  LeNet: its step is
    reproducible bit for bit (no atomically accumulated statistics)."""
    do.write_fake_cifar(tmp_path, per_file=16)
    wm, train_m, _ = _setup(tmp_path, 16, model="lenet", mixup=0.8, mix_prob=0.0)
    x, y = train_m.next()
    y2, lam = train_m.last_mix
    assert train_m.last_params == dd.NO_MIX and torch.equal(lam, torch.ones_like(lam))
    assert torch.equal(y2, y.flip(0))
    loss_m, hits_m = wm.train_step(x, y, mix=(y2, lam))
    wm.finish()

    wp, train_p, _ = _setup(tmp_path, 16, model="lenet")
    px, py = train_p.next()
    assert train_p.last_mix is None and torch.equal(px, x) and torch.equal(py, y)
    loss_p, hits_p = wp.train_step(px, py)
    wp.finish()
    assert torch.equal(loss_m, loss_p) and torch.equal(hits_m, hits_p), (loss_m, loss_p)


def test_the_loss_of_a_mixup_step_is_the_cpu_loss_of_its_logits(tmp_path):
    """One Mixup batch through LeNet: the batch is assemble_mix_reference's, and
    the step's loss is the CPU softmax_cross_entropy_mix of the logits the model
    gives for it, within the bf16 loss threshold of the kernel tests."""
    from distributed_ml_pytorch_amd.ops.functional import softmax_cross_entropy_mix

    do.write_fake_cifar(tmp_path, per_file=16)
    w, train, _ = _setup(tmp_path, 16, model="lenet", mixup=0.8, label_smoothing=0.1)
    order = train.epoch_order(0)[:32]
    x, y = train.next()
    y2, lam = train.last_mix
    p = train.last_params
    assert p.mode == "mixup" and 0.0 < p.pix_lam < 1.0 and p.pix_lam == p.label_lam
    xs, ys = read_cifar10_binary(str(tmp_path), True)
    cpu = dd.DeviceDataset(xs, ys, CIFAR_MEAN, CIFAR_STD, device="cpu")
    wx, wy, wy2, wlam, _ = dd.assemble_mix_reference(cpu, order, p, 0, False, train.seed, 0)
    assert torch.equal(x.cpu(), wx) and torch.equal(y.cpu(), wy)
    assert torch.equal(y2.cpu(), wy2) and torch.equal(lam.cpu(), wlam)
    with torch.no_grad():
        logits = w.model(x)
    loss, hits = w.train_step(x, y, mix=(y2, lam))
    w.finish()
    want, want_hits = softmax_cross_entropy_mix(logits.cpu(), wy, wy2, wlam, 0.1)
    tol = LOSS_TOL[torch.bfloat16]
    print(f"step loss {float(loss):.6f}, CPU loss of its logits {float(want):.6f}")
    torch.testing.assert_close(loss.cpu().float(), want.float(), rtol=tol, atol=tol)
    assert 0 <= int(hits) <= 32 and 0 <= int(want_hits) <= 32
