"""The batch assembler kernel (``csrc/data.hip``) against its definition,
``utils/device_data.assemble_reference``: bit for bit in the images, the labels
and the draws, for both forms of the kernel (images staged through LDS, and the
direct gather), plus the binding's rejections, graph capture, and training fed by
the device loader end to end."""
import math

import pytest
import torch

import data_oracle as do
from distributed_ml_pytorch_amd.utils import device_data as dd
from distributed_ml_pytorch_amd.utils.data import normalize_uint8, read_cifar10_binary

pytestmark = pytest.mark.gpu

DEV = "cuda"
MNIST = ((0.1307,), (0.3081,))
HALF = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
SEED = (0xABCD << 32) | 0x1234


def _native():
    from distributed_ml_pytorch_amd.ops._ext import native

    return native()


def _pair(n, c, h, w, seed, norm):
    """The same dataset on the CPU (for the reference) and on the GPU."""
    x, y = do.random_dataset(n, c, h, w, seed)
    return dd.DeviceDataset(x, y, *norm, device="cpu"), dd.DeviceDataset(x, y, *norm, device=DEV)


def _launch(ds, index, pad, flip, epoch, rows=None, draws=True, path=-1, seed=SEED):
    b = len(index) if rows is None else rows
    x = torch.empty((b, ds.channels, ds.height, ds.width), dtype=torch.bfloat16, device=DEV,
                    memory_format=torch.channels_last)
    y = torch.empty(b, dtype=torch.int64, device=DEV)
    d = torch.empty((b, 3), dtype=torch.int8, device=DEV) if draws else None
    _native().batch_assemble(ds.data, ds.labels, ds.lut, index.to(DEV, torch.int32), len(index),
                             x, y, d, pad, flip, seed, epoch, path)
    return x, y, d


def _assert_equal(got, want):
    for g, w, what in zip(got, want, ("x", "y", "draws")):
        assert g.shape == w.shape and g.dtype == w.dtype, what
        assert torch.equal(g.cpu(), w), f"{what} differs from assemble_reference"


CASES = {
    # name: (C, H, W, N, pad, flip, norm, index)
    "cifar": (3, 32, 32, 64, 4, True, HALF, [0, 63, 5, 5, 17, 63, 0, 31, 8, 9, 10, 11, 62, 1, 5, 40]),
    "mnist": (1, 28, 28, 12, 2, False, MNIST, [11, 0, 3, 3, 7]),
    "odd_5x7": (3, 5, 7, 9, 3, False, HALF, [8, 0, 4]),           # 105-byte images, unaligned
    "imagenet": (3, 224, 224, 4, 0, True, HALF, [3, 0]),          # too large to stage
    "rgba_3x5": (4, 3, 5, 6, 16, True, ((0.4, 0.5, 0.6, 0.7), (0.2, 0.3, 0.4, 0.5)), [5, 0, 2, 2]),
}


STAGED = ("cifar", "mnist")          # 16-byte-multiple images that fit the LDS stage


@pytest.mark.parametrize("name,path", [(n, -1) for n in sorted(CASES)] + [(n, 0) for n in STAGED])
def test_kernel_equals_reference(name, path):
    """path -1: the form the launcher picks; 0: the direct gather on a staged shape."""
    c, h, w, n, pad, flip, norm, index = CASES[name]
    cpu, gpu = _pair(n, c, h, w, 21, norm)
    assert _native().batch_assemble_is_staged(gpu.data) == (name in STAGED)   # both forms run
    index = torch.tensor(index)
    for epoch in (0, 3):
        _assert_equal(_launch(gpu, index, pad, flip, epoch, path=path),
                      dd.assemble_reference(cpu, index, pad, flip, SEED, epoch))


@pytest.mark.parametrize("path", [-1, 0], ids=["staged", "direct"])
def test_whole_dataset_in_one_launch(path):
    """4096 samples of 8x8, pad 1, flip: all 18 draws occur, many workgroups."""
    cpu, gpu = _pair(4096, 3, 8, 8, 2, HALF)
    index = torch.arange(4096)
    got = _launch(gpu, index, 1, True, 0, path=path, seed=1234)
    _assert_equal(got, dd.assemble_reference(cpu, index, 1, True, 1234, 0))
    assert len(torch.unique(got[2].cpu().to(torch.int64), dim=0)) == 18


def test_no_augmentation_is_the_host_normalisation():
    x, y = do.random_dataset(40, 3, 32, 32, 8)
    gpu = dd.DeviceDataset(x, y, *HALF, device=DEV)
    index = torch.tensor([39, 0, 7, 7, 20])
    gx, gy, gd = _launch(gpu, index, 0, False, 5)
    assert torch.equal(gx.cpu(), normalize_uint8(x)[index].to(torch.bfloat16))
    assert torch.equal(gy.cpu(), y[index]) and int(gd.abs().max()) == 0


@pytest.mark.parametrize("name,offset", [("cifar", 16), ("cifar", 3), ("odd_5x7", 5)])
def test_count_below_rows_leaves_the_rest_untouched(name, offset):
    """Output carved out of a larger sentinel-filled buffer (16-byte aligned and
    not): rows >= count and the bytes on both sides stay as they were."""
    c, h, w, n, pad, flip, norm, _ = CASES[name]
    cpu, gpu = _pair(n, c, h, w, 4, norm)
    rows, count, img = 8, 5, c * h * w
    index = torch.arange(count) % n
    sx = torch.full((offset + rows * img + 64,), -7.0, dtype=torch.bfloat16, device=DEV)
    sy = torch.full((rows + 6,), 4242, dtype=torch.int64, device=DEV)
    sd = torch.full((rows + 2, 3), 99, dtype=torch.int8, device=DEV)
    out_x = sx[offset:offset + rows * img].view(rows, h, w, c).permute(0, 3, 1, 2)
    out_y, out_d = sy[3:3 + rows], sd[1:1 + rows]
    _native().batch_assemble(gpu.data, gpu.labels, gpu.lut, index.to(DEV, torch.int32), count,
                             out_x, out_y, out_d, pad, flip, SEED, 1)
    want = dd.assemble_reference(cpu, index, pad, flip, SEED, 1)
    _assert_equal((out_x[:count], out_y[:count], out_d[:count]), want)
    lo, hi = offset + count * img, offset + rows * img
    assert bool((sx[:offset] == -7).all()) and bool((sx[lo:] == -7).all()) and hi <= sx.numel()
    assert bool((sy[:3] == 4242).all()) and bool((sy[3 + count:] == 4242).all())
    assert bool((sd[:1] == 99).all()) and bool((sd[1 + count:] == 99).all())


def test_draws_none_and_out_of_range_index():
    cpu, gpu = _pair(9, 3, 8, 8, 6, HALF)
    index = torch.tensor([2, 9, -1, 8, 1 << 20])
    gx, gy, none = _launch(gpu, index, 2, True, 0, draws=False)
    assert none is None
    wx, wy, wd = dd.assemble_reference(cpu, index, 2, True, SEED, 0)
    assert torch.equal(gx.cpu(), wx) and torch.equal(gy.cpu(), wy)
    assert wy.tolist()[1:3] == [-100, -100] and wy.tolist()[4] == -100
    assert torch.equal(gx[1].cpu(), cpu.lut[:, 0].view(3, 1, 1).expand(3, 8, 8))   # all padding
    _assert_equal(_launch(gpu, index, 2, True, 0), (wx, wy, wd))


def test_dataset_that_does_not_fit_is_refused(monkeypatch):
    """Less free device memory than the dataset plus the stated margin: refused
    before anything is uploaded."""
    x, y = do.random_dataset(64, 3, 32, 32, 0)
    need = x.numel() + 8 * 64
    monkeypatch.setattr(torch.cuda, "mem_get_info",
                        lambda dev=None: (need + dd.DEVICE_MARGIN_BYTES - 1, 1 << 40))
    with pytest.raises(MemoryError, match="MiB free"):
        dd.DeviceDataset(x, y, *HALF, device=DEV)
    monkeypatch.setattr(torch.cuda, "mem_get_info",
                        lambda dev=None: (need + dd.DEVICE_MARGIN_BYTES, 1 << 40))
    assert len(dd.DeviceDataset(x, y, *HALF, device=DEV)) == 64


def test_binding_rejections():
    nat = _native()
    _, ds = _pair(8, 3, 8, 8, 1, HALF)
    idx = torch.arange(4, dtype=torch.int32, device=DEV)

    def call(data=ds.data, labels=ds.labels, lut=ds.lut, index=idx, count=4, x=None, y=None,
             draws=None, pad=1):
        x = torch.empty((4, 3, 8, 8), dtype=torch.bfloat16, device=DEV,
                        memory_format=torch.channels_last) if x is None else x
        y = torch.empty(4, dtype=torch.int64, device=DEV) if y is None else y
        nat.batch_assemble(data, labels, lut, index, count, x, y, draws, pad, True, 1, 0)

    call()                                                               # the valid form
    with pytest.raises(RuntimeError, match="uint8"):
        call(data=ds.data.to(torch.int8))
    with pytest.raises(RuntimeError, match="labels"):
        call(labels=ds.labels.to(torch.int32))
    with pytest.raises(RuntimeError, match="index"):
        call(index=idx.to(torch.int64))
    with pytest.raises(RuntimeError, match="out_x"):
        call(x=torch.empty((4, 3, 8, 8), dtype=torch.float16, device=DEV,
                           memory_format=torch.channels_last))
    with pytest.raises(RuntimeError, match="channels_last"):
        call(x=torch.empty((4, 3, 8, 8), dtype=torch.bfloat16, device=DEV))   # NCHW-contiguous
    with pytest.raises(RuntimeError, match="out_x"):
        call(x=torch.empty((3, 3, 8, 8), dtype=torch.bfloat16, device=DEV,
                           memory_format=torch.channels_last))                 # fewer rows than count
    with pytest.raises(RuntimeError, match="out_y"):
        call(y=torch.empty(4, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="pad"):
        call(pad=17)
    with pytest.raises(RuntimeError, match="pad"):
        call(pad=-1)
    with pytest.raises(RuntimeError, match="lut"):
        call(lut=torch.zeros((4, 256), dtype=torch.bfloat16, device=DEV))
    with pytest.raises(RuntimeError, match="lut"):
        call(lut=ds.lut.float())
    with pytest.raises(RuntimeError, match="draws"):
        call(draws=torch.zeros((4, 3), dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="GPU"):
        call(labels=ds.labels.cpu())
    with pytest.raises(RuntimeError, match="index"):
        call(count=5)                                                     # index shorter than count


def test_two_launches_in_one_graph_replay_the_eager_bits():
    _, gpu = _pair(64, 3, 32, 32, 3, HALF)
    nat = _native()
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(0)).to(DEV, torch.int32)
    outs = []
    for _ in range(2):
        outs.append((torch.empty((16, 3, 32, 32), dtype=torch.bfloat16, device=DEV,
                                 memory_format=torch.channels_last).zero_(),
                     torch.zeros(16, dtype=torch.int64, device=DEV),
                     torch.zeros((16, 3), dtype=torch.int8, device=DEV)))

    def both():
        for k, (x, y, d) in enumerate(outs):
            nat.batch_assemble(gpu.data, gpu.labels, gpu.lut, perm[16 * k:16 * k + 16], 16, x, y, d,
                               4, True, SEED, 2 + k)

    both()
    torch.cuda.synchronize()
    eager = [tuple(t.clone() for t in o) for o in outs]
    for o in outs:
        for t in o:
            t.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        both()
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    for o, e in zip(outs, eager):
        for t, w in zip(o, e):
            assert torch.equal(t, w)


def _is_copy(name: str) -> bool:
    return name.startswith(("__amd_rocclr_copyBuffer", "Memcpy", "memcpy"))


@pytest.mark.strict_native
def test_training_fed_by_the_device_loader_runs_only_native_kernels(tmp_path):
    """ResNet-18, batch 32, crop + flip, graph-replayed steps from a CIFAR
    directory: the loss stays finite, and a replayed step -- the batch assembly
    included -- is dmp:: kernels only, with no copy of any kind."""
    from torch.profiler import ProfilerActivity, profile

    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import (TrainConfig, Worker,
                                                            make_device_loaders)

    do.write_fake_cifar(tmp_path, per_file=32)
    info = DistInfo(device=torch.device("cuda", 0))
    cfg = TrainConfig(model="resnet18", dataset="cifar10", data_dir=str(tmp_path), batch_size=32,
                      mode="single", lr=0.01, evaluate=False, verbose=False, device_data=True,
                      augment="crop_flip")
    w = Worker(cfg, info)
    assert w.enable_graph(True)
    train, test, source = make_device_loaders(cfg, info, w)
    assert source == "cifar10+device" and len(train) == 5 and w.static_inputs() is None
    losses = []
    batches = train.iter_into(w.static_inputs)           # one epoch: the order is uploaded once
    for _ in range(3):                                   # step 1 captures, 2 and 3 replay
        x, y = next(batches)
        losses.append(w.train_step(x, y, keep=False)[0].clone())
    gx, gy = w.static_inputs()
    assert x is gx and y is gy                           # written in place, replayed in place
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        x, y = next(batches)                             # a step inside the epoch
        loss, _ = w.train_step(x, y, keep=False)
        torch.cuda.synchronize()
    assert x is gx and y is gy and w.graph is not None
    losses.append(loss.clone())
    for x, y in train:                                   # the next epoch, fresh tensors: copied in
        losses.append(w.train_step(x, y, keep=False)[0].clone())
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    assert any("batch_assemble_kernel" in n for n in names), names
    assert sum("dmp::" in n for n in names) >= 20, names   # the replayed graph's kernels are seen
    foreign = sorted({n for n in names if "dmp::" not in n})
    assert not foreign, f"not dmp:: kernels in a device-fed replayed step: {foreign}"
    assert not [n for n in names if _is_copy(n)]
    assert all(math.isfinite(float(v.float())) and float(v.float()) > 0 for v in losses), losses
    vl, va = w.evaluate(test)                            # the device test loader, unchanged evaluate
    assert math.isfinite(vl) and 0.0 <= va <= 1.0
    w.finish()


def test_first_step_equals_the_host_fed_step_bit_for_bit(tmp_path):
    """augment none: the first training step fed by the device loader has the
    loss and the hits of the same step fed the same samples through
    normalize_uint8 + Worker.prepare.  LeNet: its forward has no atomically
    accumulated statistics, so the step itself is reproducible bit for bit."""
    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import (TrainConfig, Worker,
                                                            make_device_loaders)

    do.write_fake_cifar(tmp_path, per_file=16)
    info = DistInfo(device=torch.device("cuda", 0))
    cfg = TrainConfig(model="lenet", dataset="cifar10", data_dir=str(tmp_path), batch_size=32,
                      mode="single", lr=0.01, evaluate=False, verbose=False, device_data=True)
    w = Worker(cfg, info)
    train, _, _ = make_device_loaders(cfg, info, w)
    order = train.epoch_order(0)[:32]
    x, y = train.next()
    loss_d, hits_d = w.train_step(x, y)
    w.finish()

    xs, ys = read_cifar10_binary(str(tmp_path), True)
    w2 = Worker(cfg, info)
    hx, hy = w2.prepare(normalize_uint8(xs)[order], ys[order])
    assert torch.equal(hx, x) and torch.equal(hy, y)
    loss_h, hits_h = w2.train_step(hx, hy)
    w2.finish()
    assert torch.equal(loss_d, loss_h) and torch.equal(hits_d, hits_h), (loss_d, loss_h)


def test_fp32_compute_with_device_data_is_refused():
    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, run_training

    cfg = TrainConfig(model="lenet", mode="single", dtype="fp32", device_data=True, verbose=False)
    with pytest.raises(ValueError, match="device-data"):
        run_training(cfg, DistInfo(device=torch.device("cuda", 0)))
