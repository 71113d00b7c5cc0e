"""Device-resident datasets on the CPU: ``utils/device_data.py`` (the
definition of a batch and the loader) against the independent NumPy oracle of
``tests/data_oracle.py``.  Every comparison is bit-exact: the look-up table
leaves nothing to round."""
import numpy as np
import pytest
import torch

import data_oracle as do
from distributed_ml_pytorch_amd.utils import device_data as dd
from distributed_ml_pytorch_amd.utils.data import normalize_uint8

MNIST = ((0.1307,), (0.3081,))
HALF = ((0.5, 0.5, 0.5), (0.5, 0.5, 0.5))


def _dataset(n, c, h, w, seed, norm):
    x, y = do.random_dataset(n, c, h, w, seed)
    return x, y, dd.DeviceDataset(x, y, *norm, device="cpu")


def _check_against_numpy(x, y, ds, index, pad, flip, seed, epoch):
    gx, gy, gd = dd.assemble_reference(ds, index, pad, flip, seed, epoch)
    ex, ey, ed = do.assemble_np(x.numpy(), y.numpy(), do.bits(ds.lut), index.numpy(), pad, flip,
                                seed, epoch)
    assert gx.dtype == torch.bfloat16 and gx.shape == (len(index), *x.shape[1:])
    assert gx.is_contiguous(memory_format=torch.channels_last) or x.shape[1] == 1
    assert gd.dtype == torch.int8 and gy.dtype == torch.int64
    np.testing.assert_array_equal(gd.numpy().astype(np.int64), ed)
    np.testing.assert_array_equal(gy.numpy(), ey)
    np.testing.assert_array_equal(do.bits(gx), ex)
    return gd


@pytest.mark.parametrize("ctr,key,want", do.PHILOX_KAT)
def test_philox_known_answers(ctr, key, want):
    got = do.philox_np([np.array([c]) for c in ctr], key)
    assert tuple(int(g[0]) for g in got) == want
    got = dd.philox4x32_10([torch.tensor([c]) for c in ctr], key)
    assert tuple(int(g[0]) for g in got) == want


@pytest.mark.parametrize("c,h,w,n,pad,flip,norm", [
    (3, 32, 32, 24, 4, True, HALF),
    (1, 28, 28, 12, 2, False, MNIST),
    (3, 5, 7, 9, 3, False, HALF),
    (3, 5, 7, 9, 3, True, HALF),
])
def test_reference_equals_numpy_assembler(c, h, w, n, pad, flip, norm):
    x, y, ds = _dataset(n, c, h, w, 11, norm)
    index = torch.tensor([0, n - 1, 3, 3, 0, n // 2, 1, n - 1])
    d = _check_against_numpy(x, y, ds, index, pad, flip, seed=(5 << 32) | 77, epoch=3)
    assert int(d[:, :2].min()) >= 0 and int(d[:, :2].max()) <= 2 * pad


@pytest.mark.parametrize("c,h,w,norm", [(3, 32, 32, HALF), (1, 28, 28, MNIST)])
def test_no_augmentation_equals_the_host_path(c, h, w, norm):
    """pad 0, no flip: today's normalize_uint8(...).to(bf16) and labels[index]."""
    x, y, ds = _dataset(32, c, h, w, 5, norm)
    index = torch.tensor([7, 0, 31, 7, 12])
    gx, gy, gd = dd.assemble_reference(ds, index, 0, False, seed=9, epoch=4)
    want = normalize_uint8(x, *norm)[index].to(torch.bfloat16)
    assert torch.equal(gx, want) and torch.equal(gy, y[index])
    assert int(gd.abs().max()) == 0
    # the look-up table is that normalisation of every byte value
    every = torch.arange(256, dtype=torch.uint8).view(256, 1, 1, 1).expand(256, c, 1, 1)
    assert torch.equal(ds.lut.t().reshape(256, c, 1, 1),
                       normalize_uint8(every, *norm).to(torch.bfloat16))


def test_draw_coverage_and_independence():
    n, pad, seed = 4096, 1, 1234
    x, y, ds = _dataset(n, 3, 8, 8, 2, HALF)
    index = torch.arange(n)
    d0 = _check_against_numpy(x, y, ds, index, pad, True, seed, 0).to(torch.int64)
    d1 = dd.assemble_reference(ds, index, pad, True, seed, 1)[2].to(torch.int64)
    for d in (d0, d1):
        combos, counts = np.unique(d.numpy(), axis=0, return_counts=True)
        assert len(combos) == 18, combos                  # 3 x 3 offsets x 2 flips
        assert counts.min() >= 150 and counts.max() <= 310, counts   # 4096 / 18 = 228 each
    assert not torch.equal(d0, d1)                        # the epoch enters the counter
    assert float((d0 != d1).any(1).float().mean()) > 0.8
    # a sample's draw (and image) does not depend on where it sits in the batch
    order = torch.randperm(n, generator=torch.Generator().manual_seed(0))[:64]
    gx, _, gd = dd.assemble_reference(ds, order, pad, True, seed, 0)
    assert torch.equal(gd.to(torch.int64), d0[order])
    full = dd.assemble_reference(ds, index, pad, True, seed, 0)[0]
    assert torch.equal(gx, full[order])


def test_out_of_range_index_is_padding_with_ignored_label():
    x, y, ds = _dataset(6, 3, 5, 7, 3, HALF)
    index = torch.tensor([2, 6, -1, 5])
    _check_against_numpy(x, y, ds, index, 3, True, 1, 0)
    gx, gy, _ = dd.assemble_reference(ds, index, 3, True, 1, 0)
    assert gy.tolist() == [int(y[2]), -100, -100, int(y[5])]
    black = ds.lut[:, 0].view(1, 3, 1, 1).expand(2, 3, 5, 7)
    assert torch.equal(gx[1:3], black)


def test_dataset_rejections():
    x, y = do.random_dataset(4, 3, 4, 4, 0)
    with pytest.raises(ValueError, match="uint8"):
        dd.DeviceDataset(x.float(), y)
    with pytest.raises(ValueError, match="channels"):
        dd.DeviceDataset(torch.zeros(2, 5, 4, 4, dtype=torch.uint8), y[:2])
    with pytest.raises(ValueError, match="2 GiB"):
        dd.DeviceDataset(torch.zeros(1, 1, 1, 1, dtype=torch.uint8).expand(1 << 16, 1, 256, 128),
                         torch.zeros(1 << 16, dtype=torch.int64))
    ds = dd.DeviceDataset(x, y)
    with pytest.raises(ValueError, match="padding"):
        dd.assemble_reference(ds, torch.tensor([0]), pad=17)
    with pytest.raises(ValueError, match="padding"):
        dd.DeviceLoader(ds, 2, pad=-1)


def _epoch_indices(loader, ds):
    """Dataset indices an epoch serves, recovered from unique labels."""
    out = []
    for xb, yb in loader:
        assert xb.shape[0] == yb.shape[0]
        out.append(yb.clone())
    return torch.cat(out) if out else torch.empty(0, dtype=torch.int64)


def _labelled_by_index(n):
    x = torch.randint(0, 256, (n, 3, 4, 4), dtype=torch.uint8,
                      generator=torch.Generator().manual_seed(1))
    return dd.DeviceDataset(x, torch.arange(n), *HALF, device="cpu")   # label = dataset index


def test_loader_epochs_shards_and_remainders():
    n = 103
    ds = _labelled_by_index(n)
    full = dd.DeviceLoader(ds, 10, shuffle=True, drop_last=False, seed=3)
    assert len(full) == 11
    e0, e1 = _epoch_indices(full, ds), _epoch_indices(full, ds)
    assert sorted(e0.tolist()) == list(range(n)) == sorted(e1.tolist())   # each sample once
    assert not torch.equal(e0, e1)                                         # new order per epoch
    again = dd.DeviceLoader(ds, 10, shuffle=True, drop_last=False, seed=3)
    assert torch.equal(_epoch_indices(again, ds), e0)                      # same seed, same order
    assert torch.equal(_epoch_indices(again, ds), e1)
    other = dd.DeviceLoader(ds, 10, shuffle=True, drop_last=False, seed=4)
    assert not torch.equal(_epoch_indices(other, ds), e0)
    # the order does not depend on the batch size
    wide = dd.DeviceLoader(ds, 64, shuffle=True, drop_last=False, seed=3)
    assert torch.equal(_epoch_indices(wide, ds), e0)
    # shards of world 3: disjoint and complete
    seen = []
    for r in range(3):
        ld = dd.DeviceLoader(ds, 8, shuffle=True, drop_last=False, seed=3, rank=r, world=3)
        got = _epoch_indices(ld, ds)
        assert sorted(got.tolist()) == list(range(r, n, 3))
        seen += got.tolist()
    assert sorted(seen) == list(range(n))
    # drop_last drops the remainder; the evaluation loader serves it at its true length
    dl = dd.DeviceLoader(ds, 10, shuffle=True, drop_last=True, seed=3)
    sizes = [len(yb) for _, yb in dl]
    assert len(dl) == 10 and sizes == [10] * 10
    ev = dd.DeviceLoader(ds, 25, shuffle=False, drop_last=False)
    batches = [yb for _, yb in ev]
    assert [len(b) for b in batches] == [25, 25, 25, 25, 3] and len(ev) == 5
    assert torch.equal(torch.cat(batches), torch.arange(n))               # identity order


def test_loader_next_writes_into_given_buffers():
    ds = _labelled_by_index(20)
    ld = dd.DeviceLoader(ds, 8, shuffle=True, drop_last=True, pad=1, flip=True, seed=5)
    ref = dd.DeviceLoader(ds, 8, shuffle=True, drop_last=True, pad=1, flip=True, seed=5)
    x = torch.zeros(8, 3, 4, 4, dtype=torch.bfloat16).contiguous(memory_format=torch.channels_last)
    y = torch.zeros(8, dtype=torch.int64)
    for _ in range(5):                                   # runs over the epoch boundary
        gx, gy = ld.next(out=(x, y))
        assert gx is x and gy is y
        wx, wy = ref.next()
        assert torch.equal(x, wx) and torch.equal(y, wy)
    assert ld.epoch == 3 and ld.remaining() == 1


def test_synthetic_quantisation_round_trips():
    from distributed_ml_pytorch_amd.utils.data import SyntheticImages

    tr, te, src = dd.get_device_datasets("synthetic", "/nonexistent", (3, 8, 8), 10, 64, 16, 0,
                                         "cpu")
    assert src == "synthetic" and len(tr) == 64 and len(te) == 16
    raw = SyntheticImages(64, (3, 8, 8), 10, seed=0)
    x, y, _ = dd.assemble_reference(tr, torch.arange(64))
    assert torch.equal(y, raw.y)
    inside = raw.x.abs() < 3.9                           # not clamped by the uint8 range
    err = (x.float() - raw.x).abs()[inside]
    assert float(err.max()) <= 0.5 / 32 + 2.0 ** -7      # half a quantum + bf16 rounding below 4


def test_run_training_with_device_data_on_cpu(tmp_path):
    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, run_training

    do.write_fake_cifar(tmp_path, per_file=8)
    cfg = TrainConfig(model="lenet", dataset="cifar10", data_dir=str(tmp_path), batch_size=8,
                      test_batch_size=5, epochs=2, mode="single", cuda=False, lr=0.01,
                      log_interval=2, device_data=True, augment="crop_flip", verbose=False,
                      log_dir=str(tmp_path / "log"))
    res = run_training(cfg, DistInfo(device=torch.device("cpu")))
    assert res["data"] == "cifar10+device" and res["steps"] == 10
    assert np.isfinite(res["test_loss"]) and 0.0 <= res["test_accuracy"] <= 1.0
    # files absent: the synthetic set, quantised
    cfg = TrainConfig(model="mlp", dataset="cifar10", data_dir=str(tmp_path / "none"),
                      n_train=64, n_test=16, batch_size=16, epochs=1, mode="single", cuda=False,
                      device_data=True, evaluate=False, verbose=False,
                      log_dir=str(tmp_path / "log"))
    res = run_training(cfg, DistInfo(device=torch.device("cpu")))
    assert res["data"] == "synthetic+device" and res["steps"] == 4


def test_cli_learns_from_the_device_loader(tmp_path):
    """The run of tests/test_core_cpu.py::test_cli_single_process, fed by the
    device loader: the quantised synthetic set is as learnable as the fp32 one."""
    from distributed_ml_pytorch_amd.cli import main

    res = main(["--no-distributed", "--model", "mlp", "--epochs", "1", "--n-train", "512",
                "--n-test", "128", "--test-batch-size", "128", "--log-interval", "4",
                "--lr", "0.05", "--log-dir", str(tmp_path / "log"), "--device-data"])
    assert res["steps"] == 8 and res["data"] == "synthetic+device"
    assert res["test_accuracy"] > 0.3


def test_augment_without_device_data_is_refused(tmp_path):
    from distributed_ml_pytorch_amd.cli import build_parser, config_from_args
    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, run_training

    info = DistInfo(device=torch.device("cpu"))
    with pytest.raises(ValueError, match="--device-data"):
        run_training(TrainConfig(model="mlp", mode="single", cuda=False, augment="crop",
                                 verbose=False, log_dir=str(tmp_path)), info)
    with pytest.raises(ValueError, match="augment"):
        run_training(TrainConfig(model="mlp", mode="single", cuda=False, device_data=True,
                                 augment="mixup", verbose=False, log_dir=str(tmp_path)), info)
    with pytest.raises(ValueError, match="crop-pad"):
        run_training(TrainConfig(model="mlp", mode="single", cuda=False, device_data=True,
                                 augment="crop", crop_pad=17, verbose=False,
                                 log_dir=str(tmp_path)), info)
    a = build_parser().parse_args(["--no-distributed", "--device-data", "--augment", "crop_flip",
                                   "--crop-pad", "2"])
    cfg = config_from_args(a)
    assert cfg.device_data and cfg.augment == "crop_flip" and cfg.crop_pad == 2
    cfg = config_from_args(build_parser().parse_args(["--no-distributed"]))
    assert not cfg.device_data and cfg.augment == "none" and cfg.crop_pad == 4
