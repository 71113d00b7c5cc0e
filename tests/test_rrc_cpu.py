"""The random-resized-crop definition (``utils/device_data.py``): the integer
bilinear resample against fp64 ``F.interpolate``, the identity box against the
plain crop, the draw, the box table and the start-up refusals.  The kernel is
compared with this definition in ``test_rrc_gpu.py``."""
import pytest
import torch
import torch.nn.functional as F

import data_oracle as do
from distributed_ml_pytorch_amd.utils import device_data as dd

SEED = 0x1234567 << 20


def _dataset(c, h, w, n=3, seed=2):
    ds = dd.DeviceDataset(*do.random_dataset(n, c, h, w, seed))
    ds.lut = torch.arange(256.0).to(torch.bfloat16).repeat(c, 1)    # the byte itself, exact in bf16
    return ds


@pytest.mark.parametrize("stored,box,out", [
    ((256, 256), (0, 0, 256, 256), (224, 224)), ((128, 128), (3, 5, 73, 97), (224, 224)),
    ((40, 36), (10, 9, 17, 23), (32, 32)), ((8, 8), (4, 7, 1, 1), (8, 8)),
    ((256, 256), (5, 5, 200, 250), (7, 9)), ((12, 10), (0, 0, 12, 10), (8, 13))])
def test_resample_is_within_one_and_a_half_levels_of_fp64_interpolate(stored, box, out):
    """0.5 from the final rounding plus 2 * 255 * 0.5 / 256 from the two 8-bit weights."""
    ds = _dataset(3, *stored)
    y0, x0, bh, bw = box
    got = dd.assemble_rrc_reference(ds, torch.arange(3), out, box=box)[0].double()
    src = ds.data[:, y0:y0 + bh, x0:x0 + bw].permute(0, 3, 1, 2).double()
    want = F.interpolate(src, size=out, mode="bilinear", align_corners=False, antialias=False)
    worst = float((got - want).abs().max())
    print(f"{stored} {box} -> {out}: worst {worst:.3f} levels")
    assert worst <= 1.5


@pytest.mark.parametrize("c,h,w", [(3, 32, 32), (1, 40, 36), (2, 5, 7)])
def test_box_of_the_output_size_is_the_plain_crop(c, h, w):
    ds = dd.DeviceDataset(*do.random_dataset(4, c, h, w, 5))
    index = torch.tensor([3, 0, 9, 2])                        # 9: outside the dataset
    x, y, _ = dd.assemble_reference(ds, index)
    got = dd.assemble_rrc_reference(ds, index, (h, w), box=(0, 0, h, w))
    assert torch.equal(got[0], x) and torch.equal(got[1], y) and got[0].stride() == x.stride()
    win = (h // 4, w // 3, h - h // 2, w - w // 2)            # a window: the slice of the plain batch
    got = dd.assemble_rrc_reference(ds, index, win[2:], box=win)[0]
    assert torch.equal(got, x[:, :, win[0]:win[0] + win[2], win[1]:win[1] + win[3]])


def test_draw_depends_on_seed_epoch_and_index_only():
    t = dd.rrc_box_table(40, 36)
    index = torch.tensor([5, 1, 1 << 20, -1, 7, 0])
    d = dd.rrc_draws(index, 40, 36, t, flip=True, seed=SEED, epoch=3)
    y0, x0, bh, bw, f = d.unbind(1)
    assert bool(((bh >= 1) & (y0 >= 0) & (y0 + bh <= 40) & (bw >= 1) & (x0 >= 0) & (x0 + bw <= 36)).all())
    assert set(f.tolist()) == {0, 1}
    again = dd.rrc_draws(index.flip(0)[:4], 40, 36, t, flip=True, seed=SEED, epoch=3)
    assert torch.equal(again, d.flip(0)[:4])                  # other position, other batch size
    assert not torch.equal(dd.rrc_draws(index, 40, 36, t, flip=True, seed=SEED, epoch=4), d)
    assert not torch.equal(dd.rrc_draws(index, 40, 36, t, flip=True, seed=SEED + 1, epoch=3), d)
    assert int(dd.rrc_draws(index, 40, 36, t, seed=SEED, epoch=3)[:, 4].sum()) == 0
    fixed = dd.rrc_draws(index, 40, 36, box=(1, 2, 30, 20), seed=SEED, epoch=3)
    assert fixed.tolist() == [[1, 2, 30, 20, 0]] * 6


@pytest.mark.parametrize("size,cells", [(32, 3626), (224, 3532), (256, 3528)])
def test_default_box_table(size, cells):
    t = dd.rrc_box_table(size, size)
    assert t.dtype == torch.int16 and tuple(t.shape) == (cells, 2)
    assert int(t.min()) >= 1 and int(t.max()) <= size


def test_loader_serves_resized_batches_of_the_definition():
    ds = dd.DeviceDataset(*do.random_dataset(10, 3, 12, 10, 1))
    mix = dd.MixConfig(mixup_alpha=0.8)
    ld = dd.DeviceLoader(ds, 4, seed=3, flip=True, rrc=dd.RrcConfig(), out_hw=(8, 6), mix=mix,
                         out_dtype=torch.float32)
    x, y = ld.next()
    want = dd.assemble_rrc_mix_reference(ds, ld.epoch_order(0)[:4], ld.last_params, (8, 6),
                                         table=ld.table, flip=True, seed=3, epoch=0)
    assert x.shape == (4, 3, 8, 6) and ld.last_params == dd.mix_draw(3, 0, 0, 8, 6, 0.8)
    assert torch.equal(x, want[0].float()) and torch.equal(y, want[1])
    assert torch.equal(ld.last_mix[0], want[2]) and torch.equal(ld.last_mix[1], want[3])
    ev = dd.DeviceLoader(ds, 4, shuffle=False, drop_last=False, out_hw=(8, 6),
                         box=dd.eval_box((12, 10), (8, 6)))
    assert torch.equal(ev.next()[0], dd.assemble_reference(ds, torch.arange(4))[0][:, :, 2:10, 2:8])
    assert dd.eval_box((12, 10), (8, 16)) == (0, 0, 12, 10)


@pytest.mark.parametrize("kw,match", [
    (dict(augment="rrc", device_data=False), "--device-data"),
    (dict(augment="rrc_flip", dataset="cifar10", stored_size=40), "--stored-size"),
    (dict(augment="crop", stored_size=40), "--stored-size"),
    (dict(augment="rrc", crop_pad=2), "--crop-pad"),
    (dict(augment="rrc", rrc_scale=(0.5, 0.1)), "scale"),
    (dict(augment="rrc", rrc_scale=(0.0, 1.0)), "scale"),
    (dict(augment="rrc_flip", rrc_ratio=(2.0, 0.5)), "ratio"),
    (dict(augment="rrc_flip", rrc_ratio=(-1.0, 1.0)), "ratio")])
def test_start_up_refusals(kw, match):
    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, check_device_data_config

    cfg = TrainConfig(**{"model": "lenet", "mode": "single", "cuda": False, "device_data": True,
                         "dataset": "synthetic", "verbose": False, **kw})
    with pytest.raises(ValueError, match=match):
        check_device_data_config(cfg, DistInfo(device=torch.device("cpu")))


def test_cli_flags_and_empty_table():
    from distributed_ml_pytorch_amd.cli import build_parser, config_from_args

    argv = ["--no-distributed", "--device-data", "--augment", "rrc_flip", "--stored-size", "40"]
    cfg = config_from_args(build_parser().parse_args(argv + ["--rrc-scale", "0.25", "1"]))
    assert (cfg.augment, cfg.stored_size, cfg.rrc_scale) == ("rrc_flip", 40, (0.25, 1.0))
    assert cfg.rrc_ratio == dd.RrcConfig().ratio
    with pytest.raises(ValueError, match="--crop-pad"):
        config_from_args(build_parser().parse_args(argv + ["--crop-pad", "4"]))
    with pytest.raises(ValueError, match="no random-resized-crop box"):
        dd.rrc_box_table(1, 4096)                             # every cell is taller than the image
    ds = dd.DeviceDataset(*do.random_dataset(4, 3, 1, 64, 0))
    with pytest.raises(ValueError, match="no random-resized-crop box"):
        dd.DeviceLoader(ds, 2, rrc=dd.RrcConfig((0.5, 1.0)), out_hw=(8, 8))
