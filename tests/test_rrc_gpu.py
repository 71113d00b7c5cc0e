"""The random-resized-crop batch assembler (``csrc/data_rrc.hip``) against its
definition, ``utils/device_data.assemble_rrc_reference`` / ``_mix_reference``: bit
for bit in images, labels, draws (and partner labels and weights), in the staged
and the direct form; rows beyond ``count``, the fixed evaluation box, graph
replay, the binding's rejections and a training run fed by it."""
import pytest
import torch

import data_oracle as do
from distributed_ml_pytorch_amd.utils import device_data as dd

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = (0xC0FFEE << 24) | 77
# name: (C, Hs, Ws, N, (Ho, Wo), index -- one of them outside [0, N))
CASES = {"updown": (3, 12, 10, 9, (8, 8), [4, 0, 8, 99, 2, 7]),      # down in y, up and down boxes
         "cifar": (3, 32, 32, 12, (32, 32), [3, 11, -1, 0, 7, 5]),
         "odd": (1, 40, 36, 6, (17, 13), [5, 1, 64, 0, 3, 2]),        # 221 values: scalar stores
         "imagenet": (3, 256, 256, 3, (224, 224), [2, 5]),            # 28 strips of 8 rows
         "direct": (3, 1024, 1024, 2, (8, 8), [1, 0, 2])}
SENTINEL = {"x": -7.0, "y": 4242, "y2": 4343, "lam": 9.5, "draws": 99}
_DS, _REF = {}, {}          # datasets and references, built once and shared


def _native():
    from distributed_ml_pytorch_amd.ops._ext import native

    return native()


def _pair(name):
    if name not in _DS:
        c, hs, ws, n, _, _ = CASES[name]
        x, y = do.random_dataset(n, c, hs, ws, 21)
        norm = ((0.4,) * c, (0.3,) * c)
        _DS[name] = (dd.DeviceDataset(x, y, *norm), dd.DeviceDataset(x, y, *norm, device=DEV),
                     dd.rrc_box_table(hs, ws).to(DEV))
    return _DS[name]


def _reference(name, flip, epoch, params=None, box=None):
    key = (name, flip, epoch, params, box)
    if key not in _REF:
        cpu, _, table = _pair(name)
        src = dict(box=box) if box else dict(table=table)
        index = torch.tensor(CASES[name][5])
        _REF[key] = dd.assemble_rrc_reference(cpu, index, CASES[name][4], flip=flip, seed=SEED,
                                              epoch=epoch, **src) if params is None else \
            dd.assemble_rrc_mix_reference(cpu, index, params, CASES[name][4], flip=flip, seed=SEED,
                                          epoch=epoch, **src)
    return _REF[key]


def _buffers(name, rows):
    c, (ho, wo) = CASES[name][0], CASES[name][4]
    shapes = {"x": ((rows, c, ho, wo), torch.bfloat16), "y": ((rows,), torch.int64),
              "y2": ((rows,), torch.int64), "lam": ((rows,), torch.float32),
              "draws": ((rows, 5), torch.int16)}
    out = [torch.full(shape, SENTINEL[k], dtype=dt, device=DEV) for k, (shape, dt) in shapes.items()]
    return (out[0].contiguous(memory_format=torch.channels_last), *out[1:])


def _assert_rows(got, want, count, what, parts=("x", "y", "y2", "lam", "draws")):
    """Rows [0, count) are the reference's, the rows beyond hold their sentinel."""
    for g, w, part in zip(got, want, parts):
        assert g.dtype == w.dtype and g.shape[1:] == w.shape[1:], (what, part)
        assert torch.equal(g[:count].cpu(), w[:count]), f"{what}: {part} differs from the reference"
        assert bool((g[count:] == SENTINEL[part]).all()), f"{what}: {part} written beyond count"


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_equals_reference(name):
    """Flip on and off, two epochs, an even and an odd count, buffers two rows
    longer than the batch; the form is the one the planner picks."""
    _, gpu, table = _pair(name)
    c, hs, ws, _, (ho, wo), index = CASES[name]
    staged, strip, _, lds = _native().batch_assemble_rrc_plan(hs, ws, c, ho, wo, False)
    assert staged == (name != "direct") and lds <= 64 * 1024
    assert name != "imagenet" or (strip == 8 and ho // strip == 28)
    idx = torch.tensor(index, dtype=torch.int32, device=DEV)
    for flip in (False, True):
        for epoch in (0, 3):
            want = _reference(name, flip, epoch)
            for count in (len(index), len(index) - 1):
                bx, by, _, _, bd = _buffers(name, len(index) + 2)
                dd.assemble_rrc(gpu, idx, count, bx, by, bd, table, None, flip, SEED, epoch)
                _assert_rows((bx, by, bd), want, count, f"{name} flip {flip} epoch {epoch} "
                             f"count {count}", ("x", "y", "draws"))


@pytest.mark.parametrize("path", [-1, 0], ids=["staged", "direct"])
@pytest.mark.parametrize("name", ["updown", "cifar", "imagenet"])
def test_mixing_equals_reference(name, path):
    """No mix, Mixup, and a CutMix box that starts and ends inside an 8-value store
    group at C = 3; the out-of-range index is a row and a partner."""
    _, gpu, table = _pair(name)
    (ho, wo), index = CASES[name][4], CASES[name][5]
    box = (ho // 4, ho - 3, 1, wo - 5)
    lam = float(torch.tensor(0.3172, dtype=torch.float32))
    area = float(torch.tensor(1 - (box[1] - box[0]) * (box[3] - box[2]) / (ho * wo), dtype=torch.float32))
    idx = torch.tensor(index, dtype=torch.int32, device=DEV)
    for params in (dd.NO_MIX, dd.MixParams("mixup", lam, lam, (0, 0, 0, 0)),
                   dd.MixParams("cutmix", 1.0, area, box)):
        bufs = _buffers(name, len(index) + 1)
        dd.assemble_rrc_mix(gpu, idx, len(index), *bufs, params, table, None, True, SEED, 1, path)
        _assert_rows(bufs, _reference(name, True, 1, params), len(index), f"{name} {params}")


@pytest.mark.parametrize("name,box", [("imagenet", (16, 16, 224, 224)), ("cifar", (0, 0, 32, 32))])
def test_fixed_box_of_the_output_size_is_a_slice_through_the_lut(name, box):
    cpu, gpu, _ = _pair(name)
    index = [i for i in CASES[name][5] if 0 <= i < cpu.n]
    bx, by, _, _, bd = _buffers(name, len(index))
    dd.assemble_rrc(gpu, torch.tensor(index, dtype=torch.int32, device=DEV), len(index), bx, by, bd,
                    box=box, seed=SEED)
    y0, x0, bh, bw = box
    window = cpu.data[index, y0:y0 + bh, x0:x0 + bw].long()
    want = cpu.lut[torch.arange(cpu.channels), window].permute(0, 3, 1, 2)
    assert torch.equal(bx.cpu(), want) and torch.equal(by.cpu(), cpu.labels[index])
    assert bd.cpu().tolist() == [[*box, 0]] * len(index)


def test_graph_replay_rewrites_the_eager_bits():
    _, gpu, table = _pair("cifar")
    idx = torch.tensor(CASES["cifar"][5], dtype=torch.int32, device=DEV)
    plain, mixed = _buffers("cifar", 6), _buffers("cifar", 6)
    params = dd.MixParams("mixup", 0.25, 0.25, (0, 0, 0, 0))

    def both(check):
        dd.assemble_rrc(gpu, idx, 6, plain[0], plain[1], plain[4], table, None, True, SEED, 2,
                        check_table=check)
        dd.assemble_rrc_mix(gpu, idx, 6, *mixed, params, table, None, True, SEED, 5, check_table=check)

    both(True)
    torch.cuda.synchronize()
    written = (plain[0], plain[1], plain[4], *mixed)
    eager = [t.clone() for t in written]
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        both(False)                       # the table was read back by the eager launch
    for _ in range(2):
        for t in written:
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        for t, e in zip(written, eager):
            assert torch.equal(t, e)
    assert torch.equal(eager[0].cpu(), _reference("cifar", True, 2)[0])


@pytest.mark.parametrize("bad,match", [("table", "table entry"), ("box", "inside"), ("nchw", "out_x"),
                                       ("channels", "out_x"), ("rows", "out_x")])
def test_binding_rejections(bad, match):
    _, ds, table = _pair("updown")
    idx = torch.arange(4, dtype=torch.int32, device=DEV)
    x = torch.empty((4, 3, 8, 8), dtype=torch.bfloat16, device=DEV, memory_format=torch.channels_last)
    tab, box = table, None
    if bad == "table":
        tab = tab.clone()
        tab[5, 0] = 13                                        # taller than the 12-row image
    elif bad == "box":
        tab, box = None, [3, 0, 10, 10]                       # rows 3..12 of 12
    elif bad == "nchw":
        x = torch.empty((4, 3, 8, 8), dtype=torch.bfloat16, device=DEV)
    elif bad == "channels":
        x = torch.empty((4, 2, 8, 8), dtype=torch.bfloat16, device=DEV, memory_format=torch.channels_last)
    else:
        x = x[:3]
    with pytest.raises(RuntimeError, match=match):
        _native().batch_assemble_rrc(ds.data, ds.labels, ds.lut, idx, 4, tab, box, x,
                                     torch.empty(4, dtype=torch.int64, device=DEV), None, True, 1, 0)


def test_three_training_steps_fed_by_resized_crops():
    """resnet18, synthetic 40 x 40 images, rrc_flip: the first step's batch and loss
    are those of the same model stepped on the reference-assembled batch; steps 2
    and 3 replay the captured graph on batches written into its own inputs."""
    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import (TrainConfig, Worker,
                                                            make_device_loaders)

    info = DistInfo(device=torch.device("cuda", 0))
    cfg = TrainConfig(model="resnet18", dataset="synthetic", n_train=64, n_test=16, batch_size=8,
                      test_batch_size=8, mode="single", lr=0.01, evaluate=False, verbose=False,
                      device_data=True, augment="rrc_flip", stored_size=40)
    w = Worker(cfg, info)
    assert w.enable_graph(True)
    train, test, _ = make_device_loaders(cfg, info, w)
    assert (train.ds.height, train.out_h, test.box) == (40, 32, (4, 4, 32, 32))
    batches = train.iter_into(w.static_batch_buffers)
    x, y = next(batches)
    first = x.clone()
    losses = [w.train_step(x, y)[0]]
    for _ in range(2):
        x, y = next(batches)
        assert x is w.static_inputs()[0] and w.graph is not None     # written in place, replayed
        losses.append(w.train_step(x, y)[0])
    vl, va = w.evaluate(test)
    w.finish()

    cpu = dd.DeviceDataset(train.ds.data.cpu().permute(0, 3, 1, 2), train.ds.labels.cpu(),
                           train.ds.mean, train.ds.std)
    rx, ry, _ = dd.assemble_rrc_reference(cpu, train.epoch_order(0)[:8], (32, 32),
                                          table=train.table, flip=True, seed=cfg.seed, epoch=0)
    assert torch.equal(first.cpu(), rx)
    w2 = Worker(cfg, info)
    assert w2.enable_graph(True)
    loss_ref, _ = w2.train_step(*w2.prepare(rx, ry))
    w2.finish()
    assert torch.equal(losses[0], loss_ref), (losses[0], loss_ref)
    assert all(torch.isfinite(v.float()) and float(v) > 0 for v in losses) and 0.0 <= va <= 1.0
