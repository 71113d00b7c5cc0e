"""The mixing form of the batch assembler (``csrc/data.hip``,
``batch_assemble_mix``) against its definition,
``utils/device_data.assemble_mix_reference``: bit for bit in the images, both
label vectors, the weights and the draws, in the staged and the direct form, for
the three modes; rows beyond ``count``, the binding's rejections and graph
capture."""
import pytest
import torch

import data_oracle as do
import mix_oracle as mo
from distributed_ml_pytorch_amd.utils import device_data as dd

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEED = mo.SEED
_REF = {}          # (case, params, epoch) -> reference, computed once and shared


def _native():
    from distributed_ml_pytorch_amd.ops._ext import native

    return native()


def _pair(name, seed=21):
    c, h, w, n, pad, flip, norm, index = mo.CASES[name]
    x, y = do.random_dataset(n, c, h, w, seed)
    return (dd.DeviceDataset(x, y, *norm, device="cpu"), dd.DeviceDataset(x, y, *norm, device=DEV),
            pad, flip, index)


def _reference(name, cpu, index, params, pad, flip, epoch):
    key = (name, tuple(index), params, pad, flip, epoch)
    if key not in _REF:
        _REF[key] = dd.assemble_mix_reference(cpu, torch.tensor(index), params, pad, flip, SEED, epoch)
    return _REF[key]


def _launch(ds, index, params, pad, flip, epoch, path=-1):
    b = len(index)
    x = torch.empty((b, ds.channels, ds.height, ds.width), dtype=torch.bfloat16, device=DEV,
                    memory_format=torch.channels_last)
    y = torch.empty(b, dtype=torch.int64, device=DEV)
    y2 = torch.empty(b, dtype=torch.int64, device=DEV)
    lam = torch.empty(b, dtype=torch.float32, device=DEV)
    d = torch.empty((b, 3), dtype=torch.int8, device=DEV)
    dd.assemble_mix(ds, torch.tensor(index, dtype=torch.int32, device=DEV), b, x, y, y2, lam, d,
                    params, pad, flip, SEED, epoch, path)
    return x, y, y2, lam, d


def _assert_equal(got, want, what=""):
    for g, w, part in zip(got, want, ("x", "y", "y2", "lam", "draws")):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, part)
        assert torch.equal(g.cpu(), w), f"{what}: {part} differs from assemble_mix_reference"


def _modes(h, w):
    """One parameter set per mode; the CutMix box starts and ends inside an
    8-value store group at C = 3."""
    box = mo.boxes(h, w)["midgroup"] if h < 16 else (h // 4, h - 3, 1, w - 5)
    area = (box[1] - box[0]) * (box[3] - box[2])
    return [dd.NO_MIX, dd.MixParams("mixup", mo.f32(0.3172), mo.f32(0.3172), (0, 0, 0, 0)),
            dd.MixParams("cutmix", 1.0, mo.f32(1 - area / (h * w)), box)]


@pytest.mark.parametrize("name,path", [(n, -1) for n in sorted(mo.CASES)] + [(n, 0) for n in mo.STAGED])
def test_kernel_equals_reference(name, path):
    """Three modes, two epochs, even and odd count (224 x 224: count 2, several
    chunks per image).  path -1: the form the launcher picks; 0: the direct
    gather on a staged shape."""
    cpu, gpu, pad, flip, index = _pair(name)
    assert _native().batch_assemble_is_staged(gpu.data) == (name in mo.STAGED)   # both forms run
    counts = [index] if name == "imagenet" else [index, index[:-1]]
    assert name != "imagenet" or (len(index) == 2 and 3 * 224 * 224 > 8 * 1024)
    for idx in counts:
        for params in _modes(cpu.height, cpu.width):
            for epoch in (0, 3):
                _assert_equal(_launch(gpu, idx, params, pad, flip, epoch, path),
                              _reference(name, cpu, idx, params, pad, flip, epoch),
                              f"{name} {params} epoch {epoch}")


@pytest.mark.parametrize("name,path", [(n, -1) for n in mo.SMALL] + [(n, 0) for n in mo.STAGED])
def test_every_blend_weight_and_box(name, path):
    cpu, gpu, pad, flip, index = _pair(name)
    h, w = cpu.height, cpu.width
    for v in mo.PIX_LAMS:
        p = dd.MixParams("mixup", mo.f32(v), mo.f32(v), (0, 0, 0, 0))
        _assert_equal(_launch(gpu, index, p, pad, flip, 1, path),
                      _reference(name, cpu, index, p, pad, flip, 1), f"{name} {p}")
    for bname, box in mo.boxes(h, w).items():
        # a box on top of a blend: the three kinds of pixel in one launch
        p = dd.MixParams("cutmix", mo.f32(0.5), mo.f32(0.25), box)
        _assert_equal(_launch(gpu, index, p, pad, flip, 1, path),
                      _reference(name, cpu, index, p, pad, flip, 1), f"{name} box {bname}")


def test_out_of_range_index_as_row_and_as_partner():
    cpu, gpu, _, _, _ = _pair("odd_5x7")
    index = [2, 9, -1, 8, 1 << 20, 4]
    for params in _modes(5, 7):
        _assert_equal(_launch(gpu, index, params, 2, True, 0),
                      _reference("odd_5x7", cpu, index, params, 2, True, 0), str(params))


@pytest.mark.parametrize("name,offset", [("cifar", 16), ("cifar", 3), ("odd_5x7", 5)])
def test_count_below_rows_leaves_the_rest_untouched(name, offset):
    """Outputs carved out of larger sentinel-filled buffers (16-byte aligned and
    not): rows, y2 and lam at and beyond count stay as they were."""
    cpu, gpu, pad, flip, _ = _pair(name, seed=4)
    c, h, w = cpu.channels, cpu.height, cpu.width
    rows, count, img = 8, 5, c * h * w
    index = [k % cpu.n for k in range(count)]
    sx = torch.full((offset + rows * img + 64,), -7.0, dtype=torch.bfloat16, device=DEV)
    sy = torch.full((rows + 6,), 4242, dtype=torch.int64, device=DEV)
    sy2 = torch.full((rows + 6,), 4343, dtype=torch.int64, device=DEV)
    sl = torch.full((rows + 6,), 9.5, dtype=torch.float32, device=DEV)
    sd = torch.full((rows + 2, 3), 99, dtype=torch.int8, device=DEV)
    out_x = sx[offset:offset + rows * img].view(rows, h, w, c).permute(0, 3, 1, 2)
    out_y, out_y2, out_l, out_d = sy[3:3 + rows], sy2[3:3 + rows], sl[3:3 + rows], sd[1:1 + rows]
    params = _modes(h, w)[1]._replace(box=mo.boxes(h, w)["midgroup"])
    dd.assemble_mix(gpu, torch.tensor(index + [0, 1, 2], dtype=torch.int32, device=DEV), count,
                    out_x, out_y, out_y2, out_l, out_d, params, pad, flip, SEED, 1)
    want = dd.assemble_mix_reference(cpu, torch.tensor(index), params, pad, flip, SEED, 1)
    _assert_equal((out_x[:count], out_y[:count], out_y2[:count], out_l[:count], out_d[:count]), want)
    lo = offset + count * img
    assert bool((sx[:offset] == -7).all()) and bool((sx[lo:] == -7).all())
    for s, v in ((sy, 4242), (sy2, 4343), (sl, 9.5)):
        assert bool((s[:3] == v).all()) and bool((s[3 + count:] == v).all())
    assert bool((sd[:1] == 99).all()) and bool((sd[1 + count:] == 99).all())


def test_binding_rejections():
    nat = _native()
    _, ds, _, _, _ = _pair("odd_5x7")
    idx = torch.arange(4, dtype=torch.int32, device=DEV)

    def call(x=None, y=None, y2=None, lam=None, pix_lam=0.5, label_lam=0.5, box=(1, 3, 2, 6),
             count=4, data=ds.data):
        x = torch.empty((4, 3, 5, 7), dtype=torch.bfloat16, device=DEV,
                        memory_format=torch.channels_last) if x is None else x
        y = torch.empty(4, dtype=torch.int64, device=DEV) if y is None else y
        y2 = torch.empty(4, dtype=torch.int64, device=DEV) if y2 is None else y2
        lam = torch.empty(4, dtype=torch.float32, device=DEV) if lam is None else lam
        nat.batch_assemble_mix(data, ds.labels, ds.lut, idx, count, x, y, y2, lam, None, 1, True, 1,
                               0, pix_lam, label_lam, *box)

    call()                                                               # the valid form
    call(box=(0, 0, 0, 0), pix_lam=1.0, label_lam=1.0)
    call(box=(0, 5, 0, 7), pix_lam=0.0, label_lam=0.0)
    with pytest.raises(RuntimeError, match="out_y2"):
        call(y2=torch.empty(4, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="out_y2"):
        call(y2=torch.empty(4, dtype=torch.int64))                         # on the CPU
    with pytest.raises(RuntimeError, match="out_y2"):
        call(y2=torch.empty(3, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match="out_y2"):
        call(y2=torch.empty(8, dtype=torch.int64, device=DEV)[::2])      # not contiguous
    with pytest.raises(RuntimeError, match="out_lam"):
        call(lam=torch.empty(4, dtype=torch.float64, device=DEV))
    with pytest.raises(RuntimeError, match="out_lam"):
        call(lam=torch.empty(4, dtype=torch.float32))
    with pytest.raises(RuntimeError, match="out_lam"):
        call(lam=torch.empty(3, dtype=torch.float32, device=DEV))
    for box in ((0, 6, 0, 7), (0, 5, 0, 8), (-1, 3, 0, 7), (0, 5, -1, 7), (3, 2, 0, 7), (0, 5, 6, 5)):
        with pytest.raises(RuntimeError, match="box"):
            call(box=box)
    for bad in (1.5, float("nan"), -0.25, float("inf")):
        with pytest.raises(RuntimeError, match="pix_lam"):
            call(pix_lam=bad)
        with pytest.raises(RuntimeError, match="label_lam"):
            call(label_lam=bad)
    # the checks batch_assemble applies hold here too
    with pytest.raises(RuntimeError, match="out_x"):
        call(x=torch.empty((4, 3, 5, 7), dtype=torch.float16, device=DEV,
                           memory_format=torch.channels_last))
    with pytest.raises(RuntimeError, match="out_y"):
        call(y=torch.empty(4, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="index"):
        call(count=5)
    with pytest.raises(RuntimeError, match="uint8"):
        call(data=ds.data.to(torch.int8))


def test_two_mixed_launches_in_one_graph_replay_the_eager_bits():
    _, gpu, pad, flip, _ = _pair("cifar", seed=3)
    perm = torch.randperm(64, generator=torch.Generator().manual_seed(0)).to(DEV, torch.int32)
    modes = _modes(32, 32)[1:]
    outs = []
    for _ in range(2):
        outs.append((torch.empty((16, 3, 32, 32), dtype=torch.bfloat16, device=DEV,
                                 memory_format=torch.channels_last).zero_(),
                     torch.zeros(16, dtype=torch.int64, device=DEV),
                     torch.zeros(16, dtype=torch.int64, device=DEV),
                     torch.zeros(16, dtype=torch.float32, device=DEV),
                     torch.zeros((16, 3), dtype=torch.int8, device=DEV)))

    def both():
        for k, (x, y, y2, lam, d) in enumerate(outs):
            dd.assemble_mix(gpu, perm[16 * k:16 * k + 16], 16, x, y, y2, lam, d, modes[k], pad, flip,
                            SEED, 2 + k)

    both()
    torch.cuda.synchronize()
    eager = [tuple(t.clone() for t in o) for o in outs]
    assert all(float(e[3][0]) == m.label_lam for e, m in zip(eager, modes))
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
