"""Stochastic depth (drop path) on the CPU: the draw's known answer and its
NumPy oracle, the rate ramp, the ViT in train and eval mode against a plain
re-implementation, state-dict keys, the checkpoint round trip and the refusals."""
import numpy as np
import pytest
import torch

import kernel_oracles as ko

from distributed_ml_pytorch_amd.models import build_model, vit_tiny
from distributed_ml_pytorch_amd.ops import functional as DF

SEED = 11          # every branch has kept and dropped samples at steps 0..2 (B = 6, p = 0.5)
KEEP_STEP0 = [[0, 0, 0, 1, 0, 0], [1, 0, 0, 1, 0, 0], [0, 0, 1, 1, 1, 0], [1, 1, 1, 0, 0, 0]]

VIT_TINY_KEYS = [
    "cls_token", "pos_embed", "patch_embed.weight", "patch_embed.bias",
    *[f"blocks.{i}.{n}.{wb}" for i in range(2)
      for n in ("norm1", "attn.qkv", "attn.proj", "norm2", "fc1", "fc2")
      for wb in ("weight", "bias")],
    "norm.weight", "norm.bias", "head.weight", "head.bias"]


def table_ref(seed, step, rates, B):
    """NumPy form of the specification: word b & 3 of philox(ctr = (b >> 2, j,
    step, "drop"), key = seed halves), kept when >= dropout_threshold(p_j)."""
    out = np.zeros((len(rates), B), np.float32)
    b = np.arange(B)
    for j, p in enumerate(rates):
        w = ko.philox4x32_10((b >> 2, np.full(B, j), np.full(B, step & 0xFFFFFFFF),
                              np.full(B, 0x64726F70)), (seed & 0xFFFFFFFF, seed >> 32))
        word = np.stack(w, 0)[b & 3, b]
        keep = word >= np.uint32(ko.dropout_threshold(p))
        out[j] = np.where(keep, np.float32(1) / np.float32(1 - p), np.float32(0))
    return out


def table_cpu(seed, step, rates, B):
    thr, sc = DF.drop_path_consts(rates)
    state = torch.tensor([step], dtype=torch.int64)
    t = DF.drop_path_table(state, thr, sc, B, seed)
    assert int(state[0]) == step + 1
    return t


def test_table_known_answer():
    t = table_cpu(SEED, 0, [0.5] * 4, 6)
    assert t.dtype == torch.float32 and t.shape == (4, 6)
    assert (t != 0).int().tolist() == KEEP_STEP0
    assert set(t.unique().tolist()) == {0.0, 2.0}
    for step in range(3):
        keep = table_ref(SEED, step, [0.5] * 4, 6) != 0
        assert keep.any(1).all() and (~keep).any(1).all(), (step, keep)


@pytest.mark.parametrize("B", [1, 3, 4, 6, 257])
def test_table_matches_numpy_oracle(B):
    rates = [0.5, 0.0, 0.1, 0.9, 0.25]
    for step in range(3):
        got = table_cpu(SEED, step, rates, B).numpy()
        ref = table_ref(SEED, step, rates, B)
        assert got.tobytes() == ref.tobytes(), (B, step)
        assert (got[1] == 1.0).all()                       # p = 0: always kept, scale exactly 1


def test_rates():
    assert DF.drop_path_rates(0.3, 1) == [0.3]
    assert DF.drop_path_rates(0.0, 4) == [0.0] * 4
    r = DF.drop_path_rates(0.1, 12)
    assert r[0] == 0.0 and r[-1] == 0.1 and len(r) == 12
    assert r == [0.1 * i / 11 for i in range(12)]
    np.testing.assert_allclose(r, np.linspace(0, 0.1, 12), rtol=1e-12)
    m = vit_tiny(drop_path=0.5, drop_path_seed=SEED)
    assert m.drop_path_rates == [0.0, 0.0, 0.5, 0.5]       # both branches of a block share p_i
    for bad in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError):
            DF.drop_path_rates(bad, 4)
        with pytest.raises(ValueError):
            vit_tiny(drop_path=bad)
        with pytest.raises(ValueError):
            build_model("vit_tiny", drop_path=bad)


def _plain_vit(m, x, S):
    """x + S[j][:, None, None] * branch, written out with stock torch ops."""
    import torch.nn.functional as F

    def ln(mod, t):
        return F.layer_norm(t, (t.shape[-1],), mod.weight, mod.bias, mod.eps)

    def attn(blk, t):
        B, N, D = t.shape
        H = blk.attn.heads
        q, k, v = blk.attn.qkv(t).view(B, N, 3, H, D // H).permute(2, 0, 3, 1, 4)
        p = torch.softmax(q @ k.transpose(-1, -2) * (D // H) ** -0.5, -1)
        return blk.attn.proj((p @ v).transpose(1, 2).reshape(B, N, D))

    h = F.conv2d(x, m.patch_embed.weight, m.patch_embed.bias, stride=m.patch)
    h = h.flatten(2).transpose(1, 2)
    h = torch.cat([m.cls_token.expand(h.shape[0], -1, -1), h], 1) + m.pos_embed
    for i, blk in enumerate(m.blocks):
        h = h + S[2 * i][:, None, None] * attn(blk, ln(blk.norm1, h))
        y = ln(blk.norm2, h)
        h = h + S[2 * i + 1][:, None, None] * blk.fc2(F.gelu(blk.fc1(y), approximate="tanh"))
    return m.head(ln(m.norm, h)[:, 0])


def test_vit_train_mode_matches_plain_reimplementation():
    torch.manual_seed(3)
    m = vit_tiny(drop_path=0.5, drop_path_seed=SEED).train()
    x = torch.randn(6, 3, 32, 32)
    assert m.drop_path_step.dtype == torch.int64 and int(m.drop_path_step) == 0
    S = torch.from_numpy(table_ref(SEED, 0, m.drop_path_rates, 6))
    assert (S[:2] == 1).all() and (S[2:] == 0).any() and (S[2:] == 2).any()
    with torch.no_grad():
        got = m(x)
        assert int(m.drop_path_step) == 1
        ref = _plain_vit(m, x, S)
        torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-5)
        # the masks matter at this tolerance, and the next forward draws step 1
        none = _plain_vit(m, x, torch.ones_like(S))
        assert float((got - none).abs().max()) > 1e-3
        got1 = m(x)
        S1 = torch.from_numpy(table_ref(SEED, 1, m.drop_path_rates, 6))
        torch.testing.assert_close(got1, _plain_vit(m, x, S1), rtol=1e-5, atol=1e-5)
    assert int(m.drop_path_step) == 2


def test_vit_train_mode_gradients_flow_through_the_scales():
    torch.manual_seed(4)
    m = vit_tiny(drop_path=0.5, drop_path_seed=SEED).train()
    x = torch.randn(6, 3, 32, 32)
    m(x).square().sum().backward()
    got = {n: p.grad.clone() for n, p in m.named_parameters()}
    m.zero_grad()
    S = torch.from_numpy(table_ref(SEED, 0, m.drop_path_rates, 6))
    _plain_vit(m, x, S).square().sum().backward()
    for n, p in m.named_parameters():
        torch.testing.assert_close(got[n], p.grad, rtol=1e-4, atol=1e-5, msg=n)


def test_eval_is_bit_identical_to_the_plain_model():
    torch.manual_seed(5)
    m = vit_tiny(drop_path=0.5, drop_path_seed=SEED)
    plain = vit_tiny()
    plain.load_state_dict({k: v for k, v in m.state_dict().items() if k != "drop_path_step"})
    x = torch.randn(6, 3, 32, 32)
    with torch.no_grad():
        assert torch.equal(m.eval()(x), plain.eval()(x))
    assert int(m.drop_path_step) == 0


def test_state_dict_keys_without_drop_path_are_unchanged():
    assert list(vit_tiny().state_dict().keys()) == VIT_TINY_KEYS
    assert list(vit_tiny(drop_path=0.0).state_dict().keys()) == VIT_TINY_KEYS
    assert sorted(vit_tiny(drop_path=0.2).state_dict()) == sorted(VIT_TINY_KEYS + ["drop_path_step"])
    assert not hasattr(vit_tiny(), "drop_path_step")


def test_counter_round_trips_through_a_worker_checkpoint(tmp_path):
    from distributed_ml_pytorch_amd.utils.checkpoint import (load_worker_model,
                                                            save_worker_checkpoint)

    m = vit_tiny(drop_path=0.5, drop_path_seed=SEED).train()
    x = torch.randn(6, 3, 32, 32)
    with torch.no_grad():
        for _ in range(3):
            m(x)
    assert int(m.drop_path_step) == 3
    path = str(tmp_path / "w.pt")
    save_worker_checkpoint(path, m, step=3)
    m2 = vit_tiny(drop_path=0.5, drop_path_seed=SEED).train()
    assert load_worker_model(path, m2) == 3
    assert int(m2.drop_path_step) == 3 and m2.drop_path_step.dtype == torch.int64
    with torch.no_grad():
        assert torch.equal(m(x), m2(x))                    # both draw the table of step 3


def test_seed_defaults_to_torch_generator():
    torch.manual_seed(7)
    a = vit_tiny(drop_path=0.1).drop_path_seed
    torch.manual_seed(7)
    b = vit_tiny(drop_path=0.1).drop_path_seed
    torch.manual_seed(8)
    c = vit_tiny(drop_path=0.1).drop_path_seed
    assert a == b != c and 0 <= a < 2 ** 62


def test_refusals():
    from distributed_ml_pytorch_amd.cli import build_parser, config_from_args
    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, Worker, run_training

    with pytest.raises(ValueError, match="ViT"):
        build_model("resnet18", drop_path=0.1)
    info = DistInfo(device=torch.device("cpu"))
    a = build_parser().parse_args(["--model", "resnet18", "--drop-path", "0.1", "--no-distributed"])
    cfg = config_from_args(a)
    assert cfg.drop_path == 0.1
    with pytest.raises(ValueError, match="--drop-path"):
        run_training(cfg, info)
    a = build_parser().parse_args(["--model", "vit_tiny", "--drop-path", "1.0", "--no-distributed"])
    with pytest.raises(ValueError, match="--drop-path"):
        run_training(config_from_args(a), info)
    with pytest.raises(ValueError, match="--drop-path"):
        Worker(TrainConfig(model="lenet", drop_path=0.2, mode="single", cuda=False), info)
    a = build_parser().parse_args(["--model", "vit_tiny", "--augment", "crop", "--no-distributed"])
    with pytest.raises(ValueError, match="--device-data"):
        run_training(config_from_args(a), info)
    assert config_from_args(build_parser().parse_args([])).drop_path == 0.0


def test_cpu_worker_trains_with_drop_path():
    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, Worker

    for mode in ("asgd", "sync", "single"):
        cfg = TrainConfig(model="vit_tiny", batch_size=6, mode=mode, ps="local", drop_path=0.5,
                          cuda=False, evaluate=False, verbose=False, lr=0.01)
        w = Worker(cfg, DistInfo(device=torch.device("cpu")))
        x, y = w.prepare(torch.randn(6, 3, 32, 32), torch.randint(0, 10, (6,)))
        losses = [float(w.train_step(x, y)[0]) for _ in range(2)]
        w.finish()
        assert all(l == l for l in losses), (mode, losses)
        assert int(w.model.drop_path_step) == 2
