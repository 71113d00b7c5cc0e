"""ConvNeXt on the CPU: registry, parameter count, the block against a plain-torch
re-statement, state-dict keys, drop-path plumbing and a two-step AdamW run."""
import pytest
import torch
import torch.nn.functional as F

from distributed_ml_pytorch_amd.models import build_model


def test_convnext_tiny_registry_and_parameter_count():
    model, shape, nc = build_model("convnext_tiny")
    assert shape == (3, 224, 224) and nc == 1000
    assert sum(p.numel() for p in model.parameters()) == 28_589_128     # the published count
    assert model.no_weight_decay() <= {n for n, _ in model.named_parameters()}


def _plain_forward(m, x):
    """The model re-stated in plain torch ([B, C, H, W] throughout)."""
    def ln(mod, t):      # LayerNorm over channels of an NCHW tensor
        return F.layer_norm(t.permute(0, 2, 3, 1), (t.shape[1],), mod.weight, mod.bias,
                            mod.eps).permute(0, 3, 1, 2)

    h = ln(m.stem_norm, F.conv2d(x, m.stem.weight, m.stem.bias, stride=m.patch))
    for i, stage in enumerate(m.stages):
        if i > 0:
            c = m.down_convs[i - 1]
            h = F.conv2d(ln(m.down_norms[i - 1], h), c.weight, c.bias, stride=2)
        for b in stage:
            y = F.conv2d(h, b.dwconv.weight, b.dwconv.bias, padding=3, groups=h.shape[1])
            y = ln(b.norm, y).permute(0, 2, 3, 1)
            y = F.linear(F.gelu(F.linear(y, b.fc1.weight, b.fc1.bias), approximate="tanh"),
                         b.fc2.weight, b.fc2.bias)
            h = h + (b.gamma * y).permute(0, 3, 1, 2)
    return F.linear(F.layer_norm(h.mean((2, 3)), (h.shape[1],), m.norm.weight, m.norm.bias,
                                 m.norm.eps), m.head.weight, m.head.bias)


def test_convnext_mini_forward_matches_plain_torch():
    torch.manual_seed(0)
    model, shape, _ = build_model("convnext_mini")
    with torch.no_grad():
        for blk in (b for st in model.stages for b in st):
            blk.gamma.fill_(0.5)             # the 1e-6 init would hide the branch
    assert "drop_path_step" not in model.state_dict()
    x = torch.randn(3, *shape)
    torch.testing.assert_close(model(x), _plain_forward(model, x), rtol=1e-4, atol=1e-5)


def test_drop_path_is_for_vit_and_convnext_only():
    model, _, _ = build_model("convnext_mini", drop_path=0.1)
    assert "drop_path_step" in model.state_dict()
    assert model.drop_path_rates == pytest.approx([0.0, 0.1 / 3, 0.2 / 3, 0.1])
    with pytest.raises(ValueError, match="ViT"):
        build_model("resnet18", drop_path=0.1)


def test_two_adamw_steps_train_on_the_cpu():
    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, Worker

    cfg = TrainConfig(model="convnext_mini", batch_size=4, mode="single", optimizer="adamw",
                      lr=1e-3, drop_path=0.1, cuda=False, evaluate=False, verbose=False)
    w = Worker(cfg, DistInfo(device=torch.device("cpu")))
    g = torch.Generator().manual_seed(0)
    x, y = w.prepare(torch.randn(4, *w.input_shape, generator=g),
                     torch.randint(0, w.num_classes, (4,), generator=g))
    before = w.arena.p32.clone()
    for _ in range(2):
        loss, _ = w.train_step(x, y)
        assert torch.isfinite(loss.float()).all()
    w.finish()
    assert not torch.equal(before, w.arena.p32)
    assert int(w.model.drop_path_step) == 2
