"""Swin on the CPU: the registry, swin_tiny's parameter count against plain
torch.nn modules built from the architecture, and swin_mini's forward against a
plain-torch composition (roll, partition, bias gather, mask, softmax, reverse)."""
import torch
import torch.nn as nn
import torch.nn.functional as F


def _plain_swin_tiny_params(num_classes=1000):
    dims, depths, heads, ws = (96, 192, 384, 768), (2, 2, 6, 2), (3, 6, 12, 24), 7
    mods = [nn.Conv2d(3, dims[0], 4, 4), nn.LayerNorm(dims[0])]
    for i, (d, n, h) in enumerate(zip(dims, depths, heads)):
        for _ in range(n):
            mods += [nn.LayerNorm(d), nn.Linear(d, 3 * d), nn.Linear(d, d), nn.LayerNorm(d),
                     nn.Linear(d, 4 * d), nn.Linear(4 * d, d),
                     nn.Embedding((2 * ws - 1) ** 2, h)]          # the bias table
        if i < 3:
            mods += [nn.LayerNorm(4 * d), nn.Linear(4 * d, 2 * d, bias=False)]
    mods += [nn.LayerNorm(dims[-1]), nn.Linear(dims[-1], num_classes)]
    return sum(p.numel() for m in mods for p in m.parameters())


def test_registry_and_swin_tiny_parameter_count():
    from distributed_ml_pytorch_amd.models import REGISTRY, build_model, has_drop_path

    assert REGISTRY["swin_tiny"][1:] == ((3, 224, 224), 1000)
    assert REGISTRY["swin_mini"][1:] == ((3, 32, 32), 10)
    assert has_drop_path("swin_tiny") and has_drop_path("swin-mini")
    model, shape, nc = build_model("swin_tiny", drop_path=0.2)
    n = sum(p.numel() for p in model.parameters())
    assert n == _plain_swin_tiny_params() == 28_288_354      # the published 28.29 M
    assert (shape, nc) == ((3, 224, 224), 1000)
    names = dict(model.named_parameters())
    nwd = model.no_weight_decay()
    assert len(nwd) == 12 and all(names[k].shape[0] == 169 for k in nwd)
    # every second block of a stage shifts by half a window, but not on the 7 x 7 map
    assert [[b.attn.shift for b in st] for st in model.stages] == \
        [[0, 3], [0, 3], [0, 3, 0, 3, 0, 3], [0, 0]]


def _plain_attention(y, a, Hm, Wm):
    B, ws, sh, nh = y.shape[0], a.window, a.shift, a.heads
    C, N = y.shape[-1], a.window ** 2
    x = torch.roll(y, (-sh, -sh), (1, 2))
    x = x.view(B, Hm // ws, ws, Wm // ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(-1, N, C)
    q, k, v = F.linear(x, a.qkv.weight, a.qkv.bias).view(-1, N, 3, nh, C // nh).permute(
        2, 0, 3, 1, 4)
    s = q @ k.transpose(-1, -2) * (C // nh) ** -0.5
    c = torch.stack(torch.meshgrid(torch.arange(ws), torch.arange(ws), indexing="ij")).flatten(1)
    rel = c[:, :, None] - c[:, None, :] + ws - 1
    s = s + a.table[rel[0] * (2 * ws - 1) + rel[1]].permute(2, 0, 1)
    if sh:
        img = torch.zeros(Hm, Wm)
        cnt = 0
        for ys in (slice(0, -ws), slice(-ws, -sh), slice(-sh, None)):
            for xs in (slice(0, -ws), slice(-ws, -sh), slice(-sh, None)):
                img[ys, xs] = cnt
                cnt += 1
        m = img.view(Hm // ws, ws, Wm // ws, ws).permute(0, 2, 1, 3).reshape(-1, N)
        m = (m[:, None, :] - m[:, :, None]).ne(0).float() * -100.0
        s = (s.view(B, -1, nh, N, N) + m[None, :, None]).view(-1, nh, N, N)
    o = (s.softmax(-1) @ v).transpose(1, 2).reshape(-1, ws, ws, C)
    o = o.view(B, Hm // ws, Wm // ws, ws, ws, C).permute(0, 1, 3, 2, 4, 5).reshape(B, Hm, Wm, C)
    return F.linear(torch.roll(o, (sh, sh), (1, 2)), a.proj.weight, a.proj.bias)


def _plain_forward(m, x):
    ln = lambda n, t: F.layer_norm(t, (t.shape[-1],), n.weight, n.bias, n.eps)
    h = F.conv2d(x, m.patch_embed.weight, m.patch_embed.bias, stride=m.patch).permute(0, 2, 3, 1)
    h = ln(m.patch_norm, h)
    for i, stage in enumerate(m.stages):
        if i > 0:
            B, Hm, Wm, C = h.shape
            g = h.view(B, Hm // 2, 2, Wm // 2, 2, C).permute(0, 1, 3, 2, 4, 5).reshape(
                B, Hm // 2, Wm // 2, 4 * C)
            h = F.linear(ln(m.merges[i - 1].norm, g), m.merges[i - 1].reduction.weight)
        for b in stage:
            h = h + _plain_attention(ln(b.norm1, h), b.attn, h.shape[1], h.shape[2])
            y = F.gelu(F.linear(ln(b.norm2, h), b.fc1.weight, b.fc1.bias), approximate="tanh")
            h = h + F.linear(y, b.fc2.weight, b.fc2.bias)
    return F.linear(ln(m.norm, h).mean(dim=(1, 2)), m.head.weight, m.head.bias)


def test_swin_mini_cpu_forward_matches_plain_torch():
    from distributed_ml_pytorch_amd.models import swin_mini

    torch.manual_seed(0)
    m = swin_mini().eval()
    with torch.no_grad():
        for n, p in m.named_parameters():  # tables and biases large enough to matter
            if n.endswith(("table", "bias")):
                p.normal_(0, 0.5)
        x = torch.randn(3, 3, 32, 32)
        got, ref = m(x), _plain_forward(m, x)
    assert [[b.attn.shift for b in st] for st in m.stages] == [[0, 2], [0, 0]]
    torch.testing.assert_close(got, ref, rtol=1e-4, atol=1e-5)
