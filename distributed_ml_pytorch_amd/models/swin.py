"""Swin Transformer (Liu et al. 2021, "Hierarchical Vision Transformer using Shifted
Windows"): the window-attention model of the AdamW / stochastic-depth / EMA /
Mixup-CutMix / random-resized-crop recipe.  Not in the reference.

The residual stream is kept in map order, ``[B, Hm, Wm, C]`` rows.  A block is
pre-norm like the ViT's: LayerNorm -> qkv Linear -> shifted-window attention ->
proj, then LayerNorm -> fc1 -> GELU -> fc2; every residual add is fused into the
LayerNorm that reads its result, with the per-sample stochastic-depth scale
(two branches per block, linear ramp over the blocks, the ViT's draw).  The
attention (``ops.functional.window_attention``, ``csrc/attention_window.hip``)
reads the qkv rows where the Linear wrote them: the cyclic shift, the window
partition and their inverses are address arithmetic in the kernels, and every
second block of a stage whose map is larger than the window shifts by half a
window.  A stage whose map is no larger than the window uses the map as its
window and no shift, as Swin does.

Patch merging is the paper's: the 2x2 gather to ``4C`` (the patch-matrix kernel
of ``csrc/im2col.hip``, channel order (row, column, c)), LayerNorm(4C), then
Linear(4C, 2C) without bias.  The gather is linear, so the last block's pending
MLP output is gathered beside the stream and the add is fused into that
LayerNorm too.  The head is LayerNorm, global average pool, Linear.

The GELU is this project's tanh form and the gather order is not timm's: no
weight compatibility is claimed.  Swin-T has 28,288,354 parameters with a
1000-class head.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..ops import functional as DF
from ..ops import layers as L
from ..ops.linear import mlp, mlp_ok
from .vit import LayerNorm, PatchEmbed


class WindowAttention(nn.Module):
    def __init__(self, dim: int, heads: int, window: int, shift: int):
        super().__init__()
        assert dim % heads == 0
        self.heads, self.window, self.shift = heads, window, shift
        self.qkv = L.Linear(dim, 3 * dim)
        self.proj = L.Linear(dim, dim)
        # relative-position bias, fp32: the kernels read the parameter itself
        self.table = nn.Parameter(torch.zeros((2 * window - 1) ** 2, heads))
        nn.init.trunc_normal_(self.table, std=0.02)

    def forward(self, y):
        o = DF.window_attention(self.qkv(y), self.heads, self.window, self.shift, self.table)
        return self.proj(o)


class Block(nn.Module):
    def __init__(self, dim: int, heads: int, window: int, shift: int, mlp_ratio: float = 4.0):
        super().__init__()
        self.norm1 = LayerNorm(dim, eps=1e-5)
        self.attn = WindowAttention(dim, heads, window, shift)
        self.norm2 = LayerNorm(dim, eps=1e-5)
        hidden = int(dim * mlp_ratio)
        self.fc1 = L.Linear(dim, hidden)
        self.fc2 = L.Linear(hidden, dim)

    def mlp(self, y):
        if mlp_ok(y, self.fc1, self.fc2):
            return mlp(y, self.fc1, self.fc2)       # GELU fused into the GEMM epilogues
        return self.fc2(DF.gelu(self.fc1(y)))

    def forward(self, h, pending=None, pending_scale=None, attn_scale=None):
        """Stream ``h`` plus the previous block's unadded MLP output ``pending``
        (``models.vit.Block.forward_fused``): returns ``(h, mlp_out)``."""
        if pending is None:
            h, y = self.norm1.stream_forward(h)
        else:
            h, y = self.norm1.add_forward(h, pending, pending_scale)
        h, y = self.norm2.add_forward(h, self.attn(y), attn_scale)
        return h, self.mlp(y)


class PatchMerging(nn.Module):
    def __init__(self, dim: int):
        super().__init__()
        self.norm = LayerNorm(4 * dim, eps=1e-5)
        self.reduction = L.Linear(4 * dim, 2 * dim, bias=False)

    def forward(self, h, pending, pending_scale):
        _, y = self.norm.add_forward(DF.patch_gather(h, 2), DF.patch_gather(pending, 2),
                                     pending_scale)
        return self.reduction(y)


class SwinTransformer(nn.Module):
    def __init__(self, image_size: int = 224, patch: int = 4, window: int = 7,
                 depths=(2, 2, 6, 2), dims=(96, 192, 384, 768), heads=(3, 6, 12, 24),
                 mlp_ratio: float = 4.0, num_classes: int = 1000, in_chans: int = 3,
                 drop_path: float = 0.0, drop_path_seed: int | None = None):
        """``drop_path``: stochastic depth, the rate of the last block of the linear
        ramp over all blocks (both branches of a block share its rate);
        ``drop_path_seed``: its Philox key, drawn from torch's generator when None."""
        super().__init__()
        assert len(depths) == len(dims) == len(heads) >= 1
        assert image_size % (patch * 2 ** (len(depths) - 1)) == 0
        self.patch = patch
        self.patch_embed = PatchEmbed(in_chans, dims[0], kernel_size=patch, stride=patch)
        self.patch_norm = LayerNorm(dims[0], eps=1e-5)
        stages = []
        for i, (n, d, nh) in enumerate(zip(depths, dims, heads)):
            side = image_size // patch // 2 ** i
            ws = min(window, side)
            assert side % ws == 0, f"window {ws} does not divide the {side} x {side} map"
            stages.append(nn.ModuleList(
                Block(d, nh, ws, ws // 2 if (j % 2 and side > ws) else 0, mlp_ratio)
                for j in range(n)))
        self.stages = nn.ModuleList(stages)
        self.merges = nn.ModuleList(PatchMerging(d) for d in dims[:-1])
        for a, b in zip(dims[:-1], dims[1:]):
            assert b == 2 * a, "patch merging doubles the width"
        self.norm = LayerNorm(dims[-1], eps=1e-5)
        self.pool = L.GlobalAvgPool()
        self.head = L.Linear(dims[-1], num_classes)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
        # stochastic depth: branch 2k = attention of block k, 2k + 1 = its MLP
        rates = DF.drop_path_rates(drop_path, sum(depths))
        self.drop_path = float(drop_path)
        self.drop_path_rates = [r for r in rates for _ in range(2)]
        if self.drop_path > 0:
            self.drop_path_seed = int(torch.randint(0, 2**62, (1,)).item()) \
                if drop_path_seed is None else int(drop_path_seed)
            self.register_buffer("drop_path_step", torch.zeros(1, dtype=torch.int64))

    def no_weight_decay(self):
        """The relative-position bias tables (2-D, so the 1-D rule misses them)."""
        return {f"stages.{i}.{j}.attn.table" for i, st in enumerate(self.stages)
                for j in range(len(st))}

    def _drop_path_scales(self, batch: int):
        """One scale row per branch for this forward (``None`` where the rate is
        0): a single draw launch, only in training with a non-zero rate."""
        rates = self.drop_path_rates
        if not (self.training and self.drop_path > 0):
            return [None] * len(rates)
        step = self.drop_path_step
        consts = self.__dict__.get("_dmp_drop_consts")
        if consts is None or consts[0].device != step.device:
            consts = DF.drop_path_consts(rates, step.device)
            self.__dict__["_dmp_drop_consts"] = consts
        table = DF.drop_path_table(step, *consts, batch, self.drop_path_seed)
        return [table[j] if p > 0 else None for j, p in enumerate(rates)]

    def forward(self, x):
        B, _, H, W = x.shape
        h = self.patch_norm(self.patch_embed(x))                      # [B, N, C] tokens
        h = h.reshape(B, H // self.patch, W // self.patch, h.shape[-1])
        scales = self._drop_path_scales(B)
        k = 0
        pending = pscale = None
        for i, stage in enumerate(self.stages):
            if i > 0:
                h, pending, pscale = self.merges[i - 1](h, pending, pscale), None, None
            for blk in stage:
                h, pending = blk(h, pending, pscale, scales[2 * k])
                pscale = scales[2 * k + 1]
                k += 1
        _, y = self.norm.add_forward(h, pending, pscale)
        return self.head(self.pool(y.permute(0, 3, 1, 2)))


def swin_tiny(num_classes: int = 1000, image_size: int = 224, drop_path: float = 0.0,
              drop_path_seed: int | None = None) -> SwinTransformer:
    return SwinTransformer(image_size, 4, 7, (2, 2, 6, 2), (96, 192, 384, 768), (3, 6, 12, 24),
                           num_classes=num_classes, drop_path=drop_path,
                           drop_path_seed=drop_path_seed)


def swin_mini(num_classes: int = 10, drop_path: float = 0.0,
              drop_path_seed: int | None = None) -> SwinTransformer:
    """32 x 32 images in 4 x 4 patches, window 4: two stages of two blocks, 64 and
    128 channels, 2 and 4 heads.  Stage 1 is an 8 x 8 map of four windows (its
    second block shifts by 2), stage 2 a single 4 x 4 window (no shift).  For tests
    and smoke runs."""
    return SwinTransformer(32, 4, 4, (2, 2), (64, 128), (2, 4), num_classes=num_classes,
                           drop_path=drop_path, drop_path_seed=drop_path_seed)
