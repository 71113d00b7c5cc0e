"""ConvNeXt (Liu et al. 2022, "A ConvNet for the 2020s"): the convolutional model
of the AdamW / stochastic-depth / EMA / Mixup-CutMix / random-resized-crop recipe.

A block is depthwise 7x7 conv (bias) -> LayerNorm (eps 1e-6) -> fc1 to 4C -> GELU
-> fc2 to C -> layer scale -> residual add, as in the paper and torchvision.  The
residual stream is kept channels-last, ``[B, H, W, C]``: its rows feed LayerNorm
and the MLP GEMMs without a copy, and the same memory, seen as a channels-last
``[B, C, H, W]`` view, feeds the depthwise conv.  On the GPU every op is native:
the depthwise kernels (``csrc/dwconv.hip``), LayerNorm (``csrc/transformer.hip``),
the fused fc1 + GELU / fc2 + GELU' MLP (``ops.linear.mlp``), and the block's
closing ``x + gamma * branch`` (``csrc/layer_scale.hip``), which also consumes the
per-sample stochastic-depth scale.  The stem is a ``patch x patch`` / stride
``patch`` conv through ``PatchEmbed``'s GEMM, then LayerNorm; between stages a
LayerNorm and a 2x2 / stride-2 conv; the head is global average pool, LayerNorm,
Linear.

The GELU is this project's tanh form, as in the ViT; it differs from torchvision's
erf form by less than bf16 resolution, and no weight compatibility is claimed.
ConvNeXt-T has 28,589,128 parameters with a 1000-class head.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..ops import functional as DF
from ..ops import layers as L
from ..ops.linear import mlp, mlp_ok
from .vit import LayerNorm, PatchEmbed


class Block(nn.Module):
    def __init__(self, dim: int, layer_scale_init: float):
        super().__init__()
        self.dwconv = L.Conv2d(dim, dim, kernel_size=7, padding=3, groups=dim)
        self.norm = LayerNorm(dim, eps=1e-6)
        self.fc1 = L.Linear(dim, 4 * dim)
        self.fc2 = L.Linear(4 * dim, dim)
        self.gamma = nn.Parameter(torch.full((dim,), float(layer_scale_init)))

    def forward(self, h, scale=None):
        """``h``: ``[B, H, W, C]``; ``scale``: the block's per-sample stochastic-depth
        scales (``None``: the branch is added as it is)."""
        # the conv hands h back as a second output: h's two readers (conv, add)
        # become one, and the add's gradient joins the conv's data gradient in
        # its epilogue instead of in an autograd add over the stream
        y, ha = self.dwconv(h.permute(0, 3, 1, 2), alias=True)
        y = self.norm(y.permute(0, 2, 3, 1))
        if mlp_ok(y, self.fc1, self.fc2):
            y = mlp(y, self.fc1, self.fc2)          # GELU fused into the GEMM epilogues
        else:
            y = self.fc2(DF.gelu(self.fc1(y)))
        slots = DF.layer_scale_slots(self, self.gamma) if y.is_cuda else None
        return DF.layer_scale_add(ha.permute(0, 2, 3, 1), y, self.gamma, scale, slots)


class ConvNeXt(nn.Module):
    def __init__(self, depths=(3, 3, 9, 3), dims=(96, 192, 384, 768), patch: int = 4,
                 num_classes: int = 1000, layer_scale_init: float = 1e-6, drop_path: float = 0.0,
                 drop_path_seed: int | None = None, in_chans: int = 3):
        """``drop_path``: stochastic depth, the rate of the last block of the linear
        ramp over all blocks (one branch per block); ``drop_path_seed``: its Philox
        key, drawn from torch's generator when None."""
        super().__init__()
        assert len(depths) == len(dims) and len(depths) >= 1
        self.patch = patch
        self.stem = PatchEmbed(in_chans, dims[0], kernel_size=patch, stride=patch)
        self.stem_norm = LayerNorm(dims[0], eps=1e-6)
        self.stages = nn.ModuleList(
            nn.ModuleList(Block(d, layer_scale_init) for _ in range(n))
            for n, d in zip(depths, dims))
        self.down_norms = nn.ModuleList(LayerNorm(d, eps=1e-6) for d in dims[:-1])
        self.down_convs = nn.ModuleList(L.Conv2d(a, b, kernel_size=2, stride=2)
                                        for a, b in zip(dims[:-1], dims[1:]))
        self.pool = L.GlobalAvgPool()
        self.norm = LayerNorm(dims[-1], eps=1e-6)
        self.head = L.Linear(dims[-1], num_classes)
        for m in self.modules():
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.trunc_normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
        self.drop_path = float(drop_path)
        self.drop_path_rates = DF.drop_path_rates(drop_path, sum(depths))
        if self.drop_path > 0:
            self.drop_path_seed = int(torch.randint(0, 2**62, (1,)).item()) \
                if drop_path_seed is None else int(drop_path_seed)
            # the step counter of the draws: the only persistent state (a model
            # built without drop_path has no such state_dict key)
            self.register_buffer("drop_path_step", torch.zeros(1, dtype=torch.int64))

    def no_weight_decay(self):
        """The layer-scale ``gamma``s: 1-D, so AdamW's weight decay skips them
        anyway; named for clarity."""
        return {f"stages.{i}.{j}.gamma" for i, st in enumerate(self.stages)
                for j in range(len(st))}

    def _drop_path_scales(self, batch: int):
        """One scale row per block for this forward (``None`` where the rate is 0):
        a single draw launch, only in training with a non-zero rate."""
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
        h = self.stem_norm(self.stem(x))                              # [B, N, C] tokens
        h = h.reshape(B, H // self.patch, W // self.patch, h.shape[-1])
        scales = self._drop_path_scales(B)
        j = 0
        for i, stage in enumerate(self.stages):
            if i > 0:
                y = self.down_norms[i - 1](h).permute(0, 3, 1, 2)
                h = self.down_convs[i - 1](y).permute(0, 2, 3, 1)
            for blk in stage:
                h = blk(h, scales[j])
                j += 1
        return self.head(self.norm(self.pool(h.permute(0, 3, 1, 2))))


def convnext_tiny(num_classes: int = 1000, drop_path: float = 0.0,
                  drop_path_seed: int | None = None) -> ConvNeXt:
    return ConvNeXt((3, 3, 9, 3), (96, 192, 384, 768), 4, num_classes, drop_path=drop_path,
                    drop_path_seed=drop_path_seed)


def convnext_mini(num_classes: int = 10, drop_path: float = 0.0,
                  drop_path_seed: int | None = None) -> ConvNeXt:
    """Two stages of two blocks, 64 and 128 channels, for 32 x 32 images: tests and
    smoke runs."""
    return ConvNeXt((2, 2), (64, 128), 4, num_classes, drop_path=drop_path,
                    drop_path_seed=drop_path_seed)
