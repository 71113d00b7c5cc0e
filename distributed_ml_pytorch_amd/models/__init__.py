"""Model zoo: the reference's LeNet/AlexNet plus the BASELINE.json families."""
from __future__ import annotations

from .cnn import MLP, AlexNet, LeNet
from .resnet import ResNet, resnet18, resnet34, resnet50, resnet101
from .vit import VisionTransformer, vit_b16, vit_mini_long, vit_tiny

# name -> (constructor, input shape (C,H,W), num_classes)
REGISTRY = {
    "mlp": (lambda nc=10: MLP(num_classes=nc), (1, 28, 28), 10),
    "lenet": (lambda nc=10: LeNet(nc), (3, 32, 32), 10),
    "alexnet": (lambda nc=10: AlexNet(nc), (3, 32, 32), 10),
    "resnet18": (lambda nc=10: resnet18(nc, stem="cifar"), (3, 32, 32), 10),
    "resnet34": (lambda nc=10: resnet34(nc, stem="cifar"), (3, 32, 32), 10),
    "resnet50": (lambda nc=1000: resnet50(nc, stem="imagenet"), (3, 224, 224), 1000),
    "resnet50_cifar": (lambda nc=10: resnet50(nc, stem="cifar"), (3, 32, 32), 10),
    "resnet101": (lambda nc=1000: resnet101(nc, stem="imagenet"), (3, 224, 224), 1000),
    "vit_b16": (lambda nc=1000, **kw: vit_b16(nc, **kw), (3, 224, 224), 1000),
    "vit_b16_384": (lambda nc=1000, **kw: vit_b16(nc, image_size=384, **kw), (3, 384, 384), 1000),
    "vit_tiny": (lambda nc=10, **kw: vit_tiny(nc, **kw), (3, 32, 32), 10),
    "vit_mini_long": (lambda nc=10, **kw: vit_mini_long(nc, **kw), (3, 80, 80), 10),
}


def is_vit(name: str) -> bool:
    return _key(name).startswith("vit_")


def _key(name: str) -> str:
    key = name.lower().replace("-", "_").replace("/", "")
    return "vit_b16" if key == "vit_b_16" else key


def build_model(name: str, num_classes: int | None = None, drop_path: float = 0.0):
    """Return ``(model, input_shape, num_classes)`` for a registry name.
    ``drop_path``: stochastic depth rate, for the ViTs only."""
    key = _key(name)
    if key not in REGISTRY:
        raise KeyError(f"unknown model {name!r}; choose from {sorted(REGISTRY)}")
    ctor, shape, nc = REGISTRY[key]
    nc = nc if num_classes is None else num_classes
    if not 0.0 <= drop_path < 1.0:
        raise ValueError(f"drop path rate must be in [0, 1), got {drop_path}")
    if drop_path > 0:
        if not is_vit(key):
            raise ValueError(f"drop_path {drop_path} with model {name!r}: stochastic depth exists "
                             "for the ViT models only (their residual adds carry it)")
        return ctor(nc, drop_path=drop_path), shape, nc
    return ctor(nc), shape, nc


__all__ = ["MLP", "AlexNet", "LeNet", "ResNet", "resnet18", "resnet34", "resnet50", "resnet101",
           "VisionTransformer", "vit_b16", "vit_mini_long", "vit_tiny", "REGISTRY", "build_model",
           "is_vit"]
