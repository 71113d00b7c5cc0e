"""GroupNorm on the CPU: the ``*_gn`` ResNets (parameter counts, no buffers, a
forward / backward), ``L.GroupNorm`` against ``F.group_norm``, the BatchNorm
models' unchanged state dicts, and the planner of the native kernels
(csrc/group_norm_plan.h) through csrc/group_norm_plan_check.cpp, built stand-alone
under AddressSanitizer + UndefinedBehaviorSanitizer and run."""
import os
import re
import shutil
import subprocess

import pytest
import torch
import torch.nn.functional as F

from distributed_ml_pytorch_amd.models import build_model
from distributed_ml_pytorch_amd.ops import layers as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed_ml_pytorch_amd", "csrc")


@pytest.mark.parametrize("name,params", [("resnet18", 11_173_962), ("resnet50", 25_557_032)])
def test_gn_models_count_and_bn_keys(name, params):
    gn, _, _ = build_model(name + "_gn")
    bn, _, _ = build_model(name)
    assert sum(p.numel() for p in gn.parameters()) == params
    assert sum(p.numel() for p in bn.parameters()) == params
    assert list(gn.buffers()) == []
    assert not any(isinstance(m, torch.nn.modules.batchnorm._BatchNorm) for m in gn.modules())
    # the BatchNorm model keeps its keys: the GN model's, plus three buffers per BN
    keys = set(bn.state_dict())
    extra = {k for k in keys if k.rsplit(".", 1)[1] in
             ("running_mean", "running_var", "num_batches_tracked")}
    assert keys - extra == set(gn.state_dict())
    assert len(extra) == 3 * sum(isinstance(m, L.BatchNorm2d) for m in bn.modules())


def test_resnet18_gn_cpu_step_and_no_mode():
    torch.manual_seed(0)
    model, shape, nc = build_model("resnet18_gn")
    x = torch.randn(2, *shape)
    loss = F.cross_entropy(model(x), torch.tensor([1, 3]))
    loss.backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.parameters())
    with torch.no_grad():
        assert torch.equal(model.eval()(x), model.train()(x))


@pytest.mark.parametrize("relu,res", [(False, False), (True, False), (False, True), (True, True)])
def test_layer_matches_torch_group_norm(relu, res):
    g = torch.Generator().manual_seed(3)
    layer = L.GroupNorm(4, 24, relu=relu)
    with torch.no_grad():
        layer.weight.copy_(torch.randn(24, generator=g))
        layer.bias.copy_(torch.randn(24, generator=g))
    x = torch.randn(3, 24, 5, 7, generator=g) + 3
    r = torch.randn(3, 24, 5, 7, generator=g) if res else None
    ref = F.group_norm(x, 4, layer.weight, layer.bias, layer.eps)
    ref = ref + r if res else ref
    ref = torch.relu(ref) if relu else ref
    assert list(layer.state_dict()) == ["weight", "bias"]
    torch.testing.assert_close(layer(x, residual=r), ref, rtol=1e-5, atol=1e-5)


def test_group_norm_plan_check_clean(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "group_norm_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(CSRC, "group_norm_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    out = r.stdout
    assert r.returncode == 0, out
    assert "FAIL" not in out and "runtime error" not in out and "AddressSanitizer" not in out, out
    m = re.search(r"group_norm_plan_check: (\d+) checks, (\d+) failed", out)
    assert m and int(m.group(1)) > 100000 and int(m.group(2)) == 0, out
    assert "plan N 128 112x112x64 fwd: stream" in out
    assert "plan N 512 32x32x64 fwd: resident" in out
