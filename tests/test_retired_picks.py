"""Tune-cache picks of retired kernel arms are refused by name (no GPU needed): only a
private cache written with the old opt-in switches on can still hold one."""
import pytest
import torch


def test_cached_split_k_pick_outside_wgrad_raises(monkeypatch):
    from distributed_ml_pytorch_amd.ops import linear as L

    a = torch.zeros(16, 64, dtype=torch.bfloat16)
    b = torch.zeros(32, 64, dtype=torch.bfloat16)
    c = torch.full((16, 32), 7.0, dtype=torch.bfloat16)
    key = ("gemm", 0, 0, 16, 32, 64, False, False, False, False)
    monkeypatch.setitem(L.TUNER.cache, key, L._enc(4, 2))
    with pytest.raises(RuntimeError, match=r"only in the weight-gradient mode") as e:
        L.gemm(0, 0, a, b, c)
    assert str(key) in str(e.value)
    assert bool((c == 7.0).all())


def test_cached_patch_matrix_wgrad_pick_raises(monkeypatch):
    from distributed_ml_pytorch_amd.ops import conv as C

    x = torch.zeros(2, 64, 8, 8, dtype=torch.bfloat16)
    dy = torch.zeros(2, 64, 8, 8, dtype=torch.bfloat16)
    key = ("wgrad", 2, 64, 8, 8, 64, 64, 3, 3, 1, 1)
    monkeypatch.setitem(C.TUNER.cache, key, 30001)
    with pytest.raises(RuntimeError, match=r"retired patch-matrix weight-gradient route") as e:
        C._wgrad_cfg(dy, x, (64, 64, 3, 3), 1, 1)
    assert str(key) in str(e.value)
