"""CPU side of the streaming attention route (csrc/attention_stream.hip):

* floors: the streaming precision model (attention_stream_oracle.stream_fwd_emul,
  ko.attention_bwd_emul) against the fp64 references, over every cell of the GPU
  file and three input seeds, at ONE THIRD of the thresholds the GPU file uses;
* the planner (csrc/attn_plan.h) through csrc/attn_plan_check.cpp, built with
  the host compiler: routes, coverage, LDS and the refusals;
* the Python surface: the token cap, the route switch, the registry entries.
"""
import os
import shutil
import subprocess

import pytest
import torch

import attention_stream_oracle as so
import kernel_oracles as ko

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "distributed_ml_pytorch_amd", "csrc")
SEEDS = (0, 1, 2)


# --------------------------------------------------------------------- floors
@pytest.mark.parametrize("B,N,H,regime", so.STREAM_CELLS + [so.STREAM_CAP_CELL])
def test_stream_emulation_floor(B, N, H, regime):
    cell = (B, N, H, regime)
    for seed in SEEDS:
        qkv, dout = so.stream_inputs(B, N, H, regime, seed)
        out, lse2 = so.stream_fwd_emul(qkv, H)
        so.check_fwd(out, lse2, B, N, H, regime, margin=1 / 3, seed=seed)
        if cell != so.STREAM_CAP_CELL:
            dqkv = ko.attention_bwd_emul(qkv, out.to(torch.bfloat16), dout, lse2, H)
            so.check_bwd(dqkv, B, N, H, regime, margin=1 / 3, seed=seed)
    so.fwd_ref.cache_clear()
    so.bwd_ref.cache_clear()
    so.stream_inputs.cache_clear()


@pytest.mark.parametrize("B,N,H,regime", so.ROUTE_CELLS)
def test_stream_emulation_floor_at_resident_sizes(B, N, H, regime):
    """Route 1 at N <= 256 is held to the resident route's thresholds as they are."""
    for seed in SEEDS:
        qkv, dout = so.stream_inputs(B, N, H, regime, seed)
        out, lse2 = so.stream_fwd_emul(qkv, H)
        so.check_fwd(out, lse2, B, N, H, regime, margin=1 / 3, seed=seed, out_tol=ko.ATTN_OUT_TOL)
        dqkv = ko.attention_bwd_emul(qkv, out.to(torch.bfloat16), dout, lse2, H)
        so.check_bwd(dqkv, B, N, H, regime, margin=1 / 3, seed=seed)
    so.fwd_ref.cache_clear()
    so.bwd_ref.cache_clear()
    so.stream_inputs.cache_clear()


def test_loud_first_sets_the_max_in_the_first_tile():
    """The regime does what its name says: the loud token is token 0, and
    streaming in tiles changes the rounding (the model is not the resident one)."""
    B, N, H = 2, 385, 2
    qkv, _ = so.stream_inputs(B, N, H, "loud_first")
    loud, _ = so.stream_inputs(B, N, H, "loud")
    assert torch.equal(qkv, loud.flip(1))
    x = qkv.float().view(B, N, 3, H, 64)
    assert float(x[:, 0].abs().mean()) > 10 * float(x[:, 1:].abs().mean())
    sc1, _ = so.stream_inputs(B, N, H, "sc1")
    a, _ = so.stream_fwd_emul(sc1, H)
    b, _ = ko.attention_fwd_emul(sc1, H)
    assert not torch.equal(a, b)
    one, lse_one = so.stream_fwd_emul(sc1, H, kt=N)        # one tile: the resident model
    assert torch.equal(one, b)
    torch.testing.assert_close(lse_one, ko.attention_fwd_emul(sc1, H)[1], atol=1e-12, rtol=0)


# -------------------------------------------------------------------- planner
FIELDS = ("N route q_blocks k_blocks q_block k_block k_tile q_tile k_tiles q_tiles stages waves "
          "lds_fwd lds_dq lds_dkv grid_fwd grid_dq grid_dkv").split()


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("attn_plan") / "attn_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC,
                    os.path.join(CSRC, "attn_plan_check.cpp"), "-o", exe], check=True)

    def run(route, first, last, bh=1):
        r = subprocess.run([exe, str(route), str(first), str(last), str(bh)], check=True,
                           stdout=subprocess.PIPE, text=True)
        plans = {}
        for ln in r.stdout.splitlines():
            w = ln.split()
            plans[int(w[0])] = None if w[1] == "refused" else dict(zip(FIELDS, map(int, w)))
        assert sorted(plans) == list(range(first, last + 1))
        return plans

    return run


def test_planner_routes_and_coverage(plan_check):
    bh = 24
    plans = plan_check(-1, 0, 4097, bh)
    assert plans[0] is None and plans[4097] is None
    for N in range(1, 4097):
        p = plans[N]
        assert p is not None, N
        assert p["route"] == (0 if N <= 256 else 1), (N, p)
        # blocks x block size and tiles x tile size cover N, the last one is not empty
        for nb, size in (("q_blocks", "q_block"), ("k_blocks", "k_block"), ("k_tiles", "k_tile"),
                         ("q_tiles", "q_tile")):
            assert p[nb] * p[size] >= N > (p[nb] - 1) * p[size], (N, nb, p)
        assert max(p["lds_fwd"], p["lds_dq"], p["lds_dkv"]) <= 160 * 1024, (N, p)
        assert p["grid_fwd"] == p["grid_dq"] == bh * p["q_blocks"], (N, p)
        assert p["grid_dkv"] == bh * p["k_blocks"], (N, p)
        if p["route"] == 1:
            assert p["q_block"] == 16 * p["waves"] and p["k_tile"] == so.KT, (N, p)
            assert p["stages"] == 2 and 2 * p["lds_dkv"] <= 160 * 1024, (N, p)
            assert p["lds_fwd"] == p["stages"] * 2 * p["k_tile"] * 72 * 2, (N, p)
        else:
            assert p["q_blocks"] == p["k_tiles"] == 1 and p["stages"] == 1, (N, p)


def test_planner_forced_routes(plan_check):
    resident = plan_check(0, 0, 4097)
    assert all(resident[N] is not None and resident[N]["route"] == 0 for N in range(1, 257))
    assert all(resident[N] is None for N in [0] + list(range(257, 4098)))
    stream = plan_check(1, 0, 4097)
    assert all(stream[N] is not None and stream[N]["route"] == 1 for N in range(1, 4097))
    assert stream[0] is None and stream[4097] is None
    assert stream[1]["q_blocks"] == 1 and stream[4096]["q_blocks"] == 32
    for route in (2, -2):
        assert all(p is None for p in plan_check(route, 196, 258).values())
    # a grid past 2^31 - 1 is refused, not wrapped
    assert plan_check(1, 4096, 4096, (2**31 - 1) // 32)[4096] is not None
    assert plan_check(1, 4096, 4096, (2**31 - 1) // 32 + 1)[4096] is None


# ------------------------------------------------------------- Python surface
def test_python_surface(monkeypatch):
    from distributed_ml_pytorch_amd.models import REGISTRY, build_model
    from distributed_ml_pytorch_amd.ops import functional as DF

    assert DF.ATTENTION_MAX_TOKENS == 4096
    monkeypatch.delenv("DMP_ATTN_STREAM", raising=False)
    assert DF.attention_route() == -1
    monkeypatch.setenv("DMP_ATTN_STREAM", "1")
    assert DF.attention_route() == 1
    # CPU tensors never take the fused route, whatever N
    assert not DF.fused_attention_supported(torch.zeros(1, 300, 192, dtype=torch.bfloat16), 1)
    assert REGISTRY["vit_b16_384"][1:] == ((3, 384, 384), 1000)
    m, shape, nc = build_model("vit_mini_long")
    assert shape == (3, 80, 80) and nc == 10
    assert m.num_patches + 1 == 401 and len(m.blocks) == 2
    assert m.blocks[0].attn.heads == 2 and m.pos_embed.shape == (1, 401, 128)
    with torch.no_grad():
        y = m(torch.randn(2, *shape))
    assert y.shape == (2, 10) and bool(torch.isfinite(y).all())
