"""The sparse block top-k push wire on the CPU (parallel/wire_topk.py and its plumbing).

1. The format on crafted 256-element blocks: slot order against a selection
   written out element by element here, ``densify + residual == x`` exactly,
   unselected elements bit-identical, the zero-value and address skip rules.
2. Error feedback telescopes: over T pushes ``master_topk + accumulator`` equals
   the fp32-wire master up to fp32 summation rounding.
3. The central PS over gloo (1 PS + 2 workers), plain and with policy ``damp``.
4. Start-up refusals, the K range, the CLI flags, the server's K errors.
"""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.nn as nn

from test_dist_cpu import _run

from distributed_ml_pytorch_amd.parallel import messaging as M
from distributed_ml_pytorch_amd.parallel import wire, wire_topk

B = wire_topk.BLOCK
K = 8


def crafted_blocks():
    """Named 256-element blocks (fp32) that sit on the edges of the format (the
    ties are placed for K = 8); the last one is a 64-element tail."""
    g = torch.Generator().manual_seed(7)

    def small():
        # background below every crafted magnitude, no two magnitudes equal
        return (torch.rand(B, generator=g) + 0.5) * 1e-3 * torch.sign(torch.randn(B, generator=g))

    blocks = {}
    blocks["zero"] = torch.zeros(B)
    few = torch.zeros(B)
    few[3], few[77], few[255] = -0.25, 3.0, 1e-20
    blocks["few"] = few
    t = small()
    t[4], t[6] = 0.5, -0.5                    # one group of four (one lane of the kernel)
    blocks["tie_in_group"] = t
    t = small()
    t[10], t[77], t[200] = -0.75, 0.75, 0.75
    blocks["tie_across_groups"] = t
    t = small()
    t[0], t[255] = 2.0, -2.0
    blocks["tie_ends"] = t
    t = torch.zeros(B)
    t[[5, 17, 33, 64, 90, 128, 250]] = torch.tensor([9.0, -8.0, 7.0, 6.5, -6.0, 5.0, 4.0])
    t[100], t[200], t[201] = 1.5, -1.5, 1.0   # 8th and 9th largest equal: 100 in, 200 out
    blocks["tie_kth"] = t
    t = small()
    # halfway between two bf16 values (7 mantissa bits): to the even one
    t[:6] = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8),
                          2 + 2.0 ** -7, 2 + 3 * 2.0 ** -7])
    blocks["bf16_ties"] = t
    t = torch.zeros(B)
    # below half of bf16's smallest subnormal (2^-133): sent as zero, the slot is
    # skipped and the residual is x; 2^-134 is the tie (to even: zero); 2^-130 is a
    # bf16 subnormal and is sent exactly
    t[[2, 9, 40, 41]] = torch.tensor([2.0 ** -140, -(2.0 ** -149), 2.0 ** -134, 2.0 ** -130])
    blocks["subnormal"] = t
    t = small()
    t[12], t[13] = 2 - 2.0 ** -9, -3.999                  # round up into the next binade
    blocks["carry"] = t
    t = torch.randn(B, generator=g)
    t[3] = float("inf")
    blocks["inf"] = t
    t = torch.randn(B, generator=g)
    t[255] = float("nan")
    blocks["nan"] = t
    t = torch.randn(B, generator=g)
    t[[1, 2, 30, 31, 32, 100, 101, 180, 254]] = float("inf")
    t[[2, 100]] = float("-inf")
    t[[60, 181]] = float("nan")               # 11 non-finite values, more than K
    blocks["many_nonfinite"] = t
    blocks["tail64"] = torch.randn(64, generator=g) * 0.1
    return blocks


def crafted():
    blocks = crafted_blocks()
    names = list(blocks)
    assert names[-1] == "tail64"
    return names, torch.cat([blocks[k] for k in names])


def reference_selection(x: torch.Tensor, k: int):
    """Per block the (idx, bits) of the selected elements in slot order, written
    out element by element: larger magnitude bits first, then the lower index;
    zeros never."""
    bits = x.view(torch.int32).tolist()
    out = []
    for b0 in range(0, x.numel(), B):
        cand = [((bits[i] & 0x7FFFFFFF), i - b0) for i in range(b0, min(b0 + B, x.numel()))]
        cand = sorted((c for c in cand if c[0] > 0), key=lambda c: (-c[0], c[1]))[:k]
        out.append([i for _, i in cand])
    return out


def bf16_bits(bits: int) -> int:
    """fp32 bits -> bf16 bits in integer arithmetic: round to nearest even, one NaN."""
    bits &= 0xFFFFFFFF
    if bits & 0x7FFFFFFF > 0x7F800000:
        return 0x7FC0
    return ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16) & 0xFFFF


def check_spec(x: torch.Tensor, k: int):
    """Every property of the format that holds for any input."""
    n = x.numel()
    payload, resid = wire_topk.sparsify(x, k)
    nblk, nwords = wire_topk.layout(n, k)
    assert payload.dtype == torch.int32 and payload.numel() == nwords and resid.numel() == n
    assert resid.dtype == torch.float32
    want = reference_selection(x, k)
    bits = x.view(torch.int32).tolist()
    words = payload.view(nblk, k)
    selected = torch.zeros(n, dtype=torch.bool)
    for b, idxs in enumerate(want):
        got = words[b].tolist()
        assert [w & 0xFF for w in got[: len(idxs)]] == idxs, f"slot order in block {b}"
        assert all(w & 0xFF00 == 0 for w in got)
        assert got[len(idxs):] == [0] * (k - len(idxs)), f"empty slots of block {b}"
        for r, i in enumerate(idxs):
            assert ((got[r] >> 16) & 0xFFFF) == bf16_bits(bits[b * B + i])
            selected[b * B + i] = True
    # finite values: the integer rounding above is torch's conversion
    fin = torch.isfinite(x)
    assert [bf16_bits(v) for v, f in zip(bits, fin.tolist()) if f] == \
        (x[fin].to(torch.bfloat16).view(torch.int16).to(torch.int32) & 0xFFFF).tolist()
    # unselected elements: untouched, bits included
    assert torch.equal(resid.view(torch.int32)[~selected], x.view(torch.int32)[~selected])
    dense = wire_topk.densify(payload, n, k)
    finite = torch.isfinite(x)
    # the identity the error feedback rests on: exact
    assert torch.equal((dense + resid)[finite], x[finite])
    assert bool((dense[~selected] == 0).all())
    # selected non-finite values are sent and leave nothing behind
    bad = selected & ~finite
    assert bool((resid[bad] == 0).all())
    assert bool(((dense[bad] == x[bad]) | (torch.isnan(dense[bad]) & torch.isnan(x[bad]))).all())
    return payload, resid, dense


def test_layout():
    assert wire_topk.layout(0, 8) == (0, 0)
    assert wire_topk.layout(64, 8) == (1, 8)
    assert wire_topk.layout(256, 1) == (1, 1)
    assert wire_topk.layout(320, 32) == (2, 64)
    assert wire_topk.layout(65_600, 8) == (257, 2056)
    big = 86_567_656
    assert 4 * wire_topk.layout(big, 8)[1] / big < 0.1251       # 0.125 B per parameter
    for bad in (0, 33, -1, 2.5, True):
        with pytest.raises(ValueError):
            wire_topk.layout(256, bad)
    with pytest.raises(ValueError):
        wire_topk.layout(-1, 8)
    assert wire_topk.k_of(2056, 65_600) == 8
    for nwords in (2055, 0, 257 * 33):
        with pytest.raises(ValueError):
            wire_topk.k_of(nwords, 65_600)


def test_crafted_blocks():
    names, x = crafted()
    n = x.numel()
    assert n % B == 64
    payload, resid, dense = check_spec(x, K)
    at = {k: i * B for i, k in enumerate(names)}
    words = payload.view(-1, K)
    slot = {k: [w & 0xFF for w in words[i].tolist()] for i, k in enumerate(names)}

    assert words[names.index("zero")].tolist() == [0] * K
    assert slot["few"][:3] == [77, 3, 255] and words[names.index("few")][3:].tolist() == [0] * 5
    assert slot["tie_in_group"][:2] == [4, 6]
    assert slot["tie_across_groups"][:3] == [10, 77, 200]
    assert slot["tie_ends"][:2] == [0, 255]
    assert slot["tie_kth"] == [5, 17, 33, 64, 90, 128, 250, 100]
    u = at["tie_kth"]
    assert float(resid[u + 200]) == -1.5 and float(resid[u + 100]) == 0.0

    u = at["bf16_ties"]
    assert dense[u: u + 6].tolist() == [1.0, 1 + 2.0 ** -6, -1.0, -(1 + 2.0 ** -6), 2.0,
                                        2 + 2.0 ** -5]
    assert resid[u: u + 2].tolist() == [2.0 ** -8, -(2.0 ** -8)]

    u = at["subnormal"]
    w = words[names.index("subnormal")].tolist()
    assert slot["subnormal"][:4] == [41, 40, 2, 9]
    assert [x_ & 0x7FFF0000 for x_ in w[1:4]] == [0, 0, 0] and w[3] == (0x8000 << 16 | 9) - 2 ** 32
    assert dense[u + 41].item() == 2.0 ** -130 and resid[u + 41].item() == 0.0
    for i in (2, 9, 40):                       # skipped by every consumer: nothing is lost
        assert dense[u + i].item() == 0.0 and resid[u + i].item() == x[u + i].item() != 0.0

    u = at["carry"]
    assert dense[u + 12].item() == 2.0 and dense[u + 13].item() == -4.0
    assert resid[u + 12].item() == x[u + 12].item() - 2.0

    assert slot["inf"][0] == 3 and dense[at["inf"] + 3].item() == float("inf")
    assert slot["nan"][0] == 255 and words[names.index("nan")][0].item() >> 16 == 0x7FC0
    assert slot["many_nonfinite"] == [60, 181, 1, 2, 30, 31, 32, 100]     # NaN above Inf
    u = at["many_nonfinite"]
    assert torch.isinf(resid[u + 101]) and torch.isinf(resid[u + 254])    # out: still there

    assert torch.equal(dense[at["tail64"]:],
                       wire_topk.densify(wire_topk.sparsify(x[at["tail64"]:], K)[0], 64, K))


def test_random_blocks_sizes_and_ks():
    g = torch.Generator().manual_seed(11)
    for n in (64, 256, 320, 1000, 65_600):
        nblk = -(-n // B)
        mag = torch.exp2(torch.rand(nblk, generator=g) * 40 - 30).repeat_interleave(B)[:n]
        x = torch.randn(n, generator=g) * mag
        for k in (1, 8, 32):
            check_spec(x, k)
    # any shape in, flat out; an empty payload
    p, r = wire_topk.sparsify(torch.ones(3, 5), 4)
    assert r.shape == (15,) and wire_topk.densify(p, 15, 4).tolist() == [1.0] * 4 + [0.0] * 11
    p, r = wire_topk.sparsify(torch.zeros(0), 4)
    assert p.numel() == 0 and r.numel() == 0 and wire_topk.densify(p, 0, 4).numel() == 0
    for bad in (torch.zeros(8, dtype=torch.int64), torch.zeros(7, dtype=torch.int32),
                torch.zeros(8, dtype=torch.float32)):
        with pytest.raises(ValueError):
            wire_topk.densify(bad, 256, 8)


def test_consumers_skip_zero_values_and_foreign_addresses():
    n = 320
    payload = torch.zeros(2 * K, dtype=torch.int32)
    one = 0x3F80 << 16
    payload[0] = one | 5                       # block 0, offset 5
    payload[1] = 0 | 17                        # value +0 with an index: skipped
    payload[2] = (0x8000 << 16 | 9) - 2 ** 32  # value -0: skipped
    payload[K] = one | 63                      # block 1, the tail's last element
    payload[K + 1] = one | 200                 # 256 + 200 >= n: ignored
    at, val = wire_topk.entries(payload, n, K)
    assert at.tolist() == [5, 256 + 63] and val.tolist() == [1.0, 1.0]
    master = torch.full((n,), -0.0)
    wire.codec(payload).apply(master, payload, 0.5)
    want = torch.full((n,), -0.0)
    want[5] = want[319] = 0.5
    assert torch.equal(master.view(torch.int32), want.view(torch.int32))    # -0 stays -0


def test_codec():
    c = wire.topk(K)
    assert c is wire.topk(8) and c is wire.codec(M.topk(8)) and c is not wire.topk(4)
    assert c.payload_shape(320) == (16, 16, torch.int32) and c.header == "topk8"
    h = M.make_header(M.MessageCode.GradientUpdate, 1, 2, 3, 320, c.header)
    assert int(h[5]) == 16 + 8 and M.parse_header(h)[5] == "topk8"
    assert [M.make_header(0, 0, dtype=d)[5].item()
            for d in (torch.float32, torch.bfloat16, torch.float16, M.MX8)] == [0, 1, 2, 3]
    assert M.payload_buffer(320, M.topk(4)).shape == (8,)
    assert M.payload_buffer(320, M.topk(4)).dtype == torch.int32
    buf = c.new_payload(320, "cpu")
    assert buf.dtype == torch.int32 and not buf.any()
    g = torch.Generator().manual_seed(3)
    acc = torch.randn(320, generator=g)
    x = acc.clone()
    c.handoff(acc, buf)
    assert torch.equal(c.decode(buf, 320) + acc, x)
    # an int32 tensor finds its reader; K comes from the size, and a size that does
    # not divide is an error
    reader = wire.codec(buf)
    assert reader.k is None and torch.equal(reader.decode(buf, 320), c.decode(buf, 320))
    with pytest.raises(ValueError):
        reader.decode(buf[:15], 320)
    with pytest.raises(ValueError):
        wire.topk(4).apply(torch.zeros(320), buf, 1.0)        # a K = 8 payload
    with pytest.raises(ValueError):
        reader.payload_shape(320)


# ------------------------------------------------------------- error feedback
def _mlp():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(8, 16), nn.ReLU(), nn.Linear(16, 4))


def _local_run(push_wire: str, pushes: int, **kw):
    from distributed_ml_pytorch_amd.parallel.asgd import Asynchronous
    from distributed_ml_pytorch_amd.parallel.clients import LocalPSClient

    m = _mlp()
    client = LocalPSClient(staleness=0)
    client.request_pull = lambda step: None          # pulls off: the runs share a trajectory
    opt = Asynchronous(m.parameters(), lr=0.05, n_push=1, n_pull=1, model=m, client=client,
                       shadow_dtype=None, push_wire=push_wire, **kw)
    g = torch.Generator().manual_seed(5)
    for _ in range(pushes):
        x = torch.randn(16, 8, generator=g)
        y = torch.randn(16, 4, generator=g)
        opt.zero_grad()
        nn.functional.mse_loss(m(x), y).backward()
        opt.step()
    opt.finish()
    return client, opt


def test_error_feedback_telescopes():
    """master_topk + accumulator == master_fp32 up to fp32 summation rounding: each
    of the T pushes adds one fp32 sum per element on either side (accumulate,
    apply, and what stayed behind carried into the next accumulate), hence
    8 T eps32 max|master| -- the bound of test_wire8_cpu, by the same argument."""
    T = 12
    c32, o32 = _local_run("same", T)
    ck, ok = _local_run("topk", T, push_topk=K)
    assert c32.pushes == ck.pushes == T
    assert torch.equal(o32.arena.p32, ok.arena.p32)          # same local trajectory
    assert float(o32.acc.abs().max()) == 0.0
    assert float(ok.acc.abs().max()) > 0.0                   # what was not sent is kept
    n = ok.acc.numel()
    assert ck.bytes_sent == T * 4 * -(-n // B) * K and c32.bytes_sent == T * 4 * n
    atol = 8 * T * 2.0 ** -23 * float(c32.master.abs().max())
    err = float((ck.master.double() + ok.acc.double() - c32.master.double()).abs().max())
    lost = float((ck.master - c32.master).abs().max())
    print("telescoping err", err, "atol", atol, "master alone is off by", lost)
    assert err <= atol
    assert lost > atol            # without the accumulator the masters do differ


# ------------------------------------------------- start-up refusals, the CLI
def test_unsupported_flavours_raise_at_start_up():
    from distributed_ml_pytorch_amd.parallel.asgd import Asynchronous
    from distributed_ml_pytorch_amd.parallel.async_sharded import AsyncShardedPSClient
    from distributed_ml_pytorch_amd.parallel.clients import (LocalPSClient, SharedPS,
                                                             SharedPSClient, ShardedPSClient)
    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, Worker

    for make in (lambda: ShardedPSClient(), lambda: SharedPSClient(SharedPS()),
                 lambda: AsyncShardedPSClient(), lambda: ShardedPSClient(push_wire="topk")):
        m = _mlp()
        with pytest.raises(ValueError, match="LocalPSClient.*GlooPSClient.*RcclPSClient"):
            Asynchronous(m.parameters(), lr=0.1, n_push=1, n_pull=1, model=m, client=make(),
                         shadow_dtype=None, push_wire="topk")
    with pytest.raises(ValueError, match="'same' or 'mx8' or 'topk'"):
        LocalPSClient(push_wire="top")
    for bad in (0, 33, -8):
        with pytest.raises(ValueError, match="1..32"):
            LocalPSClient(push_wire="topk", push_topk=bad)
        m = _mlp()
        with pytest.raises(ValueError, match="1..32"):
            Asynchronous(m.parameters(), lr=0.1, n_push=1, n_pull=1, model=m,
                         client=LocalPSClient(), shadow_dtype=None, push_wire="topk",
                         push_topk=bad)
    info = DistInfo(device=torch.device("cpu"))
    base = dict(model="mlp", cuda=False, push_wire="topk", verbose=False, evaluate=False)
    for kw in (dict(mode="sync"), dict(mode="single"), dict(mode="asgd", ps="sharded"),
               dict(mode="asgd", ps="sharded_async")):
        with pytest.raises(ValueError, match="--push-wire topk is not supported"):
            Worker(TrainConfig(**base, **kw), info)
    with pytest.raises(ValueError, match="SharedPSClient .virtual workers."):
        Worker(TrainConfig(**base, mode="asgd"), info, client=SharedPSClient(SharedPS()))
    with pytest.raises(ValueError, match="1..32"):
        Worker(TrainConfig(**base, mode="asgd", ps="local", push_topk=40), info)
    # the supported single-process flavour starts, at the configured K
    w = Worker(TrainConfig(**base, mode="asgd", ps="local", push_topk=4), info)
    assert w.opt.client.push_codec is wire.topk(4) and not w.opt.client.mx8


def test_cli_flags():
    from distributed_ml_pytorch_amd.cli import build_parser, config_from_args

    cfg = config_from_args(build_parser().parse_args([]))
    assert cfg.push_wire == "same" and cfg.push_topk == 8
    cfg = config_from_args(build_parser().parse_args(["--push-wire", "topk", "--push-topk", "4"]))
    assert cfg.push_wire == "topk" and cfg.push_topk == 4
    assert config_from_args(build_parser().parse_args(["--push-wire", "topk"])).push_topk == 8


# ------------------------------------------------------- central PS over gloo
PUSHES, LR, S = 6, 0.05, 1
SCENARIOS = {"plain": dict(stale_policy="off", delta_scale=0.5),
             "damp": dict(stale_policy="damp", stale_bound=S, delta_scale="sum")}


def _central_worker(rank):
    from distributed_ml_pytorch_amd.parallel.asgd import Asynchronous
    from distributed_ml_pytorch_amd.parallel.clients import GlooPSClient

    class Recording(GlooPSClient):
        """Keeps a copy of every payload it pushes."""

        def _handoff(self, n=None):
            buf = super()._handoff(n)
            self.sent.append(buf.clone())
            return buf

    m = _mlp()
    client = Recording(ps_rank=0, staleness=0)
    client.sent = []
    # one pull at step 0, then none: every later push is computed from version <= 1,
    # so its staleness grows with the PS version and policy damp has work to do
    opt = Asynchronous(m.parameters(), lr=LR, n_push=1, n_pull=1000, model=m, client=client,
                       shadow_dtype=None, push_wire="topk", push_topk=K)
    init = opt.arena.p32.clone()
    g = torch.Generator().manual_seed(100 + rank)
    for _ in range(PUSHES):
        x = torch.randn(16, 8, generator=g)
        y = torch.randn(16, 4, generator=g)
        opt.zero_grad()
        nn.functional.mse_loss(m(x), y).backward()
        opt.step()
    opt.finish()
    return {"pushes": client.pushes, "bytes_sent": client.bytes_sent, "n": opt.acc.numel(),
            "init": init.numpy(), "sent": torch.stack(client.sent).numpy(),
            "residual": opt.acc.clone().numpy()}


def _central(rank, world):
    from distributed_ml_pytorch_amd.parallel.server import ParameterServer

    out = {}
    for name, kw in SCENARIOS.items():
        dist.barrier()
        if rank == 0:
            ps = ParameterServer(model=_mlp(), workers=[1, 2], push_topk=K, **kw)
            st = ps.run()
            out[name] = {"stats": st, "master": ps.parameters().clone().numpy(),
                         "log": list(ps.gate.log), "scale": ps.delta_scale}
        else:
            out[name] = _central_worker(rank)
    return out


@pytest.fixture(scope="module")
def central():
    return _run(_central, 3)


@pytest.mark.slow
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_central_ps_over_gloo(central, name):
    ps = central[0][name]
    st, log = ps["stats"], ps["log"]
    n = central[1][name]["n"]
    nwords = wire_topk.layout(n, K)[1]
    for r in (1, 2):
        w = central[r][name]
        assert w["pushes"] == PUSHES and w["bytes_sent"] / w["pushes"] == 4 * nwords
        assert w["sent"].shape == (PUSHES, nwords)
        assert float(abs(torch.from_numpy(w["residual"])).max()) > 0
    assert st["counts"]["GradientUpdate"] == 2 * PUSHES == len(log)
    assert st["bytes_in"] == 2 * (4 * n + PUSHES * 4 * nwords)       # the init + the pushes
    # master = init + sum_k scale * f_k * densify(payload_k), in float64, with the
    # factor the PS logged for each push (a worker's pushes arrive in its own order)
    want = torch.from_numpy(central[1][name]["init"]).double()
    dense = {r: [wire_topk.densify(torch.from_numpy(p), n, K).double()
                 for p in central[r][name]["sent"]] for r in (1, 2)}
    nxt = {1: 0, 2: 0}
    for w, tau, f in log:
        want = want + ps["scale"] * f * dense[w][nxt[w]]
        nxt[w] += 1
    assert nxt == {1: PUSHES, 2: PUSHES}
    got = torch.from_numpy(ps["master"]).double()
    # fp32 rounding: every apply rounds the factor, the product and the sum once
    tol = len(log) * 3 * 2.0 ** -24 * max(1.0, float(want.abs().max()))
    err = float((got - want[: got.numel()]).abs().max())
    print(name, "master err", err, "tol", tol, "damped", st["damped"])
    assert err <= tol
    assert float((got - torch.from_numpy(central[1][name]["init"]).double()).abs().max()) > 0
    if name == "damp":
        assert st["damped"] > 0 and any(f != 1.0 for _, _, f in log)
    else:
        assert st["damped"] == 0


# ------------------------------------------------------------- server errors
@pytest.fixture
def world1():
    """A one-rank gloo world in this process (the server only asks that one exists)."""
    made = not dist.is_initialized()
    if made:
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=0, world_size=1)
    yield
    if made:
        dist.destroy_process_group()


def test_server_refuses_a_foreign_k(world1):
    from distributed_ml_pytorch_amd.parallel.server import ParameterServer

    code = M.MessageCode.GradientUpdate
    n = 320
    ps = ParameterServer(numel=n, workers=[], push_topk=K)
    with pytest.raises(RuntimeError, match="K = 4.*push_topk = 8"):
        ps.handle(code, 1, 0, 0, n, M.topk(4))
    off = ParameterServer(numel=n, workers=[])
    with pytest.raises(RuntimeError, match="K = 8.*push_topk = 0"):
        off.handle(code, 1, 0, 0, n, M.topk(8))
    with pytest.raises(RuntimeError, match="parameters on the top-k wire"):
        ps.handle(M.MessageCode.ParameterUpdate, 1, 0, 0, n, M.topk(8))
    with pytest.raises(ValueError, match="1..32"):
        ParameterServer(numel=n, workers=[], push_topk=33)
    # the other wires are as before: an MX8 header still reaches the payload receive
    assert wire.topk(K) in ps._codecs() and wire.topk(K) not in off._codecs()
    assert off._codecs() == (wire.FP32, wire.BF16, wire.MX8)
