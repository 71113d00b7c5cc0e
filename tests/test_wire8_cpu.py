"""The block-scaled 8-bit push wire on the CPU (parallel/wire8.py and its plumbing).

1. The format on crafted blocks: scale rule, RNE ties, the saturating band,
   E4M3 subnormals, a 4-element tail block, non-finite blocks, the exact
   ``dequant + residual == x`` identity and the per-element half-quantum bound.
2. Error feedback telescopes: over T pushes ``master_mx8 + residual`` equals the
   fp32-wire master up to fp32 summation rounding.
3. The central PS over gloo (1 PS + 2 workers), plain and with policy ``damp``.
4. Unsupported flavours refuse ``push_wire="mx8"`` at start-up.
"""
import pytest
import torch
import torch.distributed as dist
import torch.nn as nn

from test_dist_cpu import _run

from distributed_ml_pytorch_amd.parallel import wire8

B = wire8.BLOCK


def crafted_blocks():
    """Named 32-element blocks (fp32) that sit on the edges of the format."""
    g = torch.Generator().manual_seed(7)
    blocks = {}
    blocks["zero"] = torch.zeros(B)
    # amax an exact power of two: 2^-3 -> E = 124, sb = 116, amax scales to exactly 256
    p2 = (torch.rand(B, generator=g) - 0.5) * 0.2
    p2[5] = 0.125
    blocks["pow2"] = p2
    # saturating band: amax = 1.96875 (E = 127, sb = 119, scale 2^-8) scales to 504;
    # everything in amax * [0.875, 1) scales into [441, 504), most of it past 448
    sat = 1.96875 * (0.875 + 0.125 * torch.rand(B, generator=g))
    sat[::2] *= -1
    sat[0], sat[1], sat[2], sat[3] = 1.96875, 1.75, -1.8125, 1.9     # 504, 448, -464, 486.4
    blocks["sat"] = sat
    # amax 300 (E = 135, sb = 127, scale 1): exact ties of the 3-bit mantissa and of
    # the subnormal grid (quantum 2^-9)
    ties = torch.zeros(B)
    ties[:12] = torch.tensor([300.0, 17.0, 19.0, -21.0, 23.0, 2.0 ** -10, 3 * 2.0 ** -10,
                              -5 * 2.0 ** -10, 0.0146484375, 272.0, 1.0625, -1.1875])
    blocks["ties"] = ties
    # values that land in E4M3's subnormal range (scaled magnitude below 2^-6)
    sub = torch.zeros(B)
    sub[:10] = torch.tensor([256.0, 2.0 ** -7, 5 * 2.0 ** -9, 2.0 ** -9, 1e-3, -1e-3, 1e-5, 3e-3,
                             -7e-3, 0.0155])
    blocks["subnormal"] = sub
    # the ends of the scale byte: fp32 subnormals only (sb clamps at 0), near fp32 max
    blocks["tiny"] = torch.rand(B, generator=g) * 2.0 ** -140
    big = (torch.rand(B, generator=g) - 0.5) * 1e38
    big[9] = 3.0e38
    blocks["huge"] = big
    inf = torch.randn(B, generator=g)
    inf[3] = float("inf")
    blocks["inf"] = inf
    nan = torch.randn(B, generator=g)
    nan[31] = float("nan")
    blocks["nan"] = nan
    blocks["tail4"] = torch.tensor([0.3, -0.7, 0.011, 0.5])
    return blocks


def crafted():
    blocks = crafted_blocks()
    names = list(blocks)
    assert names[-1] == "tail4"
    return names, torch.cat([blocks[k] for k in names])


def half_quantum_bound(x: torch.Tensor, sb: torch.Tensor) -> torch.Tensor:
    """Largest |residual| the format allows for element ``x`` at scale byte ``sb``
    (float64).  With s = |x| * 2^-(sb - 127) the scaled magnitude:

    * s > 448 (clamped): exactly s - 448, and below 64 since s < 512;
    * 2^-6 <= s <= 448 (E4M3 normal, 3 mantissa bits): half an ulp of s's own
      binade, 2^(floor(log2 s) - 4);
    * s < 2^-6 (E4M3 subnormal, quantum 2^-9): 2^-10.
    """
    s = torch.ldexp(x.double().abs(), 127 - sb)
    _, ex = torch.frexp(s)                           # s = m * 2^ex, m in [0.5, 1)
    normal = torch.ldexp(torch.ones_like(s), ex - 1 - 4)
    bound = torch.where(s < 2.0 ** -6, torch.full_like(s, 2.0 ** -10), normal)
    bound = torch.where(s > 448, s - 448, bound)
    assert bool((s < 512).all())
    return torch.ldexp(bound, sb - 127)


def per_element_scale(payload, n):
    _, so, _ = wire8.layout(n)
    nblk = -(-n // B)
    return payload[so: so + nblk].to(torch.int32).repeat_interleave(B)[:n]


def check_spec(x: torch.Tensor):
    """Every property of the format that holds for any input."""
    n = x.numel()
    payload, resid = wire8.quantize(x)
    co, so, nbytes = wire8.layout(n)
    assert payload.dtype == torch.uint8 and payload.numel() == nbytes and resid.numel() == n
    deq = wire8.dequantize(payload, n)
    sb = per_element_scale(payload, n)
    finite = sb != 255
    # the identity the error feedback rests on: exact, bit for bit
    back = deq + resid
    assert torch.equal(back[finite].view(torch.int32), x[finite].view(torch.int32))
    bound = half_quantum_bound(x[finite], sb[finite])
    over = resid[finite].double().abs() - bound
    assert float(over.max()) <= 0.0, float(over.max())
    # non-finite blocks: E8M0 NaN, NaN everywhere, nothing kept back
    assert bool(torch.isnan(deq[~finite]).all()) and bool((resid[~finite] == 0).all())
    assert bool((payload[:n][~finite] == 0).all())
    # pad bytes are zero
    nblk = -(-n // B)
    assert bool((payload[n:so] == 0).all()) and bool((payload[so + nblk:] == 0).all())
    return payload, resid, deq, sb


def test_layout():
    assert wire8.layout(0) == (0, 0, 0)
    assert wire8.layout(4) == (0, 16, 20)
    assert wire8.layout(64) == (0, 64, 68)
    assert wire8.layout(65_540) == (0, 65_552, 65_552 + 2052)
    for n in (1, 31, 32, 33, 1000, 65_540, 11_173_962):
        co, so, nb = wire8.layout(n)
        assert co == 0 and so % 16 == 0 and 0 <= so - n < 16
        assert nb % 4 == 0 and 0 <= nb - (so + -(-n // 32)) < 4
    big = 86_567_656
    assert wire8.layout(big)[2] / big < 1.032          # 1.03 B per parameter
    with pytest.raises(ValueError):
        wire8.layout(-1)


def test_crafted_blocks():
    names, x = crafted()
    n = x.numel()
    assert n % B == 4
    payload, resid, deq, sb = check_spec(x)
    at = {k: i * B for i, k in enumerate(names)}
    scale_of = {k: int(sb[at[k]]) for k in names}
    code = payload[:n]

    assert scale_of["zero"] == 0
    assert bool((code[at["zero"]: at["zero"] + B] == 0).all())

    assert scale_of["pow2"] == 124 - 8
    assert int(code[at["pow2"] + 5]) == 0x78 and float(deq[at["pow2"] + 5]) == 0.125   # 256

    s = at["sat"]
    assert scale_of["sat"] == 127 - 8
    q = 2.0 ** -8
    assert code[s: s + 4].tolist() == [0x7E, 0x7E, 0xFE, 0x7E]           # +-448
    assert resid[s: s + 4].tolist() == [1.96875 - 1.75, 0.0, -1.8125 + 1.75,
                                        float(torch.tensor(1.9) - 1.75)]
    band = x[s: s + B].abs() > 448 * q
    assert int(band.sum()) > B // 2
    assert bool((resid[s: s + B][band].abs() < 64 * q).all())
    assert bool(((code[s: s + B][band] & 0x7F) == 0x7E).all())

    t = at["ties"]
    assert scale_of["ties"] == 127
    want = [288.0, 16.0, 20.0, -20.0, 24.0, 0.0, 2.0 ** -8, -2.0 ** -8, 0.015625, 256.0, 1.0, -1.25]
    assert deq[t: t + 12].tolist() == want

    u = at["subnormal"]
    assert scale_of["subnormal"] == 127
    grid = deq[u + 1: u + 10] * 2.0 ** 9
    assert torch.equal(grid, grid.round()) and float(grid.abs().max()) <= 8.0
    assert deq[u + 1: u + 4].tolist() == [2.0 ** -7, 5 * 2.0 ** -9, 2.0 ** -9]    # on the grid
    assert float(deq[u + 6]) == 0.0 and float(resid[u + 6]) == float(torch.tensor(1e-5))

    assert scale_of["tiny"] == 0 and scale_of["huge"] == 254 - 8
    assert scale_of["inf"] == 255 and scale_of["nan"] == 255

    assert wire8.layout(n)[1] - n == 12            # the tail block's codes end mid-way
    assert torch.equal(deq[at["tail4"]:], wire8.dequantize(*_q(x[at["tail4"]:])))


def _q(x):
    return wire8.quantize(x)[0], x.numel()


def test_random_blocks_and_sizes():
    g = torch.Generator().manual_seed(11)
    for n in (4, 64, 100, 65_540):
        nblk = -(-n // B)
        mag = torch.exp2(torch.rand(nblk, generator=g) * 40 - 30).repeat_interleave(B)[:n]
        x = torch.randn(n, generator=g) * mag
        check_spec(x)
    # any shape in, flat out; an empty payload
    p, r = wire8.quantize(torch.ones(3, 5))
    assert r.shape == (15,) and wire8.dequantize(p, 15).tolist() == [1.0] * 15
    p, r = wire8.quantize(torch.zeros(0))
    assert p.numel() == 0 and r.numel() == 0 and wire8.dequantize(p, 0).numel() == 0
    with pytest.raises(ValueError):
        wire8.dequantize(torch.zeros(8, dtype=torch.uint8), 4)


# ------------------------------------------------------------- error feedback
def _mlp():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(8, 16), nn.ReLU(), nn.Linear(16, 4))


def _local_run(push_wire: str, pushes: int):
    from distributed_ml_pytorch_amd.parallel.asgd import Asynchronous
    from distributed_ml_pytorch_amd.parallel.clients import LocalPSClient

    m = _mlp()
    client = LocalPSClient(staleness=0)
    client.request_pull = lambda step: None          # pulls off: the runs share a trajectory
    opt = Asynchronous(m.parameters(), lr=0.05, n_push=1, n_pull=1, model=m, client=client,
                       shadow_dtype=None, push_wire=push_wire)
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
    """master_mx8 + residual == master_fp32 up to fp32 summation rounding: each of
    the T pushes adds one fp32 sum per element on either side (accumulate, apply,
    and the residual carried into the next accumulate), hence 8 T eps32 max|master|."""
    T = 12
    c32, o32 = _local_run("same", T)
    c8, o8 = _local_run("mx8", T)
    assert c32.pushes == c8.pushes == T
    assert torch.equal(o32.arena.p32, o8.arena.p32)          # same local trajectory
    assert float(o32.acc.abs().max()) == 0.0
    assert float(o8.acc.abs().max()) > 0.0                   # the residual is kept
    n = o8.acc.numel()
    assert c8.bytes_sent == T * wire8.layout(n)[2] and c32.bytes_sent == T * 4 * n
    atol = 8 * T * 2.0 ** -23 * float(c32.master.abs().max())
    err = float((c8.master.double() + o8.acc.double() - c32.master.double()).abs().max())
    lost = float((c8.master - c32.master).abs().max())
    print("telescoping err", err, "atol", atol, "master alone is off by", lost)
    assert err <= atol
    assert lost > atol            # without the residual the masters do differ


# ---------------------------------------------------- unsupported flavours
def test_unsupported_flavours_raise_at_start_up():
    from distributed_ml_pytorch_amd.parallel.asgd import Asynchronous
    from distributed_ml_pytorch_amd.parallel.async_sharded import AsyncShardedPSClient
    from distributed_ml_pytorch_amd.parallel.clients import (LocalPSClient, SharedPS,
                                                             SharedPSClient, ShardedPSClient)
    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, Worker

    for make in (lambda: ShardedPSClient(), lambda: SharedPSClient(SharedPS()),
                 lambda: AsyncShardedPSClient(), lambda: ShardedPSClient(push_wire="mx8")):
        m = _mlp()
        with pytest.raises(ValueError, match="LocalPSClient.*GlooPSClient.*RcclPSClient"):
            Asynchronous(m.parameters(), lr=0.1, n_push=1, n_pull=1, model=m, client=make(),
                         shadow_dtype=None, push_wire="mx8")
    with pytest.raises(ValueError, match="'same' or 'mx8'"):
        LocalPSClient(push_wire="fp8")
    info = DistInfo(device=torch.device("cpu"))
    base = dict(model="mlp", cuda=False, push_wire="mx8", verbose=False, evaluate=False)
    for kw in (dict(mode="sync"), dict(mode="single"), dict(mode="asgd", ps="sharded"),
               dict(mode="asgd", ps="sharded_async")):
        with pytest.raises(ValueError, match="--push-wire mx8 is not supported"):
            Worker(TrainConfig(**base, **kw), info)
    # the supported single-process flavour starts
    w = Worker(TrainConfig(**base, mode="asgd", ps="local"), info)
    assert w.opt.client.mx8


def test_cli_flag():
    from distributed_ml_pytorch_amd.cli import build_parser, config_from_args

    assert config_from_args(build_parser().parse_args([])).push_wire == "same"
    assert config_from_args(build_parser().parse_args(["--push-wire", "mx8"])).push_wire == "mx8"


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
                       shadow_dtype=None, push_wire="mx8")
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
            ps = ParameterServer(model=_mlp(), workers=[1, 2], **kw)
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
    nbytes = wire8.layout(n)[2]
    for r in (1, 2):
        w = central[r][name]
        assert w["pushes"] == PUSHES and w["bytes_sent"] / w["pushes"] == nbytes
        assert w["sent"].shape == (PUSHES, nbytes)
        assert float(abs(torch.from_numpy(w["residual"])).max()) > 0
    assert st["counts"]["GradientUpdate"] == 2 * PUSHES == len(log)
    assert st["bytes_in"] == 2 * (4 * n + PUSHES * nbytes)       # the init + the pushes
    # master = init + sum_k scale * f_k * dequant(payload_k), in float64, with the
    # factor the PS logged for each push (a worker's pushes arrive in its own order)
    want = torch.from_numpy(central[1][name]["init"]).double()
    deq = {r: [wire8.dequantize(torch.from_numpy(p), n).double()
               for p in central[r][name]["sent"]] for r in (1, 2)}
    nxt = {1: 0, 2: 0}
    for w, tau, f in log:
        want = want + ps["scale"] * f * deq[w][nxt[w]]
        nxt[w] += 1
    assert nxt == {1: PUSHES, 2: PUSHES}
    got = torch.from_numpy(ps["master"]).double()
    # fp32 rounding: every apply rounds the factor, the product and the sum once
    tol = len(log) * 3 * 2.0 ** -24 * max(1.0, float(want.abs().max()))
    err = float((got - want[: got.numel()]).abs().max())
    print(name, "master err", err, "tol", tol, "damped", st["damped"])
    assert err <= tol
    if name == "damp":
        assert st["damped"] > 0 and any(f != 1.0 for _, _, f in log)
    else:
        assert st["damped"] == 0
