"""Delay compensation (DC-ASGD) on the CPU: parallel/wire.py ``dc_delta`` /
``apply_dc``, the central PS's per-worker backups, configuration and resume.

1. The compensated delta is the first-order Taylor expansion of the fresh one
   (derived bound, no tuning).
2. Degenerate cases: no movement, ``c = 0``, a NaN delta.
3. The central PS over gloo (1 PS + 2 workers): the master replayed bit for bit
   from the server's event log and the workers' recorded payloads.
4. The flag, the coefficient, the refused flavours.
5. Backups are dropped by a checkpoint load.

The specification is written out here (``spec_apply``) independently of the
implementation: seven fp32 operations, each a torch op of its own.
"""
import os
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.nn as nn

from test_dist_cpu import _run

from distributed_ml_pytorch_amd.parallel import wire

N = 65_540
CODECS = {"fp32": wire.FP32, "bf16": wire.BF16, "mx8": wire.MX8}


def f32(x):
    return torch.tensor(x, dtype=torch.float32)


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8),
                                              b.contiguous().view(torch.uint8))


def spec_delta(d, s, bak, c):
    t = s - bak
    q = d * d
    r = q * t
    u = f32(c) * r
    return d - u


def spec_apply(s, bak, d, scale, c, factor=None):
    sc = f32(scale)
    if factor is not None:
        sc = sc * f32(factor)
    p = sc * spec_delta(d, s, bak, c)
    return s + p


def _payload(codec, acc: torch.Tensor) -> torch.Tensor:
    buf = codec.new_payload(acc.numel(), acc.device)
    codec.handoff(acc.clone(), buf)
    return buf


def _seeded(n, seed):
    g = torch.Generator().manual_seed(seed)
    acc = torch.randn(n, generator=g) * torch.exp2(torch.randint(-12, 4, (n,), generator=g))
    master = torch.randn(n, generator=g)
    bak = master + 0.05 * torch.randn(n, generator=g)
    return acc, master, bak


# ------------------------------------------------------- 1. first-order property
@pytest.mark.parametrize("lr", [0.008, 0.05, 1.0])
def test_first_order_property(lr):
    """f(w) = -sum(log w): g = -1/w and H = g^2, so with lambda = 1 (c = 1/lr) the
    compensated delta is the first-order expansion of the fresh delta d* = lr / s.
    With D = s - bak:  |e - d*| = lr D^2 / (bak^2 (bak + D)),  |d - d*| = lr |D| /
    (bak (bak + D)), ratio |D| / bak <= 0.05; the bound 0.1 leaves 2x for fp32."""
    g = torch.Generator().manual_seed(int(lr * 1000))
    bak = (0.5 + 1.5 * torch.rand(N, generator=g, dtype=torch.float64))
    ratio = 0.01 + 0.04 * torch.rand(N, generator=g, dtype=torch.float64)
    sign = torch.where(torch.rand(N, generator=g) < 0.5, -1.0, 1.0).double()
    s = (bak + sign * ratio * bak).float()
    bak = bak.float()
    payload = _payload(wire.FP32, (lr / bak.double()).float())     # d = -lr g(bak), one step
    d = wire.FP32.decode(payload, N)
    e = wire.dc_delta(d, s, bak, 1.0 / lr)
    assert same_bits(e, spec_delta(d, s, bak, 1.0 / lr))
    fresh = lr / s.double()
    err_e = (e.double() - fresh).abs()
    err_d = (d.double() - fresh).abs()
    worst = float((err_e / err_d).max())
    print("lr", lr, "max |e - d*| / |d - d*|", worst)
    assert bool((err_e <= 0.1 * err_d).all()), worst
    # and through the apply: the master moves by the compensated delta
    m = s.clone()
    wire.FP32.apply_dc(m, bak, payload, 1.0, 1.0 / lr)
    assert same_bits(m, s + e)


# ------------------------------------------------------------ 2. degenerate cases
@pytest.mark.parametrize("name", sorted(CODECS))
def test_degenerate_cases(name):
    c = CODECS[name]
    acc, master, bak = _seeded(N, 5)
    payload = _payload(c, acc)
    d = c.decode(payload, N)
    assert bool(d.any())
    # no movement since the pull: nothing to compensate
    assert same_bits(wire.dc_delta(d, master, master.clone(), 37.5), d)
    # c = 0: the plain apply, as two separately rounded operations
    for sc, factor in ((1.0, None), (1 / 3, None), (0.5, 1 / 3)):
        m = master.clone()
        c.apply_dc(m, bak, payload, sc, 0.0, factor=factor)
        k = f32(sc) if factor is None else f32(sc) * f32(factor)
        assert same_bits(m, master + k * d), (sc, factor)
    # the general case against the written-out specification
    m = master.clone()
    c.apply_dc(m, bak, payload, 1 / 3, 2.5, factor=4.0)
    assert same_bits(m, spec_apply(master, bak, d, 1 / 3, 2.5, 4.0))
    assert not torch.equal(m, master + (f32(1 / 3) * f32(4.0)) * d)     # c was used
    # a non-finite delta poisons its element (MX8: its whole block) and no other
    bad = acc.clone()
    bad[77] = float("nan")
    payload = _payload(c, bad)
    m = master.clone()
    c.apply_dc(m, bak, payload, 1.0, 2.5)
    nan = torch.isnan(m)
    assert bool(nan[77])
    want = torch.zeros(N, dtype=torch.bool)
    if name == "mx8":
        want[64:96] = True
    else:
        want[77] = True
    assert torch.equal(nan, want)


def test_fp16_wire_through_decode():
    acc, master, bak = _seeded(64, 2)
    c = wire.codec(torch.float16)
    payload = _payload(c, acc)
    m = master.clone()
    c.apply_dc(m, bak, payload, 0.5, 1.5)
    assert same_bits(m, spec_apply(master, bak, payload.float(), 0.5, 1.5))


# ---------------------------------------------------- 3. central PS over gloo
PUSHES, LR, S, C = 7, 0.05, 1, 20.0          # c = lambda / (lr n_push), lambda = 1
SCENARIOS = {"fp32": dict(kw=dict(delta_scale=0.5), push_wire="same"),
             "mx8": dict(kw=dict(delta_scale="sum"), push_wire="mx8"),
             "damp": dict(kw=dict(stale_policy="damp", stale_bound=S, delta_scale="sum"),
                          push_wire="same")}


def _mlp():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(8, 16), nn.ReLU(), nn.Linear(16, 4))


def _central_worker(rank, push_wire):
    from distributed_ml_pytorch_amd.parallel.asgd import Asynchronous
    from distributed_ml_pytorch_amd.parallel.clients import GlooPSClient

    class Recording(GlooPSClient):
        """Keeps every payload it pushes and every reply it lands."""

        def _handoff(self, n=None):
            buf = super()._handoff(n)
            self.sent.append(buf.clone())
            return buf

        def _land(self, pend):
            pend.work.wait()
            self.landed.append(pend.buf.clone())
            super()._land(pend)

    m = _mlp()
    client = Recording(ps_rank=0, staleness=0)
    client.sent, client.landed = [], []
    # a push every step, a pull every second one: the push right after a pull sees
    # s == bak unless the other worker pushed in between, the one after it sees at
    # least this worker's own previous push
    opt = Asynchronous(m.parameters(), lr=LR, n_push=1, n_pull=2, model=m, client=client,
                       shadow_dtype=None, push_wire=push_wire)
    init = opt.arena.p32.clone()
    g = torch.Generator().manual_seed(100 + rank)
    for _ in range(PUSHES):
        x = torch.randn(16, 8, generator=g)
        y = torch.randn(16, 4, generator=g)
        opt.zero_grad()
        nn.functional.mse_loss(m(x), y).backward()
        opt.step()
    opt.finish()
    return {"n": opt.acc.numel(), "init": init.numpy(),
            "sent": torch.stack(client.sent).numpy(),
            "landed": torch.stack(client.landed).numpy()}


def _central(rank, world):
    from distributed_ml_pytorch_amd.parallel.server import ParameterServer

    out = {}
    for name, sc in SCENARIOS.items():
        dist.barrier()
        if rank == 0:
            ps = ParameterServer(model=_mlp(), workers=[1, 2], delay_comp=C, **sc["kw"])
            st = ps.run()
            out[name] = {"stats": st, "master": ps.parameters().clone().numpy(),
                         "dc_log": list(ps.dc_log), "stale_log": list(ps.gate.log),
                         "scale": ps.delta_scale}
        else:
            out[name] = _central_worker(rank, sc["push_wire"])
    return out


@pytest.fixture(scope="module")
def central():
    return _run(_central, 3)


@pytest.mark.slow
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_central_ps_over_gloo(central, name):
    ps = central[0][name]
    st = ps["stats"]
    n = central[1][name]["n"]
    sent = {r: [torch.from_numpy(p) for p in central[r][name]["sent"]] for r in (1, 2)}
    landed = {r: [torch.from_numpy(p) for p in central[r][name]["landed"]] for r in (1, 2)}
    factors = [f for _, _, f in ps["stale_log"]]
    master = torch.from_numpy(central[1][name]["init"]).clone()
    bak, nxt, seen = {}, {1: 0, 2: 0}, {1: 0, 2: 0}
    moved = pushes = 0
    for ev in ps["dc_log"]:
        if ev[0] == "reply":
            w = ev[1]
            bak[w] = master.clone()
            # the invariant: what the worker landed is its backup, bit for bit
            assert same_bits(landed[w][seen[w]][:n], bak[w]), (name, ev, seen[w])
            seen[w] += 1
            continue
        _, w, compensated = ev
        payload = sent[w][nxt[w]]
        nxt[w] += 1
        f = factors[pushes]
        pushes += 1
        assert compensated == (w in bak)
        if compensated:
            d = wire.codec(payload).decode(payload, n)
            moved += bool((master - bak[w]).any())
            master = spec_apply(master, bak[w], d, ps["scale"], C, f)
        else:
            wire.codec(payload).apply(master, payload, ps["scale"] * f)
    assert nxt == {1: PUSHES, 2: PUSHES} and pushes == 2 * PUSHES == len(factors)
    assert seen == {1: len(landed[1]), 2: len(landed[2])} and min(seen.values()) >= 3
    assert same_bits(torch.from_numpy(ps["master"]), master)
    assert moved >= 1
    assert st["delay_comp"] == C
    assert st["compensated"] == sum(1 for e in ps["dc_log"] if e[0] == "push" and e[2]) > 0
    assert st["compensated"] + st["uncompensated"] == 2 * PUSHES
    if name == "damp":
        assert st["damped"] > 0 and any(f != 1.0 for f in factors)


# ------------------------------------------------------------- 4. configuration
def test_cli_flag_and_coefficient():
    from distributed_ml_pytorch_amd.cli import build_parser, config_from_args
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, delay_comp_coefficient

    assert config_from_args(build_parser().parse_args([])).delay_comp == 0.0
    assert TrainConfig().delay_comp == 0.0
    cfg = config_from_args(build_parser().parse_args(
        ["--delay-comp", "0.04", "--lr", "0.01", "--num-push", "5"]))
    assert cfg.delay_comp == 0.04
    assert delay_comp_coefficient(cfg) == 0.04 / (0.01 * 5)
    assert delay_comp_coefficient(TrainConfig()) == 0.0


def test_refused_combinations():
    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import (TrainConfig, Worker,
                                                            check_delay_comp_config)

    multi = DistInfo(1, 3, 1, "gloo", torch.device("cpu"))
    single = DistInfo(device=torch.device("cpu"))
    lam = dict(delay_comp=0.04)
    check_delay_comp_config(TrainConfig(ps="central", **lam), multi)           # the flavour
    check_delay_comp_config(TrainConfig(ps="central", momentum=0.9, **lam), multi)
    for ps in ("local", "sharded", "sharded_async"):                           # off: anywhere
        check_delay_comp_config(TrainConfig(ps=ps), multi)
    check_delay_comp_config(TrainConfig(mode="sync", optimizer="adamw"), multi)
    for mode in ("sync", "single"):
        with pytest.raises(ValueError, match=f"--mode {mode}"):
            check_delay_comp_config(TrainConfig(mode=mode, **lam), multi)
    for ps in ("local", "sharded", "sharded_async"):
        with pytest.raises(ValueError, match=f"--ps {ps}"):
            check_delay_comp_config(TrainConfig(ps=ps, **lam), multi)
    with pytest.raises(ValueError, match="--ps local"):
        check_delay_comp_config(TrainConfig(ps="central", **lam), single)
    with pytest.raises(ValueError, match="--optimizer adamw"):
        check_delay_comp_config(TrainConfig(ps="central", optimizer="adamw", **lam), multi)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="--delay-comp"):
            check_delay_comp_config(TrainConfig(ps="central", delay_comp=bad), multi)
    # raised at start-up, by the worker itself
    with pytest.raises(ValueError, match="--ps local"):
        Worker(TrainConfig(model="mlp", ps="local", cuda=False, **lam), single)


def test_configurations_start():
    from distributed_ml_pytorch_amd.parallel.clients import SharedPS
    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, check_delay_comp_config
    from distributed_ml_pytorch_amd.runtime.virtual import VirtualWorkers

    cfg = TrainConfig(model="mlp", mode="asgd", ps="central", lr=0.05, n_push=2, n_pull=2,
                      delay_comp=0.04, cuda=False, evaluate=False, verbose=False)
    vw = VirtualWorkers(cfg, 2, device=torch.device("cpu"))
    assert vw.shared.delay_comp == 0.04 / (0.05 * 2)
    w0 = vw.workers[0]
    g = torch.Generator().manual_seed(0)
    for _ in range(6):
        vw.step([w0.prepare(torch.randn(8, *w0.input_shape, generator=g),
                            torch.randint(0, w0.num_classes, (8,), generator=g))
                 for _ in range(2)])
    vw.finish()
    st = vw.ps_stats()
    assert st["compensated"] > 0 and st["compensated"] + st["uncompensated"] == 6
    assert bool(torch.isfinite(vw.master()).all())
    with pytest.raises(ValueError, match="adamw"):
        VirtualWorkers(TrainConfig(model="mlp", optimizer="adamw", delay_comp=0.04, cuda=False),
                       2, device=torch.device("cpu"))
    # the defaults: no backups, the calls of before
    assert SharedPS().delay_comp == 0.0 and SharedPS().bak == {}
    # a central worker's configuration passes the start-up check (no PS contacted)
    check_delay_comp_config(cfg, DistInfo(1, 3, 1, "gloo", torch.device("cpu")))


# ----------------------------------------------------------------- 5. checkpoint
@pytest.fixture
def world1():
    made = not dist.is_initialized()
    if made:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(_free_port())
        dist.init_process_group("gloo", rank=0, world_size=1)
    yield
    if made:
        dist.destroy_process_group()


def _free_port():
    import socket

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_checkpoint_drops_backups(world1, monkeypatch):
    from distributed_ml_pytorch_amd.parallel import messaging as M
    from distributed_ml_pytorch_amd.parallel.server import ParameterServer

    n = 64
    ps = ParameterServer(numel=n, workers=[1, 2], delay_comp=2.0)
    g = torch.Generator().manual_seed(0)
    inbox = []
    sent = []

    def recv(buf, src=None, group=None, tag=0):
        buf.copy_(inbox.pop(0))

    class Done:
        def wait(self):
            pass

        def is_completed(self):
            return True

    def isend(buf, dst, group=None, tag=0):
        sent.append((dst, buf.clone()))
        return Done()

    monkeypatch.setattr(dist, "recv", recv)
    monkeypatch.setattr(dist, "isend", isend)

    def push(w):
        inbox.append(torch.randn(n, generator=g) * 0.1)
        ps.handle(M.MessageCode.GradientUpdate, w, 0, ps.version, n, torch.float32)

    def request(w):
        ps.handle(M.MessageCode.ParameterRequest, w, 0, 0, 0, torch.float32)

    push(1)                      # no reply yet
    request(1), request(2)
    push(1), push(2)
    assert [e for e in ps.dc_log if e[0] == "push"] == [("push", 1, False), ("push", 1, True),
                                                        ("push", 2, True)]
    # every reply carried the backup of the time, and the stamp
    assert [d for d, _ in sent] == [1, 2]
    assert same_bits(sent[1][1][:n], ps._backup(2)[:n]) and float(sent[1][1][n]) == 1.0
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "ps.pt")
        ps.save_checkpoint(path)
        ps.load_checkpoint(path)
    assert ps.has_backup == {1: False, 2: False}
    mark = len(ps.dc_log)
    push(1), push(2)
    request(1)
    push(1), push(2)
    assert ps.dc_log[mark:] == [("push", 1, False), ("push", 2, False), ("reply", 1),
                                ("push", 1, True), ("push", 2, False)]
    st = ps.stats()
    assert (st["compensated"], st["uncompensated"]) == (3, 4)
