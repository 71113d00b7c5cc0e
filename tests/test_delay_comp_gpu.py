"""Delay compensation on the device: the ``ps_apply_dc`` / ``ps_snapshot`` kernels
against the CPU codec bit for bit, then the central PS (device links, through
``ParameterServer.handle`` with a delayed-copy transport of the stream semantics
of tests/test_staleness_gpu.py), the shared PS of the virtual workers, and what
the bindings refuse.

Sizes: 64 (the smallest arena) and 65,540 (several blocks, the grid-stride tail,
n % 32 == 4: a short last MX8 block).  The specification is written out here
(``spec_apply``), independently of parallel/wire.py.
"""
import os
import socket
from collections import defaultdict, deque

import pytest
import torch
import torch.distributed as dist

from distributed_ml_pytorch_amd.parallel import wire

pytestmark = pytest.mark.gpu

N = 65_540
C = 0.3                      # not a power of two: c * r rounds
CODECS = {"fp32": wire.FP32, "bf16": wire.BF16, "mx8": wire.MX8}


def _native():
    from distributed_ml_pytorch_amd.ops._ext import native

    return native()


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


def _seeded(n, seed=None):
    """CPU-seeded accumulator (magnitudes over many binades: MX8 blocks of different
    scales), master and backup."""
    g = torch.Generator().manual_seed(n if seed is None else seed)
    acc = torch.randn(n, generator=g) * torch.exp2(torch.randint(-12, 4, (n,), generator=g))
    master = torch.randn(n, generator=g)
    bak = master + 0.05 * torch.randn(n, generator=g) * \
        torch.exp2(torch.randint(-6, 2, (n,), generator=g))
    return acc, master, bak


def _payload(codec, acc):
    buf = codec.new_payload(acc.numel(), acc.device)
    codec.handoff(acc.clone(), buf)
    return buf


def _apply_native(nat, name, *a):
    return (nat.ps_apply_dc_mx8 if name == "mx8" else nat.ps_apply_dc)(*a)


# ---------------------------------- 6. the kernels against the CPU codec, bit for bit
@pytest.fixture(scope="module")
def cpu_cases():
    """Inputs and CPU payloads, once per (wire, n)."""
    out = {}
    for name, c in CODECS.items():
        for n in (64, N):
            acc, master, bak = _seeded(n)
            out[name, n] = (_payload(c, acc), master, bak)
    return out


@pytest.mark.parametrize("factor", [None, 1 / 3, 4.0], ids=["nofactor", "f1_3", "f4"])
@pytest.mark.parametrize("sc", [1.0, 0.5, 1 / 3], ids=["1", "0.5", "1_3"])
@pytest.mark.parametrize("n", [64, N])
@pytest.mark.parametrize("name", sorted(CODECS))
def test_dc_apply_matches_cpu_codec(cpu_cases, name, n, sc, factor):
    nat = _native()
    c = CODECS[name]
    payload, master0, bak = cpu_cases[name, n]
    ref = master0.clone()
    c.apply_dc(ref, bak, payload, sc, C, factor=factor)
    # the codec's CPU form is the written-out specification
    assert same_bits(ref, spec_apply(master0, bak, c.decode(payload, n), sc, C, factor))
    assert not torch.equal(ref, master0)
    slot = None if factor is None else torch.tensor([factor, 2.0], device="cuda")
    pg, bg = payload.cuda(), bak.cuda()
    plain, mirror = master0.cuda(), torch.empty(n, dtype=torch.bfloat16, device="cuda")
    _apply_native(nat, name, plain, pg, bg, mirror, sc, C, False, slot)
    atomic = master0.cuda()
    _apply_native(nat, name, atomic, pg, bg, None, sc, C, True, slot)
    assert same_bits(plain.cpu(), ref)
    assert same_bits(mirror.cpu(), ref.to(torch.bfloat16))
    assert same_bits(atomic.cpu(), ref)            # one stream: the same bits
    assert same_bits(bg.cpu(), bak) and same_bits(pg.cpu(), payload)
    # and through the codec's own GPU path
    via = master0.cuda()
    c.apply_dc(via, bg, pg, sc, C, atomic=False, factor=slot)
    assert same_bits(via.cpu(), ref)


# ------------------------------------------------------------ 7. bak == shard
@pytest.mark.parametrize("atomic", [False, True], ids=["plain", "atomic"])
@pytest.mark.parametrize("sc", [1.0, 0.5])
@pytest.mark.parametrize("n", [64, N])
@pytest.mark.parametrize("name", sorted(CODECS))
def test_no_movement_is_the_existing_apply(cpu_cases, name, n, sc, atomic):
    """s == bak: e == d, and sc * d is exact for sc = 1, 0.5, so the existing
    apply's one rounding (fp32 / bf16 wire) or two give the same bits."""
    nat = _native()
    payload, master0, _ = cpu_cases[name, n]
    pg = payload.cuda()
    old, new = master0.cuda(), master0.cuda()
    (nat.ps_apply_mx8 if name == "mx8" else nat.ps_apply)(old, pg, None, sc, atomic)
    _apply_native(nat, name, new, pg, master0.cuda(), None, sc, C, atomic, None)
    assert same_bits(new.cpu(), old.cpu())
    assert not torch.equal(old.cpu(), master0)


# -------------------------------------------------------------- 8. ps_snapshot
@pytest.mark.parametrize("outs", range(1, 8))
@pytest.mark.parametrize("n", [64, N])
def test_ps_snapshot(n, outs):
    nat = _native()
    _, master0, _ = _seeded(n)
    shard = master0.cuda()
    o32 = torch.zeros(n, device="cuda") if outs & 1 else None
    o16 = torch.zeros(n, dtype=torch.bfloat16, device="cuda") if outs & 2 else None
    bak = torch.zeros(n, device="cuda") if outs & 4 else None
    nat.ps_snapshot(shard, o32, o16, bak)
    if o32 is not None:
        assert same_bits(o32.cpu(), master0)
    if o16 is not None:
        assert same_bits(o16.cpu(), master0.to(torch.bfloat16))
    if bak is not None:
        assert same_bits(bak.cpu(), master0)
    assert same_bits(shard.cpu(), master0)


# ------------------------------------------------------- the delayed-copy transport
class _EvWork:
    def __init__(self, ev):
        self.ev = ev

    def wait(self):
        torch.cuda.current_stream().wait_event(self.ev)

    def is_completed(self):
        return self.ev.query()


class DelayedCopyTransport:
    def __init__(self, cycles: dict):
        self.cycles = cycles                # {peer: wire time in device clock cycles}
        self.outbox = defaultdict(deque)    # peer -> tensors the peer "sends" to us
        self.inbox = defaultdict(list)      # peer -> tensors we sent to the peer
        self.comm = {p: torch.cuda.Stream() for p in cycles}
        for cs in self.comm.values():       # first use now, not in a transfer
            with torch.cuda.stream(cs):
                torch.cuda._sleep(1000)

    def _op(self, peer, fn):
        cs = self.comm[peer]
        cs.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(cs):
            torch.cuda._sleep(self.cycles[peer])
            fn()
            b = torch.cuda.Event()
            b.record()
        return _EvWork(b)

    def irecv(self, buf, peer):
        src = self.outbox[peer].popleft()
        return self._op(peer, lambda: buf.copy_(src))

    def isend(self, buf, peer):
        out = torch.empty_like(buf)
        self.inbox[peer].append(out)
        return self._op(peer, lambda: out.copy_(buf))


@pytest.fixture(scope="module")
def world1():
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


def _server(policy, deltas, scale=0.5):
    from distributed_ml_pytorch_amd.parallel.server import ParameterServer

    tr = DelayedCopyTransport({1: 200_000, 2: 100_000})
    for w, ds in deltas.items():
        tr.outbox[w].extend(d.cuda() for d in ds)
    ps = ParameterServer(numel=N, workers=[1, 2], payload="rccl", device="cuda:0", transport=tr,
                         delta_scale=scale, stale_policy=policy, stale_bound=0, delay_comp=C)
    _, master0, _ = _seeded(N, 11)
    ps.shard.copy_(master0)
    torch.cuda.synchronize()
    return ps, tr, master0


# --------------------------------------------------------- 9. the device-link PS
@pytest.mark.parametrize("policy", ["off", "damp"])
def test_device_link_ps_replays_bit_for_bit(world1, policy):
    from distributed_ml_pytorch_amd.parallel import messaging as M

    g = torch.Generator().manual_seed(9)
    deltas = {w: [torch.randn(N, generator=g) * 0.05 for _ in range(2)] for w in (1, 2)}
    ps, tr, master0 = _server(policy, deltas)
    # (kind, worker, base version of a push = the stamp of the worker's last reply)
    script = [("req", 1, 0), ("req", 2, 0), ("push", 1, 0), ("push", 2, 0), ("req", 1, 0),
              ("push", 2, 0), ("push", 1, 2)]
    for step, (kind, w, base) in enumerate(script):
        if kind == "req":
            ps.handle(M.MessageCode.ParameterRequest, w, step, 0, 0, torch.float32)
        else:
            ps.handle(M.MessageCode.GradientUpdate, w, step, base, N, torch.float32)
        ps._sync_device()            # the apply order is the handled order
        torch.cuda.synchronize()
    ps.finish()
    assert ps.dc_log == [("reply", 1), ("reply", 2), ("push", 1, True), ("push", 2, True),
                         ("reply", 1), ("push", 2, True), ("push", 1, True)]
    if policy == "damp":
        entries = ps.stale_log()["entries"]
        # S = 0: tau = 0, 1, 2, 1 -> 1, 1/2, 1/3, 1/2 (one correctly rounded division)
        assert [t for t, _ in entries] == [0, 1, 2, 1]
        factors = [f for _, f in entries]
        assert factors == [1.0, 0.5, float(f32(1.0) / f32(3.0)), 0.5]
    else:
        factors = [None] * 4
    master, bak = master0.clone(), {}
    nxt, replies, applied, moved = {1: 0, 2: 0}, {1: 0, 2: 0}, 0, []
    for ev in ps.dc_log:
        w = ev[1]
        if ev[0] == "reply":
            bak[w] = master.clone()
            reply = tr.inbox[w][replies[w]].cpu()
            replies[w] += 1
            assert same_bits(reply[:N], bak[w]), ev
            assert float(reply[N]) == float(applied), ev
        else:
            moved.append(bool((master - bak[w]).any()))
            master = spec_apply(master, bak[w], deltas[w][nxt[w]], 0.5, C, factors[applied])
            nxt[w] += 1
            applied += 1
    assert moved == [False, True, True, True]     # the first push: D = 0, still compensated
    assert same_bits(ps.parameters().cpu(), master)
    st = ps.stats()
    assert (st["compensated"], st["uncompensated"]) == (4, 0)
    assert st["delay_comp"] == C and st["applied"] == 4 and st["version"] == 4


# ---------------------------------------------------------- 10. concurrent links
def test_concurrent_links_land_on_a_candidate(world1):
    """Both workers hold the same snapshot s0 and push at the same time on their own
    link streams.  Per element the master is, up to the order of two atomic adds
    (4 ulp of the largest candidate), one of: 1 before 2, 2 before 1, neither saw
    the other.  Which one is not asserted."""
    from distributed_ml_pytorch_amd.parallel import messaging as M

    g = torch.Generator().manual_seed(10)
    deltas = {w: [torch.randn(N, generator=g) * 0.05] for w in (1, 2)}
    ps, tr, s0 = _server("off", deltas, scale=1.0)
    for w in (1, 2):
        ps.handle(M.MessageCode.ParameterRequest, w, 0, 0, 0, torch.float32)
    ps._sync_device()
    torch.cuda.synchronize()
    for w in (1, 2):
        ps.handle(M.MessageCode.GradientUpdate, w, 1, 0, N, torch.float32)
    ps.finish()
    got = ps.parameters().cpu()
    d1, d2 = deltas[1][0], deltas[2][0]
    p1 = f32(1.0) * spec_delta(d1, s0, s0, C)        # what each adds when it reads s0
    p2 = f32(1.0) * spec_delta(d2, s0, s0, C)
    cands = torch.stack([spec_apply(s0 + p1, s0, d2, 1.0, C),      # 1 before 2
                         spec_apply(s0 + p2, s0, d1, 1.0, C),      # 2 before 1
                         (s0 + p1) + p2])                          # neither sees the other
    top = cands.abs().max(0).values.clamp_min(2.0 ** -100)
    ulp = torch.exp2((torch.frexp(top).exponent - 24).float())
    dist_ulp = ((cands.double() - got.double()).abs() / ulp.double()).min(0).values
    print("concurrent links: worst distance to a candidate", float(dist_ulp.max()), "ulp")
    assert bool((dist_ulp <= 4).all()), float(dist_ulp.max())
    assert ps.stats()["compensated"] == 2


# ------------------------------------------------------- 11. SharedPS on the GPU
@pytest.mark.parametrize("wire_dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_shared_ps_matches_cpu(wire_dtype):
    from distributed_ml_pytorch_amd.parallel.clients import SharedPS

    g = torch.Generator().manual_seed(12)
    _, master0, _ = _seeded(N, 12)
    deltas = [torch.randn(N, generator=g) * 0.05 for _ in range(4)]
    script = [("snap", 0), ("snap", 1), ("apply", 0), ("apply", 1), ("snap", 0), ("apply", 1),
              ("apply", 0)]

    def run(device):
        ps = SharedPS(delay_comp=C)
        assert ps.adopt_or_set(master0.to(device))
        snaps, k = [], 0
        for kind, w in script:
            if kind == "snap":
                buf, ev = ps.snapshot(wire_dtype, worker=w)
                if ev is not None:
                    ev.synchronize()
                snaps.append(buf.cpu())
                assert same_bits(ps.bak[w].cpu().to(wire_dtype), snaps[-1])
            else:
                ps.apply(deltas[k].to(device), worker=w)
                k += 1
        if device == "cuda":
            torch.cuda.synchronize()
        return snaps, ps.master.cpu(), ps.stats()

    snaps_g, master_g, st_g = run("cuda")
    snaps_c, master_c, st_c = run("cpu")
    assert len(snaps_g) == 3 and all(same_bits(a, b) for a, b in zip(snaps_g, snaps_c))
    assert same_bits(master_g, master_c)
    assert st_g == st_c and st_g["compensated"] == 4 and st_g["uncompensated"] == 0


def test_virtual_workers_with_delay_comp():
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig
    from distributed_ml_pytorch_amd.runtime.virtual import VirtualWorkers
    from distributed_ml_pytorch_amd.utils.data import DeviceBatchPool

    device = torch.device("cuda", 0)
    k, steps, batch = 2, 20, 32
    cfg = TrainConfig(model="mlp", batch_size=batch, mode="asgd", lr=0.05, n_push=2, n_pull=2,
                      delay_comp=0.04, cuda=True, evaluate=False, verbose=False)
    vw = VirtualWorkers(cfg, k, device=device)
    assert vw.shared.delay_comp == 0.04 / (0.05 * 2)
    assert vw.enable_graph(True)
    w0 = vw.workers[0]
    pools = [DeviceBatchPool(batch, w0.input_shape, w0.num_classes, device, n_batches=2,
                             dtype=w0.compute_dtype, seed=i, learnable=True, signal=1.0,
                             channels_last=True) for i in range(k)]
    losses = []
    for _ in range(steps):
        losses.append([float(l.float()) for l in vw.step([p.next() for p in pools])])
    vw.finish()
    torch.cuda.synchronize()
    assert all(x == x and abs(x) != float("inf") for row in losses for x in row), losses
    assert all(w.use_graph and w.graph is not None for w in vw.workers)    # capture held
    st = vw.ps_stats()
    assert st["compensated"] > 0
    assert st["compensated"] + st["uncompensated"] == k * steps // 2 == st["version"]
    assert bool(torch.isfinite(vw.master()).all())


# ------------------------------------------------------------ 12. bindings reject
def test_bindings_reject():
    nat = _native()
    n = 64
    shard = torch.zeros(n, device="cuda")
    delta = torch.zeros(n, device="cuda")
    bak = torch.zeros(n, device="cuda")
    mx8 = torch.zeros(nat.mx8_layout(n)[2], dtype=torch.uint8, device="cuda")
    nat.ps_apply_dc(shard, delta, bak, None, 1.0, C, False, None)        # the good call
    nat.ps_apply_dc(shard, delta, torch.zeros(n + 4, device="cuda"), None, 1.0, C)   # bak >= n
    for fn, payload in ((nat.ps_apply_dc, delta), (nat.ps_apply_dc_mx8, mx8)):
        bad_baks = {"dtype": torch.zeros(n, dtype=torch.bfloat16, device="cuda"),
                    "length": torch.zeros(n - 4, device="cuda"),
                    "device": torch.zeros(n),
                    "alias": shard}
        for why, b in bad_baks.items():
            with pytest.raises(RuntimeError, match="bak"):
                fn(shard, payload, b, None, 1.0, C, False, None)
        for bad_c in (-1.0, float("nan"), float("inf")):
            with pytest.raises(RuntimeError, match="coefficient"):
                fn(shard, payload, bak, None, 1.0, bad_c, False, None)
        with pytest.raises(RuntimeError, match="mirror"):
            fn(shard, payload, bak, torch.zeros(n, dtype=torch.bfloat16, device="cuda"), 1.0, C,
               True, None)
    with pytest.raises(RuntimeError, match="no output"):
        nat.ps_snapshot(shard, None, None, None)
    with pytest.raises(RuntimeError):
        nat.ps_snapshot(shard, torch.zeros(n, dtype=torch.bfloat16, device="cuda"), None, None)
    with pytest.raises(RuntimeError):
        nat.ps_snapshot(shard, None, torch.zeros(n, device="cuda"), None)
    with pytest.raises(RuntimeError):
        nat.ps_snapshot(shard, None, None, torch.zeros(n - 4, device="cuda"))
    with pytest.raises(RuntimeError, match="alias"):
        nat.ps_snapshot(shard, None, None, shard)
    with pytest.raises(RuntimeError):
        nat.ps_snapshot(shard, torch.zeros(n), None, None)
    torch.cuda.synchronize()
    assert not bool(shard.any())
