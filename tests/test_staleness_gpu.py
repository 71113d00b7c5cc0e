"""Staleness bound on the device path (parallel/staleness.py, csrc/optim.hip).

``ps_stale_factor`` and the factor-aware ``ps_apply`` on their own, then the
central PS driven through ``ParameterServer.handle`` with a delayed-copy
transport of the same stream semantics as tests/test_links_gpu.py (RCCL refuses
two ranks on one device): every peer has its own "comm" stream, an operation
makes it wait on the caller's current stream, ``torch.cuda._sleep`` stands in
for the wire time, a device copy moves the bytes, ``work.wait()`` makes the
caller's current stream wait for the copy.

Sizes: 65,540 elements (a multiple of 4, not of the 256-thread block: the
grid-stride tails run); only the two-link timing scenario uses 1 << 20.
"""
import json
import os
import socket
import subprocess
import sys
from collections import defaultdict, deque

import pytest
import torch
import torch.distributed as dist

pytestmark = pytest.mark.gpu

N = 65_540


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
        self.spans = []

    def _op(self, peer, kind, fn):
        cs = self.comm[peer]
        cs.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(cs):
            a = torch.cuda.Event(enable_timing=True)
            a.record()
            torch.cuda._sleep(self.cycles[peer])
            fn()
            b = torch.cuda.Event(enable_timing=True)
            b.record()
        self.spans.append((kind, peer, a, b))
        return _EvWork(b)

    def irecv(self, buf, peer):
        src = self.outbox[peer].popleft()
        return self._op(peer, "recv", lambda: buf.copy_(src))

    def isend(self, buf, peer):
        out = torch.empty_like(buf)
        self.inbox[peer].append(out)
        return self._op(peer, "send", lambda: out.copy_(buf))


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


def _native():
    from distributed_ml_pytorch_amd.ops._ext import native

    return native()


def _f32(x: float) -> float:
    return float(torch.tensor(x, dtype=torch.float32))


def _factor(tau: int, s: int) -> float:
    """f(tau) as one correctly rounded fp32 division, which is what the kernel does."""
    one = torch.ones((), dtype=torch.float32)
    return 1.0 if tau <= s else float(one / torch.tensor(float(1 + tau - s), dtype=torch.float32))


# ------------------------------------------------------------ 4. the kernel alone
def test_ps_stale_factor_kernel():
    from distributed_ml_pytorch_amd.parallel.links import AppliedCount
    from distributed_ml_pytorch_amd.parallel.staleness import DeviceStaleLog

    nat = _native()
    dev = torch.device("cuda", 0)
    s = 2
    applied = AppliedCount(dev, nat)
    log = DeviceStaleLog(dev, nat, applied, s)
    # (count, base): tau = 0, S, S + 1, S + 5 at base 0, the same above a base of 7,
    # and a count below the base (tau clamps to 0)
    cases = [(0, 0), (s, 0), (s + 1, 0), (s + 5, 0), (7 + s + 1, 7), (3, 7), (0, 1)]
    want = []
    for cnt, base in cases:
        applied.set(cnt)
        slot = log.factor("a", base)
        tau = max(0, cnt - base)
        got = slot.tolist()
        assert got == [_factor(tau, s), float(tau)], (cnt, base, got)
        want.append((tau, _factor(tau, s)))
    assert [w[0] for w in want] == [0, s, s + 1, s + 5, s + 1, 0, 0]
    r = log.read()
    assert r["count"] == len(cases)
    assert r["entries"] == want
    assert r["tau_max"] == s + 5
    assert r["damped"] == 3 == sum(1 for t, _ in want if t > s)
    # the ring wraps at 1024 entries: the newest 1024, in apply order
    for k in range(1030 - len(cases)):
        applied.set(k % 7)
        log.factor("a", 0)
        want.append((k % 7, _factor(k % 7, s)))
    assert applied.value() == (1030 - len(cases) - 1) % 7     # the count is only read
    r = log.read()
    assert r["count"] == 1030 and len(r["entries"]) == 1024
    assert r["entries"] == want[-1024:]
    assert r["tau_max"] == s + 5
    with pytest.raises(RuntimeError):
        nat.ps_stale_factor(applied.dev, 0, -1, log.slot("a"), log.log)
    # the clamp: the count is taken as at most `cap` (the host's enqueue count)
    applied.set(9)
    assert log.factor("a", 0, cap=4).tolist() == [_factor(4, s), 4.0]
    assert log.factor("a", 3, cap=4).tolist() == [1.0, 1.0]
    assert log.factor("a", 6, cap=4).tolist() == [1.0, 0.0]         # cap below the base
    assert log.factor("a", 0, cap=20).tolist() == [_factor(9, s), 9.0]
    assert log.factor("a", 0).tolist() == [_factor(9, s), 9.0]


# ----------------------------------------------------- 5. the factor-aware apply
@pytest.mark.parametrize("atomic", [False, True], ids=["plain", "atomic"])
@pytest.mark.parametrize("wire", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_factor_aware_apply(wire, atomic):
    nat = _native()
    g = torch.Generator(device="cuda").manual_seed(3)
    shard0 = torch.randn(N, device="cuda", generator=g)
    delta = torch.randn(N, device="cuda", generator=g).to(wire)
    scale = 0.5

    def run(factor):
        out = shard0.clone()
        mirror = None if atomic else torch.empty(N, device="cuda", dtype=torch.bfloat16)
        if factor is None:
            nat.ps_apply(out, delta, mirror, scale, atomic)
        else:
            nat.ps_apply(out, delta, mirror, scale, atomic, factor)
        return out, mirror

    base, base_m = run(None)
    # factor 1: bit-identical to the call without a factor pointer (one stream, so
    # the atomic order is fixed too)
    one, one_m = run(torch.tensor([1.0, 0.0], device="cuda"))
    assert torch.equal(one, base)
    if not atomic:
        assert torch.equal(one_m.view(torch.int16), base_m.view(torch.int16))
    # factor 1/3 against float64; fp32 rounding of one multiply-add
    slot = torch.tensor([1.0 / 3.0, 4.0], device="cuda")
    third, third_m = run(slot)
    want = shard0.double() + scale * slot[0].double() * delta.double()
    err = float((third.double() - want).abs().max())
    bound = 1e-6 * float(want.abs().max())
    print(wire, atomic, "err", err, "bound", bound)
    assert err <= bound
    assert float((third - base).abs().max()) > 0.1      # the factor was used
    if not atomic:
        assert torch.equal(third_m.view(torch.int16),
                           third.to(torch.bfloat16).view(torch.int16))


# ------------------------------------------------------- 6. one link, six pushes
def _handle_pushes(ps, order, n):
    from distributed_ml_pytorch_amd.parallel import messaging as M

    for step, (w, base) in enumerate(order):
        ps.handle(M.MessageCode.GradientUpdate, w, step, base, n, torch.float32)


def test_one_link_six_pushes_damped(world1):
    from distributed_ml_pytorch_amd.parallel.server import ParameterServer

    s = 2
    tr = DelayedCopyTransport({1: 200_000})
    g = torch.Generator(device="cuda").manual_seed(1)
    deltas = [torch.randn(N, device="cuda", generator=g) for _ in range(6)]
    tr.outbox[1].extend(deltas)
    ps = ParameterServer(numel=N, workers=[1], payload="rccl", device="cuda:0", transport=tr,
                         stale_bound=s, stale_policy="damp")
    _handle_pushes(ps, [(1, 0)] * 6, N)        # every push carries base version 0
    ps.finish()
    log = ps.stale_log()
    facs = [1.0, 1.0, 1.0, _f32(1 / 2), _f32(1 / 3), _f32(1 / 4)]
    assert log["count"] == 6
    assert log["entries"] == list(zip(range(6), facs)), log["entries"]
    assert log["tau_max"] == 5 and log["damped"] == 3
    want = sum(f * d.double() for f, d in zip(facs, deltas))
    err = float((ps.parameters().double() - want).abs().max())
    print("six pushes err", err)
    assert err < 5e-5        # six fp32 accumulations of values of order 10
    st = ps.stats()
    assert st["staleness_max_landed"] == 5 and st["damped"] == 3
    assert st["staleness_max"] == 5 and st["applied"] == 6 and st["version"] == 6
    assert st["stale_policy"] == "damp" and st["stale_bound"] == s


# --------------------------------------------- 7. two links, one 5x slower (damp)
def _uneven_scenario():
    """In a process of its own (16 hardware queues, as tests/test_links_gpu.py: at
    HIP's default of 4 the two comm streams can share a queue and run back to back)."""
    from distributed_ml_pytorch_amd.parallel.server import ParameterServer

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        n, s = 1 << 20, 0
        tr = DelayedCopyTransport({1: 50_000_000, 2: 10_000_000})
        g = torch.Generator(device="cuda").manual_seed(0)
        deltas = {w: [torch.randn(n, device="cuda", generator=g) for _ in range(2)]
                  for w in (1, 2)}
        for w in (1, 2):
            tr.outbox[w].extend(deltas[w])
        ps = ParameterServer(numel=n, workers=[1, 2], payload="rccl", device="cuda:0",
                             transport=tr, stale_bound=s, stale_policy="damp")
        torch.cuda.synchronize()
        order = [(1, 0), (2, 0), (1, 1), (2, 1)]
        _handle_pushes(ps, order, n)
        host_tau = list(ps.staleness)          # the host's version - base, per push
        ps.finish()
        torch.cuda.synchronize()
        log = ps.stale_log()
        # each apply runs on its link stream right behind its receive, and the wire
        # times are milliseconds apart: the applies ran in the order the receives ended
        recvs = [(p, a, b) for k, p, a, b in tr.spans if k == "recv"]
        t0 = recvs[0][1]
        ends = [t0.elapsed_time(b) for _, _, b in recvs]
        ran = sorted(range(4), key=lambda i: ends[i])      # push index, in apply order
        want = torch.zeros(n, dtype=torch.float64, device="cuda")
        seen = {1: 0, 2: 0}
        per_push = []
        for (tau, f), i in zip(log["entries"], ran):
            w = order[i][0]
            want += f * deltas[w][seen[w]].double()
            seen[w] += 1
            per_push.append({"push": i, "worker": w, "base": order[i][1], "tau_dev": tau,
                             "factor": f, "tau_host": host_tau[i],
                             "recv_end_ms": round(ends[i], 3)})
        st = ps.stats()
        return {"per_push": per_push, "count": log["count"], "tau_max": log["tau_max"],
                "damped": log["damped"],
                "master_err": float((ps.parameters().double() - want).abs().max()),
                "stats": {k: st[k] for k in ("staleness_max_landed", "damped", "staleness_max",
                                             "version", "applied", "clock_drift_max")}}
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def uneven():
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16", DMP_STALENESS_SCENARIO="uneven")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True,
                       text=True, timeout=100, env=env, cwd=root)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    print(out)
    return out


def test_two_links_master_is_the_factor_weighted_sum(uneven):
    r = uneven
    assert r["count"] == 4 and r["stats"]["version"] == 4 and r["stats"]["applied"] == 4
    # worker 2's applies did not wait for worker 1's slow payloads
    assert [p["worker"] for p in r["per_push"]] == [2, 2, 1, 1], r
    for p in r["per_push"]:
        tau = p["tau_dev"]
        assert p["factor"] == (1.0 if tau == 0 else _f32(1.0 / (1 + tau))), p
        # never more than the host has enqueued in all on top of the push's base
        assert tau <= r["stats"]["version"] - p["base"], p
    assert r["master_err"] < 1e-4, r
    assert r["stats"]["staleness_max_landed"] == r["tau_max"] == \
        max(p["tau_dev"] for p in r["per_push"])
    assert r["stats"]["damped"] == r["damped"] == sum(1 for p in r["per_push"] if p["tau_dev"] > 0)


def test_two_links_device_tau_is_at_most_the_hosts(uneven):
    """Every logged device tau is at most the host's ``version - base`` of that push.

    The host logs ``version - base`` when the HEADER is handled (all four within
    microseconds, interleaved 1, 2, 1, 2); ``ps_stale_factor`` reads the landed
    count when the APPLY runs, behind its receive.  Worker 1's wire is 5x slower,
    so both of its applies run after both of worker 2's have landed (the raw
    device count then reads 2 and 3 for pushes the host saw at 0 and 2).  The
    kernel clamps the count to the host's enqueue count at the push's arrival:
    pushes the server ordered BEHIND this one do not count against it."""
    for p in uneven["per_push"]:
        print(p)
    for p in uneven["per_push"]:
        assert p["tau_dev"] <= p["tau_host"], uneven["per_push"]


# ----------------------------------------------------- 8. block on the device path
def test_block_defers_the_reply_on_the_device_path(world1):
    from distributed_ml_pytorch_amd.parallel import messaging as M
    from distributed_ml_pytorch_amd.parallel.server import ParameterServer

    tr = DelayedCopyTransport({1: 200_000, 2: 200_000})
    g = torch.Generator(device="cuda").manual_seed(2)
    d1 = [torch.randn(N, device="cuda", generator=g) for _ in range(3)]
    d2 = [torch.randn(N, device="cuda", generator=g) for _ in range(2)]
    tr.outbox[1].extend(d1)
    tr.outbox[2].extend(d2)
    ps = ParameterServer(numel=N, workers=[1, 2], payload="rccl", device="cuda:0", transport=tr,
                         stale_bound=1, stale_policy="block")
    _handle_pushes(ps, [(1, 0), (1, 1), (1, 2)], N)
    ps.handle(M.MessageCode.ParameterRequest, 1, 3, 0, 0, torch.float32)
    assert ps.links.counts["send"] == 0 and ps.gate.waiting(1)      # 3 ahead of worker 2
    _handle_pushes(ps, [(2, 0)], N)
    assert ps.links.counts["send"] == 0                             # still 2 ahead
    _handle_pushes(ps, [(2, 1)], N)
    assert ps.links.counts["send"] == 1 and not ps.gate.waiting(1)
    ps.finish()
    assert ps.links.counts["send"] == 1                             # nothing left to drain
    reply = tr.inbox[1][-1]
    assert float(reply[N]) >= 3.0
    own = d1[0] + d1[1] + d1[2]
    cands = [own, own + d2[0], own + d2[0] + d2[1]]      # per element: a prefix of worker 2's
    err = float(torch.stack([(reply[:N] - c).abs() for c in cands]).min(0).values.max())
    assert err < 1e-4
    st = ps.stats()
    assert st["deferred"] == {1: 1, 2: 0} and st["clock_drift_max"] == 3
    assert st["staleness_max_landed"] is None and st["damped"] == 0
    assert float((ps.parameters() - cands[2]).abs().max()) < 1e-4


def test_finish_answers_a_deferred_request(world1):
    from distributed_ml_pytorch_amd.parallel import messaging as M
    from distributed_ml_pytorch_amd.parallel.server import ParameterServer

    tr = DelayedCopyTransport({1: 100_000, 2: 100_000})
    tr.outbox[1].extend(torch.ones(N, device="cuda") for _ in range(2))
    ps = ParameterServer(numel=N, workers=[1, 2], payload="rccl", device="cuda:0", transport=tr,
                         stale_bound=0, stale_policy="block")
    _handle_pushes(ps, [(1, 0), (1, 1)], N)
    ps.handle(M.MessageCode.ParameterRequest, 1, 2, 0, 0, torch.float32)
    assert ps.links.counts["send"] == 0
    ps.finish()                                   # no worker is left hanging at shutdown
    assert ps.links.counts["send"] == 1
    assert float(tr.inbox[1][-1][N]) == 2.0


# ------------------------------------------- the co-located shard server (damp)
def test_shard_server_local_apply_is_damped():
    from distributed_ml_pytorch_amd.parallel.async_sharded import ShardServer

    g = torch.Generator(device="cuda").manual_seed(4)
    init = torch.randn(N, device="cuda", generator=g)
    deltas = [torch.randn(N, device="cuda", generator=g) for _ in range(3)]
    srv = ShardServer(0, 1, init, None, {}, {}, scale=0.5, stale_bound=0, stale_policy="damp")
    for d in deltas:
        srv.apply(d, base_version=0)              # tau = 0, 1, 2
    log = srv.stale_log()
    facs = [1.0, _f32(1 / 2), _f32(1 / 3)]
    assert log["entries"] == list(zip(range(3), facs))
    want = init.double() + sum(0.5 * f * d.double() for f, d in zip(facs, deltas))
    assert float((srv.master.double() - want).abs().max()) < 1e-5
    st = srv.stats()
    assert st["damped"] == 2 and st["staleness_max_landed"] == 2 and st["clock_drift_max"] == 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert os.environ.get("DMP_STALENESS_SCENARIO") == "uneven"
    print(json.dumps(_uneven_scenario()), flush=True)
