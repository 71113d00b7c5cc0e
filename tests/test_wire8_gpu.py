"""The block-scaled 8-bit push wire on the GPU (csrc/optim.hip push_handoff_mx8,
ps_apply_mx8) against its CPU specification (parallel/wire8.py).

Sizes: 65,540 elements (a multiple of 4, not of 32 or 256: the tail block and
the grid-stride tails run) and 64, the smallest arena.  The central PS is
driven through ``ParameterServer.handle`` with a delayed-copy transport (a
private copy of the one in tests/test_staleness_gpu.py: RCCL refuses two ranks
on one device).
"""
import os
import socket
from collections import defaultdict, deque

import pytest
import torch
import torch.distributed as dist
import torch.nn as nn

from test_wire8_cpu import B, crafted_blocks

from distributed_ml_pytorch_amd.parallel import wire8

pytestmark = pytest.mark.gpu

N = 65_540
SIZES = [64, N]


@pytest.fixture(scope="module")
def nat():
    from distributed_ml_pytorch_amd.ops._ext import native

    return native()


def make_input(n: int, seed: int = 0) -> torch.Tensor:
    """Random normal data times a per-block magnitude 2^U(-30, 10), with the
    crafted blocks of the CPU tests laid over the front and the 4-element tail."""
    g = torch.Generator().manual_seed(seed)
    nblk = -(-n // B)
    mag = torch.exp2(torch.rand(nblk, generator=g) * 40 - 30).repeat_interleave(B)[:n]
    x = torch.randn(n, generator=g) * mag
    blocks = crafted_blocks()
    tail = blocks.pop("tail4")
    names = list(blocks) if n > 64 else ["sat", "subnormal"]
    for i, k in enumerate(names):
        x[i * B: (i + 1) * B] = blocks[k]
    if n % B == 4:
        x[-4:] = tail
    return x


@pytest.fixture(scope="module")
def cases():
    """Per size: input, CPU payload / residual / dequantised values (computed once)."""
    out = {}
    for n in SIZES:
        x = make_input(n)
        payload, resid = wire8.quantize(x)
        out[n] = {"x": x, "payload": payload, "resid": resid,
                  "deq": wire8.dequantize(payload, n)}
    return out


def same_or_both_nan(a: torch.Tensor, b: torch.Tensor) -> bool:
    return bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def test_layout_matches_the_specification(nat):
    for n in (0, 4, 64, 100, N, 11_173_962, 86_567_656):
        assert tuple(nat.mx8_layout(n)) == wire8.layout(n)
    with pytest.raises(RuntimeError):
        nat.mx8_layout(-4)


@pytest.mark.parametrize("n", SIZES)
def test_push_handoff_mx8_is_bit_identical(nat, cases, n):
    c = cases[n]
    _, so, nbytes = wire8.layout(n)
    nblk = -(-n // B)
    acc = c["x"].cuda()
    payload = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    nat.push_handoff_mx8(acc, payload)
    got, want = payload.cpu(), c["payload"]
    assert torch.equal(got[so: so + nblk], want[so: so + nblk]), "scale bytes"
    gc, wc = got[:n], want[:n]
    nonzero = ((gc & 0x7F) != 0) | ((wc & 0x7F) != 0)        # -0 may differ in sign only
    assert torch.equal(gc[nonzero], wc[nonzero]), "code bytes"
    assert same_or_both_nan(wire8.dequantize(got, n), c["deq"])
    assert bool((got[n:so] == 0).all()) and bool((got[so + nblk:] == 0).all())   # pads untouched
    assert torch.equal(acc.cpu().view(torch.int32), c["resid"].view(torch.int32)), "residual"


def test_bindings_reject_bad_arguments(nat):
    acc = torch.zeros(64, device="cuda")
    good = torch.zeros(wire8.layout(64)[2], dtype=torch.uint8, device="cuda")
    for bad in (torch.zeros(64, dtype=torch.uint8, device="cuda"),           # no scale bytes
                torch.zeros(wire8.layout(64)[2], dtype=torch.int8, device="cuda"),
                good.cpu()):
        with pytest.raises(RuntimeError):
            nat.push_handoff_mx8(acc, bad)
        with pytest.raises(RuntimeError):
            nat.ps_apply_mx8(acc, bad)
    with pytest.raises(RuntimeError):
        nat.push_handoff_mx8(torch.zeros(66, device="cuda"), good)             # n % 4
    with pytest.raises(RuntimeError):                                           # mirror + atomic
        nat.ps_apply_mx8(acc, good, torch.zeros(64, dtype=torch.bfloat16, device="cuda"), 1.0,
                         True)


def _within_one_ulp(got: torch.Tensor, want: torch.Tensor) -> bool:
    inf = torch.full_like(want, float("inf"))
    ok = (got >= torch.nextafter(want, -inf)) & (got <= torch.nextafter(want, inf))
    return bool((ok | (torch.isnan(got) & torch.isnan(want))).all())


@pytest.mark.parametrize("shape", ["plain", "atomic", "factor", "atomic_factor"])
@pytest.mark.parametrize("n", SIZES)
def test_ps_apply_mx8(nat, cases, n, shape):
    c = cases[n]
    g = torch.Generator().manual_seed(9)
    shard0 = torch.randn(n, generator=g)
    payload = c["payload"].cuda()
    atomic = shape.startswith("atomic")
    with_factor = shape.endswith("factor")

    def run(scale, factor):
        out = shard0.cuda()
        mirror = None if atomic else torch.empty(n, device="cuda", dtype=torch.bfloat16)
        slot = None if factor is None else torch.tensor([factor, 3.0], device="cuda")
        nat.ps_apply_mx8(out, payload, mirror, scale, atomic, slot)
        return out.cpu(), None if mirror is None else mirror.cpu()

    # scale 1, factor 1: one rounding on either side, bit-equal
    one, one_m = run(1.0, 1.0 if with_factor else None)
    want = shard0 + c["deq"]
    assert bool(torch.isnan(want).any()) == (n > 64)      # the non-finite blocks poison
    assert same_or_both_nan(one, want)
    fin = ~torch.isnan(want)
    assert torch.equal(one[fin].view(torch.int32), want[fin].view(torch.int32))
    if one_m is not None:
        assert torch.equal(one_m[fin].view(torch.int16),
                           one.to(torch.bfloat16)[fin].view(torch.int16))
    # scale 0.5 (and factor 1/3): the kernel may fuse the multiply-add, the oracle
    # rounds the product and the sum: within 1 ulp of the result
    f = float(torch.tensor(1.0) / 3) if with_factor else None
    sf = torch.tensor(0.5) * torch.tensor(f) if with_factor else torch.tensor(0.5)
    half, half_m = run(0.5, f)
    want = shard0 + sf * c["deq"]
    assert _within_one_ulp(half, want)
    assert float((half[fin] - one[fin]).abs().max()) > 0
    if half_m is not None:
        assert torch.equal(half_m[fin].view(torch.int16),
                           half.to(torch.bfloat16)[fin].view(torch.int16))


def test_two_atomic_applies_on_two_streams(nat):
    """Two payloads applied at once from two streams both land (order free, so a
    tolerance, as test_ps_apply_atomic_concurrent_streams)."""
    g = torch.Generator().manual_seed(21)
    shard0 = torch.randn(N, generator=g)
    payloads = [wire8.quantize(torch.randn(N, generator=g))[0] for _ in range(2)]
    ref = shard0.double() + sum(0.25 * wire8.dequantize(p, N).double() for p in payloads)
    shard = shard0.cuda()
    dev = [p.cuda() for p in payloads]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream() for _ in dev]
    for s, p in zip(streams, dev):
        with torch.cuda.stream(s):
            nat.ps_apply_mx8(shard, p, None, 0.25, True)
    torch.cuda.synchronize()
    torch.testing.assert_close(shard.cpu().double(), ref, rtol=1e-5, atol=1e-5)


# ------------------------------------------------- the central PS, device path
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


@pytest.mark.parametrize("policy", ["off", "damp"])
def test_central_ps_applies_mx8_pushes(world1, policy):
    """Two workers, two MX8 pushes each, one reply.  With ``damp`` at a bound no
    push exceeds every factor is 1: the factor-pointer kernels give the same sum."""
    from distributed_ml_pytorch_amd.parallel import messaging as M
    from distributed_ml_pytorch_amd.parallel.server import ParameterServer

    tr = DelayedCopyTransport({1: 200_000, 2: 100_000})
    g = torch.Generator().manual_seed(31)
    sent = {w: [wire8.quantize(torch.randn(N, generator=g) * 0.01)[0] for _ in range(2)]
            for w in (1, 2)}
    for w in (1, 2):
        tr.outbox[w].extend(p.cuda() for p in sent[w])
    ps = ParameterServer(numel=N, workers=[1, 2], payload="rccl", device="cuda:0", transport=tr,
                         stale_bound=8, stale_policy=policy)
    for step, w in enumerate([1, 2, 1, 2]):
        ps.handle(M.MessageCode.GradientUpdate, w, step, 0, N, M.MX8)
    ps._sync_device()                            # all four applies have landed
    ps.handle(M.MessageCode.ParameterRequest, 1, 4, 0, 0, torch.float32)
    ps.finish()
    deq = [wire8.dequantize(p, N).double() for w in (1, 2) for p in sent[w]]
    want = sum(deq)
    # four fp32 adds per element in any order: each rounds by at most 2^-24 of a
    # partial sum, itself at most sum |terms|
    tol = 4 * 2.0 ** -24 * float(sum(d.abs() for d in deq).max())
    got = ps.parameters().cpu().double()
    err = float((got - want).abs().max())
    print(policy, "master err", err, "tol", tol)
    assert err <= tol
    reply = tr.inbox[1][-1].cpu()
    assert float(reply[N]) == 4.0                # stamped with the applied count
    assert torch.equal(reply[:N].double(), got)
    st = ps.stats()
    assert st["applied"] == 4 and st["version"] == 4
    assert st["bytes_in"] == 4 * wire8.layout(N)[2]
    if policy == "damp":
        assert ps.stale_log()["count"] == 4 and st["damped"] == 0
    with pytest.raises(RuntimeError, match="elements"):
        ps.handle(M.MessageCode.GradientUpdate, 1, 9, 0, N - 4, M.MX8)


# ---------------------------------------------------------------- local PS
def _net():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(40, 50), nn.ReLU(), nn.Linear(50, 3))


def _local(device):
    from distributed_ml_pytorch_amd.parallel.asgd import Asynchronous
    from distributed_ml_pytorch_amd.parallel.clients import LocalPSClient

    m = _net().to(device)
    client = LocalPSClient(staleness=0)
    opt = Asynchronous(m.parameters(), lr=0.1, n_push=1, n_pull=1, model=m, client=client,
                       shadow_dtype=None, push_wire="mx8")
    return opt, client


def test_gpu_and_cpu_local_ps_agree():
    """The same accumulator contents for three pushes: equal masters, equal residuals."""
    og, cg = _local("cuda")
    oc, cc = _local("cpu")
    n = oc.acc.numel()
    assert og.acc.numel() == n and torch.equal(cg.master.cpu(), cc.master)
    g = torch.Generator().manual_seed(41)
    for k in range(3):
        inc = torch.randn(n, generator=g) * 10.0 ** (-k)
        oc.acc.add_(inc)
        og.acc.add_(inc.cuda())
        cc.push(k)
        cg.push(k)
        torch.cuda.synchronize()
        assert torch.equal(og.acc.cpu().view(torch.int32), oc.acc.view(torch.int32)), k
        assert torch.equal(cg.master.cpu().view(torch.int32), cc.master.view(torch.int32)), k
    assert float(oc.acc.abs().max()) > 0
    assert cg.bytes_sent == cc.bytes_sent == 3 * wire8.layout(n)[2]


@pytest.mark.strict_native
def test_mx8_push_runs_only_native_kernels():
    from torch.profiler import ProfilerActivity, profile

    og, cg = _local("cuda")
    og.acc.copy_(torch.randn(og.acc.numel()))
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        cg.push(0)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    foreign = sorted({k for k in names if "dmp::" not in k
                      and not k.startswith(("__amd_rocclr_copyBuffer", "Memcpy", "memcpy"))})
    assert not foreign, f"non-native device kernels in an MX8 push: {foreign}"
    assert any("push_handoff_mx8" in k for k in names), names
    # the apply kernel is a template over the wire reader: ps_apply_kernel<dmp::WireMX8>
    assert any("ps_apply" in k and "mx8" in k.lower() for k in names), names
