"""The sparse block top-k push wire on the GPU (csrc/optim.hip push_handoff_topk,
ps_apply_topk, ps_apply_dc_topk) against its CPU specification
(parallel/wire_topk.py).

Sizes: 64 (one short block, most lanes of the wave past the end), 256, 320 (a
full block and a 64-element tail) and 65,600 = 256 * 256 + 64 (several
workgroups, grid-stride tails, a tail block); K in {1, 8, 32}.  The central PS
is driven through ``ParameterServer.handle`` with a delayed-copy transport (a
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

from test_wire_topk_cpu import B, crafted_blocks

from distributed_ml_pytorch_amd.parallel import messaging as M
from distributed_ml_pytorch_amd.parallel import wire, wire_topk

pytestmark = pytest.mark.gpu

N = 65_600
SIZES = [64, 256, 320, N]
KS = [1, 8, 32]


@pytest.fixture(scope="module")
def nat():
    from distributed_ml_pytorch_amd.ops._ext import native

    return native()


def make_input(n: int, seed: int = 0) -> torch.Tensor:
    """Random normal data times a per-block magnitude 2^U(-30, 10), with the
    crafted blocks of the CPU tests laid over the front and the 64-element tail."""
    g = torch.Generator().manual_seed(seed)
    nblk = -(-n // B)
    mag = torch.exp2(torch.rand(nblk, generator=g) * 40 - 30).repeat_interleave(B)[:n]
    x = torch.randn(n, generator=g) * mag
    blocks = crafted_blocks()
    tail = blocks.pop("tail64")
    names = list(blocks) if n >= N else {64: ["tie_in_group"], 256: ["tie_kth"],
                                         320: ["bf16_ties"]}[n]
    for i, k in enumerate(names):
        m = min(B, n - i * B)
        x[i * B: i * B + m] = blocks[k][:m]
    if n % B == 64 and n > 64:
        x[-64:] = tail
    x[n // 2 + 1] = -0.0                   # a key-0 element whose bits must survive
    return x


@pytest.fixture(scope="module")
def cases():
    """Per size the input, per (size, K) the CPU payload / residual / entries
    (computed once, never written to)."""
    out = {}
    for n in SIZES:
        x = make_input(n)
        out[n] = {"x": x}
        for k in KS:
            payload, resid = wire_topk.sparsify(x, k)
            out[n, k] = {"payload": payload, "resid": resid,
                         "entries": wire_topk.entries(payload, n, k),
                         "dense": wire_topk.densify(payload, n, k)}
    return out


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def same_bits_or_both_nan(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit for bit, except that two NaNs need not share their payload bits."""
    a, b = a.cpu(), b.cpu()
    return bool(((bits(a) == bits(b)) | (torch.isnan(a) & torch.isnan(b))).all())


def test_words_match_the_specification(nat):
    for n in (0, 64, 256, 320, N, 11_173_962, 86_567_656):
        for k in KS:
            assert nat.topk_words(n, k) == wire_topk.layout(n, k)[1]
    for n, k in ((64, 0), (64, 33), (-4, 8)):
        with pytest.raises(RuntimeError):
            nat.topk_words(n, k)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("n", SIZES)
def test_push_handoff_topk_is_bit_identical(nat, cases, n, k):
    c = cases[n, k]
    acc = cases[n]["x"].cuda()
    # every slot is written, the empty ones with 0: start from all-ones words
    payload = torch.full((wire_topk.layout(n, k)[1],), -1, dtype=torch.int32, device="cuda")
    nat.push_handoff_topk(acc, payload, k)
    assert torch.equal(payload.cpu(), c["payload"]), "payload words"
    assert torch.equal(bits(acc), bits(c["resid"])), "residual"


@pytest.mark.parametrize("n", [320, N])
def test_push_handoff_topk_inside_a_larger_allocation(nat, cases, n):
    """16-B aligned, but not at the start of its allocation; the neighbours stay."""
    k = 8
    c = cases[n, k]
    nwords = c["payload"].numel()
    big = torch.full((n + 72,), 123.0, device="cuda")
    pbig = torch.full((nwords + 24,), 77, dtype=torch.int32, device="cuda")
    acc, payload = big[36: 36 + n], pbig[12: 12 + nwords]
    acc.copy_(cases[n]["x"])
    nat.push_handoff_topk(acc, payload, k)
    assert torch.equal(payload.cpu(), c["payload"])
    assert torch.equal(bits(acc), bits(c["resid"]))
    assert bool((big[:36] == 123.0).all()) and bool((big[36 + n:] == 123.0).all())
    assert bool((pbig[:12] == 77).all()) and bool((pbig[12 + nwords:] == 77).all())


def test_bindings_reject_bad_arguments(nat):
    acc = torch.zeros(320, device="cuda")
    good = torch.zeros(16, dtype=torch.int32, device="cuda")
    for bad in (torch.zeros(15, dtype=torch.int32, device="cuda"),           # not nblk * k
                torch.zeros(16, dtype=torch.float32, device="cuda"),
                torch.zeros(32, dtype=torch.int32, device="cuda")[::2],
                good.cpu()):
        with pytest.raises(RuntimeError):
            nat.push_handoff_topk(acc, bad, 8)
        with pytest.raises(RuntimeError):
            nat.ps_apply_topk(acc, bad, None, 1.0, False, None, 8)
        with pytest.raises(RuntimeError):
            nat.ps_apply_dc_topk(acc, bad, torch.zeros(320, device="cuda"), None, 1.0, 0.5,
                                 False, None, 8)
    for k in (0, 33, 4):                                                     # range; 16 != 2 * 4
        with pytest.raises(RuntimeError):
            nat.push_handoff_topk(acc, good, k)
        with pytest.raises(RuntimeError):
            nat.ps_apply_topk(acc, good, None, 1.0, False, None, k)
    with pytest.raises(RuntimeError):
        nat.push_handoff_topk(torch.zeros(322, device="cuda"), good, 8)        # n % 4
    with pytest.raises(RuntimeError):                                           # mirror + atomic
        nat.ps_apply_topk(acc, good, torch.zeros(320, dtype=torch.bfloat16, device="cuda"), 1.0,
                          True, None, 8)
    with pytest.raises(RuntimeError):                                           # bak aliases
        nat.ps_apply_dc_topk(acc, good, acc, None, 1.0, 0.5, False, None, 8)


# -------------------------------------------------------------------- applies
SCALES = [1.0, 0.5, -0.3]
THIRD = float(torch.tensor(1.0) / 3)


def _shard0(n: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(9)
    s = torch.randn(n, generator=g)
    s[::7] = -0.0                          # untouched elements keep their bits, -0 included
    return s


def _sc(scale: float, factor) -> torch.Tensor:
    sc = torch.tensor(scale, dtype=torch.float32)
    return sc if factor is None else sc * torch.tensor(factor, dtype=torch.float32)


@pytest.mark.parametrize("form", ["plain", "mirror", "atomic", "plain_factor", "mirror_factor",
                                  "atomic_factor"])
@pytest.mark.parametrize("n", SIZES)
def test_ps_apply_topk(nat, cases, n, form):
    """Every form equals the CPU expression -- the product and the sum rounded
    separately -- bit for bit; untouched elements of shard and mirror keep theirs."""
    atomic = form.startswith("atomic")
    with_mirror = form.startswith("mirror")
    factor = THIRD if form.endswith("factor") else None
    shard0 = _shard0(n)
    mirror0 = torch.full((n,), 7.0, dtype=torch.bfloat16)
    for k in KS:
        at, val = cases[n, k]["entries"]
        payload = cases[n, k]["payload"].cuda()
        touched = torch.zeros(n, dtype=torch.bool)
        touched[at] = True
        assert int(touched.sum()) == at.numel() > 0          # distinct addresses
        for scale in SCALES:
            out = shard0.cuda()
            mirror = mirror0.cuda() if with_mirror else None
            slot = None if factor is None else torch.tensor([factor, 3.0], device="cuda")
            nat.ps_apply_topk(out, payload, mirror, scale, atomic, slot, k)
            want = shard0.clone()
            p = _sc(scale, factor) * val
            want[at] = want[at] + p
            assert same_bits_or_both_nan(out, want), (k, scale)
            assert torch.equal(bits(out)[~touched], bits(shard0)[~touched])
            if mirror is not None:
                fin = touched & ~torch.isnan(want)
                assert torch.equal(bits(mirror)[fin], bits(want.to(torch.bfloat16))[fin])
                assert bool(torch.isnan(mirror.cpu()[touched & ~fin].float()).all())
                assert torch.equal(bits(mirror)[~touched], bits(mirror0)[~touched])
    assert bool(torch.isnan(want).any()) == (n == N)         # the non-finite blocks poison


@pytest.mark.parametrize("form", ["plain", "atomic", "plain_factor", "atomic_factor"])
@pytest.mark.parametrize("n", SIZES)
def test_ps_apply_dc_topk(nat, cases, n, form):
    """Equals wire._apply_dc_cpu on the densified payload, bit for bit on the
    touched elements; every other element keeps its bits."""
    atomic = form.startswith("atomic")
    factor = THIRD if form.endswith("factor") else None
    shard0 = _shard0(n)
    g = torch.Generator().manual_seed(13)
    bak = shard0 + 0.01 * torch.randn(n, generator=g)
    bak_gpu = bak.cuda()
    c = 0.7
    for k in KS:
        at, _ = cases[n, k]["entries"]
        payload = cases[n, k]["payload"].cuda()
        touched = torch.zeros(n, dtype=torch.bool)
        touched[at] = True
        for scale in SCALES:
            out = shard0.cuda()
            slot = None if factor is None else torch.tensor([factor, 3.0], device="cuda")
            nat.ps_apply_dc_topk(out, payload, bak_gpu, None, scale, c, atomic, slot, k)
            want = shard0.clone()
            wire._apply_dc_cpu(want, bak, cases[n, k]["dense"], scale, c, factor)
            assert same_bits_or_both_nan(out.cpu()[touched], want[touched]), (k, scale)
            assert torch.equal(bits(out)[~touched], bits(shard0)[~touched])
    # the mirror form, once: the touched elements' bf16 cast, the rest untouched
    k, scale = 8, 0.5
    at, _ = cases[n, k]["entries"]
    if not atomic:
        out, mirror = shard0.cuda(), torch.full((n,), 7.0, dtype=torch.bfloat16, device="cuda")
        nat.ps_apply_dc_topk(out, cases[n, k]["payload"].cuda(), bak_gpu, mirror, scale, c, False,
                             None, k)
        got = out.cpu()
        fin = torch.zeros(n, dtype=torch.bool)
        fin[at] = True
        fin &= ~torch.isnan(got)
        assert torch.equal(bits(mirror)[fin], bits(got.to(torch.bfloat16))[fin])
        rest = torch.ones(n, dtype=torch.bool)
        rest[at] = False
        assert bool((mirror.cpu()[rest].float() == 7.0).all())


def test_codec_paths_agree_with_the_cpu(cases):
    """wire.topk(k) on the GPU and on the CPU: hand-off, apply and apply_dc."""
    n, k = 320, 8
    codec = wire.topk(k)
    acc_c, acc_g = cases[n]["x"].clone(), cases[n]["x"].cuda()
    buf_c, buf_g = codec.new_payload(n, "cpu"), codec.new_payload(n, "cuda")
    assert not buf_g.any()
    codec.handoff(acc_c, buf_c)
    codec.handoff(acc_g, buf_g)
    assert torch.equal(buf_g.cpu(), buf_c) and torch.equal(bits(acc_g), bits(acc_c))
    m_c = _shard0(n)
    m_g = m_c.cuda()
    bak = m_c + 0.5
    wire.codec(buf_c).apply(m_c, buf_c, 0.5)
    wire.codec(buf_g).apply(m_g, buf_g, 0.5)                 # the reader of an int32 tensor
    assert torch.equal(bits(m_g), bits(m_c))
    codec.apply_dc(m_c, bak, buf_c, 0.5, 0.7)
    codec.apply_dc(m_g, bak.cuda(), buf_g, 0.5, 0.7)
    assert torch.equal(bits(m_g), bits(m_c))
    assert torch.equal(codec.decode(buf_g, n), codec.decode(buf_c, n))


# --------------------------------------------------------------------- guards
def test_consumers_ignore_zero_values_and_foreign_addresses(nat):
    """A hand-built payload for n = 320 at K = 8: one word of the tail block
    addresses 256 + 200, one carries value bits 0 with a non-zero index.  Both are
    ignored by every form.  The shard is a view inside a larger tensor of
    sentinels, so the foreign address lies in the same allocation: without the
    guard the sentinel changes, nothing faults."""
    n, k, lo = 320, 8, 64
    one = 0x3F80 << 16
    payload = torch.zeros(2 * k, dtype=torch.int32)
    payload[0] = one | 5
    payload[k] = one | 200                     # block 1: 456 >= n
    payload[k + 1] = 0 | 17                    # value +0, index 17 (address 273 < n)
    payload[k + 2] = one | 63                  # the last element of the shard
    payload[k + 3] = (0x8000 << 16 | 30) - 2 ** 32     # value -0
    payload = payload.cuda()
    want = torch.zeros(n)
    want[5] = want[319] = 0.5
    for atomic in (False, True):
        for dc in (False, True):
            big = torch.full((lo + n + 448,), 123.0, device="cuda")
            mbig = torch.full((lo + n + 448,), 7.0, dtype=torch.bfloat16, device="cuda")
            shard, mirror = big[lo: lo + n], None if atomic else mbig[lo: lo + n]
            shard.zero_()
            if dc:
                nat.ps_apply_dc_topk(shard, payload, torch.zeros(n, device="cuda"), mirror, 0.5,
                                     0.7, atomic, None, k)
            else:
                nat.ps_apply_topk(shard, payload, mirror, 0.5, atomic, None, k)
            got = big.cpu()
            assert torch.equal(got[lo: lo + n], want), (atomic, dc)
            assert bool((got[:lo] == 123.0).all()) and bool((got[lo + n:] == 123.0).all())
            if mirror is not None:
                m = mbig.cpu().float()
                assert m[lo + 5] == 0.5 and m[lo + 319] == 0.5
                m[lo + 5] = m[lo + 319] = 7.0
                assert bool((m == 7.0).all())


# -------------------------------------------------------------- graph capture
def test_handoff_and_apply_replay_in_a_graph(nat, cases):
    """The hand-off and one plain apply captured in one graph on one stream (no
    parallel branches), replayed twice, against two eager rounds."""
    n, k = N, 8
    nwords = wire_topk.layout(n, k)[1]
    x, shard0 = cases[n]["x"], _shard0(n)

    def fresh():
        return x.cuda(), torch.zeros(nwords, dtype=torch.int32, device="cuda"), shard0.cuda()

    def round_(acc, payload, shard):
        nat.push_handoff_topk(acc, payload, k)
        nat.ps_apply_topk(shard, payload, None, 0.5, False, None, k)

    eager = fresh()
    for _ in range(2):                          # also the warm-up outside the capture
        round_(*eager)
    torch.cuda.synchronize()
    graphed = fresh()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        round_(*graphed)
    for _ in range(2):
        graph.replay()
    torch.cuda.synchronize()
    for name, e, g in zip(("acc", "payload", "shard"), eager, graphed):
        assert same_bits_or_both_nan(g, e) if e.is_floating_point() else torch.equal(g, e), name
    # the second round sent what the first left behind
    assert not torch.equal(eager[1].cpu(), cases[n, k]["payload"])


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
def test_central_ps_applies_topk_pushes(world1, policy):
    """Two workers, two top-k pushes each, one reply.  With ``damp`` at a bound no
    push exceeds every factor is 1: the factor-pointer kernels give the same sum."""
    from distributed_ml_pytorch_amd.parallel.server import ParameterServer

    k = 8
    nwords = wire_topk.layout(N, k)[1]
    tr = DelayedCopyTransport({1: 200_000, 2: 100_000})
    g = torch.Generator().manual_seed(31)
    sent = {w: [wire_topk.sparsify(torch.randn(N, generator=g) * 0.01, k)[0] for _ in range(2)]
            for w in (1, 2)}
    for w in (1, 2):
        tr.outbox[w].extend(p.cuda() for p in sent[w])
    ps = ParameterServer(numel=N, workers=[1, 2], payload="rccl", device="cuda:0", transport=tr,
                         stale_bound=8, stale_policy=policy, push_topk=k)
    for step, w in enumerate([1, 2, 1, 2]):
        ps.handle(M.MessageCode.GradientUpdate, w, step, 0, N, M.topk(k))
    ps._sync_device()                            # all four applies have landed
    ps.handle(M.MessageCode.ParameterRequest, 1, 4, 0, 0, torch.float32)
    ps.finish()
    dense = [wire_topk.densify(p, N, k).double() for w in (1, 2) for p in sent[w]]
    want = sum(dense)
    assert int((want != 0).sum()) >= N // B * k     # the pushes do land
    # four fp32 adds per touched element in any order: each rounds by at most 2^-24
    # of a partial sum, itself at most sum |terms|
    tol = 4 * 2.0 ** -24 * float(sum(d.abs() for d in dense).max())
    got = ps.parameters().cpu().double()
    err = float((got - want).abs().max())
    print(policy, "master err", err, "tol", tol)
    assert err <= tol
    reply = tr.inbox[1][-1].cpu()
    assert float(reply[N]) == 4.0                # stamped with the applied count
    assert torch.equal(reply[:N].double(), got)
    st = ps.stats()
    assert st["applied"] == 4 and st["version"] == 4
    assert st["bytes_in"] == 4 * 4 * nwords
    if policy == "damp":
        assert ps.stale_log()["count"] == 4 and st["damped"] == 0
    with pytest.raises(RuntimeError, match="elements"):
        ps.handle(M.MessageCode.GradientUpdate, 1, 9, 0, N - 4, M.topk(k))
    with pytest.raises(RuntimeError, match="K = 4.*push_topk = 8"):
        ps.handle(M.MessageCode.GradientUpdate, 1, 9, 0, N, M.topk(4))


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
                       shadow_dtype=None, push_wire="topk", push_topk=8)
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
        assert torch.equal(bits(og.acc), bits(oc.acc)), k
        assert torch.equal(bits(cg.master), bits(cc.master)), k
    assert float(oc.acc.abs().max()) > 0
    assert cg.bytes_sent == cc.bytes_sent == 3 * 4 * wire_topk.layout(n, 8)[1]


@pytest.mark.strict_native
def test_topk_push_runs_only_native_kernels():
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
    assert not foreign, f"non-native device kernels in a top-k push: {foreign}"
    assert any("push_handoff_topk" in k for k in names), names
    assert any("ps_apply_topk" in k for k in names), names
