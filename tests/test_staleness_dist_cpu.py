"""Version-based staleness bound of the parameter servers over gloo on CPU.

Topology: the reference's 1 PS + 2 workers (central), and 3 co-located shard
servers (``sharded_async``).  Every worker trains the same small MLP with
``n_push = n_pull = 2`` and landing staleness 0 for ``STEPS = 40`` steps (20
pushes each); the slow worker sleeps ``SLEEP = 0.02`` s per step, the fast one
does not (a step of this MLP takes well under a millisecond).  Ungated, the
fast worker has sent all of its 20 pushes while the slow one has sent one or
two: ``clock_drift_max`` is in the high teens, far above the ``2 * (S + 1) = 4``
the ungated run must show for the gated assertions to mean anything.  A
scenario takes ``STEPS * SLEEP`` = 0.8 s; the three central scenarios share one
set of processes.
"""
import time

import pytest
import torch
import torch.distributed as dist
import torch.nn as nn

from test_dist_cpu import _run

pytestmark = pytest.mark.slow

STEPS, SLEEP, S, LR = 40, 0.02, 1, 0.05
PUSHES = STEPS // 2


def _mlp():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(8, 16), nn.ReLU(), nn.Linear(16, 4))


def _train(opt, model, rank, slow):
    g = torch.Generator().manual_seed(100 + rank)
    done = 0
    for _ in range(STEPS):
        if rank == slow:
            time.sleep(SLEEP)
        x = torch.randn(16, 8, generator=g)
        y = torch.randn(16, 4, generator=g)
        opt.zero_grad()
        nn.functional.mse_loss(model(x), y).backward()
        opt.step()
        done += 1
    opt.finish()
    return done


def _central_worker(rank, slow):
    from distributed_ml_pytorch_amd.parallel.asgd import Asynchronous
    from distributed_ml_pytorch_amd.parallel.clients import GlooPSClient

    class Recording(GlooPSClient):
        """Keeps a copy of every delta it pushes."""

        def _handoff(self, n=None):
            buf = super()._handoff(n)
            self.deltas.append(buf.clone())
            return buf

    m = _mlp()
    client = Recording(ps_rank=0, staleness=0)
    client.deltas = []
    opt = Asynchronous(m.parameters(), lr=LR, n_push=2, n_pull=2, model=m, client=client,
                       shadow_dtype=None)
    init = opt.arena.p32.clone()
    done = _train(opt, m, rank, slow)
    return {"steps": done, "pushes": client.pushes, "pulls": client.pulls,
            "init": init.numpy(), "deltas": torch.stack(client.deltas).numpy()}


def _central(rank, world):
    """off, block and damp, one after the other, on the same three processes."""
    from distributed_ml_pytorch_amd.parallel.server import ParameterServer

    out = {}
    for policy in ("off", "block", "damp"):
        dist.barrier()                      # every scenario starts together
        if rank == 0:
            ps = ParameterServer(model=_mlp(), workers=[1, 2], stale_bound=S,
                                 stale_policy=policy)
            st = ps.run()
            out[policy] = {"stats": st, "master": ps.parameters().clone().numpy(),
                           "log": list(ps.gate.log)}
        else:
            out[policy] = _central_worker(rank, slow=2)
    return out


@pytest.fixture(scope="module")
def central():
    return _run(_central, 3)


def test_ungated_run_drifts_far_beyond_the_bound(central):
    st = central[0]["off"]["stats"]
    print(st)
    assert st["stale_policy"] == "off" and st["stale_bound"] == S
    # the premise of the gated test: without the gate the fast worker runs away
    assert st["clock_drift_max"] >= 2 * (S + 1), st
    assert st["deferred"] == {1: 0, 2: 0} and st["damped"] == 0
    assert st["counts"]["GradientUpdate"] == 2 * PUSHES


def test_block_policy_bounds_drift_and_staleness(central):
    st = central[0]["block"]["stats"]
    print(st)
    world_workers = 2
    assert st["stale_policy"] == "block"
    assert st["clock_drift_max"] <= S + 1, st
    fast, slow = 1, 2
    assert st["deferred"][fast] > 0 and st["deferred"][slow] == 0, st
    assert st["deferred_s"] > 0
    assert st["staleness_max"] <= (world_workers - 1) * (2 * S + 1), st
    assert st["staleness_max_landed"] == st["staleness_max"]      # CPU: synchronous applies
    # nobody hangs, nothing is lost: every step, push and pull of both workers
    for r in (fast, slow):
        w = central[r]["block"]
        assert w["steps"] == STEPS and w["pushes"] == PUSHES and w["pulls"] == PUSHES, r
    assert st["counts"]["GradientUpdate"] == 2 * PUSHES
    assert st["counts"]["ParameterRequest"] == 2 * PUSHES
    assert st["dropped"] == []
    assert torch.isfinite(torch.from_numpy(central[0]["block"]["master"])).all()


def test_damp_policy_scales_stale_pushes(central):
    from distributed_ml_pytorch_amd.parallel.staleness import damp_factor

    ps = central[0]["damp"]
    st, log = ps["stats"], ps["log"]
    print(st)
    assert len(log) == 2 * PUSHES
    assert st["damped"] > 0 and st["damped"] == sum(1 for _, tau, _ in log if tau > S)
    assert st["staleness_max"] == max(tau for _, tau, _ in log)
    # the expected master, in float64: init + sum_k f(tau_k) * delta_k with the tau
    # the PS logged for each push (a worker's pushes arrive in its own order)
    want = torch.from_numpy(central[1]["damp"]["init"]).double()
    assert torch.equal(want.float(), torch.from_numpy(central[2]["damp"]["init"]))
    deltas = {r: torch.from_numpy(central[r]["damp"]["deltas"]).double() for r in (1, 2)}
    nxt = {1: 0, 2: 0}
    for w, tau, f in log:
        assert f == damp_factor(tau, S)
        want = want + damp_factor(tau, S) * deltas[w][nxt[w]]
        nxt[w] += 1
    assert nxt == {1: PUSHES, 2: PUSHES}
    got = torch.from_numpy(ps["master"]).double()
    # fp32 rounding: each of the 40 applies rounds the factor, the product and the sum
    # once (3 * 2^-24 relative to the largest value involved)
    tol = len(log) * 3 * 2.0 ** -24 * max(1.0, float(want.abs().max()))
    err = float((got - want[: got.numel()]).abs().max())
    print("damp master err", err, "tol", tol)
    assert err <= tol
    # and the damping did something: the undamped sum is elsewhere
    plain = torch.from_numpy(central[1]["damp"]["init"]).double() + deltas[1].sum(0) + \
        deltas[2].sum(0)
    assert float((got - plain[: got.numel()]).abs().max()) > 100 * tol


def _sharded(rank, world):
    from distributed_ml_pytorch_amd.parallel.asgd import Asynchronous
    from distributed_ml_pytorch_amd.parallel.async_sharded import AsyncShardedPSClient

    m = _mlp()
    client = AsyncShardedPSClient(staleness=0, stale_bound=S, stale_policy="block")
    opt = Asynchronous(m.parameters(), lr=LR, n_push=2, n_pull=2, model=m, client=client,
                       shadow_dtype=None)
    dist.barrier()
    done = _train(opt, m, rank, slow=world - 1)
    st = opt.stats()
    return {"steps": done, "stats": st,
            "finite": bool(torch.isfinite(client.master).all())}


def test_block_policy_sharded_async():
    """Three co-located shard servers, rank 2 slow: every shard's gate holds the
    two fast ranks (a peer's request or the local worker's own snapshot) to the
    same bounds as the central PS."""
    world = 3
    out = _run(_sharded, world)
    slow = world - 1
    for r in range(world):
        st = out[r]["stats"]
        print(r, {k: st[k] for k in ("clock_drift_max", "deferred", "deferred_s",
                                     "shard_staleness_max", "shard_version")})
        assert st["stale_policy"] == "block" and st["stale_bound"] == S
        assert st["clock_drift_max"] <= S + 1, (r, st)
        for fast in range(world - 1):
            assert st["deferred"][fast] > 0, (r, st)
        assert st["deferred"][slow] == 0, (r, st)
        assert st["shard_staleness_max"] <= (world - 1) * (2 * S + 1), (r, st)
        assert out[r]["steps"] == STEPS and st["pushes"] == PUSHES and st["pulls"] == PUSHES
        assert st["shard_version"] == world * PUSHES
        assert out[r]["finite"]
