"""The staleness gate (parallel/staleness.py) on its own: no process group."""
import pytest

from distributed_ml_pytorch_amd.parallel.staleness import (StalenessGate, check_policy,
                                                           damp_factor)


class _Clock:
    def __init__(self):
        self.t = 0.0

    def __call__(self):
        return self.t


def test_damp_factor_table():
    s = 2
    assert damp_factor(0, s) == 1.0
    assert damp_factor(s, s) == 1.0
    assert damp_factor(s + 1, s) == 1.0 / 2
    assert damp_factor(s + 5, s) == 1.0 / 6
    g = StalenessGate([1, 2], bound=s, policy="damp")
    assert [g.note_push(1, t) for t in (0, s, s + 1, s + 5)] == [1.0, 1.0, 0.5, 1.0 / 6]
    assert g.damped == 2
    assert g.log == [(1, 0, 1.0), (1, 2, 1.0), (1, 3, 0.5), (1, 7, 1.0 / 6)]
    # only "damp" scales anything
    assert StalenessGate([1], bound=0, policy="off").note_push(1, 9) == 1.0
    assert StalenessGate([1], bound=0, policy="block").note_push(1, 9) == 1.0


def test_policy_and_bound_are_checked():
    with pytest.raises(ValueError):
        check_policy("sometimes", 1)
    with pytest.raises(ValueError):
        check_policy("block", -1)
    with pytest.raises(ValueError):
        StalenessGate([1], bound=1.5, policy="block")


def test_clocks_and_drift_are_kept_with_policy_off():
    g = StalenessGate([1, 2, 3], bound=0, policy="off")
    for _ in range(4):
        assert g.on_push(1) == []
    g.on_push(2)
    assert g.clock == {1: 4, 2: 1, 3: 0}
    assert g.clock_drift_max == 4
    assert g.on_request(1)                 # never deferred
    assert g.stats()["deferred"] == {1: 0, 2: 0, 3: 0}


def test_slowest_worker_is_never_deferred():
    for s in (0, 1, 3):
        g = StalenessGate([1, 2, 3], bound=s, policy="block")
        for _ in range(s + 1):
            g.on_push(1)
        g.on_push(2)
        # 3 is the slowest (clock 0), 2 is within the bound for s >= 1, 1 is s + 1 ahead
        assert g.on_request(3)
        assert g.on_request(2) is (1 <= s)
        assert not g.on_request(1)
        assert g.deferred[1] == 1 and g.deferred[3] == 0
        # all at the same clock: everybody is the slowest
        g2 = StalenessGate([1, 2], bound=s, policy="block")
        assert g2.on_request(1) and g2.on_request(2)


def test_deferred_requests_are_released_in_fifo_order():
    now = _Clock()
    g = StalenessGate([1, 2, 3], bound=0, policy="block", now=now)
    g.on_push(2)
    g.on_push(1)
    assert not g.on_request(2, "a")        # queued first
    now.t = 1.0
    assert not g.on_request(1, "b")
    assert g.waiting(1) and g.waiting(2) and not g.waiting(3)
    assert g.release() == []               # 3 has not moved
    now.t = 3.0
    assert g.on_push(3) == [(2, "a"), (1, "b")]
    assert not g.waiting(1) and not g.waiting(2)
    assert g.deferred == {1: 1, 2: 1, 3: 0}
    assert g.deferred_s == pytest.approx(3.0 + 2.0)
    # an ineligible request at the head does not hold back an eligible one behind it
    g.on_push(1)
    g.on_push(1)
    g.on_push(2)                           # clocks 1: 3, 2: 2, 3: 1
    assert not g.on_request(1, "c")
    assert not g.on_request(2, "d")
    assert g.on_push(3) == [(2, "d")]      # clocks 3, 2, 2
    assert g.on_push(3) == []              # 3, 2, 3: the slowest is now 2
    assert g.on_push(2) == [(1, "c")]


def test_a_second_request_of_a_waiting_worker_stays_behind_the_first():
    g = StalenessGate([1, 2], bound=0, policy="block")
    g.on_push(1)
    assert not g.on_request(1, "first")
    assert not g.on_request(1, "second")
    assert g.on_push(2) == [(1, "first"), (1, "second")]


def test_shutdown_or_drop_leaves_the_active_set_and_releases():
    g = StalenessGate([1, 2, 3], bound=1, policy="block")
    for _ in range(3):
        g.on_push(1)
    g.on_push(2)
    g.on_push(2)                           # clocks 3, 2, 0
    assert not g.on_request(1, "x")
    assert not g.on_request(2, "y")
    # worker 3 shuts down (or is dropped): the slowest active worker is now 2
    assert g.leave(3) == [(1, "x"), (2, "y")]
    assert g.active == {1, 2}
    # a worker that has left is never deferred, and never holds anyone back
    assert g.on_request(3)
    for _ in range(5):
        g.on_push(1)
    assert not g.on_request(1, "z")
    assert g.leave(2) == [(1, "z")]
    # drift is measured against active workers only
    assert g.clock_drift_max == 8 - 2


def test_drain_answers_everything():
    g = StalenessGate([1, 2], bound=0, policy="block")
    g.on_push(1)
    assert not g.on_request(1, "p")
    assert g.drain() == [(1, "p")]
    assert g.drain() == [] and not g.waiting(1)


def test_policy_needs_a_ps_that_can_enforce_it():
    import torch

    from distributed_ml_pytorch_amd.cli import build_parser, config_from_args
    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import (TrainConfig, Worker,
                                                            check_stale_config)

    cpu = torch.device("cpu")
    single, multi = DistInfo(device=cpu), DistInfo(1, 3, 1, "gloo", cpu)
    a = build_parser().parse_args(["--stale-policy", "block", "--stale-bound", "2",
                                   "--ps", "sharded_async"])
    cfg = config_from_args(a)
    assert (cfg.stale_policy, cfg.stale_bound) == ("block", 2)
    assert TrainConfig().stale_policy == "off" and TrainConfig().stale_bound == 0
    for ps in ("central", "sharded_async"):
        for policy in ("damp", "block"):
            check_stale_config(TrainConfig(ps=ps, stale_policy=policy, stale_bound=1), multi)
    # off is accepted everywhere
    check_stale_config(TrainConfig(ps="local"), single)
    check_stale_config(TrainConfig(ps="sharded", mode="sync"), multi)
    for policy in ("damp", "block"):
        with pytest.raises(ValueError, match="cannot be enforced"):
            check_stale_config(TrainConfig(ps="sharded", stale_policy=policy), multi)
        with pytest.raises(ValueError, match="cannot be enforced"):
            check_stale_config(TrainConfig(ps="local", stale_policy=policy), multi)
        with pytest.raises(ValueError, match="cannot be enforced"):
            check_stale_config(TrainConfig(ps="central", stale_policy=policy), single)
        with pytest.raises(ValueError, match="cannot be enforced"):
            check_stale_config(TrainConfig(mode="sync", stale_policy=policy), multi)
    # a worker refuses at construction, before any model is built
    with pytest.raises(ValueError, match="cannot be enforced"):
        Worker(TrainConfig(model="mlp", ps="local", stale_policy="block", cuda=False), single)
    with pytest.raises(ValueError):
        check_stale_config(TrainConfig(ps="central", stale_policy="block", stale_bound=-1), multi)
