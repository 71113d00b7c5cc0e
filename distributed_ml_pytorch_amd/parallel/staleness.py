"""Version-based staleness bound of the parameter servers.

The reference PS has no version at all (its asgd/optim/Asynchronous.py:17-18,
48-59): a fast worker runs arbitrarily far ahead of a slow one, and the slow
worker's very old delta is added at full weight.  Both servers here
(:class:`~.server.ParameterServer`, :class:`~.async_sharded.ShardServer`) share
the same header loop, so the bookkeeping lives once, in :class:`StalenessGate`:

* **always** (also with policy ``off``): a clock per worker, ``clock[w]`` = number
  of ``GradientUpdate`` s received from ``w``, and ``clock_drift_max``, the running
  maximum of ``clock[w] - min(clock of active workers)``.  A worker is active
  until liveness drops it or it sends ``Shutdown``.
* policy ``block`` -- stale-synchronous parallel, enforced where pulls are
  served: a ``ParameterRequest`` from ``w`` is answered only while
  ``clock[w] - min(active clocks) <= S``; otherwise it is queued and re-checked,
  in FIFO order, after every push, shutdown and liveness drop.  The slowest
  active worker has drift 0 <= S, so it is never deferred: somebody always
  makes progress.  The worker needs no protocol change, it already waits for the
  reply when the pull is due (``PSClient.land_due``).
* policy ``damp`` -- a push whose staleness ``tau`` (applied count minus the base
  version in its header: the existing ``staleness`` stat, the worker's own
  applies included) exceeds ``S`` is applied at weight
  ``f(tau) = 1 / (1 + tau - S)`` (``f = 1`` up to ``S``), multiplied into
  ``delta_scale``.  On CPU ``tau`` is the host count; on GPU it is read on the
  device by ``ps_stale_factor`` (``csrc/optim.hip``) on the applying stream, with
  no host sync, clamped to the host's enqueue count at the push's arrival, and
  recorded in a :class:`DeviceStaleLog`.

Bounds of policy ``block`` (``S`` = ``stale_bound``, ``W`` workers):

* **clock drift.**  A worker's clock moves only at a push, and between two of
  its pushes it has had a pull answered if ``n_push == n_pull`` and the landing
  delay is below ``n_push`` (it waits for the reply before the next push).  That
  reply was sent while ``clock[w] - min <= S`` and the minimum never falls while
  its owner stays active, so after the next push ``clock[w] - min <= S + 1``:
  ``clock_drift_max <= S + 1``.  In general a worker pushes up to
  ``ceil((n_pull + staleness) / n_push)`` times between sending a request and
  having to wait for its reply, so
  ``clock_drift_max <= S + ceil((n_pull + staleness) / n_push)``.
* **version staleness** (central PS on CPU, where applies are synchronous).
  Worker ``w`` is given a snapshot while its clock is ``c`` and pushes next at
  clock ``c + 1``.  When the snapshot was served, every other active worker's
  clock was at least ``c - S`` (else ``w`` would have been deferred); until
  ``w``'s next push is applied another worker can be served pulls, and so keep
  pushing, only while its clock is at most ``c + S`` at the request, which lets
  it reach ``c + S + 1``.  Another worker's clock therefore moves from at least
  ``c - S`` to at most ``c + S + 1`` in between: at most ``2S + 1`` applies each,
  and there are ``W - 1`` others, so each push's version staleness is at most
  ``(W - 1) * (2S + 1)``.
"""
from __future__ import annotations

import time
from collections import deque

POLICIES = ("off", "damp", "block")


def check_policy(policy: str, bound: int):
    if policy not in POLICIES:
        raise ValueError(f"stale_policy must be one of {POLICIES}, got {policy!r}")
    if int(bound) != bound or bound < 0:
        raise ValueError(f"stale_bound must be an integer >= 0, got {bound!r}")


def damp_factor(tau: int, bound: int) -> float:
    """``f(tau)``: 1 up to the bound, ``1 / (1 + tau - bound)`` above it."""
    return 1.0 if tau <= bound else 1.0 / (1 + tau - bound)


class StalenessGate:
    """Worker clocks, the pull gate (``block``) and the host damping factor (``damp``).

    Not thread-safe: :class:`~.async_sharded.ShardServer` calls it under its lock.
    ``now`` is injectable for tests."""

    def __init__(self, workers, bound: int = 0, policy: str = "off", now=time.monotonic):
        check_policy(policy, bound)
        self.bound, self.policy = int(bound), policy
        self.clock = {w: 0 for w in workers}
        self.active = set(self.clock)
        self.clock_drift_max = 0
        self.deferred = {w: 0 for w in self.clock}
        self.deferred_s = 0.0
        self.damped = 0
        self.log: list = []            # (worker, tau, factor) of every push, in apply order
        self._queue: deque = deque()   # (worker, token, time queued)
        self._now = now

    # ------------------------------------------------------------------ clocks
    def _min_active(self):
        return min((self.clock[w] for w in self.active), default=None)

    def drift(self, w) -> int:
        lo = self._min_active()
        return 0 if lo is None else max(0, self.clock.get(w, 0) - lo)

    def on_push(self, w) -> list:
        """A ``GradientUpdate`` from ``w`` arrived -> the queued requests it releases."""
        self.clock[w] = self.clock.get(w, 0) + 1
        self.deferred.setdefault(w, 0)
        if w in self.active:
            self.clock_drift_max = max(self.clock_drift_max, self.drift(w))
        return self.release()

    def leave(self, w) -> list:
        """``w`` sent ``Shutdown`` or was dropped -> the queued requests that releases."""
        self.active.discard(w)
        return self.release()

    # -------------------------------------------------------------------- gate
    def eligible(self, w) -> bool:
        if self.policy != "block" or w not in self.active:
            return True
        return self.drift(w) <= self.bound

    def on_request(self, w, token=None) -> bool:
        """``True``: answer now.  ``False``: queued; it comes back from
        :meth:`release` (as ``(w, token)``) once ``w`` is eligible."""
        # behind an earlier request of its own still queued: replies stay in order
        if self.eligible(w) and not self.waiting(w):
            return True
        self.deferred[w] = self.deferred.get(w, 0) + 1
        self._queue.append((w, token, self._now()))
        return False

    def waiting(self, w) -> bool:
        return any(q[0] == w for q in self._queue)

    def _pop(self, keep) -> list:
        out, rest, now = [], deque(), self._now()
        for w, token, t0 in self._queue:
            if keep(w):
                rest.append((w, token, t0))
            else:
                self.deferred_s += now - t0
                out.append((w, token))
        self._queue = rest
        return out

    def release(self) -> list:
        """Every queued request that is now eligible, oldest first."""
        if not self._queue:
            return []
        return self._pop(lambda w: not self.eligible(w))

    def drain(self) -> list:
        """Everything still queued (shutdown: nobody is left waiting)."""
        return self._pop(lambda w: False)

    # -------------------------------------------------------------------- damp
    def note_push(self, w, tau: int) -> float:
        """Host factor of a push of staleness ``tau`` (1.0 unless policy ``damp``)."""
        f = damp_factor(tau, self.bound) if self.policy == "damp" else 1.0
        if f != 1.0:
            self.damped += 1
        self.log.append((w, int(tau), f))
        return f

    def stats(self) -> dict:
        return {"stale_policy": self.policy, "stale_bound": self.bound,
                "clock_drift_max": self.clock_drift_max,
                "deferred": dict(self.deferred), "deferred_s": round(self.deferred_s, 6),
                "damped": self.damped}


class DeviceStaleLog:
    """Device side of policy ``damp``: one ``{factor, tau}`` slot per applying
    stream and the log ``ps_stale_factor`` keeps (apply count, max tau, damped
    count, a 1024-entry ring of ``(tau, factor)``).

    With device links the applies of different workers run concurrently, so the
    host's enqueue count overstates what has landed; the factor comes from the
    device applied count (:class:`.links.AppliedCount`), read on the applying
    stream right before the apply.  ``tau`` is therefore the staleness when the
    factor kernel ran, a lower bound on the staleness when the apply lands, and
    (see :meth:`factor`) never above the host's figure for the same push."""

    def __init__(self, device, native, applied, bound: int, keys=()):
        import torch

        self.nat, self.applied, self.bound = native, applied, int(bound)
        self.device = device
        self.log = torch.zeros(native.ps_stale_log_numel(), dtype=torch.int32, device=device)
        self._slots: dict = {}
        for k in keys:                 # up front: no allocation between transfers
            self.slot(k)

    def slot(self, key):
        import torch

        s = self._slots.get(key)
        if s is None:
            s = self._slots[key] = torch.zeros(2, dtype=torch.float32, device=self.device)
        return s

    def factor(self, key, base: int, cap: int | None = None):
        """Launch ``ps_stale_factor`` on the CURRENT stream for a push whose header
        carries ``base`` -> the slot to hand to ``ps_apply(factor=...)``.

        ``cap``: the host's enqueue count when the push arrived.  The device count
        is clamped to it, so the device ``tau`` never exceeds the host's
        ``version - base`` of the same push: with completion-ordered applies a
        faster link's LATER pushes may land before this apply runs, and the server
        ordered those behind this push."""
        s = self.slot(key)
        self.nat.ps_stale_factor(self.applied.dev, int(base), self.bound, s, self.log,
                                 None if cap is None else int(cap))
        return s

    def read(self) -> dict:
        """The log (host sync: stats and tests only).  ``entries``: the last
        ``min(count, 1024)`` applies' ``(tau, factor)`` in apply-index order."""
        import torch

        host = self.log.cpu()
        count, tau_max, damped = (int(x) for x in host[:3])
        ring = host[4:].view(-1, 2)
        n = ring.shape[0]
        idx = [i % n for i in range(max(0, count - n), count)]
        taus = ring[idx, 0].tolist()
        facs = ring[idx, 1].contiguous().view(torch.float32).tolist()
        return {"count": count, "tau_max": tau_max, "damped": damped,
                "entries": list(zip(taus, facs))}
