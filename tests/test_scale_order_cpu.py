"""CPU tests of the schedule that walks a frame's scales out of sigma order inside three Gaussian volumes (pipeline.run_scale_schedule)."""
import itertools

from test_hip_scale_order import N_FITTING, _fits, _orders


def _replay(n, order, est=None):
    """-> the actions ('S', k) / ('W', k) of a frame, checked as they come: steps in sigma order, a walk only of a sampled scale, never
    more than three Gaussians alive, the newest one kept for the next step."""
    from nellie_amd import pipeline as pl
    log, pending = [], []

    def step(k):
        assert k == sum(1 for a, _ in log if a == "S")
        busy = set(pending) | ({k - 1} if k else set())
        assert len(busy) <= 2, (log, k)
        pending.append(k)
        log.append(("S", k))

    def walk(k):
        assert k in pending
        pending.remove(k)
        log.append(("W", k))

    def choose(pend, steps_left):
        assert sorted(pend) == sorted(pending) and steps_left == n - sum(1 for a, _ in log if a == "S")
        return min(pend, key=lambda k: (est[k], k))

    ok = pl.run_scale_schedule(n, order, step, walk, choose)
    return ok, log


def test_the_orders_that_fit_three_volumes():
    from nellie_amd import pipeline as pl
    for n in range(1, 7):
        mine = _orders(n)
        assert [p for p in itertools.permutations(range(n)) if pl.scale_order_fits(p)] == mine
        if n in N_FITTING:
            assert len(mine) == N_FITTING[n]
        for p in mine:
            ok, log = _replay(n, list(p))
            assert ok and [k for a, k in log if a == "W"] == list(p)
    assert _fits((2, 1, 0, 3, 4)) and not _fits((3, 0, 1, 2, 4)) and not _fits((0, 4, 1, 2, 3))
    ok, log = _replay(5, [3, 0, 1, 2, 4])
    assert not ok and not any(a == "W" for a, _ in log)          # refused before anything is walked twice


def test_auto_walks_the_smallest_forecast_and_holds_the_last_step():
    # the mask fractions of the headline volume: 3 first; 1 before 2 on the tie-break; step 5 waits until scale 2 has left its volume
    ok, log = _replay(5, None, est=[0.254, 0.255, 0.154, 0.174, 0.210])
    assert ok and log == [("S", 0), ("S", 1), ("S", 2), ("W", 2), ("W", 0), ("S", 3), ("W", 3), ("W", 1), ("S", 4), ("W", 4)]
    for n in range(1, 7):
        for est in itertools.permutations([0.1 * (k + 1) for k in range(n)]):
            ok, log = _replay(n, None, est=list(est))
            assert ok
            at = log.index(("S", n - 1))
            walked = {k for a, k in log[:at] if a == "W"}
            assert set(range(n - 1)) - walked <= {n - 2}, "the last cascade step ran while its third volume held a pending scale"
    ok, log = _replay(4, None, est=[0.2, 0.2, 0.2, 0.2])        # ties: sigma order
    assert [k for a, k in log if a == "W"] == [0, 1, 2, 3]
