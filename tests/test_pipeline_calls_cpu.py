"""
The library calls a frame makes, in order and with their scalar arguments, pinned against a recording (tests/golden/pipeline_calls.json).

The order of the calls is where the measured overlap of a frame comes from (the chain's chain_flush -> tail_enqueue -> chain_finish, the next
cascade step enqueued before a scale's sampling, the ghost planes that leave right after a step): host-side changes of nellie_amd/pipeline.py
and nellie_amd/sharded.py must leave every sequence as it is.  A scripted context that does no work answers every entry point with a fixed
plausible value and logs (name, scalar arguments; arrays as shape and dtype); a communicator of the same kind logs into the same list.  Shapes
cost nothing here: they only steer the decisions.

    python tests/test_pipeline_calls_cpu.py        rewrites the recording from the nellie_amd package on the import path
"""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
RECORDING = os.path.join(HERE, "golden", "pipeline_calls.json")
ISO = {"X": 0.1, "Y": 0.1, "Z": 0.1, "T": 1.0}
ENV = ("NELLIE_SCALE_ORDER", "NELLIE_CHAIN_AHEAD", "NELLIE_CHAIN_HIST", "NELLIE_PAIR_HIST", "NELLIE_HALO", "NELLIE_GAUSS_AHEAD",
       "NELLIE_GAUSS_FUSED", "NELLIE_DEVICE_CHAIN_SLABS")


def _show(v):
    if v is None or isinstance(v, (bool, str)):
        return v
    if isinstance(v, np.ndarray) and v.ndim:
        return ["array", list(v.shape), str(v.dtype)]
    if isinstance(v, (int, np.integer)):
        return int(v)
    if isinstance(v, (float, np.floating)) or (isinstance(v, np.ndarray) and v.ndim == 0):
        return float(v)
    if isinstance(v, (tuple, list)):
        return [_show(x) for x in v]
    raise TypeError(f"an argument the log cannot show: {type(v)}")


def _tail_record():
    from nellie_amd.pipeline import percentile_from_order_statistics
    thr, gamma = percentile_from_order_statistics(100, 1.0, 2.0, 1)
    return dict(n_samples=100, a=np.float32(1.0), b=np.float32(2.0), gamma=np.float32(gamma), thr=np.float32(thr), n_positive=77)


def _range_hist(*a, **k):
    from nellie_amd.utils.gpu_functions import histogram_edges
    counts = (np.arange(256, dtype=np.int64) * 37) % 101 + 1
    return np.float32(1.0), np.float32(2.0), 1000, counts, histogram_edges(1.0, 2.0, 256), 1


def _answers(n_scales):
    n = n_scales
    return {
        "set_ndim": None, "close": None, "info": lambda key: {"gauss_yx_max_r": 12.0, "nan_hessian": 0.0}[key],
        "one_pass_available": True, "chain_available": True,
        "input_load": None, "filter_begin": None, "filter_load": None,
        "gauss_step": None, "gauss_commit": None, "gauss_step_fused": True, "set_spacing": None, "set_frob_norm": None,
        "sample_range_hist": _range_hist, "sample_range_hist2": lambda *a, **k: (_range_hist(), _range_hist()),
        "sample_minmax": (np.float32(1.0), np.float32(2.0), 1000), "sample_hist": lambda *a, **k: _range_hist()[3],
        "sample_gather": lambda *a, **k: np.array([0.0, 1.0, 2.0, 3.0, 4.0], np.float32),
        "sample_gather_positive": lambda *a, **k: np.array([1.0, 2.0, 3.0, 4.0], np.float32),
        "sample_gather_positive_begin": None, "sample_gather_positive_end": lambda: np.array([1.0, 2.0, 3.0, 5.0], np.float32),
        "flat_sample_gather": lambda *a, **k: np.array([0.0, 1.0, 2.0], np.float32),
        "flat_sample_gather_positive": lambda *a, **k: np.array([1.0, 2.0], np.float32),
        "hessian_stats": (np.float32(2.0), np.float32(64.0), False),
        "vesselness_spec": (np.float32(2.0), np.float32(64.0), False, False),
        "vesselness_resolve": True, "vesselness_count": 5, "vesselness_step": 7,
        "filter_finish": 100, "log2d_step": None, "log2d_finish": 50, "remove_edges": 30,
        "chain_begin": None, "chain_scale": None, "chain_begin_unordered": None, "chain_sample": None, "chain_walk": None,
        "chain_estimates": lambda: np.linspace(0.5, 0.1, n).astype(np.float32), "chain_flush": None,
        "chain_finish": lambda: (np.zeros(n, np.int32), np.full(n, 0.25), np.full(n, 2.0), np.full(n, 1.5), np.arange(n, dtype=np.int64) + 3),
        "chain_log": lambda k, which: (_range_hist()[3], _range_hist()[4], np.array([1.0, 2.0], np.float32), {}),
        "tail_enqueue": None, "tail_finish": lambda commit=True: _tail_record(),
        "mask_volume_dev": lambda *a, **k: {k_: v for k_, v in _tail_record().items() if k_ != "n_positive"},
        "mask_volume": None, "mask_volume_fused": 42,
    }


class StubCtx:
    """Every entry point the frame pipelines drive, answered from a table; `script` overrides an answer (a list: one answer per call)."""

    def __init__(self, log, n_scales, script=None):
        self._log = log
        self._table = _answers(n_scales)
        self._table.update(script or {})

    def __getattr__(self, name):
        if name.startswith("_") or name not in self._table:
            raise AttributeError(name)

        def call(*a, **k):
            self._log.append([name] + [_show(x) for x in a] + [[key, _show(v)] for key, v in sorted(k.items())])
            ans = self._table[name]
            if isinstance(ans, list):
                ans = ans.pop(0)
            return ans(*a, **k) if callable(ans) else ans
        return call


class StubComm:
    """A communicator of world 2 whose other rank holds what this one holds: reductions and gathers hand the argument back."""

    def __init__(self, log):
        self._log = log

    def exchange_halo(self, ctx, field, depth, offset=0, run_async=False):
        self._log.append(["comm.exchange_halo", int(field), int(depth), int(offset), bool(run_async)])

    def allreduce(self, arr, op):
        self._log.append(["comm.allreduce", _show(np.asarray(arr)), op])
        return np.asarray(arr)

    def allgather(self, arr):
        self._log.append(["comm.allgather", _show(np.asarray(arr))])
        return np.asarray(arr)


def _frame(shape):
    return np.broadcast_to(np.float32(0), shape)          # (no memory behind it: the stub never reads a voxel)


def _trace(pipe):
    t = pipe.trace
    return dict(scales=[[_show(getattr(sc, f)) for f in ("sigma", "gamma", "max_abs", "frob_thr", "mask_count", "skipped", "one_pass")]
                        for sc in t.scales], n_positive=_show(t.n_positive), percentile_thr=_show(t.percentile_thr))


# name -> (shape, settings).  Settings: env, sigmas, params (FilterParams fields), attrs (switches set on the pipeline), script (answers of
# the stub), frame (hand a frame over instead of restarting from the resident one), call ("filter" keywords) and what the run must report.
def _flagged(n, k):
    flags = np.zeros(n, np.int32)
    flags[k] = 4
    return lambda: (flags, np.full(n, 0.25), np.full(n, 2.0), np.full(n, 1.5), np.arange(n, dtype=np.int64) + 3)


SYNC = {"_device_chain": False}
CASES = {
    "chain_sigma_order_step_ahead": ((128, 512, 512), {}),
    "chain_sigma_order_step_ahead_from_a_frame": ((128, 512, 512), {"frame": True}),
    "chain_auto_order": ((512, 512, 512), {"expect": {"last_scale_order": [2, 1, 3, 0, 4]}}),
    "chain_auto_order_without_forecasts": ((512, 512, 512), {"script": {"chain_estimates": lambda: np.full(5, -1.0, np.float32)},
                                                             "expect": {"last_scale_order": [0, 1, 2, 3, 4]}}),
    "chain_env_sigma": ((512, 512, 512), {"env": {"NELLIE_SCALE_ORDER": "sigma"}, "expect": {"last_scale_order": None}}),
    "chain_env_explicit_order": ((512, 512, 512), {"env": {"NELLIE_SCALE_ORDER": "3,2,1,4,5"}, "expect": {"last_scale_order": [2, 1, 0, 3, 4]}}),
    "chain_no_step_ahead_env": ((128, 512, 512), {"env": {"NELLIE_CHAIN_AHEAD": "0", "NELLIE_SCALE_ORDER": "sigma"}}),
    "chain_checks_the_device_edges": ((128, 512, 512), {"attrs": {"check_device_edges": True}}),
    "chain_flag_falls_back": ((128, 512, 512), {"frame": True, "script": {"chain_finish": _flagged(5, 2)},
                                                "expect": {"chain_fallbacks": 1, "last_chain_flags": [0, 0, 4, 0, 0]}}),
    "chain_flag_falls_back_resident": ((128, 512, 512), {"script": {"chain_finish": _flagged(5, 0)}, "expect": {"chain_fallbacks": 1}}),
    "chain_seventeen_scales": ((64, 64, 64), {"sigmas": [1.0 + 0.1 * i for i in range(17)], "expect": {"chain_fallbacks": 1}}),
    "sync_one_pass_hit": ((128, 512, 512), {"attrs": SYNC}),
    "sync_one_pass_miss": ((128, 512, 512), {"attrs": SYNC, "script": {"vesselness_resolve": [True, False, True, False, False]}}),
    "sync_one_pass_inf": ((128, 512, 512), {"attrs": SYNC, "script": {
        "vesselness_spec": [(np.float32(2.0), np.float32(64.0), False, False), (np.float32(2.0), np.float32(64.0), True, False)] * 2
        + [(np.float32(2.0), np.float32(64.0), False, False)],
        "hessian_stats": (np.float32(2.0), np.float32(64.0), True)}}),
    "sync_one_pass_queue_overflow": ((128, 512, 512), {"attrs": SYNC, "script": {"vesselness_spec": (np.float32(2.0), np.float32(64.0), False, True)}}),
    "sync_no_bracket": ((128, 512, 512), {"attrs": SYNC, "script": {"sample_range_hist2": lambda *a, **k: (_range_hist(), (0.0, 0.0, 0) + _range_hist()[3:])}}),
    "sync_no_gamma_samples": ((128, 512, 512), {"attrs": SYNC, "script": {"sample_range_hist2": lambda *a, **k: ((0.0, 0.0, 0) + _range_hist()[3:], _range_hist())}}),
    "sync_two_pass": ((128, 512, 512), {"attrs": dict(SYNC, one_pass=False)}),
    "sync_separate_histograms": ((128, 512, 512), {"attrs": SYNC, "env": {"NELLIE_PAIR_HIST": "0"}}),
    "sync_two_call_histograms": ((128, 512, 512), {"attrs": SYNC, "env": {"NELLIE_CHAIN_HIST": "0"}}),
    "sync_step_ahead": ((128, 512, 512), {"attrs": dict(SYNC, _gauss_ahead=True)}),
    "sync_forced_miss": ((128, 512, 512), {"attrs": dict(SYNC, _one_pass_test_scale=1.5)}),
    "mask_false": ((128, 512, 512), {"call": {"mask": False}}),
    "fixed_frob_thresh": ((128, 512, 512), {"params": {"frob_thresh": 0.5}}),
    "division_zero": ((128, 512, 512), {"params": {"frob_thresh_division": 0}}),
    "radius_13_step_not_ahead_chain": ((64, 96, 96), {"sigmas": [1.0, 4.4, 4.6]}),
    "radius_13_step_not_ahead_sync": ((64, 96, 96), {"sigmas": [1.0, 4.4, 4.6], "attrs": dict(SYNC, _gauss_ahead=True)}),
    "repeated_sigma_zero_delta": ((64, 96, 96), {"sigmas": [1.0, 1.0, 2.0]}),
    "repeated_sigma_zero_delta_sync": ((64, 96, 96), {"sigmas": [1.0, 1.0, 2.0], "attrs": dict(SYNC, _gauss_ahead=True)}),
    "image_chain": ((300, 400), {"frame": True}),
    "image_sync": ((300, 400), {"frame": True, "attrs": SYNC}),
    "image_mask_false": ((300, 400), {"frame": True, "call": {"mask": False}}),
    "remove_edges": ((128, 512, 512), {"call": {"remove_edges": True}}),
    "remove_edges_nothing_left": ((128, 512, 512), {"call": {"remove_edges": True}, "script": {"remove_edges": 0}}),
    "tail_ok_false": ((128, 512, 512), {"attrs": {"_tail_ok": False}}),
    "device_tail_false": ((128, 512, 512), {"attrs": {"_device_tail": False}}),
    "no_tail_at_all": ((128, 512, 512), {"attrs": {"_tail_ok": False, "_device_tail": False}}),
    "no_tail_no_positive_sample": ((128, 512, 512), {"attrs": {"_tail_ok": False, "_device_tail": False},
                                                     "script": {"sample_gather_positive": lambda *a, **k: np.zeros(0, np.float32)}}),
    "sync_device_tail": ((128, 512, 512), {"attrs": SYNC}),
    "sync_host_epilogue": ((128, 512, 512), {"attrs": dict(SYNC, _device_tail=False)}),
    "two_step_epilogue": ((128, 512, 512), {"attrs": {"_fused_epilogue": False}}),
    "two_step_epilogue_on_the_host": ((128, 512, 512), {"attrs": {"_fused_epilogue": False, "_device_tail": False}}),
    "tail_record_without_samples": ((128, 512, 512), {"script": {
        "tail_finish": lambda commit=True: dict(_tail_record(), n_samples=0),
        "mask_volume_dev": lambda *a, **k: dict(n_samples=0, a=np.float32(0), b=np.float32(0), gamma=np.float32(0), thr=np.float32(0))}}),
    "every_scale_skipped": ((128, 512, 512), {"attrs": SYNC, "script": {"vesselness_spec": (np.float32(0.0), np.float32(0.0), False, False),
                                                                         "filter_finish": 0}}),
    "every_scale_skipped_two_pass": ((128, 512, 512), {"attrs": dict(SYNC, one_pass=False),
                                                       "script": {"hessian_stats": (np.float32(0.0), np.float32(0.0), False)}}),
}
SLAB_CASES = {
    "slab_steps_rank0_host_reductions": ((64, 48, 40), {"halo_mode": "steps"}),
    "slab_steps_rank0_with_raw_ghosts": ((64, 48, 40), {"halo_mode": "steps", "ghosts": True}),
    "slab_fat_rank0_host_reductions": ((64, 48, 40), {"halo_mode": "fat"}),
    "slab_steps_rank0_remove_edges": ((64, 48, 40), {"halo_mode": "steps", "call": {"remove_edges": True}}),
}


def run_case(name, monkeypatch=None):
    """-> the log of one case, its results at the end."""
    from nellie_amd import pipeline as pl
    slab = name in SLAB_CASES
    shape, s = (SLAB_CASES if slab else CASES)[name]
    env = s.get("env", {})
    for key in ENV:
        os.environ.pop(key, None) if monkeypatch is None else monkeypatch.delenv(key, raising=False)
    for key, v in env.items():
        os.environ.__setitem__(key, v) if monkeypatch is None else monkeypatch.setenv(key, v)
    fast, pl._FAST_PERCENTILE = pl._FAST_PERCENTILE, True      # (the device epilogue is on whatever this numpy's np.percentile does)
    sigmas = s.get("sigmas")
    p = pl.FilterParams(dim_res=dict(ISO) if len(shape) == 3 else {"X": 0.1, "Y": 0.1, "Z": None, "T": 1.0}, sigmas=sigmas, **s.get("params", {}))
    log = []
    n = len(p.resolved_sigmas())
    try:
        if slab:
            from nellie_amd.sharded import ShardedFramePipeline
            pipe = ShardedFramePipeline(shape, 0, 2, lambda ctx: StubComm(log), p, halo_mode=s["halo_mode"],
                                        ctx_factory=lambda lshape, dev, gz0, gnz, own: StubCtx(log, n, s.get("script")))
            lo, hi = pipe.own
            g_lo, g_hi = pipe.raw_ghost_needed() if s.get("ghosts") else (0, 0)
            frame = _frame((hi - lo + g_lo + g_hi,) + tuple(shape[1:]))
        else:
            pipe = pl.FramePipeline(shape, ctx=StubCtx(log, n, s.get("script")))
            frame = _frame(shape) if s.get("frame") else None
        # the switches a process reads at import: pinned here whatever the environment of the test run says
        pipe._device_chain, pipe._device_tail = True, True
        if not slab:
            pipe._gauss_ahead = False
        pipe.check_device_edges = False
        for attr, v in s.get("attrs", {}).items():
            setattr(pipe, attr, v)
        log.append(["-- frame"])
        got = pipe.filter(frame, p, **s.get("call", {}))
        log.append(["-- result", _show(got), _trace(pipe), int(pipe.chain_fallbacks), _show(getattr(pipe, "last_chain_flags", None)),
                    _show(pipe.last_scale_order)])
        for attr, v in s.get("expect", {}).items():
            assert getattr(pipe, attr) == v, f"{name}: {attr} = {getattr(pipe, attr)!r}, the case is built for {v!r}"
    finally:
        pl._FAST_PERCENTILE = fast
        if monkeypatch is None:
            for key in env:
                os.environ.pop(key, None)
    return json.loads(json.dumps(log))


def _recording():
    with open(RECORDING) as f:
        return json.load(f)


def _first_difference(got, want):
    for i, (a, b) in enumerate(zip(got, want)):
        if a != b:
            return f"call {i}: {a!r}, recorded: {b!r}"
    return f"{len(got)} calls, recorded: {len(want)}"


@pytest.mark.parametrize("name", list(CASES) + list(SLAB_CASES))
def test_library_calls_of_a_frame(name, monkeypatch):
    got, want = run_case(name, monkeypatch), _recording()[name]
    assert got == want, _first_difference(got, want)


def test_the_recording_holds_these_cases_and_their_order_matters():
    """The recording has exactly the cases above, and two swapped calls do not compare equal (the chain's flush and the epilogue it precedes)."""
    rec = _recording()
    assert sorted(rec) == sorted(list(CASES) + list(SLAB_CASES))
    calls = rec["chain_sigma_order_step_ahead"]
    names = [c[0] for c in calls]
    i = names.index("chain_flush")
    assert names[i:i + 3] == ["chain_flush", "tail_enqueue", "chain_finish"]
    swapped = calls[:i] + [calls[i + 1], calls[i]] + calls[i + 2:]
    assert swapped != calls


def test_compute_vesselness_alone(monkeypatch):
    """compute_vesselness(frame, p) on its own (the stage classes' run_frame): the scales, then the product -- no epilogue left pending."""
    from nellie_amd import pipeline as pl
    for key in ENV:
        monkeypatch.delenv(key, raising=False)
    for chain in (True, False):
        log = []
        pipe = pl.FramePipeline((128, 512, 512), ctx=StubCtx(log, 5))
        pipe._device_chain, pipe._device_tail, pipe._gauss_ahead = chain, True, False
        assert pipe.compute_vesselness(None, pl.FilterParams(dim_res=dict(ISO))) == 100
        names = [c[0] for c in log]
        assert names[-1] == "filter_finish" and "tail_enqueue" not in names and "tail_finish" not in names
        assert ("chain_finish" in names) == chain
        with pytest.raises(ValueError, match="max_threshold_samples"):
            pipe.compute_vesselness(None, pl.FilterParams(dim_res=dict(ISO), max_threshold_samples=0))


if __name__ == "__main__":
    try:
        import nellie_amd  # noqa: F401
    except ImportError:
        sys.path.insert(1, os.path.dirname(HERE))
    out = {name: run_case(name) for name in list(CASES) + list(SLAB_CASES)}
    with open(RECORDING, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")
    print(f"{len(out)} cases, {sum(len(v) for v in out.values())} calls -> {RECORDING}")
