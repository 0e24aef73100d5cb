"""
GPU tests (-m gpu) of the scales of a frame walked out of sigma order (NELLIE_SCALE_ORDER; csrc/nellie_hip.hip: nl_chain_begin_unordered).

The frame is max_s(v_s) * AND_s(m_s), so every walk order must give the same bits.  The reference in every case is this build with
NELLIE_SCALE_ORDER=sigma -- the loop the rest of the suite pins against the oracle -- computed once per case on a fresh context and never
modified.  Compared byte for byte: the Frangi frame, the labels, the label count, every field of the per-scale trace, the chain's flags.

Frames: the fused cascade step is forced at small sizes (NELLIE_GAUSS_FUSED=1, the cascade step not running ahead on the side stream, and
NELLIE_RESOLVE_DEFER=2 so that the held-back resolve kernel runs as it does at 2^26 voxels).  (24, 80, 136) and (70, 50, 200): no tile
multiples (the walk's 60-column strips, the cascade step's 48- / 32-row tiles), thinner than / just over one 64-plane Z chunk.
"""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(24, 80, 136), (70, 50, 200)]
N_FITTING = {1: 1, 2: 2, 3: 6, 4: 16, 5: 44}        # orders that fit three volumes (worked out by hand for 1..3, by _fits beyond)

_VOL = {}
_REF = {}


def _volume(shape, seed):
    from nellie_amd.synthetic import make_volume
    if (shape, seed) not in _VOL:
        v = make_volume(shape, seed)
        v.setflags(write=False)
        _VOL[(shape, seed)] = v
    return _VOL[(shape, seed)]


def _fits(order):
    """Independent of the product's scheduler: a search over every interleaving of cascade steps (sigma order) and walks (`order`).  A
    volume is busy while its scale is sampled but not walked, and the newest Gaussian is the next step's source."""
    n = len(order)
    seen, stack = set(), [(0, 0)]
    while stack:
        done, pos = stack.pop()
        if pos == n:
            return True
        if (done, pos) in seen:
            continue
        seen.add((done, pos))
        walked = set(order[:pos])
        busy = {k for k in range(done) if k not in walked} | ({done - 1} if done else set())
        if done < n and len(busy) <= 2:
            stack.append((done + 1, pos))
        if order[pos] < done:
            stack.append((done, pos + 1))
    return False


def _orders(n):
    return [p for p in itertools.permutations(range(n)) if _fits(p)]


def _env(monkeypatch, order):
    monkeypatch.setenv("NELLIE_GAUSS_FUSED", "1")
    monkeypatch.setenv("NELLIE_RESOLVE_DEFER", "2")
    monkeypatch.setenv("NELLIE_SCALE_ORDER", order if isinstance(order, str) else ",".join(str(k + 1) for k in order))


def _pipe(shape, **attrs):
    from nellie_amd import pipeline as pl
    pipe = pl.FramePipeline(shape)
    pipe._chain_ahead_env = "0"
    for k, v in attrs.items():
        setattr(pipe, k, v)
    return pipe


def _params(dr, n_sigmas=5, **kw):
    from nellie_amd import pipeline as pl
    return pl.FilterParams(dim_res=dr, sigmas=[float(s) for s in pl.default_sigmas(dr)[:n_sigmas]], **kw)


def _frame(pipe, vol, p):
    """filter + label as bench.py's step runs them"""
    from nellie_amd import pipeline as pl
    pipe.filter(vol, p)
    tr = [(s.sigma, s.gamma, s.max_abs, s.frob_thr, s.mask_count, s.skipped, s.one_pass) for s in pipe.trace.scales]
    fr = pipe.download_frangi()
    n = int(pipe.label(pipe.frangi_threshold(), pl.min_area_pixels_of(p.dim_res))) if pipe.trace.n_positive > 0 else 0
    lab = pipe.download_labels() if pipe.trace.n_positive > 0 else None
    return dict(frangi=fr, labels=lab, n_labels=n, trace=tr, n_positive=pipe.trace.n_positive, pct=pipe.trace.percentile_thr,
                flags=list(pipe.last_chain_flags), prezero=int(pipe.ctx.info("prezero_used")), order=pipe.last_scale_order)


def _reference(key, vol, p, monkeypatch, **attrs):
    if key not in _REF:
        _env(monkeypatch, "sigma")
        pipe = _pipe(vol.shape, **attrs)
        try:
            ref = _frame(pipe, vol, p)
            ref["fallbacks"] = pipe.chain_fallbacks
        finally:
            pipe.close()
        assert ref["order"] is None
        ref["frangi"].setflags(write=False)
        if ref["labels"] is not None:
            ref["labels"].setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def _same(got, ref, what):
    assert got["trace"] == ref["trace"], what
    assert got["flags"] == ref["flags"], what
    assert got["n_positive"] == ref["n_positive"] and got["pct"] == ref["pct"] and got["n_labels"] == ref["n_labels"], what
    assert np.array_equal(got["frangi"].view(np.uint32), ref["frangi"].view(np.uint32)), what
    assert (got["labels"] is None) == (ref["labels"] is None), what
    if ref["labels"] is not None:
        assert np.array_equal(got["labels"], ref["labels"]), what


@pytest.mark.parametrize("aniso", [False, True], ids=["iso", "aniso"])
@pytest.mark.parametrize("n_sigmas", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("shape", SHAPES)
def test_every_order_that_fits_gives_the_same_bits(hip, shape, n_sigmas, aniso, monkeypatch):
    """`auto` and every permutation that fits, frame after frame on ONE context (each frame starts from the state the last order left)."""
    from nellie_amd.synthetic import ANISO_03, ISO_01
    dr = ANISO_03 if aniso else ISO_01
    vol, p = _volume(shape, 71), _params(dr, n_sigmas)
    ref = _reference((shape, 71, aniso, n_sigmas), vol, p, monkeypatch)
    assert ref["fallbacks"] == 0 and ref["flags"] == [0] * n_sigmas and (ref["frangi"] > 0).any() and ref["n_labels"] > 0
    pipe = _pipe(shape)
    try:
        for order in ["auto"] + _orders(n_sigmas):
            _env(monkeypatch, order)
            got = _frame(pipe, vol, p)
            assert pipe.chain_fallbacks == 0
            assert got["order"] is not None and sorted(got["order"]) == list(range(n_sigmas)), "the frame did not take the reordering path"
            if order != "auto":
                assert got["order"] == list(order)
            _same(got, ref, f"order {order}")
        _env(monkeypatch, "sigma")                 # read per frame: the same context, sigma order again
        got = _frame(pipe, vol, p)
        assert got["order"] is None
        _same(got, ref, "back to sigma")
    finally:
        pipe.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_prezero_on_and_off(hip, shape, monkeypatch):
    """The label volume is pre-zeroed by the last cascade step in sigma order and under `auto` (which holds that step back until its third
    volume is dead), is written densely where an explicit order keeps a scale pending in that volume -- and holds the same labels always."""
    from nellie_amd.synthetic import ISO_01
    vol, p = _volume(shape, 71), _params(ISO_01)
    ref = _reference((shape, 71, False, 5), vol, p, monkeypatch)
    assert ref["prezero"] == 2
    pipe = _pipe(shape)
    try:
        for order, want in (("auto", 2), ((2, 1, 0, 3, 4), 2), ((0, 1, 3, 4, 2), 0), ((2, 1, 3, 4, 0), 0)):
            assert order == "auto" or _fits(order)
            monkeypatch.delenv("NELLIE_PREZERO", raising=False)
            _env(monkeypatch, order)
            got = _frame(pipe, vol, p)
            assert got["prezero"] == want, (order, got["prezero"])
            _same(got, ref, f"order {order}")
            monkeypatch.setenv("NELLIE_PREZERO", "0")
            got = _frame(pipe, vol, p)
            assert got["prezero"] == 0
            _same(got, ref, f"order {order}, dense")
        monkeypatch.setenv("NELLIE_PREZERO", "0")
        _env(monkeypatch, "sigma")
        got = _frame(pipe, vol, p)
        assert got["prezero"] == 0 and got["order"] is None
        _same(got, ref, "sigma, dense")
    finally:
        pipe.close()


ORDERS_5 = ["auto", (2, 1, 0, 3, 4), (1, 0, 3, 2, 4), (0, 2, 1, 4, 3)]


def test_an_empty_scale_while_later_scales_are_pending(hip, monkeypatch):
    """frob_thresh_division = 0.03 puts the threshold of scale 1 above its largest norm (worked out with the float64-free restatement of
    filtering.py: threshold / max norm per scale = 0.038, 0.022, 0.030, 0.022, 0.022), so its mask is empty while scales 2 and 3 wait: the
    chain flags it (NL_CF_EMPTY = 256), the frame is redone in sigma order and equals the sigma-order frame, on a context that goes on."""
    from nellie_amd.synthetic import ISO_01
    shape = (24, 80, 136)
    vol, p = _volume(shape, 61), _params(ISO_01, frob_thresh_division=0.03)
    ref = _reference((shape, 61, "empty"), vol, p, monkeypatch)
    assert ref["fallbacks"] == 1 and ref["flags"][0] & 256 and not any(f & 256 for f in ref["flags"][1:]), ref["flags"]
    assert ref["trace"][0][5] and not any(t[5] for t in ref["trace"][1:])              # skipped: scale 1 alone
    plain = _params(ISO_01)
    ref_plain = _reference((shape, 61, "plain"), vol, plain, monkeypatch)
    pipe = _pipe(shape)
    try:
        for order in ORDERS_5:
            _env(monkeypatch, order)
            got = _frame(pipe, vol, p)
            assert pipe.chain_fallbacks == 1 and got["order"] is not None
            pipe.chain_fallbacks = 0
            _same(got, ref, f"order {order}")
            _same(_frame(pipe, vol, plain), ref_plain, f"the frame after, order {order}")
            assert pipe.chain_fallbacks == 0
    finally:
        pipe.close()


def test_an_all_zero_frame(hip, monkeypatch):
    from nellie_amd.synthetic import ISO_01
    shape = (24, 80, 136)
    vol, p = np.zeros(shape, np.float32), _params(ISO_01)
    ref = _reference((shape, "zeros"), vol, p, monkeypatch)
    assert ref["n_positive"] == 0 and not ref["frangi"].any()
    plain_vol = _volume(shape, 71)
    ref_plain = _reference((shape, 71, False, 5), plain_vol, p, monkeypatch)
    pipe = _pipe(shape)
    try:
        for order in ORDERS_5:
            _env(monkeypatch, order)
            _same(_frame(pipe, vol, p), ref, f"order {order}")
            _same(_frame(pipe, plain_vol, p), ref_plain, f"the frame after, order {order}")
    finally:
        pipe.close()


@pytest.mark.parametrize("scale", [0, 1, 2, 4])
def test_a_bracket_miss_in_a_delayed_scale(hip, scale, monkeypatch):
    """The prediction of ONE scale pushed off by 50 %: its walk -- delayed behind others in these orders -- misses the bracket
    (NL_CF_MISS = 128), the frame is redone synchronously and equals the sigma-order frame."""
    from nellie_amd.synthetic import ISO_01
    shape = (24, 80, 136)
    vol, p = _volume(shape, 71), _params(ISO_01)
    ref = _reference((shape, 71, False, 5), vol, p, monkeypatch)
    pipe = _pipe(shape, _chain_test_scales={scale: 1.5})
    try:
        for order in ["auto", (2, 1, 0, 3, 4), (1, 2, 0, 4, 3)]:
            _env(monkeypatch, order)
            got = _frame(pipe, vol, p)
            assert pipe.chain_fallbacks == 1 and [bool(f & 128) for f in got["flags"]] == [k == scale for k in range(5)], got["flags"]
            pipe.chain_fallbacks = 0
            got["flags"] = ref["flags"]             # (the redone frame's flags are the miss; everything else is the sigma-order frame)
            _same(got, ref, f"order {order}")
    finally:
        pipe.close()


def test_a_queue_overflow_in_the_first_walked_scale(hip, monkeypatch):
    """The dome texture of test_one_pass_queue_overflow_falls_back fills more than a queue region holds: whichever scale is walked first
    -- inside no mask at all -- reports it (NL_CF_OVERFLOW = 32), the frame is redone, same bits as in sigma order."""
    from nellie_amd.synthetic import ISO_01
    shape = (64, 64, 128)
    z, y, x = np.mgrid[:shape[0], :shape[1], :shape[2]]
    vol = np.random.default_rng(3).normal(100, 0.02, shape).astype(np.float32)
    vol += (50.0 * (np.abs(np.sin(0.15 * x)) + np.abs(np.sin(0.15 * y)) + np.abs(np.sin(0.15 * z)))).astype(np.float32)
    p = _params(ISO_01)
    ref = _reference((shape, "domes"), vol, p, monkeypatch)
    assert any(f & 32 for f in ref["flags"]), "the texture was meant to overflow a queue region"
    pipe = _pipe(shape)
    try:
        for order in ["auto", (2, 1, 0, 3, 4), (0, 2, 1, 4, 3)]:
            _env(monkeypatch, order)
            got = _frame(pipe, vol, p)
            assert got["order"] is not None and any(f & 32 for f in got["flags"]), (got["order"], got["flags"])
            if got["order"][0] == 0:               # (the scale the texture was built to overflow, inside no mask as in sigma order)
                assert got["flags"][0] & 32
            got["flags"] = ref["flags"]             # (which scales overflow depends on the masks walked before them: the frame does not)
            _same(got, ref, f"order {order}")
    finally:
        pipe.close()


def test_an_order_that_does_not_fit_is_refused(hip, monkeypatch):
    from nellie_amd.synthetic import ISO_01
    shape = (24, 80, 136)
    vol, p = _volume(shape, 71), _params(ISO_01)
    ref = _reference((shape, 71, False, 5), vol, p, monkeypatch)
    pipe = _pipe(shape)
    try:
        for bad, msg in (("4,1,2,3,5", "three Gaussian volumes"), ("1,5,2,3,4", "three Gaussian volumes"), ("1,2,3", "permutation"),
                         ("1,1,2,3,4", "permutation"), ("fastest", "expected auto, sigma or a permutation")):
            _env(monkeypatch, bad)
            with pytest.raises(ValueError, match=msg):
                pipe.filter(vol, p)
            _env(monkeypatch, (2, 1, 0, 3, 4))
            _same(_frame(pipe, vol, p), ref, f"the frame after {bad}")
    finally:
        pipe.close()


def test_frames_outside_the_fused_step_keep_sigma_order(hip, monkeypatch):
    """The two-kernel cascade step needs the third volume, an image has no walk, a small frame runs its next step ahead: an explicit
    order is not consulted there."""
    from nellie_amd import pipeline as pl
    from nellie_amd.synthetic import ISO_01
    shape = (24, 80, 136)
    vol, p = _volume(shape, 71), _params(ISO_01)
    ref = _reference((shape, 71, False, 5), vol, p, monkeypatch)
    _env(monkeypatch, (2, 1, 0, 3, 4))
    for fused, ahead in (("0", "0"), ("1", "1"), ("1", None)):
        monkeypatch.setenv("NELLIE_GAUSS_FUSED", fused)
        pipe = pl.FramePipeline(shape)
        pipe._chain_ahead_env = ahead
        try:
            got = _frame(pipe, vol, p)
            assert got["order"] is None and pipe.chain_fallbacks == 0
            _same(got, ref, f"fused {fused}, ahead {ahead}")
        finally:
            pipe.close()
