"""CPU checks of the dtype matrix (tests/dtype_cases.py): the references the GPU file compares against are themselves right, the
edge values test what they claim to, and the binding refuses what it cannot pass on faithfully."""
from fractions import Fraction

import numpy as np
import pytest

import dtype_cases as dc
from nellie_amd import hipnative
from nellie_amd.segmentation.labelling import Label


def test_dtype_list_is_the_bindings():
    assert dc.ALL == list(hipnative.DTYPE_CODES) and len(set(dc.ALL)) == len(dc.ALL)
    assert not set(dc.HOST_CAST) & set(dc.ALL)
    assert sorted(hipnative.DTYPE_CODES.values()) == list(range(len(dc.ALL)))


@pytest.mark.parametrize("dtype", dc.INTEGERS, ids=dc.ids(dc.INTEGERS))
def test_numpy_cast_is_the_exact_float32(dtype):
    """numpy's astype(float32) = exact_f32 (integer arithmetic, ties to even), bit for bit, on every integer edge value."""
    v = dc.edge_values(dtype)
    want = np.array([dc.exact_f32(int(x)) for x in v], np.float32)
    assert dc.same_bits(v.astype(np.float32), want)
    rnd = dc.random_values(dtype, 500, np.random.default_rng(1))
    assert dc.same_bits(rnd.astype(np.float32), np.array([dc.exact_f32(int(x)) for x in rnd], np.float32))


def test_exact_f32_on_fractions_denormals_and_overflow():
    f32 = np.float32
    assert dc.exact_f32(Fraction(1, 3)) == f32(1) / f32(3)
    assert dc.exact_f32(Fraction(1, 2 ** 149)) == np.nextafter(f32(0), f32(1))
    assert dc.exact_f32(Fraction(1, 2 ** 150)) == 0 and dc.exact_f32(Fraction(3, 2 ** 150)) == f32(2.0 ** -148)      # ties to even
    assert dc.exact_f32(-(2 ** 128)) == -np.inf and dc.exact_f32(2 ** 128 - 2 ** 103) == np.inf
    assert dc.exact_f32(2 ** 128 - 2 ** 103 - 1) == np.finfo(f32).max
    assert np.signbit(dc.exact_f32(Fraction(-1, 2 ** 151))) and dc.exact_f32(Fraction(-1, 2 ** 151)) == 0
    v = dc.edge_values(np.float64)
    v = v[np.isfinite(v)]
    with np.errstate(over="ignore", under="ignore"):
        got = v.astype(f32)
    want = np.array([dc.exact_f32(Fraction(float(x))) for x in v], f32)
    want = np.where((v == 0) & np.signbit(v), f32(-0.0), want)          # a Fraction has no negative zero
    assert dc.same_bits(got, want)


def test_double_rounding_witnesses_differ():
    """The 64-bit values meant to catch a conversion through float64 do give another float32 that way."""
    witnesses = {np.dtype(np.uint64): [2 ** 63 + 2 ** 39 + 1], np.dtype(np.int64): [2 ** 62 + 2 ** 38 + 1, -(2 ** 62 + 2 ** 38 + 1)]}
    for dtype, vals in witnesses.items():
        held = set(int(x) for x in dc.edge_values(dtype))
        for v in vals:
            assert v in held
            assert dc.exact_f32(v) != dc.exact_f64_then_f32(v), v
            assert np.array([v], dtype=object).astype(dtype).astype(np.float32)[0] == dc.exact_f32(v)
    assert dc.exact_f32(2 ** 63 + 2 ** 39 + 1) == np.float32(2.0 ** 63 + 2.0 ** 40) and dc.exact_f64_then_f32(2 ** 63 + 2 ** 39 + 1) == np.float32(2.0 ** 63)
    assert float(2 ** 53 + 1) != 2 ** 53 + 1                            # what the integer threshold cases rest on


@pytest.mark.parametrize("dtype", dc.ALL, ids=dc.ids(dc.ALL))
def test_frames_hold_every_edge_value(dtype):
    for shape in ((3, 5, 7), (4, 7, 129), (33, 70)):
        for finite in (False, True):
            f = dc.frame(dtype, shape, 3, finite)
            assert f.dtype == dtype and f.shape == shape and f.flags.c_contiguous
            edges = dc.edge_values(dtype, finite)
            assert len(edges) >= (3 if dtype.kind == "u" else 5)       # unsigned: min is 0
            for e in edges:
                assert any(dc.same_bits(f.reshape(-1)[i:i + 1], np.array([e], dtype)) for i in np.nonzero((f.reshape(-1) == e) | (e != e))[0]), e
            for i in dc.anchors(shape):
                assert any(dc.same_bits(f.reshape(-1)[i:i + 1], np.array([e], dtype)) for e in edges)
            if finite and dtype.kind == "f":
                with np.errstate(under="ignore"):
                    assert np.isfinite(f.astype(np.float32)).all()
    info = np.iinfo(dtype) if dtype.kind in "iu" else np.finfo(dtype)
    e = dc.edge_values(dtype)
    assert info.min in e and info.max in e and 0 in e and 1 in e
    if dtype.kind == "f":
        assert np.isnan(e).any() and np.isinf(e).sum() == 2 and (np.signbit(e) & (e == 0)).any()
    if dtype == np.uint64:
        assert (e >= 2 ** 63).sum() >= 3


def test_strided_views_and_host_casts():
    a = dc.frame(np.uint16, (3, 5, 7), 0)
    for _, v in dc.strided_views(a):
        assert not v.flags.c_contiguous and np.array_equal(v, a)
    for d in dc.HOST_CAST:
        f = dc.host_cast_frame(d, (3, 5, 7), 0)
        assert f.dtype == d and d not in hipnative.DTYPE_CODES


# --------------------------------------------------------------------------------------------- the binding's casts
def _cast(a, dtype=np.int32):
    a = np.asarray(a)
    return hipnative._frame_array(a, a.shape, "branch label", "object", dtype)


@pytest.mark.parametrize("dtype", dc.ALL + [np.dtype(np.float16), np.dtype(bool)], ids=dc.ids(dc.ALL) + ["f2", "b1"])
def test_frame_array_keeps_every_value_that_fits(dtype):
    vals = [0, 1, 100] + ([-1, -100] if dtype.kind in "if" else []) + ([2 ** 31 - 1] if dtype.itemsize >= 4 and dtype != np.float32 else []) \
        + ([-2 ** 31] if dtype in (np.int32, np.int64, np.float64) else [])
    a = np.array(vals, dtype=object).astype(dtype) if dtype != bool else np.array([False, True, True])
    got = _cast(a)
    assert got.dtype == np.int32 and got.flags.c_contiguous and [int(x) for x in got] == [int(x) for x in a]
    assert _cast(np.zeros(0, dtype)).size == 0


@pytest.mark.parametrize("value,dtype", [(2 ** 31 + 5, np.uint32), (2 ** 31, np.int64), (2 ** 40 + 3, np.int64), (-2 ** 31 - 1, np.int64),
                                         (2 ** 63 + 1, np.uint64), (2 ** 40 + 3, np.uint64), (1.5, np.float32), (-0.25, np.float64),
                                         (np.nan, np.float32), (np.inf, np.float64), (-np.inf, np.float32), (2.0 ** 31, np.float64),
                                         (-2.0 ** 31 - 1, np.float64), (3e9, np.float32), (np.nan, np.float16), (0.5, np.float16)])
def test_frame_array_refuses_a_cast_that_changes_a_value(value, dtype):
    a = np.zeros((2, 3), dtype)
    a[1, 2] = value
    keep = a.copy()
    with pytest.raises(ValueError, match="branch label") as e:
        _cast(a)
    shown = a[1, 2].item()                              # the message names the array and the offending value
    assert (str(int(shown)) if np.isfinite(shown) and shown == int(shown) else repr(shown)) in str(e.value)
    assert dc.same_bits(a, keep)


def test_frame_array_scans_nothing_when_the_dtype_matches(monkeypatch):
    a = np.arange(6, dtype=np.int32).reshape(2, 3)
    monkeypatch.setattr(hipnative, "_refuse_lossy_cast", lambda *k: (_ for _ in ()).throw(AssertionError("scanned")))
    assert _cast(a) is a                                # the int32 fast path: no scan, no copy
    f = hipnative._frame_array(np.ones((2, 3)), (2, 3), "distance", "object", np.float32)        # float targets round, as numpy does
    assert f.dtype == np.float32
    with pytest.raises(TypeError):
        hipnative._frame_array(np.ones((2, 3), np.complex64), (2, 3), "intensity", "object")


# --------------------------------------------------------------------------------------------- Label's thresholds
def _device_mask(orig, eff):
    """What the library computes from Label._effective_threshold's answer: an int is compared as integers of the image's type
    (nl_label_intensity_mask_int), a float in float64 on the converted image (intensity_mask_kernel)."""
    if isinstance(eff, int):
        assert orig.dtype.kind in "iu" and orig.dtype.itemsize == 8 and np.iinfo(orig.dtype).min <= eff <= np.iinfo(orig.dtype).max
        return np.array([int(v) > eff for v in orig.reshape(-1)]).reshape(orig.shape)
    assert isinstance(eff, float)
    with np.errstate(invalid="ignore"):
        return orig.astype(np.float64) > eff


@pytest.mark.parametrize("dtype", dc.ALL, ids=dc.ids(dc.ALL))
def test_effective_threshold_compares_as_numpy_does(dtype):
    orig = dc.frame(dtype, (3, 5, 7), 11)
    forms = set()
    for name, t in dc.thresholds(dtype):
        eff = Label._effective_threshold(orig, t)
        assert np.array_equal(_device_mask(orig, eff), dc.mask_reference(orig, t)), (name, eff)
        forms.add(type(t))
    assert forms == set(dc.THRESHOLD_FORMS)


def test_integer_threshold_beyond_2_53():
    """The issue's case: numpy says True, a comparison in float64 says False."""
    a = np.array([2 ** 53 + 1], np.uint64)
    assert dc.mask_reference(a, 2 ** 53)[0] and not (a.astype(np.float64) > float(2 ** 53))[0]
    for dtype in (np.uint64, np.int64):
        a = np.array([2 ** 53 + 1, 2 ** 53, 2 ** 53 + 2], dtype)
        for t in (2 ** 53, np.int64(2 ** 53), 2 ** 53 + 1):
            eff = Label._effective_threshold(a, t)
            assert eff == int(t) and type(eff) is int
            assert np.array_equal(_device_mask(a, eff), dc.mask_reference(a, t))
        assert Label._effective_threshold(a, -1 if dtype == np.uint64 else -2 ** 63 - 1) == -np.inf
        assert Label._effective_threshold(a, 10 ** 400) == np.inf
        assert type(Label._effective_threshold(a, 2.0 ** 53)) is float
    assert Label._effective_threshold(np.zeros(1, np.uint16), 7) == 7.0 and type(Label._effective_threshold(np.zeros(1, np.uint16), 7)) is float
