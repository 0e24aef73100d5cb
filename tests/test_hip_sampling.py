"""The single-field sampling entry points on their own (csrc/nellie_sample.hip), against numpy on small volumes: whole frames only reach
them through the pair path of a scale, and nl_sample_minmax / nl_sample_hist only on fall-back paths.  Shapes: 130 columns are two mask
words and a tail, 37 rows are odd; the strides run from every voxel to one point per axis."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPE = (7, 37, 130)
STRIDES = [(1, 1, 1), (2, 3, 5), (3, 7, 64), (9, 40, 200)]


def _volume(shape, seed):
    """float32, about half the values <= 0: negatives, exact zeros, and a positive first voxel (the one-point lattice samples it)."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(shape).astype(np.float32)
    v[rng.random(shape) < 0.1] = 0.0
    v.flat[0] = np.float32(0.75)
    return v


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _context(hipnative, vols, shape=SHAPE, **kw):
    ctx = hipnative.Context(shape, **kw)
    for field, vol in vols.items():
        ctx.planes_put(field, 0, shape[0], vol)
    return ctx


@pytest.fixture(scope="module")
def whole(hip):
    from nellie_amd import hipnative
    vols = {hipnative.FIELD_GAUSS: _volume(SHAPE, 1), hipnative.FIELD_FRANGI: _volume(SHAPE, 2)}
    ctx = _context(hipnative, vols)
    yield ctx, vols
    ctx.close()


def _check_against(ctx, field, strides, samples):
    """Every single-field entry point on the lattice `strides` against the expected samples (in lattice order)."""
    samples = np.ascontiguousarray(samples, dtype=np.float32).ravel()
    pos = samples[samples > 0]
    assert np.array_equal(_bits(ctx.sample_gather(field, strides)), _bits(samples))
    assert np.array_equal(_bits(np.sort(ctx.sample_gather_positive(field, strides))), _bits(np.sort(pos)))
    mn, mx, n = ctx.sample_minmax(field, strides)
    assert n == pos.size
    rmn, rmx, rn, counts, edges, valid = ctx.sample_range_hist(field, strides, nbins=256)
    assert rn == pos.size
    if pos.size == 0:
        assert valid == 0
        return
    assert (mn, mx) == (pos.min(), pos.max()) and (rmn, rmx) == (pos.min(), pos.max())
    want_counts, want_edges = np.histogram(pos, bins=256)
    assert valid == 1
    assert np.array_equal(_bits(edges), _bits(want_edges.astype(np.float32)))
    assert np.array_equal(counts, want_counts)
    assert np.array_equal(ctx.sample_hist(field, strides, edges), want_counts)


@pytest.mark.parametrize("strides", STRIDES)
@pytest.mark.parametrize("field_name", ["FIELD_GAUSS", "FIELD_FRANGI"])
def test_whole_volume_lattice(whole, field_name, strides):
    from nellie_amd import hipnative
    ctx, vols = whole
    field = getattr(hipnative, field_name)
    sz, sy, sx = strides
    _check_against(ctx, field, strides, vols[field][::sz, ::sy, ::sx])


def test_no_positive_sample_and_infinite_range(hip):
    from nellie_amd import hipnative
    f = hipnative.FIELD_FRANGI
    v = -np.abs(_volume(SHAPE, 3))                   # all <= 0, zeros included
    ctx = _context(hipnative, {f: v})
    for strides in STRIDES:
        mn, mx, n, counts, edges, valid = ctx.sample_range_hist(f, strides)
        assert (valid, n) == (0, 0) and not counts.any()
        assert ctx.sample_minmax(f, strides)[2] == 0 and ctx.sample_gather_positive(f, strides).size == 0
    v = _volume(SHAPE, 4)
    v[4, 6, 10] = np.inf                             # on the lattice (2, 3, 5), off the lattice (3, 7, 64)
    ctx.planes_put(f, 0, SHAPE[0], v)
    assert ctx.sample_range_hist(f, (2, 3, 5))[5] == 2
    assert ctx.sample_range_hist(f, (1, 1, 1))[5] == 2
    assert ctx.sample_range_hist(f, (3, 7, 64))[5] == 1
    ctx.close()


# ---- a slab: local planes 3..7 of a 12-plane global volume, owning global planes 4, 5 and 6 --------------------------------------
GNZ, GZ0, NZL, OWN = 12, 3, 5, (1, 4)
G_LO, G_HI = GZ0 + OWN[0], GZ0 + OWN[1]


@pytest.fixture(scope="module")
def slab(hip):
    from nellie_amd import hipnative
    gvols = {hipnative.FIELD_GAUSS: _volume((GNZ,) + SHAPE[1:], 5), hipnative.FIELD_FRANGI: _volume((GNZ,) + SHAPE[1:], 6)}
    ctx = _context(hipnative, {f: g[GZ0:GZ0 + NZL] for f, g in gvols.items()}, shape=(NZL,) + SHAPE[1:], gz0=GZ0, gnz=GNZ, own=OWN)
    yield ctx, gvols
    ctx.close()


@pytest.mark.parametrize("sz,planes", [(2, [4, 6]), (5, [5]), (8, [])])
@pytest.mark.parametrize("field_name", ["FIELD_GAUSS", "FIELD_FRANGI"])
def test_slab_lattice_samples_owned_global_planes(slab, field_name, sz, planes):
    """Lattice planes are GLOBAL z = k * sz; a slab contributes those among its owned planes."""
    from nellie_amd import hipnative
    ctx, gvols = slab
    field = getattr(hipnative, field_name)
    for sy, sx in ((1, 1), (3, 5)):
        lattice = gvols[field][::sz, ::sy, ::sx]
        want = lattice[[p // sz for p in planes]] if planes else lattice[:0]
        assert [p for p in range(0, GNZ, sz) if G_LO <= p < G_HI] == planes
        _check_against(ctx, field, (sz, sy, sx), want)
        if not planes:
            assert ctx.sample_gather(field, (sz, sy, sx)).size == 0


PLANE = SHAPE[1] * SHAPE[2]


@pytest.mark.parametrize("step", [1, 7, 1000, GNZ * PLANE + 1])
@pytest.mark.parametrize("offset", [0, 5, G_LO * PLANE + 1])
def test_slab_flat_samples(slab, offset, step):
    """flat[offset::step] of the GLOBAL volume, restricted to the indices inside the owned planes."""
    from nellie_amd import hipnative
    ctx, gvols = slab
    f = hipnative.FIELD_FRANGI
    idx = np.arange(offset, GNZ * PLANE, step)
    idx = idx[(idx >= G_LO * PLANE) & (idx < G_HI * PLANE)]
    want = gvols[f].ravel()[idx]
    assert np.array_equal(_bits(ctx.flat_sample_gather(f, offset, step)), _bits(want))
    assert np.array_equal(_bits(np.sort(ctx.flat_sample_gather_positive(f, offset, step))), _bits(np.sort(want[want > 0])))
    if want.size:
        out, n = np.empty(want.size, np.float32), C.c_int64(0)
        for name in ("nl_flat_sample_gather", "nl_flat_sample_gather_positive"):
            with pytest.raises(ValueError):
                ctx._call(name, f, offset, step, hipnative._ptr(out), want.size - 1, C.byref(n))


def test_frob_samples_from_a_warm_cache_equal_a_fresh_context(hip):
    """NL_FIELD_FROB keeps frob_sq of the lattice points per context: the second normalisation reads the cache the first one filled."""
    from nellie_amd import hipnative
    g = {hipnative.FIELD_GAUSS: _volume(SHAPE, 7)}
    spacing, strides, norms = (0.3, 0.1, 0.1), (2, 3, 5), [(1.0, 0.0), (3.5, 2.0)]

    def gather(ctx, norm):
        ctx.set_frob_norm(*norm)
        return ctx.sample_gather(hipnative.FIELD_FROB, strides)

    warm = _context(hipnative, g)
    warm.set_spacing(spacing)
    got = [gather(warm, norm) for norm in norms]
    warm.close()
    assert not np.array_equal(_bits(got[0]), _bits(got[1]))
    for norm, have in zip(norms, got):
        fresh = _context(hipnative, g)
        fresh.set_spacing(spacing)
        assert np.array_equal(_bits(gather(fresh, norm)), _bits(have))
        fresh.close()
