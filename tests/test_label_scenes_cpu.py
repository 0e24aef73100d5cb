"""The scenes of label_scenes.py, checked without a GPU: every scene reaches the path, the stage and the kernel change-over it is
built for (run counts against the scratch capacity n // 2, by a scipy restatement of the pipeline's stages), and the oracle the
device is held to equals that scipy pipeline on every scene."""
import functools

import numpy as np
import pytest

import label_scenes as ls

ndi = pytest.importorskip("scipy.ndimage")


def _n_labels(mask, min_area=1, fill=True):
    return ls.scipy_labels(mask, min_area, fill)[1]


def test_runs_counts_maximal_x_runs():
    m = np.array([[[1, 1, 0, 1], [0, 0, 0, 0]], [[1, 0, 1, 0], [1, 1, 1, 1]]], bool)
    assert ls.runs(m) == 2 + 0 + 2 + 1
    assert ls.runs(~m) == 1 + 1 + 2 + 0


@pytest.mark.parametrize("shape,fg,cap,other,labels", [((6, 9, 5), 162, 135, 108, 2), ((4, 7, 131), 1848, 1834, 1820, 65),
                                                       ((2, 3, 4097), 12294, 12291, 12288, 2048)])
def test_overflow_fg_overflows_at_the_first_labelling_only(shape, fg, cap, other, labels):
    m = ls.overflow_fg(shape)
    assert ls.cap(m) == cap
    for fill in (True, False):
        for min_area in (1, 2, 3, 5):
            assert ls.stages(m, min_area, fill) == (other, fg, other)       # the comb's background, the comb, the comb inverted by the majority filter
            assert ls.expected_path(m, min_area, fill) == ls.PATH_OVERFLOW
    assert fg > cap > other
    assert _n_labels(m) == labels


def test_overflow_bg_overflows_at_the_hole_fill_and_the_fill_matters():
    (shape, lo, size), wide = ls.OVERFLOW_BG_CASES
    m = ls.overflow_bg(shape, lo, size)
    expect = np.zeros(shape, bool)
    expect[..., 1::2] = True
    expect[3:8, 3:8, 2:7] = True
    expect[4:7, 4:7, 3:6] = False
    assert np.array_equal(m, expect)
    assert ls.cap(m) == 1080
    assert ls.stages(m, 1, True)[:2] == (1134, 885)
    mw = ls.overflow_bg(*wide)
    assert mw.shape[2] >= 129
    for mask in (m, mw):
        c = ls.cap(mask)
        assert ls.runs(~mask) > c
        for min_area in (1, 2, 3, 5):
            bg, first, last = ls.stages(mask, min_area, True)
            assert bg > c and first <= c and last <= c                      # only the hole fill overflows ...
            assert ls.expected_path(mask, min_area, True) == ls.PATH_OVERFLOW
            bg, first, last = ls.stages(mask, min_area, False)
            assert first <= c and last <= c                                 # ... and without it nothing does
            assert ls.expected_path(mask, min_area, False) == ls.PATH_RUNS
            # the cavity survives the majority filter: a labelling that lost the fill gives another answer
            assert not np.array_equal(ls.scipy_labels(mask, min_area, True)[0], ls.scipy_labels(mask, min_area, False)[0])


@pytest.mark.parametrize("shape", ls.AT_CAPACITY_EVEN_SHAPES)
def test_at_capacity_even_fills_the_scratch_exactly(shape):
    m = ls.at_capacity_even(shape)
    c = ls.cap(m)
    assert m.size % 2 == 0 and ls.runs(m) == c and ls.runs(~m) == c
    for fill in (True, False):
        for min_area in (1, 2, 3, 5):
            bg, first, last = ls.stages(m, min_area, fill)
            assert (bg, first) == (c, c) and last <= c
            assert ls.expected_path(m, min_area, fill) == ls.PATH_RUNS
    assert _n_labels(m) > 0


def test_at_capacity_odd_straddles_the_capacity_by_one_run():
    over, at = ls.at_capacity_odd(ls.AT_CAPACITY_ODD_SHAPE, 1), ls.at_capacity_odd(ls.AT_CAPACITY_ODD_SHAPE, 0)
    c = ls.cap(over)
    assert ls.runs(over) == c + 1 and ls.runs(at) == c
    assert int((over ^ at).sum()) == 1                                      # one tooth apart
    for fill in (True, False):
        for min_area in (1, 5):
            assert ls.expected_path(over, min_area, fill) == ls.PATH_OVERFLOW
            assert ls.expected_path(at, min_area, fill) == ls.PATH_RUNS
            assert ls.stages(over, min_area, fill)[0] <= c and ls.stages(over, min_area, fill)[2] <= c
    assert _n_labels(over) > 0 and _n_labels(at) > 0


def _next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def test_ruler_widths_select_every_change_over():
    wpr = {nx: (nx + 63) // 64 for nx in ls.RULER_WIDTHS}
    # rl_count_wave_kernel's P (rows of up to 64 words), 1 .. 64
    assert [_next_pow2(wpr[nx]) for nx in (64, 65, 129, 257, 513, 1025, 2049)] == [1, 2, 4, 8, 16, 32, 64]
    assert _next_pow2(3) == 4 and wpr[129] == 3 and wpr[2049] == 33         # ... with words that are no power of two
    assert (wpr[1920], wpr[1921]) == (30, 31)                               # staged / unstaged run emission
    assert (wpr[4096], wpr[4097]) == (64, 65)                               # one wave per row / one thread per row
    assert 65535 in ls.RULER_WIDTHS and 65536 in ls.RULER_WIDTHS and 65537 in ls.RULER_WIDTHS
    assert max(3 * 4 * nx for nx in ls.RULER_WIDTHS) == 786444


@pytest.mark.parametrize("nx", ls.RULER_WIDTHS)
def test_ruler_contents(nx):
    m = ls.ruler(nx)
    assert m.shape == (3, 4, nx)
    assert m[1, 0].all()                                                    # one run [0, nx): xe == nx
    assert m[2, 3, 0] and not m[2, 3, 1] and m[2, 3, nx - 1] and not m[2, 3, nx - 2]
    last = 64 * ((nx - 1) // 64)
    for b in {64, last}:
        if 0 < b < nx:
            assert m[0, 3, b - 1] and not m[0, 3, b]                        # a run that ends with the word
            assert m[2, 3, b] and not m[2, 3, b - 1]                        # a run that starts with the word
            assert m[2, 0, b - 1] and m[2, 0, b]                            # a run across the boundary
    assert ls.runs(m[0, 0, max(nx - 200, 0):]) == (min(nx, 200) + 1) // 2   # the comb
    filled = ndi.binary_fill_holes(m)
    assert not m[1, 2, nx - 1] and not filled[1, 2, nx - 1]                 # open through x = nx - 1
    if nx >= 90:
        assert not m[1, 1:3, 60:71].any() and filled[1, 1:3, 60:71].all()   # closed across a word boundary
        assert not m[1, 1, nx - 10:nx - 1].any() and filled[1, 1, nx - 10:nx - 1].all() and m[1, 1, nx - 1]
    c = ls.cap(m)
    for fill, min_area in ((True, 1), (False, 3)):
        if nx <= 65535:
            assert max(ls.stages(m, min_area, fill)) < c
        assert ls.expected_path(m, min_area, fill) == (ls.PATH_RUNS if nx <= 65535 else ls.PATH_WIDE)
        assert _n_labels(m, min_area, fill) > 0


@functools.lru_cache(maxsize=None)
def _topology():
    return ls.topology_cases()


def test_topology_scenes_fit_and_stay_on_the_run_path():
    for name, m, min_areas in _topology():
        assert m.size <= 200_000 and m.shape[1] >= 65, name
        assert m[:, 31].any() and m[:, 32].any(), name                       # a 32-row band boundary inside the scene
        for fill in (True, False):
            for min_area in min_areas:
                assert ls.expected_path(m, min_area, fill) == ls.PATH_RUNS, name
        assert len({_n_labels(m, a, f) for a in min_areas for f in (True, False)}) > 1, name    # the parameters matter


def _components(mask, conn26=True):
    return ndi.label(mask, structure=np.ones((3, 3, 3)) if conn26 else None)


def test_combs_meet_only_in_the_last_plane_and_row():
    m = ls.comb_last_plane()
    assert _components(m)[1] == 1 and _components(m[:-1])[1] == 12
    m = ls.comb_last_row()
    assert _components(m)[1] == 1 and _components(m[:, :-1])[1] == 3


def test_serpentine_is_one_path():
    m = ls.serpentine()
    assert _components(m)[1] == 1
    path = m.copy()
    path[:, :, :8] = False
    # a 1-voxel path: two ends, no voxel with more neighbours than a turn gives it (four), and cutting it anywhere splits it
    nb = ndi.convolve(path.astype(np.int32), np.ones((3, 3, 3), np.int32), mode="constant") - 1
    assert nb[path].max() <= 4 and int((nb[path] == 1).sum()) == 2
    assert {path[z].any() for z in range(m.shape[0])} == {True}
    cut = m.copy()
    cut[4, 30, 15] = False
    assert m[4, 30, 15] and _components(cut)[1] == 2
    assert ls.critical_min_areas(m) == (1, int(m.sum()), int(m.sum()) + 1)


def test_shells_and_cavities():
    m = ls.nested_shells()
    filled = ndi.binary_fill_holes(m)
    assert _components(m)[1] == 2 and _components(~m, conn26=False)[1] == 3   # outside, between the shells, the inner cavity
    assert filled[1:19, 24:42, 2:20].all() and int(filled.sum()) == 18 ** 3
    m = ls.pierced()
    filled = ndi.binary_fill_holes(m)
    assert filled[5:8, 30:33, 6:9].all() and not m[5:8, 30:33, 6:9].any()     # reached diagonally only: a hole
    assert not filled[5:8, 51:54, 6:9].any()                                  # reached through a face: no hole
    assert not filled[4, 29, 0:6].any() and not filled[6, 52, 0:6].any()      # the tunnels themselves stay open
    m = ls.face_boxes()
    filled = ndi.binary_fill_holes(m)
    assert _components(m)[1] == 12
    assert int((filled & ~m).sum()) == 6 * 27                                 # the six boxes one voxel inside, and only they
    assert int((~m).sum()) - int((~filled).sum()) == 6 * 27
    cav, ncav = _components(~m, conn26=False)
    assert ncav == 13                                # the outside, six cavities, and six open boxes: background of their own ON a face


def test_fan_meets_several_components_of_the_plane_below():
    m = ls.fan()
    assert _components(m)[1] == 1
    below, nb = ndi.label(m[2], structure=np.ones((3, 3)))
    sheet, ns = ndi.label(m[3], structure=np.ones((3, 3)))
    assert ns == 1 and nb >= 3
    touched = np.unique(below[ndi.binary_dilation(m[3], structure=np.ones((3, 3))) & m[2]])
    assert len(touched) >= 3
    above, na = ndi.label(m[6], structure=np.ones((3, 3)))
    assert na >= 3 and ndi.label(m[5], structure=np.ones((3, 3)))[1] == 1


def test_specks_fill_the_area_table_and_straddle_min_area():
    m = ls.specks()
    lab, n = _components(m)
    areas = np.bincount(lab.ravel())[1:]
    small = areas[areas <= 3]
    assert len(small) >= 5000 and set(small.tolist()) == {1, 2, 3}
    assert ls.speck_window_components(m, 4096) > 256                          # more roots than rl_area_kernel's table holds
    # two different objects inside one 64-voxel row segment (area_count_kernel's loop over distinct roots)
    seg = lab[0, 0, 64:128]
    assert len(np.unique(seg[seg > 0])) >= 2
    big = sorted(areas[areas > 3].tolist())
    a0 = ls.SPECKS_MIN_AREA
    assert big == [a0 - 1] * 4 + [a0] * 3 + [a0 + 1] * 3
    for k in np.flatnonzero(areas > 3):
        assert len(np.unique(np.argwhere(lab == 1 + k)[:, 0])) == 2           # over two planes
    assert [_n_labels(m, a) for a in (1, 2, 3, a0, a0 + 1, a0 + 2)] == [10, 10, 10, 6, 3, 0]


def _all_scenes():
    for name, m, min_areas, _, _ in ls.capacity_cases():
        yield name, m, min_areas
    for nx in ls.RULER_WIDTHS:
        yield "ruler-%d" % nx, ls.ruler(nx), (1, 3)
    yield from _topology()
    yield "ordinary", ls.ordinary((9, 14, 13)), (1, 5)


def test_oracle_equals_the_scipy_pipeline_on_every_scene():
    """the reference of test_hip_label_paths.py, verified before the device is held to it"""
    checked = 0
    for name, m, min_areas in _all_scenes():
        fr = ls.frangi_of(m)
        assert np.array_equal(fr > ls.THR, m), name
        for fill in (True, False):
            for min_area in min_areas:
                ref, n = ls.scipy_labels(m, min_area, fill)
                got = ls.oracle_labels(fr, min_area, fill)
                assert got.dtype == np.int32 and np.array_equal(got, ref), (name, min_area, fill)
                assert int(got.max()) == n
                checked += 1
    assert checked >= 100
