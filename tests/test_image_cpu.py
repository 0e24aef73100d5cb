"""CPU tests of the image level's test infrastructure and of what the package does for it without a device: the restatement
(tests/image_features_restatement.py) against every golden of the reference's Image bit for bit, the text of `features_image`, and
the block decomposition the device uses for wide groups -- items per group, base, k and n_block per item, the chain in ascending
block order, extremes merged by latest position -- against tests/node_features_restatement.py bit for bit at every k and L around
a multiple of numpy's buffer of 8192 elements.  That emulation is the argument that the device's bits are numpy's before a GPU
runs."""
import io
import warnings

import numpy as np
import pytest

import image_features_restatement as ir
import image_goldens as ig
import node_features_restatement as nr
import node_goldens as ng

NAMES = ig.names()
EDGES = [8192 * m + d for m in (1, 2, 3, 4) for d in (-1, 0, 1)]


def restated(h):
    own = ir.Image(h)
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        own.run()
    return own


def test_the_fixtures_cover_the_regimes():
    assert len(NAMES) == 12
    loaded = [ig.load(n) for n in NAMES]
    assert any(g["base"]["D"] == 2 for g in loaded) and any(g["base"]["skip_nodes"] for g in loaded) and any(g["components"]["no_t"] for g in loaded)
    assert any(g["base"]["D"] == 3 and len(set(g["base"]["spacing"])) > 1 for g in loaded)
    rows = [len(a) for a in ig.load("image_3d_empty_frame")["base"]["ref"]["coords"]]
    assert 0 in rows[1:-1] and rows[0] and rows[-1]
    for g in loaded:
        assert set(g["genuine"]) >= set(g["base"]["ref"]["stats_to_aggregate"]) and "branch_length" in g["genuine"] and "organelle_area" not in g["genuine"]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_reference(name):
    g = ig.load(name)
    own = restated(ig.double_of(g))
    ig.assert_same_image(own, g["ref"], g["base"])
    T = g["base"]["T"]
    assert len(own.aggregate_voxel_metrics) == T and [len(f) for f in own.aggregate_component_metrics] == [5] * T
    assert [len(f) for f in own.aggregate_branch_metrics] == [9] * T and all("reassigned_label" not in f for f in own.aggregate_branch_metrics)


def test_an_empty_frame_is_one_group_of_no_values():
    g = ig.load("image_3d_empty_frame")
    for level in ig.LEVELS:
        frame = g["ref"][f"agg_{level}"][2]
        for stat, keys in frame.items():
            assert all(np.isnan(keys[k]).all() for k in ("mean", "std_dev", "min", "max")) and keys["sum"].tobytes() == np.zeros((1, 1)).tobytes(), (level, stat)
        assert np.isfinite(g["ref"][f"agg_{level}"][1]["intensity" if level == "voxel" else list(frame)[0]]["sum"]).all()


@pytest.mark.parametrize("name", ["image_3d_empty_frame", "image_3d_skip_nodes", "image_2d"])
def test_the_image_table(name):
    """the text of features_image: one header, one row per frame (the empty one included: empty fields, and 0.0 for the sums),
    t and label as floats; the package's feature_frames gives the same array and header from the same object"""
    import pandas as pd
    from nellie_amd.feature_extraction.hierarchy import _disjoint_statistics, feature_frames
    g = ig.load(name)
    T, skip = g["base"]["T"], g["base"]["skip_nodes"]
    own = restated(ig.double_of(g))
    header, text = ir.feature_table(own)
    lines = text.splitlines()
    assert len(header) == 2 + (0 if skip else 20) + 55 + 45 + 25 and lines[0] == ",".join(header) and len(lines) == 1 + T
    assert header[:2] == ["t", "label"] and header[2] == ("linear_vel_mean" if skip else "divergence_mean") and header[-1] == "organelle_solidity_sum"
    assert len(set(header)) == len(header) and sum(line.startswith("t,label") for line in lines) == 1
    assert [line.split(",")[:2] for line in lines[1:]] == [[f"{t}.0", "0.0"] for t in range(T)]
    if name == "image_3d_empty_frame":
        fields = lines[3].split(",")
        assert all(f == ("0.0" if h.endswith("_sum") else "") for f, h in zip(fields[2:], header[2:]))
        assert all(f != "" for f, h in zip(lines[2].split(",")[2:], header[2:]) if h.startswith("intensity"))
    buf = io.StringIO()
    first = True
    for t in range(T):
        _disjoint_statistics(own, t)
    for t, frame, names in feature_frames(own, [np.zeros(1, np.int64)] * T):
        assert names == header and frame.shape == (1, len(header)) and frame.dtype == np.float64
        pd.DataFrame(frame, columns=names).to_csv(buf, index=False, mode="a", header=first)
        first = False
    assert buf.getvalue() == text


def test_disjoint_statistics_sees_the_component_aggregates():
    from types import SimpleNamespace
    from nellie_amd.feature_extraction.hierarchy import _disjoint_statistics
    level = SimpleNamespace(aggregate_node_metrics=[], aggregate_voxel_metrics=[{"a": {}}], aggregate_branch_metrics=[{"b": {}}],
                            aggregate_component_metrics=[{"c": {}}])
    _disjoint_statistics(level, 0)
    level.aggregate_component_metrics = [{"a": {}}]
    with pytest.raises(AssertionError, match="two levels"):
        _disjoint_statistics(level, 0)


# ---- the block decomposition -----------------------------------------------------------------------------------------------------
def test_items_and_geometry():
    off = np.concatenate([[0], np.cumsum([0, 1, 8192, 8193, 5, 20_011, 9000])])
    wide, items = ir.block_items(off, 1)
    assert wide == [(1, 0), (2, 1), (3, 2), (4, 4), (5, 5), (6, 8)] and len(items) == 1 + 1 + 2 + 1 + 3 + 2
    assert items == [(0, 0), (1, 0), (2, 0), (2, 1), (3, 0), (4, 0), (4, 1), (4, 2), (5, 0), (5, 1)]
    assert ir.block_items(off, 0) == ([], []) and ir.block_items(off, 8193)[0] == [(3, 0), (5, 2), (6, 5)]
    assert ir.block_items(off, 20_012) == ([], [])
    L = 20_011
    assert ir.block_geometry(9000, L, 0) == (0, 8192, 8192) and ir.block_geometry(9000, L, 1) == (8192, 808, 8192)
    assert ir.block_geometry(L, L, 2) == (16_384, 3627, 3627) and ir.block_geometry(8193, 8193, 1) == (8192, 1, 1)
    assert ir.block_geometry(1, L, 0) == (0, 1, 8192) and ir.block_geometry(8193, L, 1) == (8192, 1, 8192)


def values_for(rng, n):
    """float64 with whole mantissas and magnitudes over twelve decades (every addition rounds, so the order of the chain shows), a
    tenth NaN, -0.0 in the first four and no +0.0"""
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, n)
    x[rng.random(n) < 0.1] = np.nan
    x[:4] = -0.0
    return x


def differing(got, want, groups):
    return {key: [j for j in groups if not ng.same(got[key][j], want[key][j])] for key in nr.KEYS if not ng.same(got[key][groups], want[key][groups])}


@pytest.mark.parametrize("k", EDGES)
def test_blocks_equal_the_restatement(k):
    """a group of k values in rows of L > k columns, for the next L of the edges above k and for L = 40 000: every block's tree, the
    chain and the extremes, against the restatement's one pass over the padded row"""
    rng = np.random.default_rng(k)
    n = 50_000
    x = values_for(rng, n)
    for L in ([e for e in EDGES + [8192 * 4 + 2] if e > k][0], 40_000):
        lens = [k, L, 0, 1, 129]
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        idx = rng.integers(0, n, off[-1])
        idx[off[1] - 1] = 2                                       # a -0.0 last in the group of k values: the latest of the equal extremes...
        want = nr.aggregate_values(x, off, idx)
        with np.errstate(all="ignore"):
            got = ir.aggregate_by_blocks(x, off, idx, 1)
        assert not differing(got, want, [0, 1, 3, 4]), (k, L, differing(got, want, [0, 1, 3, 4]))
        assert np.isnan(got["mean"][2]) and np.isnan(got["sum"][2])           # an empty group stays on the narrow path
        narrow = ir.aggregate_by_blocks(x, off, idx, k + 1)
        assert np.isnan(narrow["sum"][[0, 2, 3, 4]]).all() and ng.same(narrow["sum"][1], want["sum"][1])


def test_the_order_of_the_chain_shows():
    """three blocks whose sums are 1, 2^-53 and 2^-53: ascending, each small one is rounded away (1.0); descending, they add up
    first (1 + 2^-52).  The restatement has numpy's, and the comparison tells the two apart."""
    n = 2 * 8192 + 1
    x = np.zeros(n)
    x[0], x[8192], x[2 * 8192] = 1.0, 2.0 ** -53, 2.0 ** -53
    off, idx = np.array([0, n]), np.arange(n)
    want = nr.aggregate_values(x, off, idx)
    got, wrong = ir.aggregate_by_blocks(x, off, idx, 1), ir.aggregate_by_blocks(x, off, idx, 1, descending=True)
    assert want["sum"][0] == 1.0 == np.sum(x) and not differing(got, want, [0])
    assert wrong["sum"][0] == 1.0 + 2.0 ** -52 and set(differing(wrong, want, [0])) >= {"sum", "mean"}


def test_extremes_merge_by_latest_position():
    """equal extremes in different blocks: the zero latest in the group decides the sign, whichever block the others are in"""
    n = 3 * 8192 + 5
    x = np.abs(np.random.default_rng(0).standard_normal(n)) + 1.0
    off, idx = np.array([0, n]), np.arange(n)
    for first, last, lo_sign in ((0.0, -0.0, True), (-0.0, 0.0, False)):
        y = x.copy()
        y[3], y[2 * 8192 + 1] = first, last                       # the minimum, twice: blocks 0 and 2
        y[8192 + 7] = y[n - 1] = 1e9                              # the maximum, twice: blocks 1 and 3
        got, want = ir.aggregate_by_blocks(y, off, idx, 1), nr.aggregate_values(y, off, idx)
        assert not differing(got, want, [0]) and np.signbit(got["min"][0]) == lo_sign and got["max"][0] == 1e9
