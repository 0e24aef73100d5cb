"""CPU tests of the node level of the hierarchy: the numpy restatement (tests/node_features_restatement.py) against every golden of
the reference's Nodes and aggregate_stats_for_class (tests/golden/nodes), its summation trees against the installed numpy, and the
text of features_nodes that the reference's saving rule gives.  The GPU tests (tests/test_hip_nodes.py) lean on all three."""
import warnings

import numpy as np
import pytest

import node_features_restatement as nr
import node_goldens as ng

NAMES = ng.names()


def test_the_public_names_exist():
    from nellie_amd import feature_extraction as fe
    assert {"Nodes", "NodeFeatures", "aggregate_stats_for_class", "Voxels", "VoxelFeatures"} <= set(fe.__all__)
    assert callable(fe.aggregate_stats_for_class) and fe.Nodes.__module__ == fe.NodeFeatures.__module__ == "nellie_amd.feature_extraction.nodes"


def test_the_goldens_cover_the_cases():
    assert len(NAMES) == 12
    longest = [L for name in NAMES for L in ng.load(name)["longest"]]
    calls = [c["L"] for c in ng.synthetic_calls()]
    assert calls == [1, 7, 8, 9, 127, 128, 129, 136, 255, 256, 257, 1000]
    assert any(8 <= L <= 128 for L in longest) and any(L > 128 for L in longest) and 0 in longest
    for name in NAMES:
        g = ng.load(name)
        assert len(g["longest"]) == (0 if g["base"]["skip_nodes"] else g["base"]["T"])
    empty = [t for name in NAMES for t in range(len(ng.load(name)["border"])) if not ng.load(name)["border"][t].any()]
    lone = [t for name in NAMES for t in range(len(ng.load(name)["border"])) if ng.load(name)["border"][t].sum() == 1]
    assert empty and lone


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_golden(name):
    g = ng.load(name)
    own = nr.Nodes(ng.hierarchy_double(g["base"], g["border"]))
    own.run()
    ng.assert_same_nodes(own, g["ref"], g["base"])
    assert own.longest == g["longest"]


def test_the_wide_calls_cover_the_cases():
    """the calls at and past numpy's buffer of 8192 elements: each has an empty, an all-NaN and a -0.0-only group, two as long as
    L, and a group of every k of 1, 7, 129, 8191, 8192, 8193 that fits"""
    calls = ng.wide_calls()
    assert [c["L"] for c in calls] == [8192, 8193, 16_385, 20_011]
    for c in calls:
        k = np.diff(c["offsets"]).tolist()
        assert max(k) == c["L"] and k.count(c["L"]) >= 2 and 0 in k and {v for v in (1, 7, 129, 8191, 8192, 8193) if v <= c["L"]} <= set(k)
        want = c["want"]["f64"]
        assert np.isnan(want["mean"][0, 2]) and want["sum"][0, 2] == 0.0 and np.isnan(want["max"][0, 1])
        assert np.signbit(want["min"][0, 3]) and np.signbit(want["max"][0, 3]) and want["sum"][0, 3].tobytes() == np.float64(0.0).tobytes()
        assert np.isnan(c["child"].f64[0]).mean() > 0.05 and c["child"].f32[0].dtype == np.float32 and c["child"].u16[0].dtype == np.uint16
        assert (np.diff(c["idx"][:c["L"]]) < 0).any() and len(np.unique(c["idx"][:c["L"]])) < c["L"]       # unsorted, with repeats


def test_restatement_equals_the_synthetic_calls():
    for call in ng.synthetic_calls() + ng.wide_calls():
        for groups in (ng.groups_of(call), (call["offsets"], call["idx"])):
            got = nr.aggregate_stats_for_class(call["child"], 0, groups)
            ng.assert_same_aggregates(got, call["want"], call["L"])


def numpy_rows(M):
    """nanmean, nanstd, nanmin, nanmax, nansum of the rows of M by numpy itself"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                           # all-NaN rows
        return {"mean": np.nanmean(M, axis=1), "std_dev": np.nanstd(M, axis=1), "min": np.nanmin(M, axis=1), "max": np.nanmax(M, axis=1),
                "sum": np.nansum(M, axis=1)}


def padded_case(rng, L, k):
    """rows of k[j] values (a tenth NaN) in CSR order, and the same as a matrix padded with NaN to L columns"""
    k = np.asarray(k, np.int64)
    off = np.concatenate([[0], np.cumsum(k)])
    x = rng.standard_normal(off[-1]) * 10.0 ** rng.integers(-3, 3, off[-1])
    x[rng.random(len(x)) < 0.1] = np.nan
    M = np.full((len(k), L), np.nan)
    for j in range(len(k)):
        M[j, :k[j]] = x[off[j]:off[j + 1]]
    return off, x, M


WIDE_L = (8191, 8192, 8193, 8200, 16_384, 16_385, 3 * 8192 + 7, 100_003)


def test_the_trees_are_numpys():
    """A numpy that sums differently shows here, not on the GPU: PaddedSum against np.nansum over the rows of the padded matrix
    and over vectors, and the mean / std_dev recipe against np.nanmean / np.nanstd, bit for bit.  Above 8192 columns numpy's ufunc
    buffer cuts every row into blocks of 8192, each a pairwise tree of its own, added in order; the blocks restart at every row
    (50 rows per matrix here).  A restatement that sums a row as a single tree over L fails this test from L = 8193 on."""
    assert np.getbufsize() == nr.BUFFER == 8192
    rng = np.random.default_rng(17)
    for L in (1, 5, 7, 8, 9, 64, 127, 128, 129, 136, 200, 255, 256, 257, 520, 700, 1031) + WIDE_L:
        G = 24 if L < 8000 else 50
        k = rng.integers(0, L + 1, G)
        k[:2] = (L, 0)
        off, x, M = padded_case(rng, L, k)
        want = numpy_rows(M)
        got = nr.aggregate_values(x, off, np.arange(len(x)))
        for key in nr.KEYS:
            assert ng.same(got[key], want[key]), (L, key)
        vec = np.where(np.isnan(x[:L]), 0.0, x[:L]) if len(x) >= L else np.zeros(L)
        assert nr.PaddedSum([0, L], L)(vec).tobytes() == np.nansum(vec[None, :], axis=1).tobytes() == np.array([np.nansum(vec)]).tobytes(), L
        if L > 8000:                                              # a vector of L = k elements, as the node statistics' nanmean takes it
            one = nr.aggregate_values(x[:L], [0, L], np.arange(L))
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                assert one["mean"].tobytes() == np.array([np.nanmean(x[:L])]).tobytes(), L
                assert one["std_dev"].tobytes() == np.array([np.nanstd(x[:L])]).tobytes(), L
    L = 30_000                                                    # the padded layout: short and long groups beside one of L
    k = np.concatenate([[1, 100, 8191, 8192, 8193, 16_385, L - 1, L], rng.integers(0, L + 1, 42)])
    off, x, M = padded_case(rng, L, k)
    want = numpy_rows(M)
    got = nr.aggregate_values(x, off, np.arange(len(x)), nr.PaddedSum(off, L))
    for key in nr.KEYS:
        assert ng.same(got[key], want[key]), (L, key, np.flatnonzero(got[key] != want[key]))
    minus = np.full(30_000, -0.0)
    for L in (3, 9, 130, 300, 8192, 8193, 16_385, 30_000):        # the identity settles the sign of a zero
        assert not np.signbit(nr.PaddedSum([0, L], L)(minus[:L])[0]) and not np.signbit(np.nansum(minus[:L]))
    for L in (8193, 16_385, 30_000):                              # rows of -0.0 alone, padded: every sum is +0.0, min and max -0.0
        k = np.array([1, 129, 8192, min(8193, L), L - 1, L])
        off = np.concatenate([[0], np.cumsum(k)])
        M = np.full((len(k), L), np.nan)
        for j in range(len(k)):
            M[j, :k[j]] = -0.0
        want = numpy_rows(M)
        got = nr.aggregate_values(np.full(off[-1], -0.0), off, np.arange(off[-1]), nr.PaddedSum(off, L))
        for key in nr.KEYS:
            assert got[key].tobytes() == want[key].tobytes(), (L, key)
        assert not np.signbit(got["sum"]).any() and not np.signbit(got["mean"]).any() and np.signbit(got["min"]).all()


def test_the_node_table_has_the_reference_columns():
    g = ng.load("nodes_3d_aniso")
    own = nr.Nodes(ng.hierarchy_double(g["base"], g["border"]))
    own.run()
    header, text = nr.feature_table(own)
    stats = g["base"]["ref"]["stats_to_aggregate"]
    assert stats == ["linear_vel", "angular_vel", "linear_acc", "angular_acc", "rel_linear_vel", "rel_angular_vel", "rel_linear_acc",
                     "rel_angular_acc", "rel_directionality", "structure", "intensity"]
    want = ["t", "label"] + [f"{s}_{k}" for s in stats for k in ("mean", "std_dev", "min", "max", "sum")] + \
        ["divergence_raw", "convergence_raw", "vergere_raw", "node_thickness_raw", "x_raw", "y_raw", "z_raw"]
    assert header == want and len(header) == 64
    lines = text.splitlines()
    assert lines[0] == ",".join(want) and len(lines) == 1 + sum(len(a) for a in g["ref"]["nodes"])
    rows = np.array([[float(x) if x else np.nan for x in line.split(",")] for line in lines[1:]])
    off = np.concatenate([[0], np.cumsum([len(a) for a in g["ref"]["nodes"]])])
    for t in range(g["base"]["T"]):
        part = rows[off[t]:off[t + 1]]
        assert np.array_equal(part[:, 0], np.full(len(part), t)) and np.array_equal(part[:, 1], np.arange(len(part)))
        assert np.array_equal(part[:, 2], g["ref"]["agg"][t]["linear_vel"]["mean"][0], equal_nan=True)
        assert np.array_equal(part[:, header.index("node_thickness_raw")], g["ref"]["node_thickness"][t], equal_nan=True)
        assert np.array_equal(part[:, header.index("z_raw")], g["ref"]["z"][t], equal_nan=True)
