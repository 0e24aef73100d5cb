"""GPU tests of the aggregation (nellie_amd.feature_extraction.aggregate_stats_for_class, csrc/nodefeat.inc nf_tree_sum) where a
group holds more than 8192 values.  numpy reduces a row in pieces of its ufunc buffer, 8192 elements, each a pairwise tree of its
own, added in order; a device routine that sums a row as one tree over L differs from it from L = 8193 on, in `sum`, `mean` or
`std_dev`, and through L in every group of the call.

References: the reference's own aggregate_stats_for_class through the fixtures of tests/golden/nodes/nodes_synthetic_wide.npz;
numpy itself on the padded matrix that the reference's default path builds (the statistic with a NaN appended, every row filled
with that last index), in pieces of at most 2^24 matrix elements; and tests/node_features_restatement.py, which equals both
without a GPU (tests/test_nodes_cpu.py).  Everything is compared for equality, float64 bit for bit, the NaN pattern included.

numpy's nanmin / nanmax of a row holding zeros of both signs depend on the numpy build, so no group here
holds both; `numpy_default_path` asserts that.  A group of -0.0 alone is kept."""
import functools
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

import node_features_restatement as nr
import node_goldens as ng
import voxel_scenes as vs
from test_hip_nodes import made_up_voxels, restated, run_nodes

pytestmark = pytest.mark.gpu
PIECE = 1 << 24                       # matrix elements numpy reduces at a time
WIDE_L = (8193, 65_537, 262_144, 1_048_583)
DTYPES = ("float32", "float64", "uint16", "int32")


@pytest.fixture(scope="module")
def hip():
    from nellie_amd import build, hipnative
    build.build(verbose=False)
    lib = hipnative.load()
    assert lib.device_count() > 0, "no HIP device"
    return lib


def numpy_default_path(values, groups, L):
    """{key: (G,) float64}: numpy's nanmean, nanstd, nanmin, nanmax and nansum over the rows of the matrix of the reference's
    default path -- the statistic with a NaN appended, gathered through an index matrix of L columns whose rows are the groups,
    filled with the index of that NaN -- a piece of whole rows at a time"""
    stat = np.append(np.array(values), np.nan)
    assert stat.dtype == np.float64
    G = len(groups)
    out = {key: np.empty(G) for key in ng.KEYS}
    step = max(1, PIECE // L)
    for a in range(0, G, step):
        part = groups[a:a + step]
        rows = np.full((len(part), L), len(stat) - 1, dtype=np.int64)
        for i, idxs in enumerate(part):
            rows[i, :len(idxs)] = idxs
        M = stat[rows]
        del rows
        zero, minus = M == 0, np.signbit(M)
        assert not ((zero & minus).any(axis=1) & (zero & ~minus).any(axis=1)).any(), "a group holds zeros of both signs"
        del zero, minus
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                       # empty and all-NaN rows
            for key, reduce in zip(ng.KEYS, (np.nanmean, np.nanstd, np.nanmin, np.nanmax, np.nansum)):
                out[key][a:a + step] = reduce(M, axis=1)
    return out


def statistic(rng, dtype, n):
    """n values of the dtype; floats: magnitudes over six decades, a tenth NaN, -0.0 in the first four, and no +0.0"""
    if dtype == "uint16":
        return rng.integers(0, 65536, n).astype(np.uint16)
    if dtype == "int32":
        return rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32)
    x = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3, n)
    x[rng.random(n) < 0.1] = np.nan
    x[:4] = -0.0
    x = x.astype(dtype)
    assert not np.any((x == 0) & ~np.signbit(x))
    return x


def differing(got, want):
    """{key: the groups whose value differs}, for the message of a failed comparison"""
    return {key: np.flatnonzero(~((got[key] == want[key]) | (np.isnan(got[key]) & np.isnan(want[key])))).tolist()[:12] for key in ng.KEYS
            if not ng.same(got[key], want[key])}


def assert_equals_numpy(stats, groups, L, what):
    """aggregate_stats_for_class over `groups` (a list of index arrays) of every array in `stats`, against numpy_default_path"""
    from nellie_amd.feature_extraction import aggregate_stats_for_class
    child = SimpleNamespace(stats_to_aggregate=list(stats), **{name: [x] for name, x in stats.items()})
    got = aggregate_stats_for_class(child, 0, nr.as_csr(groups))
    assert list(got) == list(stats)
    for name, x in stats.items():
        want = numpy_default_path(x, groups, L)
        own = {key: got[name][key][0] for key in ng.KEYS}
        assert all(got[name][key].shape == (1, len(groups)) and got[name][key].dtype == np.float64 for key in ng.KEYS)
        assert not differing(own, want), (what, name, differing(own, want))


def test_wide_fixtures(hip):
    """the reference's aggregate_stats_for_class at L = 8192, 8193, 16 385 and 20 011, groups as lists and as a CSR pair"""
    from nellie_amd.feature_extraction import aggregate_stats_for_class
    calls = ng.wide_calls()
    assert [c["L"] for c in calls] == [8192, 8193, 16_385, 20_011]
    for call in calls:
        for groups in (ng.groups_of(call), (call["offsets"], call["idx"])):
            got = aggregate_stats_for_class(call["child"], 0, groups)
            ng.assert_same_aggregates(got, call["want"], call["L"])


@functools.lru_cache(maxsize=1)
def wide_groups(L):
    """unsorted indices with repeats into 200 003 values: groups of L, 0, 1, 7, 129, 8191, 8192, 8193, L // 2, L - 1 and
    L // 3 + 5 values, and one of nine indices below 4, where a float statistic holds -0.0"""
    rng = np.random.default_rng(L)
    n = 200_003
    groups = [rng.integers(0, n, k) for k in (L, 0, 1, 7, 129, 8191, 8192, 8193, L // 2, L - 1, L // 3 + 5)] + [rng.integers(0, 4, 9)]
    assert max(len(a) for a in groups) == L and all(len(a) < 2 or (np.diff(a) < 0).any() for a in groups[:-1])
    assert len(np.unique(groups[0])) < L
    return n, groups


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L", WIDE_L)
def test_wide_groups_equal_numpy(hip, L, dtype):
    """2, 9, 32 and 129 buffer blocks in the longest row, the last one short (1 and 7 elements: a running sum) or whole; groups
    that end at, before and after a block boundary beside it"""
    n, groups = wide_groups(L)
    x = statistic(np.random.default_rng([L, DTYPES.index(dtype)]), dtype, n)
    assert_equals_numpy({dtype: x}, groups, L, L)


def test_image_and_component_shapes_equal_numpy(hip):
    """the groups of the two levels above the branches over a 300 000-value statistic: the image, one group of every index in
    order; the components, 300 groups that partition the indices, sizes heavy-tailed, the longest above 8192"""
    rng = np.random.default_rng(41)
    n = 300_000
    stats = {"f32": statistic(rng, "float32", n), "f64": statistic(rng, "float64", n), "u16": statistic(rng, "uint16", n)}
    assert_equals_numpy(stats, [np.arange(n)], n, "image")
    share = np.random.default_rng(42).pareto(1.1, 300) + 0.01
    label = rng.choice(300, n, p=share / share.sum())
    groups = [np.flatnonzero(label == j) for j in range(300)]
    k = np.array([len(a) for a in groups])
    assert k.sum() == n and 3 * 8192 < k.max() < 60_000 and np.median(k) < 1000 and np.sum(k > 8192) >= 3, (k.max(), np.median(k))
    assert_equals_numpy(stats, groups, int(k.max()), "components")


def test_scratch_neighbours(hip):
    """groups of 20 000 values (three buffer blocks, 129 leaf sums at a time in 314 doubles of scratch) alternate with groups of 0
    and 1 values (2 doubles each): a leaf sum written past a group's share, or read after the next block overwrote it, lands in a
    neighbour that runs at the same time.  Against the restatement; two runs give the same bytes."""
    from nellie_amd.feature_extraction import aggregate_stats_for_class
    rng = np.random.default_rng(23)
    n = 50_000
    x = statistic(rng, "float32", n)
    lens = np.tile([20_000, 0, 1], 100)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = rng.integers(0, n, off[-1])
    child = SimpleNamespace(stats_to_aggregate=["x"], x=[x])
    first = aggregate_stats_for_class(child, 0, (off, idx))
    again = aggregate_stats_for_class(child, 0, (off, idx))
    want = nr.aggregate_values(x, off, idx)
    own = {key: first["x"][key][0] for key in ng.KEYS}
    assert not differing(own, want), differing(own, want)
    for key in ng.KEYS:
        assert first["x"][key].tobytes() == again["x"][key].tobytes(), key
    assert np.isfinite(own["std_dev"][::3]).all() and np.isnan(own["mean"][1::3]).all()


def test_node_statistics_of_a_list_above_8192(hip):
    """a 4 x 60 x 70 frame with every voxel labelled; one node's box is the frame (16 800 voxels: three buffer blocks in the
    nanmean of its dot products, and L = 16 800 for every node's aggregates), the others' hold 8 to 256 voxels.  The whole of Nodes
    against the restatement, and divergence, convergence and vergere against np.nanmean of the dot products per voxel."""
    rng = np.random.default_rng(8)
    shape = (4, 60, 70)
    comp = rng.integers(1, 40, (1,) + shape, dtype=np.int32)
    pixel_class, distance = np.zeros(comp.shape, np.uint8), np.zeros(comp.shape, np.float32)
    spots = [(1, 30, 35), (0, 0, 0), (3, 59, 69), (2, 10, 50), (1, 45, 7), (3, 20, 20)]
    for j, at in enumerate(spots):
        pixel_class[(0,) + at], distance[(0,) + at] = 1 + j % 4, (100.0, 0.0, 1.0, 2.5, 1.5, 3.0)[j]
    border = np.zeros(comp.shape, np.uint8)
    border[0, :, 0, :] = 1
    g = vs.as_stack("wide_node", comp, comp.copy(), comp.astype(np.uint16), comp.astype(np.float32), pixel_class, distance, np.zeros((0, 8)),
                    vs.SPACING_3D, 1.0)
    h = ng.hierarchy_double(g, border, voxels=made_up_voxels(g, 12))
    nodes = run_nodes(h)
    ng.assert_same_nodes(nodes, restated(h), g)
    lists = h.voxels.node_voxel_idxs[0]
    k = [len(a) for a in lists]
    assert nodes.longest == [16_800] and len(k) == len(spots) and sorted(k)[-1] == 16_800 and sorted(k)[-2] < 400 and min(k) == 8
    coords = h.voxels.coords[0]
    for i, node in enumerate(nodes.nodes[0]):
        d = (coords[lists[i]] - node).astype(np.float64)
        norm = np.sqrt((0.0 + d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        means = []
        with np.errstate(all="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore")
            direction = np.where(norm[:, None] != 0, d / norm[:, None], np.nan)
            for vec, sign in ((h.voxels.vec01[0], -1.0), (h.voxels.vec12[0], 1.0)):
                p = (sign * vec[lists[i]].astype(np.float64)) * direction
                means.append(np.nanmean(((0.0 + p[:, 0]) + p[:, 1]) + p[:, 2]))
        want = {"convergence": -means[0], "divergence": means[1], "vergere": -means[0] + means[1]}
        for name in want:
            got = getattr(nodes, name)[0][i]
            assert ng.same(np.float64(got), np.float64(want[name])), (name, i, k[i], got, want[name])
    assert np.isfinite(nodes.divergence[0][np.argmax(k)]) and np.isfinite(nodes.convergence[0]).sum() >= 5
