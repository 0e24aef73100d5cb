"""GPU tests of the adjacency maps (nellie_amd.hipnative.Adjacency, csrc/adjacency.inc; nellie_amd.feature_extraction.Hierarchy and
adjacency_maps; run(full=True)): the reference's goldens through adjacency_maps, the three primitives against the numpy restatement
(tests/adjacency_restatement.py) at the row counts where the mask, the scan (one workgroup covers 4096 mask words of 64 rows) and the
write kernels change workgroups, Hierarchy on files against an ImageFeatures run and the restatement, and run(full=True) end to end.
Everything is integer: every comparison is exact, dtype, shape and C order included."""
import os
import pickle
from types import SimpleNamespace

import numpy as np
import pytest

import adjacency_goldens as ag
import adjacency_restatement as ar
import component_goldens as cg

pytestmark = pytest.mark.gpu
NAMES = ag.names()
CHUNK = 4096 * 64                                                  # rows per workgroup of the scan
ROWS = (0, 1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 65, 3 * CHUNK + 7)
TABLES = ("features_voxels", "features_nodes", "features_branches", "features_organelles", "features_image")


@pytest.fixture(scope="module")
def hip():
    from nellie_amd import build, hipnative
    build.build(verbose=False)
    lib = hipnative.load()
    assert lib.device_count() > 0, "no HIP device"
    return lib


@pytest.fixture(scope="module")
def adj(hip):
    from nellie_amd import hipnative
    with hipnative.Adjacency() as handle:
        yield handle


def same(got, want):
    assert isinstance(got, np.ndarray) and got.dtype == np.int64 and got.ndim == 2 and got.shape[1] == 2 and got.flags.c_contiguous, (got.dtype, got.shape)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:5]
    return True


# ---- 1. the goldens ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_adjacency_maps_equal_the_reference(hip, name):
    from nellie_amd.feature_extraction import adjacency_maps
    g = ag.load(name)
    ms = {}
    got = adjacency_maps(ag.double_of(g), kernel_ms=ms)
    assert ar.same_lists(got, g["ref"])
    assert set(ms) == {"pairs", "expand", "lookup"} and ms["pairs"] > 0


def test_adjacency_maps_take_the_csr_where_it_exists(hip):
    """this package's Voxels keeps the node lists as CSR too: the same v_n from either, and a None entry is an empty list"""
    from nellie_amd.feature_extraction import adjacency_maps
    g = ag.load("adjacency_3d_aniso")
    h = ag.double_of(g)
    want = adjacency_maps(h)["v_n"]
    h.voxels.node_labels = [[None if len(a) == 0 else a for a in frame] for frame in h.voxels.node_labels]
    assert any(a is None for a in h.voxels.node_labels[0])
    assert all(same(a, b) for a, b in zip(adjacency_maps(h)["v_n"], want))
    h.voxels.node_labels_csr = [ar.node_lists_csr(frame) for frame in h.voxels.node_labels]
    h.voxels.node_labels = None
    assert all(same(a, b) for a, b in zip(adjacency_maps(h)["v_n"], want))


# ---- 2. pairs ---------------------------------------------------------------------------------------------------------------------------
def labels_of(kind, n, dtype, rng):
    if kind == "zero":
        return np.zeros(n, dtype)
    lab = rng.integers(1, 2 ** 31 - 1 if dtype == np.int32 else 2 ** 40, n).astype(dtype)
    if kind == "half":
        lab[rng.random(n) < 0.5] = 0
    if kind == "last_word":                                       # positive in the last mask word only
        lab[:(max(n - 1, 0) // 64) * 64] = 0
    return lab


@pytest.mark.parametrize("dtype", (np.int32, np.int64))
@pytest.mark.parametrize("n", ROWS)
def test_pairs_at_the_sizes_that_decide(adj, n, dtype):
    rng = np.random.default_rng(n % 1000 + 7)
    for kind in ("zero", "positive", "half", "last_word"):
        lab = labels_of(kind, n, dtype, rng)
        for bias in (1, 0):
            assert same(adj.pairs(lab, bias), ar.pairs(lab, bias)), (kind, n, bias)
        if kind == "last_word" and n:
            assert 0 < len(ar.pairs(lab)) <= 64
    if n:
        lab = labels_of("half", n, dtype, rng)
        lab[rng.random(n) < 0.1] = -3                             # not above 0: no edge
        assert same(adj.pairs(lab, 1), ar.pairs(lab, 1))


def test_pairs_refuse_a_lossy_cast(adj):
    assert same(adj.pairs(np.array([0, 7, 0, 9], np.uint16), 1), ar.pairs([0, 7, 0, 9], 1))      # widened exactly
    with pytest.raises(ValueError, match="refusing a cast"):
        adj.pairs(np.array([1, 2 ** 63 + 5], np.uint64))
    with pytest.raises(ValueError, match="refusing a cast"):
        adj.pairs(np.array([1.0, 2.5]))
    with pytest.raises(ValueError):
        adj.pairs(np.zeros((2, 2), np.int32))
    assert same(adj.pairs(np.array([3], np.int32)), ar.pairs([3]))


# ---- 3. expand --------------------------------------------------------------------------------------------------------------------------
def csr_with_gaps(rng, start, middle, end, rows=300, most=9):
    """`rows` rows of 1 .. most values with runs of empty rows before, between and after them"""
    counts = rng.integers(1, most + 1, rows)
    half = rows // 2
    counts = np.concatenate([np.zeros(start, np.int64), counts[:half], np.zeros(middle, np.int64), counts[half:], np.zeros(end, np.int64)])
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return off, rng.integers(0, 10 ** 6, int(off[-1]))


@pytest.mark.parametrize("start, middle, end", [(0, 0, 0), (1, 1, 1), (5000, 0, 0), (0, 5000, 0), (0, 0, 5000), (5000, 5000, 5000), (3, 4999, 64)])
def test_expand_passes_over_empty_rows(adj, start, middle, end):
    off, val = csr_with_gaps(np.random.default_rng(start + 3 * middle + 7 * end), start, middle, end)
    got = adj.expand(off, val)
    assert same(got, ar.expand(off, val)) and got[0, 0] == start and got[-1, 0] == len(off) - 2 - end


def test_expand_long_rows_and_many_edges(adj):
    rng = np.random.default_rng(5)
    val = rng.integers(0, 10 ** 9, 70_000)                         # one row of 70 000 values, not sorted
    assert (np.diff(val) < 0).any()
    for off in ([0, 70_000], [0, 0, 70_000, 70_000], [0, 1, 69_999, 70_000]):
        assert same(adj.expand(off, val), ar.expand(off, val))
    counts = rng.integers(0, 4, 180_000)                            # E just above a scan workgroup's rows
    counts[-1] += CHUNK + 3 - min(int(counts.sum()), CHUNK + 3)
    off = np.concatenate([[0], np.cumsum(counts)])
    val = rng.integers(0, 500, int(off[-1]))
    assert CHUNK < len(val) < CHUNK + 70_000 and same(adj.expand(off, val), ar.expand(off, val))
    for off in ([0], [0, 0], np.zeros(6000, np.int64)):             # E = 0
        assert same(adj.expand(off, []), np.zeros((0, 2), np.int64))


def test_expand_refuses_bad_offsets(adj):
    for off, val in (([1, 3], [5, 6, 7]), ([0, 2, 1, 3], [1, 2, 3]), ([0, 2], [1, 2, 3]), ([0, 4], [1, 2, 3]), ([], [])):
        with pytest.raises(ValueError):
            adj.expand(off, val)
    assert same(adj.expand([0, 1], [4]), ar.expand([0, 1], [4]))


# ---- 4. lookup --------------------------------------------------------------------------------------------------------------------------
def test_lookup_last_position_wins(adj):
    rng = np.random.default_rng(11)
    for p, n, top in ((1, 1, 1), (50, 300, 40), (700, 5000, 300), (3000, CHUNK + 65, 2000)):
        parent = rng.integers(1, top + 1, p)                        # unsorted, with repeats
        parent[rng.integers(0, p)] = top                            # (the table reaches `top`)
        child = rng.integers(0, top + 1, n)                         # zeros and labels no parent has among them
        want = ar.lookup(child, parent)
        assert same(adj.lookup(child, parent), want)
        if p > 1:
            assert len(np.unique(parent)) < p and (child == 0).any() and len(want) < n
    assert same(adj.lookup([5, 0, 2, 9, 3], [9, 5, 3, 5]), np.array([[0, 3], [3, 0], [4, 2]], np.int64))
    assert same(adj.lookup(np.array([4, 0], np.uint8), np.array([0, 4], np.int32)), np.array([[0, 1], [1, 0]], np.int64))   # a parent 0 is a label too


def test_lookup_without_parents_or_children(adj):
    assert same(adj.lookup([1, 2, 0], []), np.zeros((0, 2), np.int64))
    assert same(adj.lookup([], [3, 1]), np.zeros((0, 2), np.int64))
    assert same(adj.lookup([], []), np.zeros((0, 2), np.int64))


def test_lookup_large_table(adj):
    rng = np.random.default_rng(13)
    parent = rng.permutation(np.arange(1, 400_001))[:150_000]
    parent[0] = 400_000                                             # a table of 400 001 entries
    child = rng.integers(0, 400_001, 3 * CHUNK + 7)
    assert same(adj.lookup(child, parent), ar.lookup(child, parent))


def test_lookup_refuses_what_the_reference_cannot_index(adj):
    child = np.zeros(70_000, np.int64)
    child[[1234, 66_000]] = 11, 12                                  # the first row above the parents' maximum is named
    with pytest.raises(ValueError, match=r"row 1234 holds label 11, above the parents' largest label 10"):
        adj.lookup(child, [3, 10, 3])
    assert same(adj.lookup([10, 3, 4], [3, 10, 3]), np.array([[0, 1], [1, 2]], np.int64))          # the handle stays usable
    with pytest.raises(ValueError, match="negative"):
        adj.lookup([1, -1], [1, 2])
    with pytest.raises(ValueError, match="negative"):
        adj.lookup([1, 2], [-4, 2])
    assert same(adj.lookup([2], [1, 2]), np.array([[0, 1]], np.int64))


# ---- 5. repeatability -------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bytes_and_nothing_is_left_behind(adj):
    rng = np.random.default_rng(17)
    big = labels_of("half", 3 * CHUNK + 7, np.int64, rng)
    parent = rng.integers(1, 5000, 4000)
    parent[0] = 4999
    child = rng.integers(0, 5000, CHUNK + 65)
    off, val = csr_with_gaps(rng, 100, 5000, 100, rows=20_000)
    small = np.array([0, 2, 0, 5, 1], np.int32)
    first = [adj.pairs(big, 1), adj.lookup(child, parent), adj.expand(off, val)]
    after_big = [adj.pairs(small, 1), adj.lookup([2, 7], [7, 7, 2]), adj.expand([0, 0, 2], [8, 6])]
    assert same(after_big[0], np.array([[1, 1], [3, 4], [4, 0]], np.int64)) and same(after_big[1], np.array([[0, 2], [1, 1]], np.int64))
    assert same(after_big[2], np.array([[1, 8], [1, 6]], np.int64))
    second = [adj.pairs(big, 1), adj.lookup(child, parent), adj.expand(off, val)]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))
    ms = adj.kernel_ms_parts()
    assert list(ms) == ["pairs", "expand", "lookup"] and all(v > 0 for v in ms.values())


def test_a_closed_handle_says_so(hip):
    from nellie_amd import hipnative
    handle = hipnative.Adjacency()
    handle.close()
    handle.close()
    with pytest.raises(hipnative.NellieHipError, match="closed"):
        handle.pairs([1])


# ---- 6. Hierarchy on files --------------------------------------------------------------------------------------------------------------
def levels_of(h, skip_nodes):
    return SimpleNamespace(skip_nodes=skip_nodes, voxels=h.voxels, nodes=h.nodes, branches=h.branches, components=h.components)


def test_hierarchy_writes_the_tables_and_the_pickle(hip, tmp_path):
    """Hierarchy(im_info).run() on a stack written with the project's ImInfo: the five tables as an ImageFeatures run writes them,
    character for character; the pickle against the restatement applied to the run's own levels; with and without skip_nodes"""
    from nellie_amd.feature_extraction import Hierarchy, ImageFeatures
    from nellie_amd.im_info.verifier import ImInfo
    gc = cg.load("components_3d_integer_flow")
    gb, g = gc["branches"], gc["base"]
    dim_res = dict(zip("ZYX", (float(s) for s in g["spacing"])), T=g["dt"])
    im_info = ImInfo(g["raw"], dim_res=dim_res, output_dir=str(tmp_path), name="hierarchy")
    paths = im_info.pipeline_paths
    for key, data in (("im_preprocessed", g["struct"]), ("im_distance", g["distance"]), ("im_skel", gb["skel"]), ("im_instance_label", g["comp"]),
                      ("im_skel_relabelled", g["branch"]), ("im_border", gb["border"]), ("im_pixel_class", g["pixel_class"])):
        im_info.allocate_memory(paths[key], dtype=str(data.dtype), data=data, description=key)
    np.save(paths["flow_vector_array"], g["flow"])
    for skip_nodes in (False, True):
        tables = [k for k in TABLES if not (skip_nodes and k == "features_nodes")]
        ImageFeatures(im_info, skip_nodes=skip_nodes).run()
        want = {k: open(paths[k]).read() for k in tables}
        for k in tables:
            os.remove(paths[k])
        viewer = SimpleNamespace(status=None)
        h = Hierarchy(im_info, skip_nodes=skip_nodes, viewer=viewer)
        h.run()
        assert viewer.status == "Done!" and {k: open(paths[k]).read() for k in tables} == want
        assert skip_nodes == (not os.path.exists(paths["features_nodes"]))
        with open(paths["adjacency_maps"], "rb") as f:
            got = pickle.load(f)
        own = ar.adjacency_lists(levels_of(h, skip_nodes))
        assert ar.same_lists(got, own) and (got["v_n"] == []) == skip_nodes
        assert sum(len(a) for a in got["v_b"]) > 0 and sum(len(a) for a in got["b_o"]) > 0 and len(got["v_o"]) == g["T"]
        assert skip_nodes or (sum(len(a) for a in got["v_n"]) > 0 and sum(len(a) for a in got["n_b"]) > 0)
        assert set(h.adjacency_kernel_ms) == {"pairs", "expand", "lookup"}
        for k in tables + ["adjacency_maps"]:
            os.remove(paths[k])
    statuses = []
    viewer = type("Viewer", (), {"status": property(lambda self: statuses[-1], lambda self, s: statuses.append(s))})()
    Hierarchy(im_info, enable_adjacency=False, viewer=viewer).run()
    assert not os.path.exists(paths["adjacency_maps"]) and all(os.path.exists(paths[k]) for k in TABLES if k != "features_nodes")
    assert statuses[-2:] == ["Finalizing run.", "Done!"]


# ---- 7. run(full=True) ------------------------------------------------------------------------------------------------------------------
def test_run_full_writes_everything_the_reference_does(hip, tmp_path, capsys):
    from nellie_amd.feature_extraction import Hierarchy
    from nellie_amd.im_info.verifier import ImInfo
    from nellie_amd.run import run
    from nellie_amd.synthetic import ISO_01, make_volume
    vols = np.stack([make_volume((16, 48, 48), 60 + t) for t in range(3)])
    im_info = ImInfo(vols, dim_res=ISO_01, output_dir=str(tmp_path), name="full")
    assert run(im_info, full=True, skeletonize="hip", timeit=True) is im_info
    out = capsys.readouterr().out
    assert all(f"[timeit] {stage}:" in out for stage in ("Filter", "Label", "Network", "Markers", "Tracking", "VoxelReassigner", "Hierarchy", "Total"))
    paths = im_info.pipeline_paths
    assert [k for k, p in paths.items() if not os.path.exists(p)] == []
    labels = np.asarray(im_info.get_memmap(paths["im_instance_label"]))
    classes = np.asarray(im_info.get_memmap(paths["im_pixel_class"]))
    assert all(frame.any() for frame in labels) and all(frame.any() for frame in classes)           # Label found objects, Network nodes
    with open(paths["adjacency_maps"], "rb") as f:
        got = pickle.load(f)
    fresh = Hierarchy(im_info, skip_nodes=False, enable_adjacency=False)
    fresh.run()
    assert ar.same_lists(got, ar.adjacency_lists(levels_of(fresh, False)))
    assert all(len(got[key]) == 3 for key in ar.KEYS) and all(len(a) > 0 for key in ar.KEYS for a in got[key])
    assert fresh.voxels.node_labels_csr and len(fresh.nodes.time) == 3
