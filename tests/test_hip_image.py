"""GPU tests of the image level of the hierarchy (nellie_amd.feature_extraction.image) and of the block path of the aggregation
(csrc/nodefeat.inc, nf_wide_block_kernel / nf_wide_chain_kernel), which sums a wide group one buffer block of 8192 elements per wave
and adds the blocks' sums in numpy's order.

Everything is compared for equality: every float bit for bit, the NaN pattern included (a NaN equals a NaN of another sign or
payload); where two device runs are compared, their bytes.  References: the goldens of the reference's Image (tests/golden/image);
numpy's nanmean / nanstd / nanmin / nanmax / nansum on the padded matrix of the reference's default path (`numpy_default_path` of
tests/test_hip_aggregate_wide.py); and the restatements (tests/image_features_restatement.py, tests/node_features_restatement.py),
which equal both without a GPU (tests/test_image_cpu.py, tests/test_nodes_cpu.py)."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import branch_goldens as bg
import component_goldens as cg
import image_features_restatement as ir
import image_goldens as ig
import node_features_restatement as nr
import node_goldens as ng
from test_hip_aggregate_wide import differing, numpy_default_path, statistic
from test_image_cpu import restated

pytestmark = pytest.mark.gpu
NAMES = ig.names()
DTYPES = ("float32", "float64", "uint16", "int32")
VOXEL_STATS = ["linear_vel", "angular_vel", "linear_acc", "angular_acc", "rel_linear_vel", "rel_angular_vel", "rel_linear_acc", "rel_angular_acc",
               "rel_directionality", "structure", "intensity"]


@pytest.fixture(scope="module")
def hip():
    from nellie_amd import build, hipnative
    build.build(verbose=False)
    lib = hipnative.load()
    assert lib.device_count() > 0, "no HIP device"
    return lib


def run_image(h):
    from nellie_amd.feature_extraction import Image
    image = Image(h)
    image.run()
    assert image._aggregator is None
    return image


def aggregate(stats, off, idx, wide_from=None):
    """{name: {key: (G,) float64}} of every array in `stats` over the groups on one handle; wide_from None: the default"""
    from nellie_amd import hipnative
    with hipnative.NodeFeatures() as eng:
        if wide_from is not None:
            eng.set_wide_from(wide_from)
        eng.groups(off, idx)
        out = {name: eng.aggregate(x) for name, x in stats.items()}
        assert eng.kernel_ms_parts()["aggregation"] > 0
    return out


def same_bytes(a, b):
    return all(a[name][key].tobytes() == b[name][key].tobytes() for name in a for key in ng.KEYS)


def assert_both_paths_equal_numpy(stats, groups, what):
    """every non-empty group on the block path (wide_from = 1), none (0) and the default threshold: identical bytes, and equal to
    numpy on the padded matrix"""
    off, idx = nr.as_csr(groups)
    L = max(len(a) for a in groups)
    block, narrow, default = (aggregate(stats, off, idx, w) for w in (1, 0, None))
    for name, x in stats.items():
        want = numpy_default_path(x, groups, L)
        for path, got in (("block", block), ("narrow", narrow)):
            assert not differing(got[name], want), (what, path, name, differing(got[name], want))
    assert same_bytes(block, narrow) and same_bytes(block, default), what


@pytest.mark.parametrize("name", NAMES)
def test_golden(hip, name):
    g = ig.load(name)
    for low_memory in (False, True):                              # accepted and ignored: the values of the default path
        got = run_image(ig.double_of(g, low_memory=low_memory))
        ig.assert_same_image(got, g["ref"], g["base"])
        assert len(got.kernel_ms) == g["base"]["T"] and all(set(p) == {"aggregation"} for p in got.kernel_ms)


def test_both_paths_on_the_same_call(hip):
    """groups of 0 to 65 537 values in one call, indices unsorted and repeated, one group all NaN and one of -0.0 only; the float
    statistics have a tenth NaN (the integer dtypes cannot hold one), and no group holds zeros of both signs"""
    rng = np.random.default_rng(19)
    n = 200_003
    ks = (0, 1, 7, 129, 8191, 8192, 8193, 16_384, 16_385, 24_583, 65_537)
    groups = [rng.integers(4, n, k) for k in ks] + [rng.integers(1000, 1020, 300), rng.integers(0, 4, 9)]
    assert all((np.diff(a) < 0).any() and len(np.unique(a)) < len(a) for a in groups if len(a) >= 8191)
    stats = {}
    for j, dtype in enumerate(DTYPES):
        x = statistic(np.random.default_rng([19, j]), dtype, n)
        if x.dtype.kind == "f":
            x[1000:1020] = np.nan
            assert 0.08 < np.isnan(x).mean() < 0.12 and np.signbit(x[:4]).all() and (x[:4] == 0).all()
        stats[dtype] = x
    assert_both_paths_equal_numpy(stats, groups, "one call")
    got = aggregate({"f": stats["float64"]}, *nr.as_csr(groups), 1)["f"]
    assert np.isnan(got["mean"][[0, 11]]).all() and got["sum"][11] == 0 and np.signbit(got["min"][12]) and np.signbit(got["max"][12])


def ordered_statistic(groups, n):
    """a float64 statistic for which the order of the chain shows whatever the rest does: along the longest group, 1 at the head
    of the first block and 2^-53 at the head of the two next, zeros elsewhere.  Ascending, each small sum is rounded away (1.0);
    any other order adds them up first (1 + 2^-52)."""
    longest = max(groups, key=len)
    assert len(longest) > 2 * 8192 and len(np.unique(longest)) == len(longest)
    x = np.zeros(n)
    x[longest[0]], x[longest[8192]], x[longest[2 * 8192]] = 1.0, 2.0 ** -53, 2.0 ** -53
    return x


def test_a_row_longer_than_a_wide_group(hip):
    """L = 20 011: a group of 9 000 values has a second block of n_block = 8192 with 808 values and padding inside the tree; the
    longest group's last block has 3 627 elements"""
    rng = np.random.default_rng(20)
    n = 60_000
    L = 20_011
    groups = [rng.integers(0, n, 9000), rng.permutation(n)[:L], rng.integers(0, n, 8193), rng.integers(0, n, 3), np.zeros(0, np.int64),
              rng.integers(0, n, 16_384)]
    assert ir.block_geometry(9000, L, 1) == (8192, 808, 8192) and ir.block_geometry(L, L, 2) == (16_384, 3627, 3627)
    stats = {dtype: statistic(np.random.default_rng([20, j]), dtype, n) for j, dtype in enumerate(DTYPES[:2])}
    assert_both_paths_equal_numpy(stats, groups, "L = 20 011")
    order = {"order": ordered_statistic(groups, n)}
    off, idx = nr.as_csr(groups)
    block, narrow = aggregate(order, off, idx, 1), aggregate(order, off, idx, 0)
    want = nr.aggregate_values(order["order"], off, idx)
    assert want["sum"][1] == 1.0 and not differing(block["order"], want) and same_bytes(block, narrow)


def test_many_wide_groups(hip):
    """100 groups of 20 000 values (three blocks each) alternate with groups of 0 and 1 values: a partial slot shared between
    neighbouring items or groups shows against the restatement; two runs give the same bytes, and so does sending the groups of
    one value through the block path as well"""
    rng = np.random.default_rng(23)
    n = 50_000
    x = statistic(rng, "float64", n)
    lens = np.tile([20_000, 0, 1], 100)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    idx = rng.integers(0, n, off[-1])
    wide, items = ir.block_items(off, 8193)
    assert len(wide) == 100 and len(items) == 300 and len(ir.block_items(off, 1)[1]) == 400
    first, again, all_wide, default = (aggregate({"x": x}, off, idx, w) for w in (8193, 8193, 1, None))
    want = nr.aggregate_values(x, off, idx)
    assert not differing(first["x"], want), differing(first["x"], want)
    assert same_bytes(first, again) and same_bytes(first, all_wide) and same_bytes(first, default)
    assert np.isfinite(first["x"]["std_dev"][::3]).all() and np.isnan(first["x"]["mean"][1::3]).all()


def test_extremes_in_different_blocks(hip):
    """the minimum in block 0 and the maximum in the last block, then the reverse; and equal extremes in two blocks"""
    n = 3 * 8192 + 5
    base = np.abs(np.random.default_rng(5).standard_normal(n)) + 1.0
    off, idx = np.array([0, n], np.int64), np.arange(n, dtype=np.int64)
    for lo_at, hi_at in ((3, n - 2), (n - 2, 3), (8192 + 1, 2 * 8192 + 1)):
        x = base.copy()
        x[lo_at], x[hi_at] = 0.25, 1e9
        x[8192 * 2 - 1] = 0.25                                    # the minimum once more, in block 1
        block, narrow = aggregate({"x": x}, off, idx, 1), aggregate({"x": x}, off, idx, 0)
        assert block["x"]["min"][0] == np.nanmin(x) == 0.25 and block["x"]["max"][0] == np.nanmax(x) == 1e9
        assert not differing(block["x"], nr.aggregate_values(x, off, idx)) and same_bytes(block, narrow)


def plain_hierarchy(rows, seed, skip_nodes=False):
    """a hierarchy of plain objects with rows[t] = (voxels, nodes, branches, components) rows per frame and random statistics
    (float32 for the voxels and the skeleton statistics, float64 otherwise) with a fifth of the rows NaN; a level without rows holds
    empty lists, as this package's levels do; (hierarchy, base)"""
    rng = np.random.default_rng(seed)
    v = SimpleNamespace(stats_to_aggregate=list(VOXEL_STATS), coords=[], **{s: [] for s in VOXEL_STATS})
    n = SimpleNamespace(stats_to_aggregate=list(bg.NODE_STATS), nodes=[], **{s: [] for s in bg.NODE_STATS})
    b = SimpleNamespace(stats_to_aggregate=list(bg.STATS_TO_AGGREGATE), **{s: [] for s in bg.STATS_TO_AGGREGATE})
    c = SimpleNamespace(stats_to_aggregate=list(cg.STATS_TO_AGGREGATE), **{s: [] for s in cg.STATS_TO_AGGREGATE})
    for counts in rows:
        v.coords.append(np.zeros((counts[0], 3), np.int64))
        n.nodes.append(np.zeros((counts[1], 3), np.int64))
        for level, count, dtype in ((v, counts[0], np.float32), (n, counts[1], np.float64), (b, counts[2], None), (c, counts[3], np.float64)):
            for j, s in enumerate(level.stats_to_aggregate):
                x = rng.standard_normal(count) * 10.0 ** rng.integers(-2, 3, count)
                x[rng.random(count) < 0.2] = np.nan
                getattr(level, s).append(x.astype(dtype or (np.float32 if j < 4 else np.float64)) if count else [])
    im_info = SimpleNamespace(no_t=False, no_z=False, file_info=SimpleNamespace(filename_no_ext="plain"))
    h = SimpleNamespace(im_info=im_info, num_t=len(rows), spacing=(0.3, 0.1, 0.1), viewer=None, skip_nodes=skip_nodes, low_memory=False,
                        voxels=v, nodes=n, branches=b, components=c)
    return h, dict(T=len(rows), D=3, skip_nodes=skip_nodes, filename="plain")


def test_image_over_uneven_frames(hip):
    """T = 3 on one handle with plain objects as children: 20 000 voxels first (three blocks), an empty frame, then 50 rows --
    nothing of a frame survives into the next; with and without skip_nodes.  Image runs under the default threshold, which the
    measurements put at 4 * 8192 + 1, so the same again with 40 000 voxels first, a wide group of five
    blocks there."""
    for voxels, skip_nodes in ((20_000, False), (20_000, True), (40_000, False), (40_000, True)):
        rows = [(voxels, 1000, 600, 40), (0, 0, 0, 0), (50, 5, 3, 2)]
        h, base = plain_hierarchy(rows, 31, skip_nodes=skip_nodes)
        got = run_image(h)
        ig.assert_same_image(got, restated(h), base)
        assert np.isnan(got.aggregate_voxel_metrics[1]["intensity"]["mean"]).all() and got.aggregate_component_metrics[1]["organelle_area"]["sum"][0, 0] == 0
        assert np.isfinite(got.aggregate_voxel_metrics[0]["intensity"]["std_dev"]).all() and "reassigned_label" not in got.aggregate_branch_metrics[0]
        assert (got.aggregate_node_metrics == []) == skip_nodes and got.kernel_ms[0]["aggregation"] > 0


def test_image_features_writes_the_reference_table(hip, tmp_path):
    """ImageFeatures(im_info).run() on a stack written with the project's ImInfo: features_image against the text the restatement
    gives when fed this package's own Voxels, Nodes, Branches and Components output, character for character; the four other
    tables as a ComponentFeatures run writes them; with and without skip_nodes"""
    from nellie_amd.feature_extraction import ComponentFeatures, ImageFeatures
    from nellie_amd.im_info.verifier import ImInfo
    gc = cg.load("components_3d_integer_flow")
    gb, g = gc["branches"], gc["base"]
    dim_res = dict(zip("ZYX", (float(s) for s in g["spacing"])), T=g["dt"])
    im_info = ImInfo(g["raw"], dim_res=dim_res, output_dir=str(tmp_path), name="image")
    paths = im_info.pipeline_paths
    for key, data in (("im_preprocessed", g["struct"]), ("im_distance", g["distance"]), ("im_skel", gb["skel"]), ("im_instance_label", g["comp"]),
                      ("im_skel_relabelled", g["branch"]), ("im_border", gb["border"]), ("im_pixel_class", g["pixel_class"])):
        im_info.allocate_memory(paths[key], dtype=str(data.dtype), data=data, description=key)
    np.save(paths["flow_vector_array"], g["flow"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ImageFeatures(im_info, device="cpu")
    others = ("features_voxels", "features_nodes", "features_branches", "features_organelles")
    for skip_nodes in (False, True):
        tables = others if not skip_nodes else tuple(k for k in others if k != "features_nodes")
        ComponentFeatures(im_info, skip_nodes=skip_nodes).run()
        want_others = {k: open(paths[k]).read() for k in tables}
        for k in tables:
            os.remove(paths[k])
        fe = ImageFeatures(im_info, skip_nodes=skip_nodes)
        assert fe.run() is fe.image and fe.image.hierarchy is fe
        assert {k: open(paths[k]).read() for k in tables} == want_others
        h = SimpleNamespace(im_info=SimpleNamespace(file_info=SimpleNamespace(filename_no_ext=fe.image.image_name[0])), num_t=g["T"],
                            skip_nodes=skip_nodes, voxels=fe.voxels, nodes=fe.nodes, branches=fe.branches, components=fe.components)
        own = restated(h)
        ig.assert_same_image(fe.image, own, dict(g, filename=fe.image.image_name[0], skip_nodes=skip_nodes))
        header, want = ir.feature_table(own)
        got = open(paths["features_image"]).read()
        lines = got.splitlines()
        assert got == want and lines[0] == ",".join(header) and len(header) == 2 + (0 if skip_nodes else 20) + 55 + 45 + 25
        assert len(lines) == 1 + g["T"] and [line.split(",")[:2] for line in lines[1:]] == [[f"{t}.0", "0.0"] for t in range(g["T"])]
        os.remove(paths["features_image"])


def test_a_short_statistic_is_refused(hip):
    from nellie_amd import hipnative
    from nellie_amd.feature_extraction import Image
    g = ig.load("image_3d_aniso")
    h = ig.double_of(g, voxels=ng.voxels_double(g["base"], fill_empty_vectors=True))
    h.voxels.intensity = [a[:-1] for a in h.voxels.intensity]        # a statistic shorter than its level
    short = Image(h)
    with pytest.raises(ValueError, match="intensity"):
        short.run()
    assert short._aggregator is None
    x = np.arange(10_000, dtype=np.float64)
    with hipnative.NodeFeatures() as eng:                         # and on the handle itself, which stays usable
        eng.groups([0, 10_000], np.arange(10_000))
        with pytest.raises(ValueError, match="9999 values"):
            eng.aggregate(x[:-1])
        with pytest.raises(ValueError):
            eng.set_wide_from(-1)
        got = eng.aggregate(x)
        assert got["sum"][0] == x.sum() == 49_995_000 and got["max"][0] == 9999
