"""GPU tests of the analysis overlay (nellie_amd.hipnative.Overlay, csrc/overlay.inc; nellie_amd.feature_extraction.FeatureOverlay,
overlay_values, overlay_frame): the frames captured from the reference through FeatureOverlay on files, at all
four levels, as float64, float32 and labels; the core functions against the sparse restatement (tests/feature_overlay_restatement.py)
at the row counts where the mask, the scan (one workgroup covers 4096 mask words of 64 voxels) and the paint's 16-byte stores and
tail change over; node runs that decide the order of the sum; the resident frame; repeatability.  Every comparison is `same`: equal
values, NaN in the same places, zeros of the same sign."""
import pickle
from types import SimpleNamespace

import numpy as np
import pytest

import feature_overlay_restatement as fr
import overlay_goldens as og

pytestmark = pytest.mark.gpu
NAMES = og.names()
TABLE_KEYS = {"voxel": "features_voxels", "node": "features_nodes", "branch": "features_branches", "organelle": "features_organelles"}
CHUNK = 4096 * 64                                                  # voxel rows per workgroup of the scan


@pytest.fixture(scope="module")
def hip():
    from nellie_amd import build, hipnative
    build.build(verbose=False)
    lib = hipnative.load()
    assert lib.device_count() > 0, "no HIP device"
    return lib


def files_of(tmp_path, labels, tables, edges, no_t=False):
    """an im_info double over files: the tables as csv, the pickle, and the label stack behind get_memmap"""
    import pandas as pd
    paths = {"im_instance_label": str(tmp_path / "labels.bin"), "adjacency_maps": str(tmp_path / "adjacency.pkl")}
    open(paths["im_instance_label"], "wb").close()
    with open(paths["adjacency_maps"], "wb") as f:
        pickle.dump(edges, f)
    for level, cols in tables.items():
        t_col, label_col = cols[0], cols[1]
        frame = {"t": np.asarray(t_col, float), "label": np.asarray(label_col, float)}           # the hierarchy's tables are float64 throughout
        frame.update({f"value{k or ''}": v for k, v in enumerate(cols[2:])})
        paths[TABLE_KEYS[level]] = str(tmp_path / f"{level}.csv")
        pd.DataFrame(frame).to_csv(str(tmp_path / f"{level}.csv"), index=False)
    stack = labels[0] if no_t else labels
    axes = ("" if no_t else "T") + ("ZYX" if labels.ndim == 4 else "YX")
    return SimpleNamespace(no_t=no_t, no_z=labels.ndim == 3, axes=axes, shape=stack.shape, pipeline_paths=paths, get_memmap=lambda p: stack)


# ---- 1. the fixtures, from files --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_feature_overlay_equals_the_reference(hip, tmp_path, name):
    from nellie_amd.feature_extraction import FeatureOverlay
    g = og.load(name)
    with FeatureOverlay(files_of(tmp_path, g["labels"], g["tables"], g["edges"])) as fo:
        for level in fo.levels:
            want = g["frames"][level]
            assert fo.columns(level) == ["value"]
            got = fo.run(level, "value")
            assert fr.same(got, want), level
            assert fr.same(fo.run(level, "value", dtype=np.float32), want.astype(np.float32)), level
            assert fr.same(fo.labels(level, "value"), fr.as_labels(want)), level
            assert fo.contrast_limits(level, "value") == g["clim"][level]
            for t in (0, len(want) - 1):
                rows = fo.values(level, "value", t)
                assert rows.dtype == np.float64 and fr.same(rows, want[t][g["labels"][t] > 0]), (level, t)
                assert fr.same(fo.labels(level, "value", t), fr.as_labels(want[t]))
        assert set(fo.kernel_ms) == {"load", "values", "paint"} and fo.kernel_ms["paint"] > 0


def test_align_branches_a_memmap_and_a_stack_without_t(hip, tmp_path):
    from nellie_amd.feature_extraction import FeatureOverlay
    g = og.load("overlay_3d_aniso")
    t_col, label_col, val_col = g["tables"]["branch"]
    im_info = files_of(tmp_path, g["labels"], g["tables"], g["edges"])
    quirk = g["frames"]["branch"]
    aligned = fr.overlay_sparse(g["labels"], "branch", t_col, label_col, val_col, g["edges"]["v_b"], align_branches=True)
    assert not fr.same(aligned, quirk) and np.isfinite(aligned).sum() > np.isfinite(quirk).sum()
    out = np.lib.format.open_memmap(str(tmp_path / "out.npy"), mode="w+", dtype=np.float64, shape=quirk.shape)
    with FeatureOverlay(im_info, align_branches=True) as fo:
        assert fo.run("branch", "value", out=out) is out and fr.same(np.asarray(out), aligned)
        assert fr.same(fo.run("organelle", "value"), g["frames"]["organelle"])                    # the other levels are as they were
        with pytest.raises(ValueError, match="out must be"):
            fo.run("branch", "value", out=np.empty(quirk.shape, np.float32))
    one = {lv: tuple(c[cols[0] == 0] for c in cols) for lv, cols in g["tables"].items()}
    single = files_of(tmp_path, g["labels"][:1], one, {k: v[:1] for k, v in g["edges"].items()}, no_t=True)
    with FeatureOverlay(single) as fo:
        for level in fo.levels:
            got = fo.run(level, "value")
            assert got.shape == g["labels"].shape[1:] and fr.same(got, g["frames"][level][0]), level


def test_node_lists_of_a_hierarchy_at_hand_replace_the_pickle(hip, tmp_path):
    """with hierarchy=, voxels.node_labels_csr serves the node level: the pickle's v_n is not read"""
    from nellie_amd.feature_extraction import FeatureOverlay
    g = og.load("overlay_3d_aniso")
    rows = [int((f > 0).sum()) for f in g["labels"]]
    csr = [(np.concatenate([[0], np.cumsum(np.bincount(e[:, 0], minlength=n))]), e[:, 1]) for e, n in zip(g["edges"]["v_n"], rows)]
    edges = dict(g["edges"], v_n=[np.array([[0, 0]])] * len(rows))                                # a pickle whose node lists are wrong
    im_info = files_of(tmp_path, g["labels"], g["tables"], edges)
    with FeatureOverlay(im_info, hierarchy=SimpleNamespace(voxels=SimpleNamespace(node_labels_csr=csr))) as fo:
        assert fr.same(fo.run("node", "value"), g["frames"]["node"])
        assert fr.same(fo.run("branch", "value"), g["frames"]["branch"])
    with FeatureOverlay(im_info) as fo:
        assert not fr.same(fo.run("node", "value"), g["frames"]["node"])


# ---- 2. the core, where the kernels change over ----------------------------------------------------------------------------------------
def frame_with(shape, n_rows, rng, ends=False):
    """an int32 label frame with n_rows labelled voxels; ends: its first and its last voxel among them"""
    n = int(np.prod(shape))
    pick = rng.permutation(n)[:n_rows] if n_rows < n - 8 else np.setdiff1d(np.arange(n), rng.permutation(n)[:n - n_rows])
    if ends and n_rows >= 2:
        pick = np.concatenate([[0, n - 1], np.setdiff1d(pick, [0, n - 1])[:n_rows - 2]])
    flat = np.zeros(n, np.int32)
    flat[pick] = rng.integers(1, 2 ** 31 - 1, len(pick))
    assert (flat > 0).sum() == n_rows
    return flat.reshape(shape)


def node_edges(n_rows, groups, rng, most=5):
    """unsorted (voxel, group) edges with repeats: 0 .. most groups per voxel; in a large frame at most two (the restatement sums
    longer runs voxel by voxel) but for its first and last 200 voxels"""
    if n_rows == 0:
        return np.zeros((0, 2), np.int64)
    counts = rng.integers(0, most + 1, n_rows)
    if n_rows > 10_000:
        counts[200:-200] = np.minimum(counts[200:-200], 2)
    counts[0] = most
    e = np.column_stack([np.repeat(np.arange(n_rows), counts), rng.integers(0, groups, int(counts.sum()))])
    e = np.concatenate([e, e[: len(e) // 4]])
    return e[rng.permutation(len(e))]


def check_core(frame, rng, groups=37):
    """overlay_values and overlay_frame of one frame at the node level (pairwise and row by row), with one group per voxel, and at
    the voxel level, against the sparse restatement"""
    from nellie_amd.feature_extraction import overlay_frame, overlay_values
    on = frame > 0
    n_rows = int(on.sum())
    cases = []
    for pad in (0, 4):
        vec = rng.normal(size=groups + pad) * 10.0 ** rng.integers(-5, 5, groups + pad)
        vec[rng.random(len(vec)) < 0.2] = np.nan
        cases.append((node_edges(n_rows, groups, rng), vec))
    single = np.column_stack([np.arange(n_rows), rng.integers(0, groups, n_rows)])[rng.random(n_rows) < 0.8]
    cases.append((single, rng.normal(size=groups + 1)))
    for edges, vec in cases:
        e = np.unique(edges, axis=0)
        want = fr.edge_values(n_rows, e, vec) if len(e) else np.full(n_rows, np.nan)
        got = overlay_values(frame, edges, vec)
        assert got.shape == (n_rows,) and fr.same(got, want), (frame.shape, n_rows, len(vec))
        dense = np.full(frame.shape, np.nan)
        dense[on] = want
        assert fr.same(overlay_frame(frame, edges, vec), dense)
        assert fr.same(overlay_frame(frame, edges, vec, dtype=np.float32), dense.astype(np.float32))
    direct = rng.normal(size=n_rows) * 1000.0
    dense = np.full(frame.shape, np.nan)
    dense[on] = direct
    assert fr.same(overlay_values(frame, None, direct), direct) and fr.same(overlay_frame(frame, None, direct), dense)
    assert fr.same(overlay_frame(frame, None, direct, dtype=np.uint64), fr.as_labels(dense))
    assert np.isnan(overlay_frame(frame, None, np.zeros(n_rows + 1))).all()                       # another length: the frame stays NaN


@pytest.mark.parametrize("n_rows", (0, 1, 63, 64, 65))
def test_core_around_one_mask_word(hip, n_rows):
    rng = np.random.default_rng(n_rows)
    check_core(frame_with((3, 7, 11), n_rows, rng), rng)
    check_core(frame_with((3, 7, 11), n_rows, rng, ends=True), rng)


@pytest.mark.parametrize("n_rows", (CHUNK - 1, CHUNK, CHUNK + 1))
def test_core_past_one_scan_workgroup(hip, n_rows):
    """a 65 x 64 x 64 frame labelled but for a few voxels: the rows of the last planes lie behind the first workgroup of the scan"""
    rng = np.random.default_rng(n_rows % 1000)
    frame = frame_with((65, 64, 64), n_rows, rng, ends=True)
    assert frame.nbytes > 10 ** 6
    check_core(frame, rng)


@pytest.mark.parametrize("shape", ((5, 7, 61), (9, 31, 1), (33, 61), (1, 1), (3, 1), (1, 2, 3), (257, 1025)))
def test_core_odd_widths_and_two_dimensions(hip, shape):
    """odd voxel counts end in a scalar tail (one voxel for float64, up to three for float32); the 16-byte stores cross row ends"""
    rng = np.random.default_rng(sum(shape))
    n = int(np.prod(shape))
    for n_rows in sorted({n, n // 2, min(n, 2)}):
        check_core(frame_with(shape, n_rows, rng, ends=True), rng)


def test_core_accepts_exact_label_types_only(hip):
    from nellie_amd.feature_extraction import overlay_values
    frame = np.zeros((4, 6), np.uint8)
    frame[1, 2:5] = 200
    assert fr.same(overlay_values(frame, None, [1.0, 2.0, 3.0]), np.array([1.0, 2.0, 3.0]))
    assert fr.same(overlay_values(frame.astype(np.float64), None, [1.0, 2.0, 3.0]), np.array([1.0, 2.0, 3.0]))
    for bad in (frame + 0.5, np.full((4, 6), 2 ** 31, np.int64)):
        with pytest.raises(ValueError, match="refusing a cast"):
            overlay_values(bad, None, [1.0])
    with pytest.raises(ValueError, match=r"edge 1 \(3, 0\) holds a voxel row beyond the frame's 3"):
        overlay_values(frame, np.array([[0, 0], [3, 0]]), [1.0])
    with pytest.raises(ValueError, match="negative group index"):
        overlay_values(frame, np.array([[0, -1]]), [1.0])
    with pytest.raises(ValueError, match="a column of 1 entries for group indices up to 4"):
        overlay_values(frame, np.array([[0, 4]]), [1.0])
    with pytest.raises(ValueError, match="2-D or 3-D"):
        overlay_values(np.zeros(5, np.int32), None, [])


# ---- 3. node runs ---------------------------------------------------------------------------------------------------------------------------
def runs_case(groups, pad, rng):
    """five voxels with runs of 0, 1, 2, 40 and 40 groups, stored descending and with repeats, as a CSR"""
    runs = [[], [groups - 1], [groups // 2, 0], sorted(rng.choice(groups, 40, replace=False))[::-1], sorted(rng.choice(groups, 40, replace=False))[::-1]]
    runs[3] = list(runs[3]) + list(runs[3][:7])
    off = np.cumsum([0] + [len(r) for r in runs])
    idx = np.array([g for r in runs for g in r], np.int64)
    vec = rng.normal(size=groups + pad) * 10.0 ** rng.integers(-8, 8, groups + pad)
    return off, idx, vec, np.column_stack([np.repeat(np.arange(5), np.diff(off)), idx])


@pytest.mark.parametrize("groups, pad", [(40, 0), (40, 1), (40, 2), (127, 0), (136, 0), (1000, 0), (1000, 5), (8192, 0), (8200, 1), (20000, 0), (20000, 3)])
def test_node_runs_follow_numpys_order(hip, groups, pad):
    """runs of 0, 1, 2 and 40 groups on one voxel each: the sum is numpy's over the dense column -- row by row when the reference's
    matrix was padded by two rows or more, else pairwise trees over pieces of 8192 entries -- checked against the literal dense form"""
    from nellie_amd.feature_extraction import overlay_values
    rng = np.random.default_rng(groups * 7 + pad)
    frame = np.zeros((2, 9), np.int32)
    frame[0, 1:4] = frame[1, 7:9] = 3
    off, idx, vec, edges = runs_case(groups, pad, rng)
    labels = np.arange(len(vec))
    want = fr.literal_values(5, "node", labels, vec, edges)
    assert np.isnan(want[0]) and want[1] == vec[groups - 1] + 0.0 and fr.same(fr.edge_values(5, np.unique(edges, axis=0), vec), want)
    assert fr.same(overlay_values(frame, (off, idx), vec), want)
    assert fr.same(overlay_values(frame, edges[::-1], vec), want)                                # as an edge list, voxels descending
    one = np.zeros((3, 3), np.int32)
    one[1, 1] = 1                                                                                # one voxel: the column is contiguous whatever the padding
    lone = edges[edges[:, 0] == 4] * [0, 1]
    assert fr.same(overlay_values(one, lone, vec), fr.literal_values(1, "node", labels, vec, lone))


def test_runs_of_zeros_and_infinities(hip):
    from nellie_amd.feature_extraction import overlay_values
    frame = np.ones((1, 6), np.int32)
    edges = np.array([[0, 0], [0, 1], [1, 0], [2, 2], [2, 3], [3, 2], [4, 3], [4, 4], [5, 4], [5, 5]])
    vec = np.array([-0.0, -0.0, np.inf, -np.inf, np.nan, -0.0])
    for pad in (0, 1, 3):
        column = np.concatenate([vec, np.full(pad, np.nan)])
        want = fr.literal_values(6, "node", np.arange(len(column)), column, edges)
        got = overlay_values(frame, edges, column)
        assert fr.same(got, want), pad
        assert got[0] == 0 and got[1] == 0 and not np.signbit(got[:2]).any()                       # numpy's sums start from +0.0
        assert np.isnan(got[2]) and got[3] == np.inf and got[4] == -np.inf and got[5] == 0 and not np.signbit(got[5])
    single = np.array([[0, 0], [1, 2], [2, 3], [3, 4]])                                            # one group per voxel: the other kernel
    assert fr.same(overlay_values(frame, single, vec), fr.literal_values(6, "node", np.arange(6), vec, single))


# ---- 4. the resident frame, repeatability ----------------------------------------------------------------------------------------------------
def test_a_second_column_on_the_resident_frame_equals_a_fresh_run(hip, tmp_path):
    from nellie_amd.feature_extraction import FeatureOverlay
    g = og.load("overlay_3d_x70")
    rng = np.random.default_rng(9)
    tables = {lv: cols + (rng.normal(size=len(cols[2])),) for lv, cols in g["tables"].items()}
    im_info = files_of(tmp_path, g["labels"], tables, g["edges"])
    with FeatureOverlay(im_info) as fo, FeatureOverlay(im_info) as fresh:
        assert fo.columns("node") == ["value", "value1"]
        for level in fo.levels:
            first = fo.frame(level, "value", 1)
            state = fo._state
            second = fo.frame(level, "value1", 1)
            assert fo._state is state and state[:2] == (1, None if level == "voxel" else level)      # neither the frame nor the groups went up again
            t_col, label_col, _, other = tables[level]
            want = fr.overlay_sparse(g["labels"], level, t_col, label_col, other, g["edges"].get(fr.EDGE_KEYS.get(level)))[1]
            assert fr.same(second, want) and fr.same(first, g["frames"][level][1]) and not fr.same(first, second), level
            assert fresh.frame(level, "value1", 1).tobytes() == second.tobytes(), level
            assert fr.same(fo.frame(level, "value", 1), first)                                     # and back


def test_two_runs_give_the_same_bytes(hip, tmp_path):
    from nellie_amd.feature_extraction import FeatureOverlay, overlay_frame
    g = og.load("overlay_3d_sparse_flow")
    im_info = files_of(tmp_path, g["labels"], g["tables"], g["edges"])
    runs = []
    for _ in range(2):
        with FeatureOverlay(im_info) as fo:
            runs.append([fo.run(level, "value", dtype=dtype).tobytes() for level in fo.levels for dtype in (np.float64, np.float32)] +
                        [fo.labels(level, "value").tobytes() for level in fo.levels])
    assert runs[0] == runs[1]
    rng = np.random.default_rng(4)
    frame = frame_with((65, 64, 64), CHUNK + 1, rng)
    edges, vec = node_edges(CHUNK + 1, 500, rng), rng.normal(size=500)
    assert overlay_frame(frame, edges, vec).tobytes() == overlay_frame(frame, edges, vec).tobytes()


def test_a_closed_handle_says_so_and_calls_come_in_order(hip):
    from nellie_amd import hipnative
    handle = hipnative.Overlay((4, 5))
    with pytest.raises(hipnative.NellieHipError, match="no frame"):
        handle.groups([0])
    assert handle.load(np.eye(4, 5, dtype=np.int32)) == 4
    with pytest.raises(hipnative.NellieHipError, match="nl_overlay_paint needs"):
        handle.paint()
    with pytest.raises(hipnative.NellieHipError, match="nl_overlay_values needs nl_overlay_groups"):
        handle.values([1.0])
    with pytest.raises(TypeError, match="float64, float32 or uint64"):
        handle.paint(np.int32)
    handle.values_direct([1.0, 2.0, 3.0, 4.0])
    handle.paint()
    assert fr.same(handle.fetch_frame()[np.eye(4, 5) > 0], np.array([1.0, 2.0, 3.0, 4.0]))
    handle.close()
    handle.close()
    with pytest.raises(hipnative.NellieHipError, match="closed"):
        handle.load(np.zeros((4, 5), np.int32))
