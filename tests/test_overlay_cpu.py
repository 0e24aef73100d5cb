"""CPU tests of the analysis overlay (nellie_amd.feature_extraction.overlay): the literal restatement
(tests/feature_overlay_restatement.py) against the frames captured from the reference, the sparse restatement against the literal
one, the host rules of the product (column by group index, edge checks, contrast limits) against both, the branch quirk, and the
order of FeatureOverlay's file checks.  Equality is `same`: equal values, NaN in the same places, zeros of the same sign."""
import os
import pickle
from types import SimpleNamespace

import numpy as np
import pytest

import feature_overlay_restatement as fr
import overlay_goldens as og
from nellie_amd.feature_extraction import overlay as ov

NAMES = og.names()


def test_the_fixtures_are_there():
    assert len(NAMES) == 13 and "overlay_3d_aniso_special" in NAMES and "overlay_2d" in NAMES and "overlay_3d_empty_frame" in NAMES


# ---- 1. the restatements and the fixtures ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_literal_and_sparse_restatement_equal_the_reference(name):
    g = og.load(name)
    for level in fr.LEVELS:
        t_col, label_col, val_col = g["tables"][level]
        edges = g["edges"].get(fr.EDGE_KEYS.get(level))
        want = g["frames"][level]
        assert want.shape == g["labels"].shape and want.dtype == np.float64
        assert fr.same(fr.overlay_literal(g["labels"], level, t_col, label_col, val_col, edges), want), level
        assert fr.same(fr.overlay_sparse(g["labels"], level, t_col, label_col, val_col, edges), want), level
        assert fr.contrast_limits(val_col) == g["clim"][level] == ov.contrast_limits(val_col), level


def test_the_fixtures_cover_what_they_should():
    seen = set()
    for name in NAMES:
        g = og.load(name)
        rows = [int((f > 0).sum()) for f in g["labels"]]
        if 0 in rows[1:-1] and rows[0] and rows[-1]:
            seen.add("empty frame between full ones")
        seen.add("2-D" if g["labels"].ndim == 3 else "3-D")
        for t, e in enumerate(g["edges"]["v_n"]):
            per = np.bincount(e[:, 0], minlength=rows[t])
            if rows[t] and per.max() >= 3:
                seen.add("a voxel with three or more nodes")         # the order of the sum matters from three terms on
            if rows[t] and per.min() == 0:
                seen.add("a voxel without a node")
        if not g["edges"]["v_n"]:
            seen.add("no node lists")
        for level in fr.LEVELS:
            v = g["tables"][level][2]
            if np.isnan(v).any() and np.isposinf(v).any() and np.isneginf(v).any() and (np.signbit(v) & (v == 0)).any():
                seen.add("NaN, +-inf and -0.0 in a column")
    assert seen == {"empty frame between full ones", "2-D", "3-D", "a voxel with three or more nodes", "a voxel without a node", "no node lists",
                    "NaN, +-inf and -0.0 in a column"}


def random_case(rng, n_rows, groups, pad):
    """unsorted edges with repeats, a table with repeated labels, labels beyond the groups (pad > 0), groups no table row names, NaN,
    infinities and -0.0 among the values, and voxels whose groups all hold NaN"""
    per = int(rng.integers(1, min(groups, 12) + 1))
    n_edges = n_rows * per
    edges = np.column_stack([rng.integers(0, n_rows, n_edges), rng.integers(0, groups, n_edges)])
    edges = np.concatenate([edges, edges[rng.integers(0, n_edges, n_edges // 3)]])
    edges = edges[rng.permutation(len(edges))]
    n_lab = int(rng.integers(1, groups + pad + 1))
    labels = rng.integers(0, groups + pad, n_lab)
    labels = np.concatenate([labels, labels[: n_lab // 4]])
    vals = rng.normal(size=len(labels)) * 10.0 ** rng.integers(-6, 6, len(labels))
    k = rng.random(len(labels))
    vals[k < 0.15] = np.nan
    vals[(k > 0.15) & (k < 0.18)] = np.inf
    vals[(k > 0.18) & (k < 0.21)] = -np.inf
    vals[(k > 0.21) & (k < 0.30)] = -0.0
    return edges, labels, vals


@pytest.mark.parametrize("seed", range(6))
def test_sparse_restatement_equals_the_literal_one_on_random_cases(seed):
    rng = np.random.default_rng(100 + seed)
    regimes = set()
    for _ in range(40):
        n_rows = int(rng.choice([1, 2, 3, 17, 64, 65, 200, 500]))
        groups = int(rng.choice([1, 2, 5, 7, 8, 9, 17, 40]))
        pad = int(rng.choice([0, 0, 1, 2, 6]))
        edges, labels, vals = random_case(rng, n_rows, groups, pad)
        want = fr.literal_values(n_rows, "node", labels, vals, edges)
        assert fr.same(fr.sparse_values(n_rows, "node", labels, vals, edges), want), (n_rows, groups, pad)
        top = int(edges[:, 1].max()) + 1
        vec = ov.attr_vector(labels, vals, top)
        assert fr.same(vec, fr.attr_vector(labels, vals, top))
        regimes.add(("pairwise" if len(vec) <= top + 1 or n_rows == 1 else "row by row", "some NaN rows" if np.isnan(want).any() else "none"))
    assert {r[0] for r in regimes} == {"pairwise", "row by row"} and ("pairwise", "some NaN rows") in regimes


@pytest.mark.parametrize("groups, pad", [(130, 0), (130, 1), (130, 3), (300, 0), (1000, 2), (9000, 0), (9000, 1), (17000, 0)])
def test_sparse_restatement_follows_numpys_tree_in_long_columns(groups, pad):
    """columns longer than a leaf of numpy's pairwise sum (128) and than its buffer (8192)"""
    rng = np.random.default_rng(groups + pad)
    for n_rows in (1, 6):
        per = 40
        edges = np.column_stack([np.repeat(np.arange(n_rows), per), rng.integers(0, groups, n_rows * per)])
        edges[0, 1] = groups - 1
        labels = np.arange(groups + pad)
        vals = rng.normal(size=groups + pad) * 10.0 ** rng.integers(-8, 8, groups + pad)
        assert fr.same(fr.sparse_values(n_rows, "node", labels, vals, edges), fr.literal_values(n_rows, "node", labels, vals, edges))


def test_frames_the_rule_leaves_nan():
    labels = np.zeros((3, 4, 5), np.int32)
    labels[0, 1, 1:4] = 7
    labels[2, 2, 2] = 1
    edges = [np.array([[0, 0], [1, 0], [2, 1]]), np.zeros((0, 2), np.int64)]                 # frame 1 empty, frame 2 beyond the list
    t_col, label_col, val_col = np.array([0, 0, 2]), np.array([0, 1, 0]), np.array([1.5, 2.5, 9.0])
    for f in (fr.overlay_literal, fr.overlay_sparse):
        got = f(labels, "organelle", t_col, label_col, val_col, edges)
        assert np.array_equal(got[0, 1, 1:4], [1.5, 1.5, 2.5]) and np.isnan(got[1:]).all() and np.isnan(got[0]).sum() == 17
        voxel = f(labels, "voxel", np.array([0, 0, 0, 2, 2]), np.arange(5), np.arange(5.0), None)    # frame 2: two values for one voxel
        assert np.array_equal(voxel[0, 1, 1:4], [0.0, 1.0, 2.0]) and np.isnan(voxel[1:]).all()


# ---- 2. the branch quirk --------------------------------------------------------------------------------------------------------------
def test_branch_quirk_and_align_branches():
    """v_b holds branch label - 1 and the table's label column the branch label: the reference paints branch L with the value of
    branch L - 1 and branch 1 with NaN; align_branches indexes the column by label - 1"""
    frame = np.zeros((1, 3, 6), np.int32)
    frame[0, 1, :] = 1
    branch_of_voxel = np.array([1, 1, 2, 3, 3, 3])
    edges = [np.column_stack([np.arange(6), branch_of_voxel - 1])]
    t_col, label_col, val_col = np.zeros(3, int), np.array([1, 2, 3]), np.array([10.0, 20.0, 30.0])
    quirk = fr.overlay_literal(frame, "branch", t_col, label_col, val_col, edges)[0, 1]
    assert fr.same(quirk, np.array([np.nan, np.nan, 10.0, 20.0, 20.0, 20.0]))
    assert fr.same(fr.overlay_sparse(frame, "branch", t_col, label_col, val_col, edges)[0, 1], quirk)
    aligned = fr.overlay_sparse(frame, "branch", t_col, label_col, val_col, edges, align_branches=True)[0, 1]
    assert fr.same(aligned, np.array([10.0, 10.0, 20.0, 30.0, 30.0, 30.0]))
    assert fr.same(ov.attr_vector(label_col, val_col, 3), np.array([np.nan, 10.0, 20.0, 30.0]))
    assert fr.same(ov.attr_vector(label_col, val_col, 3, shift=1), np.array([10.0, 20.0, 30.0]))
    with pytest.raises(ValueError, match="table row 1 holds label 0"):
        ov.attr_vector([2, 0], [1.0, 2.0], 3, shift=1)


# ---- 3. contrast limits -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("column, want", [
    ([], [0.0, 1.0]),                                                          # no values
    ([np.nan, np.inf, -np.inf], [0.0, 1.0]),                                   # none that is finite
    ([0.0, 0.0, 0.0], [0.0, 0.0]),                                             # min == percentile, and 0.01 |min| is 0
    ([-2.0, -2.0], [-2.02, -2.0]),                                             # the shrunk minimum differs from the percentile
    ([5.0], [4.95, 5.0]),
    ([-0.0, np.nan, 4.0, np.inf], [-0.0, float(np.percentile([-0.0, 4.0], 98))]),
])
def test_contrast_limits_in_every_branch(column, want):
    assert ov.contrast_limits(column) == want == fr.contrast_limits(column)


def test_contrast_limits_of_ordinary_columns():
    rng = np.random.default_rng(2)
    v = rng.normal(size=1000) * 50
    lo, hi = ov.contrast_limits(v)
    assert lo == v.min() - abs(v.min()) * 0.01 and hi == np.percentile(v, 98) and [lo, hi] == fr.contrast_limits(v)
    ints = np.arange(100)                                                       # an integer column, as pandas reads a label column
    assert ov.contrast_limits(ints) == fr.contrast_limits(ints) == [0.0, float(np.percentile(ints, 98))]


# ---- 4. the error cases ------------------------------------------------------------------------------------------------------------------
def test_edge_lists_are_checked_and_sorted():
    good = np.array([[2, 5], [0, 1], [2, 3], [0, 9], [1, 1]])
    got = ov.check_edges(good, 3)
    assert got.dtype == np.int64 and np.array_equal(got, [[0, 1], [0, 9], [1, 1], [2, 5], [2, 3]])        # stable: a voxel's groups keep their order
    off, idx = ov.edges_to_csr(got, 4)
    assert np.array_equal(off, [0, 2, 3, 5, 5]) and idx.dtype == np.int32 and np.array_equal(idx, [1, 9, 1, 5, 3])
    assert ov.check_edges(np.zeros((0, 2)), 0).shape == (0, 2)
    for bad, match in (([[0, 1], [1, -1]], r"edge 1 \(1, -1\) holds a negative group index"), ([[0, 1], [-2, 1]], r"edge 1 \(-2, 1\) holds a negative voxel row"),
                       ([[0, 1], [1, 1], [3, 0]], r"edge 2 \(3, 0\) holds a voxel row beyond the frame's 3"), ([[0, 2 ** 31 - 1]], "above")):
        with pytest.raises(ValueError, match=match):
            ov.check_edges(np.array(bad), 3)
    with pytest.raises(ValueError, match="refusing a cast"):
        ov.check_edges(np.array([[0.5, 1.0]]), 3)
    with pytest.raises(ValueError, match=r"\(E, 2\)"):
        ov.check_edges(np.zeros((3, 3), np.int64), 3)
    with pytest.raises(ValueError, match="table row 2 holds label -4: a negative label"):
        ov.attr_vector([1, 2, -4], [1.0, 2.0, 3.0], 5)
    with pytest.raises(ValueError, match="entry 1 of the CSR holds group index -1"):
        ov.check_csr([0, 2], [3, -1], 1)
    for off in ([0, 1], [1, 2, 2], [0, 2, 1], [0, 1, 3]):
        with pytest.raises(ValueError, match="offsets"):
            ov.check_csr(off, [4, 5], 2)


def test_attr_vector_keeps_the_last_row_of_a_repeated_label():
    vec = ov.attr_vector(np.array([3.0, 1.0, 3.0, 0.0]), [1.0, 2.0, np.nan, -0.0], 2)           # float labels, as the table holds them
    assert fr.same(vec, np.array([-0.0, 2.0, np.nan, np.nan]))
    assert fr.same(ov.attr_vector([], [], 3), np.full(3, np.nan)) and len(ov.attr_vector([7], [1.0], 3)) == 8


# ---- 5. files first, device second --------------------------------------------------------------------------------------------------------
def test_a_missing_file_is_named_before_any_device_work(tmp_path, monkeypatch):
    import pandas as pd
    from nellie_amd import hipnative
    from nellie_amd.feature_extraction import FeatureOverlay

    def touched(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(ov, "require_gpu", touched)
    monkeypatch.setattr(hipnative, "Overlay", touched)
    keys = ["im_instance_label", "adjacency_maps"] + list(ov.TABLE_KEYS.values())
    paths = {k: str(tmp_path / (k + ".bin")) for k in keys}
    im_info = SimpleNamespace(no_t=False, no_z=True, axes="TYX", shape=(2, 4, 4), pipeline_paths=paths, get_memmap=lambda p: np.zeros((2, 4, 4), np.int32))
    with FeatureOverlay(im_info) as fo:
        assert fo.levels == ("voxel", "node", "branch", "organelle")
        with pytest.raises(FileNotFoundError, match="features_branches"):
            fo.columns("branch")
        pd.DataFrame({"t": [0], "label": [1], "length": [2.0]}).to_csv(paths["features_branches"], index=False)
        assert fo.columns("branch") == ["length"] and fo.contrast_limits("branch", "length") == [1.98, 2.0]
        with pytest.raises(FileNotFoundError, match="adjacency_maps"):
            fo.values("branch", "length", 0)
        with open(paths["adjacency_maps"], "wb") as f:
            pickle.dump({"v_b": [np.zeros((0, 2), np.int64)] * 2}, f)
        with pytest.raises(FileNotFoundError, match="im_instance_label"):
            fo.frame("branch", "length", 0)
        with pytest.raises(KeyError, match="no column 'width'"):
            fo.values("branch", "width", 0)
        with pytest.raises(ValueError, match="no level 'image'"):
            fo.columns("image")
        open(paths["im_instance_label"], "wb").close()
        with pytest.raises(AssertionError, match="the device was touched"):
            fo.values("branch", "length", 0)
    assert os.path.exists(paths["features_branches"])
