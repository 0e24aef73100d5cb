"""CPU tests of the branch level of the hierarchy: the numpy restatement (tests/branch_features_restatement.py) against every golden
of the reference's Branches (tests/golden/branches), its region columns against closed forms on boxes, the reassigned-label mode on
ties and zeros, the package's per-branch host arithmetic (feature_extraction/branches.py: what is left once the device has touched
the voxels) against the restatement, and the text of features_branches.  The GPU tests (tests/test_hip_branches.py) lean on these."""
from types import SimpleNamespace

import numpy as np
import pytest

import branch_features_restatement as br
import branch_goldens as bg

NAMES = bg.names()


def test_the_public_names_exist():
    from nellie_amd import feature_extraction as fe
    assert {"Branches", "BranchFeatures", "Nodes", "NodeFeatures", "aggregate_stats_for_class", "Voxels", "VoxelFeatures"} <= set(fe.__all__)
    assert fe.Branches.__module__ == fe.BranchFeatures.__module__ == "nellie_amd.feature_extraction.branches"
    assert issubclass(fe.BranchFeatures, fe.NodeFeatures)
    b = fe.Branches(SimpleNamespace())
    assert b.stats_to_aggregate == bg.STATS_TO_AGGREGATE and b.features_to_save == bg.STATS_TO_AGGREGATE + ["x", "y", "z"]


def test_the_goldens_cover_the_cases():
    assert len(NAMES) == 12 and [n[len("branches_"):] for n in NAMES] == [n[len("nodes_"):] for n in bg.ng.names()]
    counts = {name: [len(a) for a in bg.load(name)["ref"]["branch_label"]] for name in NAMES}
    assert counts["branches_3d_empty_frame"][2] == 0 and all(counts["branches_3d_empty_frame"][t] for t in (0, 1, 3))
    assert bg.load("branches_3d_skip_nodes")["ref"]["agg_node"] == [] and bg.load("branches_3d_skip_nodes")["base"]["skip_nodes"]
    dims = {bg.load(name)["base"]["D"] for name in NAMES}
    assert dims == {2, 3} and len(set(bg.load("branches_3d_aniso")["base"]["spacing"])) > 1
    borders = [bg.load(name)["border"][t] for name in NAMES for t in range(4)]
    assert any(not b.any() for b in borders) and any(b.sum() == 1 and b.reshape(-1)[-1] for b in borders)
    seen = set()
    for name in NAMES:
        g = bg.load(name)
        ref = g["ref"]
        for t in range(g["base"]["T"]):
            if len(ref["branch_label"][t]) == 0:
                continue
            sk = br.skeleton_stats(g["skel"][t], g["border"][t], g["base"]["spacing"])
            for i, l in enumerate(sk["branch_label"]):
                mine = sk["labels"] == l
                tips = int((sk["degree"][mine] == 1).sum())
                seen.add(f"{min(tips, 3)} tips" if mine.sum() > 1 else "lone")
                seen.add("even" if mine.sum() % 2 == 0 else "odd")
                if np.isnan(ref["branch_aspect_ratio"][t][i]) and ref["branch_thickness"][t][i] == 0:
                    seen.add("radius 0")
            med = np.array([np.median(2.0 * sk["radius"][sk["labels"] == l]) for l in sk["branch_label"]]).astype(np.float32)
            if np.any((med != ref["branch_thickness"][t]) & ~np.isnan(med)):
                seen.add("swap")
    assert seen == {"lone", "0 tips", "1 tips", "2 tips", "3 tips", "even", "odd", "radius 0", "swap"}


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_golden(name):
    g = bg.load(name)
    own = br.Branches(bg.double_of(g))
    own.run(regions=False)
    bg.assert_same_skeleton(own, g["ref"], g["base"])


def fetched(skel, border, spacing):
    """what hipnative.BranchFeatures.fetch returns, from the restatement's per-voxel quantities"""
    sk = br.skeleton_stats(skel, border, spacing)
    lab = sk["labels"]
    with np.errstate(all="ignore"):
        median = np.array([np.median(2.0 * sk["radius"][lab == l]) for l in sk["branch_label"]])
    return dict(coords=sk["branch_idxs"], labels=lab.astype(np.int64), degree=sk["degree"], radius=sk["radius"], tips=sk["tips"], lone=sk["lone"],
                branch_label=sk["branch_label"].astype(np.int64), edges=sk["pair_counts"].astype(np.uint32), median=median), sk


def region_sums(lab):
    """what hipnative.BranchFeatures.fetch_regions returns, by numpy"""
    D = lab.ndim
    labels = np.unique(lab[lab > 0])
    rows = []
    for l in labels:
        c = np.argwhere(lab == l)
        rows.append([len(c)] + list(c.min(axis=0)) + list(c.max(axis=0)) + list(c.sum(axis=0)) +
                    [int((c[:, a] * c[:, b]).sum()) for a in range(D) for b in range(a, D)])
    return labels.astype(np.int64), np.array(rows, np.int64).reshape(len(labels), 1 + 3 * D + D * (D + 1) // 2).T


@pytest.mark.parametrize("name", NAMES)
def test_host_arithmetic_of_the_package_equals_the_golden(name):
    """skeleton_columns and region_columns of the package on per-voxel inputs computed by numpy: the float32 statistics equal the
    reference's, the region columns the restatement's, bit for bit"""
    from nellie_amd.feature_extraction import branches as pkg
    g = bg.load(name)
    base = g["base"]
    for t in range(base["T"]):
        if len(g["ref"]["branch_label"][t]) == 0:
            continue
        f, _ = fetched(g["skel"][t], g["border"][t], base["spacing"])
        cols = pkg.skeleton_columns(f, base["spacing"], base["D"])
        for k in bg.FLOAT32:
            assert bg.same(cols[k], g["ref"][k][t]), (k, t)
        labels, sums = region_sums(base["branch"][t])
        rng = np.random.default_rng(t)
        re = rng.integers(0, 4, base["branch"][t].shape).astype(np.int32)
        want = br.region_columns(base["branch"][t], base["spacing"], re)
        mode = np.array([br.reassigned_mode(re[base["branch"][t] == l]) for l in labels], np.int64)
        got = pkg.region_columns(sums, mode, base["spacing"], base["D"])
        assert np.array_equal(labels, want["label"])
        for k in bg.REGION:
            assert got[k].dtype == np.float64 and bg.same(got[k], want[k]), (k, t)
        none = pkg.region_columns(sums, np.full(len(labels), -1, np.int64), base["spacing"], base["D"])
        assert np.isnan(none["reassigned_label"]).all() and np.isnan(none["branch_solidity"]).all()


def test_label_groups_are_the_references_lists():
    from nellie_amd.feature_extraction.branches import _label_groups
    rng = np.random.default_rng(4)
    for labels in (rng.integers(0, 6, 200), rng.integers(0, 2_000_000, 500).astype(np.int32), np.zeros(7, np.int32), np.zeros(0, np.int32),
                   np.array([5, 0, -3, 5, -3, 9], np.int64)):
        off, idx = _label_groups(labels)
        want_off, want_idx = br.label_groups(labels)
        assert np.array_equal(off, want_off) and np.array_equal(idx, want_idx) and off.dtype == idx.dtype == np.int64


BOXES = [((3, 4, 5), (2, 1, 7), (0.3, 0.1, 0.1)), ((1, 1, 1), (0, 0, 0), (0.2, 0.1, 0.1)), ((7, 2, 9), (1, 30, 3), (0.29, 0.0973, 0.0973)),
         ((4, 6), (3, 2), (0.107, 0.083)), ((1, 9), (0, 0), (0.1, 0.1)), ((5, 5, 5), (20000, 30000, 32000), (0.25, 0.1, 0.1))]


@pytest.mark.parametrize("size,corner,spacing", BOXES)
def test_region_columns_on_boxes(size, corner, spacing):
    """an a x b x c box with spacing s: area a b c P, extent 1, the centroid in the middle, C_aa = (a^2 - 1) / 12 s_a^2 and C_ab = 0,
    so the axis lengths are sqrt(20 max C_aa) and sqrt(20 min C_aa) (3-D) or 4 sqrt(.) (2-D) -- to 1e-12 relative: a handful of
    float64 operations on exact integers.  The box far from the origin has coordinates whose squares cancel in n Q - S S."""
    from nellie_amd.feature_extraction import branches as pkg
    D = len(size)
    shape = tuple(c + a + 2 for a, c in zip(size, corner))
    if np.prod(shape) > 1e7:                                       # the far box: its sums without its volume
        c = np.stack(np.meshgrid(*[np.arange(k, k + a) for a, k in zip(size, corner)], indexing="ij"), axis=-1).reshape(-1, D)
        sums = np.array([len(c)] + list(c.min(axis=0)) + list(c.max(axis=0)) + list(c.sum(axis=0)) +
                        [int((c[:, a] * c[:, b]).sum()) for a in range(D) for b in range(a, D)], np.int64)[:, None]
        results = [pkg.region_columns(sums, np.array([-1]), spacing, D)]
    else:
        lab = np.zeros(shape, np.int32)
        lab[tuple(slice(k, k + a) for a, k in zip(size, corner))] = 9
        _, sums = region_sums(lab)
        results = [br.region_columns(lab, spacing), pkg.region_columns(sums, np.array([-1]), spacing, D)]
    P = float(np.prod(spacing))
    var = [(a * a - 1) / 12.0 * s * s for a, s in zip(size, spacing)]
    scale = (lambda v: np.sqrt(20.0 * v)) if D == 3 else (lambda v: 4.0 * np.sqrt(v))
    for cols in results:
        assert cols["branch_area"][0] == pytest.approx(np.prod(size) * P, rel=1e-12)
        assert cols["branch_extent"][0] == pytest.approx(1.0, rel=1e-12)
        for ax in range(D):
            assert cols["zyx"[3 - D + ax]][0] == pytest.approx((corner[ax] + (size[ax] - 1) / 2.0) * spacing[ax], rel=1e-12)
        assert np.isnan(cols["z"][0]) == (D == 2)
        assert cols["branch_axis_length_maj"][0] == pytest.approx(scale(max(var)), rel=1e-12, abs=0 if max(var) else 1e-300)
        assert cols["branch_axis_length_min"][0] == pytest.approx(scale(min(var)), rel=1e-12, abs=0 if min(var) else 1e-300)
        assert np.isnan(cols["branch_solidity"][0]) and np.isnan(cols["reassigned_label"][0])


def test_reassigned_mode_on_ties_and_zeros():
    for values in ([0, 0, 3, 3, 7], [5, 2, 2, 5], [0], [4, 4, 0, 0, 0], [9, 1, 1, 9, 9, 1], [2_000_000, 7, 2_000_000]):
        assert br.reassigned_mode(values) == int(np.argmax(np.bincount(values))), values
    lab = np.zeros((4, 6), np.int32)
    lab[0, :4], lab[2, 1:5], lab[3, 0] = 3, 8, 11
    re = np.zeros((4, 6), np.int32)
    re[0, :4] = (6, 2, 2, 6)                                       # a tie: the smaller
    re[2, 1:5] = (0, 0, 5, 5)                                      # zeros count, and win the tie
    re[3, 0] = 0
    cols = br.region_columns(lab, (0.1, 0.1), re)
    assert cols["label"].tolist() == [3, 8, 11] and cols["reassigned_label"].tolist() == [2.0, 0.0, 0.0]
    assert np.isnan(br.region_columns(lab, (0.1, 0.1))["reassigned_label"]).all()


def test_the_branch_table_has_the_reference_columns():
    from nellie_amd.feature_extraction.hierarchy import feature_frames
    g = bg.load("branches_3d_integer_flow")                      # every frame has as many node labels as branches
    own = br.Branches(bg.double_of(g))
    own.run()
    header, text = br.feature_table(own)
    vox = g["base"]["ref"]["stats_to_aggregate"]
    want = ["t", "label"] + [f"{s}_{k}" for s in bg.NODE_STATS + vox for k in bg.KEYS] + [f"{s}_raw" for s in bg.STATS_TO_AGGREGATE + ["x", "y", "z"]]
    assert header == want and len(header) == 2 + 20 + 55 + 13
    lines = text.splitlines()
    assert lines[0] == ",".join(want) and len(lines) == 1 + sum(len(a) for a in g["ref"]["branch_label"])
    rows = np.array([[float(x) if x else np.nan for x in line.split(",")] for line in lines[1:]])
    assert np.array_equal(rows[:, 1], np.concatenate(g["ref"]["branch_label"]))
    assert np.array_equal(rows[:, header.index("branch_length_raw")], np.concatenate(g["ref"]["branch_length"]).astype(np.float64), equal_nan=True)
    assert np.array_equal(rows[:, 2], np.concatenate([f["divergence"]["mean"][0] for f in g["ref"]["agg_node"]]), equal_nan=True)
    frames = list(feature_frames(own, own.branch_label))           # the package's saving rule on the same object: the same arrays
    assert [t for t, _, _ in frames] == [0, 1, 2, 3] and all(names == want for _, _, names in frames)
    assert np.array_equal(np.concatenate([a for _, a, _ in frames]), rows, equal_nan=True)


def test_the_branch_table_skips_empty_frames_and_refuses_ragged_ones():
    from nellie_amd.feature_extraction.hierarchy import feature_frames
    g = bg.load("branches_3d_empty_frame")
    own = br.Branches(bg.double_of(g, skip_nodes=True))
    own.run()
    header, text = br.feature_table(own)
    counts = [len(a) for a in g["ref"]["branch_label"]]
    assert len(header) == 2 + 55 + 13 and header[2] == "linear_vel_mean"
    rows = np.array([[float(x) if x else np.nan for x in line.split(",")] for line in text.splitlines()[1:]])
    assert rows[:, 0].tolist() == [t for t, n in enumerate(counts) for _ in range(n)] and counts[2] == 0      # the empty frame writes no rows
    frames = list(feature_frames(own, own.branch_label))
    assert [t for t, _, _ in frames] == [0, 1, 3] and np.array_equal(np.concatenate([a for _, a, _ in frames]), rows, equal_nan=True)
    own.branch_area[1] = own.branch_area[1][:-1]                  # a region less than skeleton labels
    with pytest.raises(ValueError, match="differ in length"):
        list(feature_frames(own, own.branch_label))
    ragged = br.Branches(bg.double_of(g))                         # frame 3: three node labels for five branches, as in the reference
    ragged.run()
    assert ragged.aggregate_node_metrics[3]["divergence"]["sum"].shape == (1, 3) and counts[3] == 5
    with pytest.raises(ValueError, match="differ in length"):
        list(feature_frames(ragged, ragged.branch_label))
    with pytest.raises(ValueError):
        br.feature_table(ragged)                                  # numpy refuses the ragged array the reference would build
