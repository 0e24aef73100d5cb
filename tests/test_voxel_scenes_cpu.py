"""The stacks of tests/voxel_scenes.py without a GPU: every scene of tests/test_hip_voxels_scale.py is built, the counts and
thresholds that make its kernels span workgroups are asserted, the numpy restatement runs on the large stacks with made-up flow
vectors, and the generator gives the same stack for the same seed."""
import numpy as np
import pytest

import voxel_features_restatement as vr
import voxel_scenes as vs

RA_SCAN_CHUNK = vs.RA_SCAN_CHUNK


@pytest.mark.parametrize("name", sorted(vs.SCENES))
def test_large_scenes_meet_their_requirements(name):
    g = vs.stack(name)
    assert g["T"] == 3 and g["comp"].dtype == g["branch"].dtype == np.int32
    for t in range(g["T"]):                                       # asked of the middle frame; these stacks meet them in every frame
        c = vs.assert_scale(g, t)
    assert vs.longest_list(g, 1) >= 16
    D = g["D"]
    flow = g["flow"]
    assert flow.shape[1] == 2 * D + 2 and set(np.unique(flow[:, 0])) == {0.0, 1.0}
    at = tuple(flow[flow[:, 0] == 1.0][:, 1:1 + D].astype(int).T)
    assert (g["comp"][1][at] > 0).all(), "flow rows sit at labelled voxels"
    assert (g["raw"][g["comp"] > 0] > 0).mean() > 0.9 and 0.01 < (g["raw"][g["comp"] == 0] > 0).mean() < 0.03
    ties = name.endswith("-ties")
    assert np.array_equal(flow[:, 1 + D:1 + 2 * D], np.round(flow[:, 1 + D:1 + 2 * D])) == ties
    if name == "S3-ties":
        assert g["dt"] == 0.5 and g["distance"].dtype == np.float64 and g["pixel_class"].dtype.kind == "i" and c["negative_classes"] > 0
    if name == "S3":
        assert g["raw"].dtype == np.uint16 and g["struct"].dtype == np.float32 and g["comp"].shape[1:] == (20, 120, 130) and g["dt"] == 1.0
    if name.startswith("S2"):
        assert g["raw"].dtype == np.float32 and g["struct"].dtype == np.float64 and g["comp"].shape[1:] == (600, 700) and g["dt"] == 1.7


def made_up_vectors(g, seed):
    """whole-voxel or fractional vectors per label at 70 % of the voxels, NaN rows elsewhere"""
    rng = np.random.default_rng(seed)
    vectors = {}
    for t in range(g["T"]):
        n = int((g["comp"][t] > 0).sum())
        for key in ("bw", "fw"):
            v = np.round(rng.uniform(-2, 2, (n, g["D"]))) if key == "bw" else rng.uniform(-2, 2, (n, g["D"]))
            v[rng.random(n) < 0.3] = np.nan
            vectors[(t, key)] = v
    return vectors


@pytest.mark.parametrize("name", ["S3", "S2"])
def test_restatement_runs_on_the_large_scenes(name):
    g = vs.stack(name)
    out = vr.voxels(*[g[k] for k in ("comp", "branch", "raw", "struct", "pixel_class", "distance")], g["flow"], g["spacing"], g["dt"],
                    vectors=made_up_vectors(g, 3))
    for t in range(g["T"]):
        n = len(out["coords"][t])
        assert n == int((g["comp"][t] > 0).sum())
        (noff, nval), (voff, vval) = out["node_voxels"][t], out["voxel_nodes"][t]
        assert len(noff) == vs.counts(g, t)["nodes"] + 1 and len(voff) == n + 1 and noff[-1] == voff[-1] == len(nval) == len(vval)
        for k in vr.FLOAT_ATTRS:
            assert out[k][t].dtype == np.float32 and len(out[k][t]) == n, k
        has = ~np.isnan(out["vec12" if t < g["T"] - 1 else "vec01"][t]).any(axis=1)
        assert 0.6 < has.mean() < 0.8
        assert np.isfinite(out["rel_linear_vel" if t < g["T"] - 1 else "vec01"][t][has]).all()
    # the whole-voxel backward vectors of a large label share their smallest norm: the pivot is the first voxel that holds it
    t = 1
    big = np.bincount(out["branch_labels"][t]).argmax()
    idx = np.nonzero(out["branch_labels"][t] == big)[0]
    norm = np.linalg.norm(out["flow_px"][(t, "bw")][idx] * g["spacing"], axis=1)
    assert len(idx) >= 3_000 and np.sum(norm == np.nanmin(norm)) > 1 and out["pivot01"][t][big] == idx[np.nanargmin(norm)]


def test_generator_is_deterministic():
    a, b = vs.build("S3"), vs.build("S3")
    assert a is not b
    for k in ("comp", "branch", "raw", "struct", "pixel_class", "distance", "flow"):
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k
    c = vs.SCENES["S3"]
    other = vs.draw(np.random.default_rng(c["seed"] + 1), c["shape"], 3, c["spacing"], **c["draw"])
    assert not np.array_equal(other[1], a["comp"])
    u, v = vs.uneven(), vs.uneven()
    assert all(u[k].tobytes() == v[k].tobytes() for k in ("comp", "branch", "raw", "struct", "pixel_class", "distance", "flow"))


def test_uneven_stack():
    g = vs.uneven()
    assert g["T"] == 6 and g["comp"].shape[1:] == (12, 48, 70)
    c = [vs.counts(g, t) for t in range(6)]
    assert c[0]["voxels"] > 1000 and c[0]["nodes"] > 200
    assert c[1]["voxels"] == 0 and c[1]["nodes"] == 0 and not g["raw"][1].any()
    assert c[2]["voxels"] > 1000 and c[2]["nodes"] == 0
    assert c[3]["voxels"] == 0 and c[3]["nodes"] == c[0]["nodes"]
    assert c[4]["voxels"] > 3.5 * c[0]["voxels"] and c[4]["nodes"] > 3.5 * c[0]["nodes"] and c[4]["max_label"] > 3.5 * c[0]["max_label"]
    for k in ("comp", "branch", "raw", "struct", "pixel_class", "distance"):
        assert np.array_equal(g[k][5], g[k][0]), k
    assert sorted(set(g["flow"][:, 0])) == [0.0, 1.0, 3.0, 4.0]       # no rows at the middle time point 2


def test_row_geometry_stacks():
    cases = vs.row_cases()
    assert len(cases) == 2 * (7 + 2) and {s[-1] for s, _ in cases} == {2, 63, 64, 65, 127, 128, 129}
    for shape, full in cases:
        g = vs.rows_stack(shape, full)
        n = int(np.prod(shape))
        assert n <= 2_000 and (g["pixel_class"] > 0).all() and g["T"] == 1
        share = (g["comp"] > 0).mean()
        assert share == 1.0 if full else 0.3 < share < 0.7
        radii = g["distance"].reshape(-1)
        assert radii.dtype == np.float32 and np.array_equal(radii[:7], np.array([0, 0.5, 1.0, 1.5, 1.99, 2.0, shape[-1]], np.float32))
        _, lims = vr.node_boxes(g["pixel_class"][0], g["distance"][0])
        last = lims[-1]
        assert (last[:, 0] == 0).any() and (last[:, 1] == shape[-1]).any()
        if shape[-1] >= 63:
            assert ((last[:, 1] - last[:, 0] < 6) & (last[:, 0] > 0)).any()     # a box inside one word


def test_all_labelled_frame():
    comp, branch, raw, struct, pixel_class, distance = vs.all_labelled()
    n = comp.size
    assert comp.shape == (33, 360, 360) and n > 1024 * RA_SCAN_CHUNK and (comp > 0).all()
    assert (n + RA_SCAN_CHUNK - 1) // RA_SCAN_CHUNK > 1024          # ra_scan_top_kernel takes two sums per lane
    nodes = np.flatnonzero(pixel_class)
    assert len(nodes) == 48 and nodes[0] == 0 and nodes[-1] == n - 1 and distance.max() <= 3.0 and raw.dtype == np.uint8
    # a lane of ra_scan_top_kernel owns the sums 2 k and 2 k + 1: nodes in the sums of 40 lanes or more, at both places of a lane
    chunks = nodes // RA_SCAN_CHUNK
    assert len(set(chunks // 2)) >= 40 and (chunks % 2 == 0).sum() >= 10 and (chunks % 2 == 1).sum() >= 10
