"""GPU tests of the voxel level of the hierarchy at sizes where every scan, node and pivot kernel spans workgroups (stacks:
tests/voxel_scenes.py), compared with no tolerance.

The reference is tests/voxel_features_restatement.py fed the device's own interpolation vectors: a separate pair of
FlowInterpolators is asked for the vectors at every frame's voxel coordinates (float64 rows, as the engine's own query kernel
writes them), so the restatement starts from the bits the motility kernel starts from, and from there on both do the same IEEE
operations in float64.  Exact, dtype and shape included: every integer output, both CSR lists, the limits, the NaN pattern of
everything, all 13 float attributes in 3-D and the 8 without an atan2 in 2-D (a value that is not NaN is compared by its bits:
-0.0 is not 0.0).  The five 2-D angular attributes pass through the device library's float64 atan2 and are within one float32
ulp + K_ANGULAR_2D * 2^-52 * S of the restatement.  No voxel is left out of a comparison."""
import numpy as np
import pytest

import voxel_features_restatement as vr
import voxel_goldens as vg
import voxel_scenes as vs
from test_hip_voxels import excess, flow_files, same, scale

pytestmark = pytest.mark.gpu
ANGULAR = ("angular_vel_vector", "angular_vel", "angular_acc", "rel_angular_vel", "rel_angular_acc")
# 8 x the largest measured excess of a 2-D angular attribute over the 2-D scenes of this file on an MI355X against the
# restatement, in units of 2^-52 * S, rounded up to a power of two, never below 1 (DESIGN.md section 13 has the figures).
K_ANGULAR_2D = 16.0


@pytest.fixture(scope="module")
def hip():
    from nellie_amd import build, hipnative
    build.build(verbose=False)
    lib = hipnative.load()
    assert lib.device_count() > 0, "no HIP device"
    return lib


def run_voxels(tmp_path, g):
    from nellie_amd.feature_extraction import Voxels
    h = flow_files(tmp_path, g) if g["T"] > 1 else vg.hierarchy_double(g)
    try:
        v = Voxels(h)
        v.run()
    finally:
        if g["T"] > 1:
            h.flow_interpolator_fw.close()
            h.flow_interpolator_bw.close()
    return v


_RESTATED = {}


def restated(tmp_path, g):
    """the restatement of a stack on the vectors of a pair of FlowInterpolators of its own; computed once per stack and shared"""
    if g["name"] in _RESTATED:
        return _RESTATED[g["name"]]
    vectors = None
    if g["T"] > 1:
        h = flow_files(tmp_path, g)
        vectors = {}
        try:
            for t in range(g["T"]):
                coords = np.argwhere(g["comp"][t] > 0).astype(np.float64)
                for key, fi, exists in (("bw", h.flow_interpolator_bw, t > 0), ("fw", h.flow_interpolator_fw, t < g["T"] - 1)):
                    if exists:
                        vectors[(t, key)] = fi.interpolate_coord(coords, t)          # (0, D): no voxel has a neighbour -> all NaN
        finally:
            h.flow_interpolator_fw.close()
            h.flow_interpolator_bw.close()
    want = vr.voxels(*[g[k] for k in vg.INPUTS], g["flow"], g["spacing"], g["dt"], vectors=vectors)
    _RESTATED[g["name"]] = want
    return want


def same_bits(got, want):
    """shape, dtype and NaN pattern agree, and every value that is not NaN has the same bits"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return np.array_equal(got[ok].view(np.uint32), want[ok].view(np.uint32))


def assert_equals_restatement(g, v, want, frames=None):
    """-> the largest excess per 2-D angular attribute; everything else is compared exactly"""
    worst = {}
    T, D = g["T"], g["D"]
    assert len(v.coords) == T
    for t in (range(T) if frames is None else frames):
        n = len(want["coords"][t])
        assert n == int((g["comp"][t] > 0).sum())
        for k in vg.PER_VOXEL:
            assert same(getattr(v, k)[t], want[k][t]), (k, t)
        for k in vg.FLOAT_ATTRS:
            got, ref = getattr(v, k)[t], want[k][t]
            assert got.dtype == np.float32 and got.shape == ref.shape, (k, t, got.shape, ref.shape)
            if D == 2 and k in ANGULAR:
                worst[k] = max(worst.get(k, 0.0), excess(got, ref, scale(g, k)))
            else:
                assert same_bits(got, ref), (k, t, int(np.sum(got.view(np.uint32) != ref.view(np.uint32))), "values differ")
        lims = want["node_lims"][t]
        for ax, got in enumerate((v.node_dim0_lims[t], v.node_dim1_lims[t], v.node_dim2_lims[t])):
            assert (got is None and ax >= D) or same(got, lims[ax]), ("limits", ax, t)
        for got, csr, ref in ((v.node_voxel_idxs[t], v.node_voxel_idxs_csr[t], want["node_voxels"][t]),
                              (v.node_labels[t], v.node_labels_csr[t], want["voxel_nodes"][t])):
            assert same(csr[0], ref[0]) and same(csr[1], ref[1]), ("CSR", t)
            lists = vg.split_node_lists(*ref)
            assert len(got) == len(lists) and all(same(a, b) for a, b in zip(got, lists)), ("lists", t)
    return worst


def check_angular(name, worst, D, show=True):
    for k, w in sorted(worst.items()):
        if show:
            print(f"{name} {k}: excess {w:.3g} x 2^-52 S")
    assert set(worst) == (set(ANGULAR) if D == 2 else set())
    assert all(w <= K_ANGULAR_2D for w in worst.values()), worst


@pytest.mark.parametrize("name", sorted(vs.SCENES))
def test_scene_equals_the_restatement(hip, tmp_path, name):
    g = vs.stack(name)
    c = vs.assert_scale(g, 1)
    want = restated(tmp_path, g)
    assert max(np.max(np.diff(want["voxel_nodes"][1][0])), 0) >= 16, "the longest per-voxel node list"
    v = run_voxels(tmp_path, g)
    check_angular(name, assert_equals_restatement(g, v, want), g["D"])
    # the comparison is about something: most voxels have a vector, some have none, every large label has a pivot; with
    # whole-voxel flow the pivot's norm is shared, so the lowest index decided
    vec, labels = want["flow_px"][(1, "fw")], want["branch_labels"][1]
    has = ~np.isnan(vec).any(axis=1)
    assert 0.3 < has.mean() < 1.0, has.mean()
    for lbl in (0, int(np.bincount(labels)[1:].argmax()) + 1):
        idx = np.nonzero((labels == lbl) & has)[0]
        assert len(idx) >= 1_000 and want["pivot12"][1][lbl] >= 0
        norm = np.linalg.norm(vec[idx] * g["spacing"], axis=1)
        if name.endswith("-ties"):
            assert np.sum(norm == norm.min()) >= 100 and idx[norm == norm.min()].max() - want["pivot12"][1][lbl] > 256, "a tie across workgroups"
    assert len(v.kernel_ms) == g["T"] and c["voxels"] == len(v.coords[1])


def test_two_runs_give_identical_bits_at_scale(hip, tmp_path):
    g = vs.stack("S3")
    a, b = run_voxels(tmp_path, g), run_voxels(tmp_path, g)
    for k in vg.PER_VOXEL + vg.FLOAT_ATTRS:
        for x, y in zip(getattr(a, k), getattr(b, k)):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k
    for x, y in zip(a.node_labels_csr + a.node_voxel_idxs_csr, b.node_labels_csr + b.node_voxel_idxs_csr):
        assert x[0].tobytes() == y[0].tobytes() and x[1].tobytes() == y[1].tobytes()
    for x, y in zip(a.node_dim0_lims + a.node_dim1_lims + a.node_dim2_lims, b.node_dim0_lims + b.node_dim1_lims + b.node_dim2_lims):
        assert x.tobytes() == y.tobytes()
    assert min(len(c) for c in a.coords) > 12_288 and min(len(c[1]) for c in a.node_labels_csr) > 100_000


def test_uneven_frames_on_one_engine(hip, tmp_path):
    """one engine over frames of very different sizes: nothing of an earlier frame shows in a later one"""
    g = vs.uneven()
    want = restated(tmp_path, g)
    v = run_voxels(tmp_path, g)
    assert assert_equals_restatement(g, v, want) == {}
    n = [len(c) for c in v.coords]
    assert n[1] == n[3] == 0 and n[4] > 3.5 * n[0] and len(v.node_dim0_lims[2]) == 0 and len(v.node_dim0_lims[3]) == len(v.node_dim0_lims[0]) > 0
    assert v.node_labels[1] == [] and v.node_labels[3] == [] and all(len(a) == 0 for a in v.node_voxel_idxs[3])
    assert np.isnan(v.vec12[2]).all() and np.isnan(v.vec01[3]).all() and not np.isnan(v.vec01[2]).all() and not np.isnan(v.vec01[5]).all()
    # the last frame is the first one again: every output that does not depend on t
    for k in ("coords", "x", "y", "z", "intensity", "structure", "branch_labels", "component_labels"):
        assert same(getattr(v, k)[5], getattr(v, k)[0]), k
    for attr in ("node_dim0_lims", "node_dim1_lims", "node_dim2_lims"):
        assert same(getattr(v, attr)[5], getattr(v, attr)[0]), attr
    for attr in ("node_voxel_idxs_csr", "node_labels_csr"):
        assert same(getattr(v, attr)[5][0], getattr(v, attr)[0][0]) and same(getattr(v, attr)[5][1], getattr(v, attr)[0][1]), attr


@pytest.mark.parametrize("shape,full", vs.row_cases(), ids=lambda p: "x".join(map(str, p)) if isinstance(p, tuple) else ("full" if p else "half"))
def test_node_boxes_on_every_row_geometry(hip, tmp_path, shape, full):
    """every voxel a node, rows that end before, at and after a mask word: a box's first voxel at bit 0, its last at bit 63, a box
    inside one word, boxes over whole rows, trunc of negative lower limits, frames smaller than a word or a workgroup"""
    g = vs.rows_stack(shape, full)
    want = restated(tmp_path, g)
    nodes, lims = vr.node_boxes(g["pixel_class"][0], g["distance"][0])
    assert len(nodes) == int(np.prod(shape)) and all(np.array_equal(a, b) for a, b in zip(lims, want["node_lims"][0]))
    v = run_voxels(tmp_path, g)
    check_angular(g["name"], assert_equals_restatement(g, v, want), g["D"], show=False)
    assert all(np.isnan(getattr(v, k)[0]).all() for k in vg.FLOAT_ATTRS)            # one frame: no motility


def test_scan_with_more_than_1024_workgroup_sums(hip):
    """One frame with every voxel labelled, 4 276 800 > 1024 * 4096: the per-voxel scan of the node assignment has 1045 workgroup
    sums and ra_scan_top_kernel gives each lane two of them (its `per >= 2` branch)."""
    from nellie_amd import hipnative
    comp, branch, raw, struct, pixel_class, distance = vs.all_labelled()
    n = comp.size
    coords = np.argwhere(comp > 0)
    _, lims = vr.node_boxes(pixel_class, distance)
    (node_off, node_val), (vox_off, vox_val) = vr.node_assignment(lims, coords)
    with hipnative.VoxelFeatures(comp.shape, vs.SPACING_3D, 1.0) as eng:
        assert eng.frame(comp, branch, raw, struct) == n
        vox, c, b, r, s = eng.fetch_voxels()
        assert eng.nodes(pixel_class, distance) == (48, len(node_val))
        got_lims, node_csr, vox_csr = eng.fetch_nodes()
    # A wrong workgroup offset in the scan of the 66 825 mask words (17 workgroups) moves the rank of every voxel of a chunk: the
    # next five assertions catch it.
    assert same(vox, np.arange(n, dtype=np.int64))
    for got, src in ((c, comp), (b, branch), (r, raw), (s, struct)):
        assert same(got, src.reshape(-1))
    # A wrong offset in the scan of the n per-voxel counts -- 1045 sums, two per lane of ra_scan_top_kernel -- moves the start of
    # every list behind it: this assertion catches it (the nodes sit in sums of 40 lanes and more, at both places of a lane, and
    # the corner node makes the very first sum non-zero).  The comparison of the per-voxel CSR below repeats it through Python's
    # int64 copy.
    lengths = np.diff(vox_off)
    assert same(vox_csr[0][:-1], np.concatenate([[0], np.cumsum(lengths)[:-1]]).astype(np.int64)) and vox_csr[0][-1] == lengths.sum()
    assert all(same(a, b) for a, b in zip(got_lims, lims))
    assert same(node_csr[0], node_off) and same(node_csr[1], node_val)
    assert same(vox_csr[0], vox_off) and same(vox_csr[1], vox_val)
