"""GPU tests of the branch level of the hierarchy (nellie_amd.feature_extraction.branches, csrc/branchfeat.inc): every golden of the
reference's Branches through the public `Branches`, one frame at the scale where every scan spans workgroups and one label is
larger than a workgroup's LDS could sort, ragged row widths with voxels on every face and corner, the reassigned label, uneven
frames on one handle, the branch table through `BranchFeatures` on files, determinism and the errors.

Everything is compared for equality: integers, and every float32 and float64 bit for bit, the NaN pattern included (a NaN equals a
NaN of another sign or payload).  Goldens hold what the reference computes without regionprops; the region columns, the reassigned
label and everything without a golden are compared against tests/branch_features_restatement.py, which equals the goldens bit for
bit (tests/test_branches_cpu.py).  No branch is left out of a comparison."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import branch_features_restatement as br
import branch_goldens as bg
import voxel_scenes as vs

pytestmark = pytest.mark.gpu
NAMES = bg.names()
VOXEL_STATS = ["linear_vel", "angular_vel", "linear_acc", "angular_acc", "rel_linear_vel", "rel_angular_vel", "rel_linear_acc", "rel_angular_acc",
               "rel_directionality", "structure", "intensity"]
PARTS = {"skeleton", "degree", "radii", "lists", "regions", "aggregation"}


@pytest.fixture(scope="module")
def hip():
    from nellie_amd import build, hipnative
    build.build(verbose=False)
    lib = hipnative.load()
    assert lib.device_count() > 0, "no HIP device"
    return lib


def run_branches(h):
    from nellie_amd.feature_extraction import Branches
    branches = Branches(h)
    branches.run()
    assert branches._engine is None and branches._aggregator is None
    return branches


def restated(h):
    own = br.Branches(h)
    own.run()
    return own


def assert_same(got, own, g, frames=None):
    bg.assert_same_skeleton(got, own, g, frames)
    bg.assert_same_regions(got, own, frames)


def plain_levels(g, seed):
    """plain `voxels` and `nodes` objects for the stack g: the labelled voxels and the nodes (pixel class > 0) in raster order with
    their branch labels, and random statistics (float32 for the voxels, float64 for the nodes) with a fifth of the rows NaN"""
    rng = np.random.default_rng(seed)
    v = SimpleNamespace(stats_to_aggregate=list(VOXEL_STATS), branch_labels=[], **{s: [] for s in VOXEL_STATS})
    n = SimpleNamespace(stats_to_aggregate=list(bg.NODE_STATS), branch_label=[], **{s: [] for s in bg.NODE_STATS})
    for t in range(g["T"]):
        for level, mask, names, dtype, key in ((v, g["comp"][t] > 0, VOXEL_STATS, np.float32, "branch_labels"),
                                               (n, g["pixel_class"][t] > 0, bg.NODE_STATS, np.float64, "branch_label")):
            at = np.argwhere(mask)
            getattr(level, key).append(g["branch"][t][tuple(at.T)])
            for s in names:
                x = (rng.standard_normal(len(at)) * 10.0 ** rng.integers(-2, 3, len(at))).astype(dtype)
                x[rng.random(len(at)) < 0.2] = np.nan
                getattr(level, s).append(x)
    return v, n


def row_skeleton(branch, rng, dense=()):
    """a skeleton for a branch-label frame: of every label the voxels in the row of its first voxel (a straight path, in pieces where
    the label is not convex) thinned by a tenth; of the labels in `dense` nine voxels out of ten"""
    flat = branch.reshape(-1)
    at = np.flatnonzero(flat > 0)
    labels, first = np.unique(flat[at], return_index=True)
    row = at // branch.shape[-1]
    keep = row == row[first][np.searchsorted(labels, flat[at])]
    keep &= rng.random(len(at)) < 0.9
    keep[first] = True                                             # every label keeps a voxel
    for l in dense:
        mine = flat[at] == l
        keep[mine] = rng.random(int(mine.sum())) < 0.9
    skel = np.zeros_like(flat)
    skel[at[keep]] = flat[at[keep]]
    return skel.reshape(branch.shape)


def shell(comp):
    border = np.zeros(comp.shape, np.uint8)
    for t in range(len(comp)):
        on = comp[t] > 0
        near = np.zeros_like(on)
        for ax in range(on.ndim):
            near[(slice(None),) * ax + (slice(1, None),)] |= on[(slice(None),) * ax + (slice(None, -1),)]
            near[(slice(None),) * ax + (slice(None, -1),)] |= on[(slice(None),) * ax + (slice(1, None),)]
        border[t] = near & ~on
    return border


@pytest.mark.parametrize("name", NAMES)
def test_golden(hip, name):
    g = bg.load(name)
    for low_memory in (False, True):                              # accepted and ignored: the values of the default path
        h = bg.double_of(g, low_memory=low_memory)
        branches = run_branches(h)
        bg.assert_same_skeleton(branches, g["ref"], g["base"])
        own = restated(bg.double_of(g))
        bg.assert_same_regions(branches, own)
        assert len(branches.kernel_ms) == g["base"]["T"] and all(set(p) == PARTS for p in branches.kernel_ms)
        assert sum(len(a) for a in branches.branch_label) == sum(len(a) for a in g["ref"]["branch_label"]) > 0
        for t in range(g["base"]["T"]):                           # the figures made every region a branch: the table can be written
            assert np.array_equal(branches.region_label[t], branches.branch_label[t])


def test_scale_frame(hip):
    """one frame of the S3 scene (20 x 120 x 130, X no multiple of 64, 4876 mask words: two workgroups of the skeleton scan) with
    branch labels sparse up to 2 000 000 (31 250 presence words: eight workgroups of the label scan), a skeleton of several thousand
    voxels of which the largest label has more than 2 048 (more than one workgroup could sort in LDS), and reassigned labels"""
    g = vs.stack("S3")
    g = dict(g, T=1, **{k: g[k][:1] for k in ("comp", "branch", "raw", "struct", "pixel_class", "distance")})
    rng = np.random.default_rng(8)
    labels, sizes = np.unique(g["branch"][0][g["branch"][0] > 0], return_counts=True)
    skel = row_skeleton(g["branch"][0], rng, dense=[labels[np.argmax(sizes)]])[None]
    reassigned = (g["branch"] % 7 + rng.integers(0, 2, g["branch"].shape)).astype(np.int32)
    v, n = plain_levels(g, 2)
    h = bg.hierarchy_double(g, skel, shell(g["comp"]), voxels=v, nodes=n, reassigned=reassigned)
    got = run_branches(h)
    own = restated(h)
    assert_same(got, own, g)
    count = np.bincount(np.searchsorted(labels, skel[0][skel[0] > 0]))
    assert len(got.branch_idxs[0]) > 3000 and count.max() > 2048 and count.min() >= 1 and len(labels) > 100
    assert 1_500_000 < labels.max() <= 2_000_000 and (labels.max() + 64) // 64 > 4 * vs.RA_SCAN_CHUNK
    assert np.isfinite(got.branch_thickness[0]).all() and len(set(got.reassigned_label[0].tolist())) > 3
    assert (np.asarray(own.branch_tortuosity[0]) != 1).any() and len(got.branch_label[0]) == len(labels) == len(got.region_label[0])


FACE_SHAPES = [(3, 11, 70), (4, 7, 129), (65, 129), (33, 70)]


@pytest.mark.parametrize("shape", FACE_SHAPES)
def test_ragged_widths_faces_and_corners(hip, shape):
    """x extents of 70 and 129 (no multiple of the wave or of a 64-bit mask word); skeleton and region voxels on every corner and in
    the middle of every face, edge and of the frame; scattered labels, so regions sprawl over the frame and labels come in many
    pieces; the border on one face, then on the opposite one"""
    rng = np.random.default_rng(sum(shape))
    D = len(shape)
    T = 2
    branch = (rng.integers(1, 13, (T,) + shape) * (rng.random((T,) + shape) < 0.4)).astype(np.int32)
    skel = (branch * (rng.random(branch.shape) < 0.15)).astype(np.int32)
    spots = list(np.ndindex(*(3,) * D))
    for t in range(T):
        for k, c in enumerate(spots):
            at = (t,) + tuple((0, s // 2, s - 1)[j] for j, s in zip(c, shape))
            branch[at] = skel[at] = 13 + k % 2
        for l in range(1, 13):                                     # every label keeps a skeleton voxel
            first = np.argwhere(branch[t] == l)[0]
            skel[(t,) + tuple(first)] = l
    comp = ((branch > 0) * rng.integers(1, 30, branch.shape)).astype(np.uint16)
    border = np.zeros(branch.shape, np.int16)
    border[0][..., 0] = -3                                         # the face x = 0, any value but 0
    border[1][..., -1, :] = 2                                      # the face y = last
    g = vs.as_stack("faces", comp, branch, comp, comp.astype(np.float32), (skel > 0).astype(np.uint8), np.zeros(branch.shape, np.float32),
                    np.zeros((0, 2 * D + 2)), vs.SPACING_3D if D == 3 else vs.SPACING_2D, 1.0)
    v, n = plain_levels(g, 3)
    reassigned = rng.integers(0, 3, branch.shape).astype(np.uint8)
    h = bg.hierarchy_double(g, skel, border, voxels=v, nodes=n, reassigned=reassigned)
    got = run_branches(h)
    assert_same(got, restated(h), g)
    for t in range(T):
        assert len(got.branch_label[t]) == 14 and (np.asarray(got.branch_thickness[t]) >= 0).all()
        where = {tuple(p) for p in got.branch_idxs[t].tolist()}
        assert all(tuple((0, s // 2, s - 1)[j] for j, s in zip(c, shape)) in where for c in spots)


@pytest.mark.parametrize("name", ["branches_3d_sparse_flow", "branches_2d"])
def test_reassigned_labels(hip, name):
    """with the reassigned stack (few values, so ties and zeros decide), without it, and under no_t, where the reference ignores it"""
    g = bg.load(name)
    rng = np.random.default_rng(6)
    reassigned = rng.integers(0, 3, g["skel"].shape).astype(np.uint16 if g["base"]["D"] == 2 else np.int32)
    with_re = run_branches(bg.double_of(g, reassigned=reassigned))
    own = restated(bg.double_of(g, reassigned=reassigned))
    bg.assert_same_skeleton(with_re, g["ref"], g["base"])
    bg.assert_same_regions(with_re, own)
    values = np.concatenate([np.asarray(a, np.float64) for a in with_re.reassigned_label])
    assert np.isfinite(values).all() and {0.0, 1.0} <= set(values.tolist()) <= {0.0, 1.0, 2.0}
    for kw in (dict(), dict(reassigned=reassigned, no_t=True)):
        got = run_branches(bg.double_of(g, **kw))
        bg.assert_same_regions(got, restated(bg.double_of(g, **kw)))
        assert all(np.isnan(a).all() for a in got.reassigned_label)
        for k in bg.REGION[:4] + ("z", "y", "x"):
            assert all(bg.same(a, b) for a, b in zip(getattr(got, k), getattr(with_re, k))), k


def test_uneven_frames_on_one_handle(hip):
    """T = 3 on one handle: the large frame first, an all-background frame, then a small one -- nothing of a frame survives into
    the next"""
    u = vs.uneven()
    pick = [4, 1, 0]
    parts = {k: u[k][pick] for k in ("comp", "branch", "raw", "struct", "pixel_class", "distance")}
    g = vs.as_stack("uneven_branches", flow=np.zeros((0, 8)), spacing=u["spacing"], dt=1.0, **parts)
    rng = np.random.default_rng(12)
    skel = np.stack([row_skeleton(g["branch"][t], rng) for t in range(3)])
    border = shell(g["comp"])
    v, n = plain_levels(g, 5)
    h = bg.hierarchy_double(g, skel, border, voxels=v, nodes=n)
    got = run_branches(h)
    assert_same(got, restated(h), g)
    B = [len(a) for a in got.branch_label]
    assert B[1] == 0 and B[0] > 3 * B[2] > 0 and got.aggregate_voxel_metrics[1] == {} and got.aggregate_node_metrics[1] == {}
    assert got.branch_idxs[1].shape == (0, 3) and got.branch_length[1] == [] and got.kernel_ms[1]["regions"] == 0.0


def test_branch_features_writes_the_reference_table(hip, tmp_path):
    """BranchFeatures(im_info).run() on a stack written with the project's ImInfo: features_branches against the text the restatement
    gives when fed this package's own Voxels and Nodes output, character for character; the reassigned stacks are opened only when
    both files exist"""
    from nellie_amd.feature_extraction import BranchFeatures
    from nellie_amd.im_info.verifier import ImInfo
    gb = bg.load("branches_3d_integer_flow")
    g = gb["base"]
    dim_res = dict(zip("ZYX", (float(s) for s in g["spacing"])), T=g["dt"])
    im_info = ImInfo(g["raw"], dim_res=dim_res, output_dir=str(tmp_path), name="branches")
    paths = im_info.pipeline_paths
    rng = np.random.default_rng(1)
    reassigned = rng.integers(0, 4, g["branch"].shape).astype(np.int32)
    for key, data in (("im_preprocessed", g["struct"]), ("im_distance", g["distance"]), ("im_skel", gb["skel"]), ("im_instance_label", g["comp"]),
                      ("im_skel_relabelled", g["branch"]), ("im_border", gb["border"]), ("im_pixel_class", g["pixel_class"]),
                      ("im_branch_label_reassigned", reassigned)):
        im_info.allocate_memory(paths[key], dtype=str(data.dtype), data=data, description=key)
    np.save(paths["flow_vector_array"], g["flow"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BranchFeatures(im_info, device="cpu")
    bf = BranchFeatures(im_info)
    assert bf.run() is bf.branches and bf.branches.hierarchy is bf
    assert bf.im_branch_reassigned is None and all(np.isnan(a).all() for a in bf.branches.reassigned_label)      # one file of the two
    named = dict(g, filename=bf.voxels.image_name[0][0])

    def check(bf, re):
        h = bg.hierarchy_double(named, gb["skel"], gb["border"], voxels=bf.voxels, nodes=bf.nodes, reassigned=re)
        own = restated(h)
        assert_same(bf.branches, own, named)
        for k in bg.PER_BRANCH:                                    # what does not depend on the interpolated vectors
            assert all(bg.same(a, b) for a, b in zip(getattr(bf.branches, k), gb["ref"][k])), k
        header, want = br.feature_table(own)
        got = open(paths["features_branches"]).read()
        assert got == want and got.splitlines()[0] == ",".join(header) and len(header) == 90
        assert len(got.splitlines()) == 1 + sum(len(a) for a in gb["ref"]["branch_label"])
    check(bf, None)
    assert open(paths["features_nodes"]).read().startswith("t,label,linear_vel_mean") and os.path.exists(paths["features_voxels"])
    im_info.allocate_memory(paths["im_obj_label_reassigned"], dtype="int32", data=reassigned, description="obj")
    both = BranchFeatures(im_info)
    both.run()
    assert both.im_branch_reassigned is not None and np.isfinite(np.concatenate(both.branches.reassigned_label)).all()
    check(both, reassigned)
    os.remove(paths["features_branches"])
    skipped = BranchFeatures(im_info, skip_nodes=True)
    skipped.run()
    assert skipped.branches.aggregate_node_metrics == [] and open(paths["features_branches"]).read().startswith("t,label,linear_vel_mean")


def test_two_runs_give_identical_bits(hip):
    g = bg.load("branches_3d_sparse_flow")
    rng = np.random.default_rng(2)
    reassigned = rng.integers(0, 3, g["skel"].shape).astype(np.int32)
    a, b = (run_branches(bg.double_of(g, reassigned=reassigned)) for _ in range(2))
    for k in bg.PER_BRANCH + bg.REGION + ("branch_idxs", "region_label"):
        for x, y in zip(getattr(a, k), getattr(b, k)):
            x, y = np.asarray(x), np.asarray(y)
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), k
    for frames in ("aggregate_voxel_metrics", "aggregate_node_metrics"):
        for fa, fb in zip(getattr(a, frames), getattr(b, frames)):
            assert list(fa) == list(fb)
            for s in fa:
                for key in bg.KEYS:
                    assert fa[s][key].tobytes() == fb[s][key].tobytes(), (s, key)
    assert sum(len(x) for x in a.branch_label) > 30


def test_errors(hip):
    from nellie_amd import hipnative
    from nellie_amd.feature_extraction import Branches
    g = bg.load("branches_3d_aniso")
    h = bg.double_of(g)
    h.voxels.intensity = [a[:-1] for a in h.voxels.intensity]        # a statistic shorter than the labels: the last voxel's label points past its end
    short = Branches(h)
    with pytest.raises(ValueError, match="intensity"):
        short.run()
    assert short._engine is None and short._aggregator is None
    with hipnative.NodeFeatures() as engine:                        # the device's own check of an index past the end
        engine.groups(np.array([0, 2]), np.array([0, 5]))
        with pytest.raises(ValueError):
            engine.aggregate(np.arange(5.0))
    h = bg.double_of(g)
    h.nodes.branch_label = [a[:-1] for a in h.nodes.branch_label]  # fewer labels than node statistics
    with pytest.raises(ValueError, match="divergence"):
        Branches(h).run()
    with hipnative.BranchFeatures((4, 5, 6), (0.3, 0.1, 0.1)) as engine:
        with pytest.raises(TypeError):
            engine.frame(np.zeros((4, 5, 6), np.float32), np.zeros((4, 5, 6), np.uint8), np.zeros((4, 5, 6), np.uint8))
        with pytest.raises(ValueError):
            engine.frame(np.zeros((4, 5, 7), np.int32), np.zeros((4, 5, 6), np.uint8), np.zeros((4, 5, 6), np.uint8))
        with pytest.raises(ValueError):                           # a reassigned label below 0: np.bincount refuses it too
            engine.regions(np.ones((4, 5, 6), np.int32), np.full((4, 5, 6), -1, np.int32))
        assert engine.frame(np.zeros((4, 5, 6), np.int32), np.zeros((4, 5, 6), np.uint8), np.zeros((4, 5, 6), np.uint8)) == (0, 0, 0, 0)
        assert engine.regions(np.zeros((4, 5, 6), np.int64)) == 0 and engine.fetch_regions()[1].shape == (16, 0)
