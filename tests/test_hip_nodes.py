"""GPU tests of the node level of the hierarchy (nellie_amd.feature_extraction.nodes, csrc/nodefeat.inc): every golden of the
reference's Nodes through the public `Nodes`, the synthetic calls of its aggregate_stats_for_class, the node table through
`NodeFeatures` on files, frames at the scale where every kernel spans workgroups, nodes on the frame's faces, uneven frames on one
handle, and determinism.

Everything is compared for equality: integers, and every float64 bit for bit, the NaN pattern included (a NaN equals a NaN of
another sign or payload).  Where no golden exists the reference is tests/node_features_restatement.py, which equals the goldens
bit for bit (tests/test_nodes_cpu.py).  No node is left out of a comparison."""
from types import SimpleNamespace

import numpy as np
import pytest

import node_features_restatement as nr
import node_goldens as ng
import voxel_features_restatement as vr
import voxel_goldens as vg
import voxel_scenes as vs
from test_hip_voxels import flow_files

pytestmark = pytest.mark.gpu
NAMES = ng.names()
STATS = ["linear_vel", "angular_vel", "linear_acc", "angular_acc", "rel_linear_vel", "rel_angular_vel", "rel_linear_acc", "rel_angular_acc",
         "rel_directionality", "structure", "intensity"]


@pytest.fixture(scope="module")
def hip():
    from nellie_amd import build, hipnative
    build.build(verbose=False)
    lib = hipnative.load()
    assert lib.device_count() > 0, "no HIP device"
    return lib


def run_nodes(h):
    from nellie_amd.feature_extraction import Nodes
    nodes = Nodes(h)
    nodes.run()
    assert nodes._engine is None
    return nodes


def restated(h):
    own = nr.Nodes(h)
    own.run()
    return own


def shell(comp):
    """the border of a stack: the background voxels that touch a labelled one"""
    border = np.zeros(comp.shape, np.uint8)
    for t in range(len(comp)):
        on = comp[t] > 0
        near = np.zeros_like(on)
        for ax in range(on.ndim):
            near[(slice(None),) * ax + (slice(1, None),)] |= on[(slice(None),) * ax + (slice(None, -1),)]
            near[(slice(None),) * ax + (slice(None, -1),)] |= on[(slice(None),) * ax + (slice(1, None),)]
        border[t] = near & ~on
    return border


def made_up_voxels(g, seed):
    """a plain `voxels` object for the stack g: the labelled voxels in raster order, the reference's node lists, and random
    float32 vectors and statistics with a fifth of the rows NaN"""
    rng = np.random.default_rng(seed)
    v = SimpleNamespace(stats_to_aggregate=list(STATS), coords=[], vec01=[], vec12=[], node_voxel_idxs=[], node_dim0_lims=[], node_dim1_lims=[],
                        node_dim2_lims=[], **{s: [] for s in STATS})
    for t in range(g["T"]):
        coords = np.argwhere(g["comp"][t] > 0)
        n = len(coords)
        _, lims = vr.node_boxes(g["pixel_class"][t], g["distance"][t])
        (off, val), _ = vr.node_assignment(lims, coords)
        v.coords.append(coords)
        v.node_voxel_idxs.append(vg.split_node_lists(off, val))
        for ax in range(3):
            getattr(v, f"node_dim{ax}_lims").append(lims[ax] if ax < g["D"] else None)
        for name in ("vec01", "vec12"):
            vec = rng.uniform(-2, 2, (n, g["D"])).astype(np.float32)
            vec[rng.random(n) < 0.2] = np.nan
            getattr(v, name).append(vec)
        for s in STATS[:-2]:
            x = (rng.standard_normal(n) * 10.0 ** rng.integers(-2, 3, n)).astype(np.float32)
            x[rng.random(n) < 0.2] = np.nan
            getattr(v, s).append(x)
        v.structure.append(g["struct"][t][tuple(coords.T)])
        v.intensity.append(g["raw"][t][tuple(coords.T)])
    return v


@pytest.mark.parametrize("name", NAMES)
def test_golden(hip, name):
    g = ng.load(name)
    for low_memory in (False, True):                              # accepted and ignored: the values of the default path
        nodes = run_nodes(ng.hierarchy_double(g["base"], g["border"], low_memory=low_memory))
        ng.assert_same_nodes(nodes, g["ref"], g["base"])
        if g["base"]["skip_nodes"]:
            assert nodes.kernel_ms == [] and nodes.longest == []
            continue
        assert nodes.longest == g["longest"]
        assert nodes.voxel_idxs is nodes.hierarchy.voxels.node_voxel_idxs and nodes.node_x_lims is nodes.hierarchy.voxels.node_dim2_lims
        assert len(nodes.kernel_ms) == g["base"]["T"] and all(set(p) == {"node_list", "thickness", "node_stats", "aggregation"} for p in nodes.kernel_ms)
        assert sum(len(a) for a in nodes.nodes) == sum(len(a) for a in g["ref"]["nodes"]) > 0


def test_synthetic_aggregation_calls(hip):
    from nellie_amd.feature_extraction import aggregate_stats_for_class
    for call in ng.synthetic_calls():
        for groups in (ng.groups_of(call), (call["offsets"], call["idx"])):
            got = aggregate_stats_for_class(call["child"], 0, groups)
            ng.assert_same_aggregates(got, call["want"], call["L"])
    child = SimpleNamespace(stats_to_aggregate=["a", "reassigned_label"], a=[np.arange(5.0)], reassigned_label=[np.arange(5)])
    got = aggregate_stats_for_class(child, 0, [])                  # no groups: arrays of length 0
    assert list(got) == ["a"] and all(got["a"][k].shape == (1, 0) and got["a"][k].dtype == np.float64 for k in ng.KEYS)
    got = aggregate_stats_for_class(child, 0, [np.array([]), np.array([])], low_memory=True)      # L = 0: NaN, and 0.0 for the sum
    assert all(np.isnan(got["a"][k]).all() and got["a"][k].shape == (1, 2) for k in ("mean", "std_dev", "min", "max"))
    assert got["a"]["sum"].tobytes() == np.zeros((1, 2)).tobytes()
    with pytest.raises(ValueError):
        aggregate_stats_for_class(child, 0, [np.array([5])])        # past the statistic's end
    with pytest.raises(ValueError):
        aggregate_stats_for_class(child, 0, [np.array([-1])])


def test_node_features_writes_the_reference_table(hip, tmp_path):
    """NodeFeatures(im_info).run() on a stack written with the project's ImInfo: features_nodes against the text the restatement
    gives when fed this package's own Voxels output -- both on the same device vectors, so character for character"""
    from nellie_amd.feature_extraction import NodeFeatures
    from nellie_amd.im_info.verifier import ImInfo
    gn = ng.load("nodes_3d_aniso")
    g = gn["base"]
    dim_res = dict(zip("ZYX", (float(s) for s in g["spacing"])), T=g["dt"])
    im_info = ImInfo(g["raw"], dim_res=dim_res, output_dir=str(tmp_path), name="nodes")
    paths = im_info.pipeline_paths
    for key, data in (("im_preprocessed", g["struct"]), ("im_distance", g["distance"]), ("im_skel", (g["pixel_class"] > 0).astype(np.uint8)),
                      ("im_instance_label", g["comp"]), ("im_skel_relabelled", g["branch"]), ("im_border", gn["border"]),
                      ("im_pixel_class", g["pixel_class"])):
        im_info.allocate_memory(paths[key], dtype=str(data.dtype), data=data, description=key)
    np.save(paths["flow_vector_array"], g["flow"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        NodeFeatures(im_info, device="cpu")
    nf = NodeFeatures(im_info)
    assert nf.run() is nf.nodes and nf.nodes.hierarchy is nf and nf.nodes.voxel_idxs is nf.voxels.node_voxel_idxs
    named = dict(g, filename=nf.voxels.image_name[0][0])
    h = ng.hierarchy_double(named, gn["border"], voxels=nf.voxels)
    own = restated(h)
    ng.assert_same_nodes(nf.nodes, own, named)
    for k in ("nodes", "component_label", "branch_label", "time", "node_thickness"):      # what does not depend on the interpolated vectors
        assert all(ng.same(a, b) for a, b in zip(getattr(nf.nodes, k), gn["ref"][k])), k
    header, want = nr.feature_table(own)
    got = open(paths["features_nodes"]).read()
    assert got == want and got.splitlines()[0] == ",".join(header) and len(header) == 64
    assert len(got.splitlines()) == 1 + sum(len(a) for a in gn["ref"]["nodes"])
    assert open(paths["features_voxels"]).read().startswith("t,label,linear_vel_raw")
    import os
    os.remove(paths["features_nodes"])
    skipped = NodeFeatures(im_info, skip_nodes=True)
    skipped.run()
    assert skipped.nodes.nodes == [] and not os.path.exists(paths["features_nodes"])


@pytest.mark.parametrize("name", ["S3", "S2"])
def test_scene_equals_the_restatement(hip, tmp_path, name):
    """this package's Voxels, then Nodes, against the restatement fed the same Voxels object.  About 4 600 nodes a frame (several
    workgroups of every node kernel), lists from 1 voxel (the scenes put every node on a labelled voxel, tests/voxel_scenes.py
    assert_scale; empty lists are in test_uneven_frames_on_one_handle and the goldens) to tens of thousands with two far nodes, so
    L is the frame's voxel count: more leaves than a wave takes at once; X = 130 in S3: border words straddle rows and planes."""
    from nellie_amd.feature_extraction import Voxels
    g = vs.stack(name)
    h = flow_files(tmp_path, g)
    try:
        h.voxels = Voxels(h)
        h.voxels.run()
    finally:
        h.flow_interpolator_fw.close()
        h.flow_interpolator_bw.close()
    h.num_t = 1                                                    # one frame of the three is compared: the restatement takes seconds
    h.im_border_mask, h.low_memory = shell(g["comp"][:1]), False
    nodes = run_nodes(h)
    own = restated(h)
    ng.assert_same_nodes(nodes, own, dict(g, T=1))
    k = np.diff(h.voxels.node_voxel_idxs_csr[0][0])
    assert len(nodes.nodes[0]) > 4096 and nodes.longest[0] == k.max() == len(h.voxels.coords[0]) > 12_000 and k.min() == 1
    assert np.sum(k == k.max()) >= 2 and np.isfinite(nodes.node_thickness[0]).all() and np.isfinite(nodes.divergence[0]).sum() > 1000


FACE_SHAPES = [(3, 70, 130), (65, 129)]


@pytest.mark.parametrize("shape", FACE_SHAPES)
def test_nodes_on_faces_and_corners(hip, shape):
    """nodes on every corner and face of the frame, the border on one face only, then on the opposite one: the search box is
    clipped on the node's side and grows across the whole frame"""
    rng = np.random.default_rng(len(shape))
    D = len(shape)
    comp = (rng.random((2,) + shape) < 0.3).astype(np.int32) * rng.integers(1, 50, (2,) + shape, dtype=np.int32)
    pixel_class, distance = np.zeros(comp.shape, np.uint8), np.zeros(comp.shape, np.float32)
    spots = [c for c in np.ndindex(*(3,) * D) if 0 in c or 2 in c]
    for t in range(2):
        for c in spots:
            at = tuple((0, s // 2, s - 1)[j] for j, s in zip(c, shape))
            pixel_class[(t,) + at], distance[(t,) + at] = rng.integers(1, 5), rng.uniform(0, 2.5)
            comp[(t,) + at] = 7
    border = np.zeros(comp.shape, np.int16)
    border[0][..., 0] = -3                                         # the face x = 0, any value but 0
    border[1][..., -1, :] = 2                                      # the face y = last
    g = vs.as_stack("faces", comp, comp.copy(), comp.astype(np.uint16), comp.astype(np.float32), pixel_class, distance, np.zeros((0, 2 * D + 2)),
                    vs.SPACING_3D if D == 3 else vs.SPACING_2D, 1.0)
    h = ng.hierarchy_double(g, border, voxels=made_up_voxels(g, 3))
    nodes = run_nodes(h)
    ng.assert_same_nodes(nodes, restated(h), g)
    assert len(nodes.nodes[0]) == len(spots) and np.isfinite(nodes.node_thickness[0]).all() and (nodes.node_thickness[0] == 0).any()
    far = 2 * (shape[-1] - 1) * g["spacing"][-1]
    assert nodes.node_thickness[0].max() == pytest.approx(far, rel=1e-12)


def test_uneven_frames_on_one_handle(hip):
    """T = 5 on one handle: a normal frame, one without nodes, one without a border, one with several times the nodes and
    voxels, one with nodes but no labelled voxel (every list empty) -- nothing of a frame survives into the next, and every
    buffer grows"""
    u = vs.uneven()
    pick = [0, 1, 5, 4, 3]                                         # normal, all background, the first again (border removed), the large one, nodes only
    parts = {k: u[k][pick] for k in ("comp", "branch", "raw", "struct", "pixel_class", "distance")}
    g = vs.as_stack("uneven_nodes", flow=np.zeros((0, 8)), spacing=u["spacing"], dt=1.0, **parts)
    border = shell(g["comp"])
    border[2] = 0
    h = ng.hierarchy_double(g, border, voxels=made_up_voxels(g, 5))
    nodes = run_nodes(h)
    ng.assert_same_nodes(nodes, restated(h), g)
    m = [len(a) for a in nodes.nodes]
    assert m[1] == 0 and m[0] > 0 and m[3] > 3 * m[0] and np.isnan(nodes.node_thickness[2]).all() and np.isfinite(nodes.node_thickness[3]).all()
    assert nodes.longest[1] == 0 and nodes.aggregate_voxel_metrics[1]["intensity"]["sum"].shape == (1, 0)
    assert m[4] > 0 and nodes.longest[4] == 0 and np.isnan(nodes.z[4]).all() and np.isnan(nodes.aggregate_voxel_metrics[4]["intensity"]["mean"]).all()
    assert nodes.aggregate_voxel_metrics[4]["intensity"]["sum"].tobytes() == np.zeros((1, m[4])).tobytes()


def test_two_runs_give_identical_bits(hip):
    g = ng.load("nodes_3d_sparse_flow")
    a, b = (run_nodes(ng.hierarchy_double(g["base"], g["border"])) for _ in range(2))
    for k in ng.PER_NODE:
        for x, y in zip(getattr(a, k), getattr(b, k)):
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), k
    for fa, fb in zip(a.aggregate_voxel_metrics, b.aggregate_voxel_metrics):
        for s in STATS:
            for key in ng.KEYS:
                assert fa[s][key].tobytes() == fb[s][key].tobytes(), (s, key)
    assert sum(len(x) for x in a.nodes) > 100
