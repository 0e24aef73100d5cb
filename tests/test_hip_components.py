"""GPU tests of the organelle level of the hierarchy (nellie_amd.feature_extraction.components, bf_region_rows_kernel of
csrc/branchfeat.inc): every golden of the reference's Components through the public `Components`, the region sums by row runs
against the sums per voxel and against direct summation on frames made for every path of the kernel (tests/component_scenes.py),
the reassigned label, uneven frames on one handle, the organelle table through `ComponentFeatures` on files, determinism and the
refusals.

Everything is compared for equality: integers, and every float bit for bit, the NaN pattern included (a NaN equals a NaN of another
sign or payload).  Goldens hold what the reference computes without regionprops; the region columns, the reassigned label and
everything without a golden are compared against tests/component_features_restatement.py, which equals the goldens bit for bit
(tests/test_components_cpu.py).  No region and no component is left out of a comparison."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import branch_goldens as bg
import component_features_restatement as cr
import component_goldens as cg
import component_scenes as cs

pytestmark = pytest.mark.gpu
NAMES = cg.names()
VOXEL_STATS = ["linear_vel", "angular_vel", "linear_acc", "angular_acc", "rel_linear_vel", "rel_angular_vel", "rel_linear_acc", "rel_angular_acc",
               "rel_directionality", "structure", "intensity"]
DTYPES = (np.int32, np.uint16, np.int64)


@pytest.fixture(scope="module")
def hip():
    from nellie_amd import build, hipnative
    build.build(verbose=False)
    lib = hipnative.load()
    assert lib.device_count() > 0, "no HIP device"
    return lib


def run_components(h):
    from nellie_amd.feature_extraction import Components
    components = Components(h)
    components.run()
    assert components._engine is None and components._aggregator is None
    return components


def restated(h):
    own = cr.Components(h)
    own.run()
    return own


def assert_same(got, own, base, frames=None):
    cg.assert_same_components(got, own, base, frames)
    cg.assert_same_regions(got, own, frames)


def plain_hierarchy(comp, spacing, seed, reassigned=None, skip_nodes=False):
    """a hierarchy of plain objects for the component stack `comp`: the labelled voxels in raster order, a twentieth of them as
    nodes and a thirtieth as branches with the component label of their voxel, and random statistics (float32 for the voxels and
    the four skeleton statistics, float64 otherwise) with a fifth of the rows NaN; (hierarchy, base)"""
    rng = np.random.default_rng(seed)
    v = SimpleNamespace(stats_to_aggregate=list(VOXEL_STATS), component_labels=[], **{s: [] for s in VOXEL_STATS})
    n = SimpleNamespace(stats_to_aggregate=list(bg.NODE_STATS), component_label=[], **{s: [] for s in bg.NODE_STATS})
    b = SimpleNamespace(stats_to_aggregate=list(bg.STATS_TO_AGGREGATE), component_label=[], **{s: [] for s in bg.STATS_TO_AGGREGATE})
    for t in range(len(comp)):
        mine = comp[t][comp[t] > 0]
        for level, share, dtype, key in ((v, 1.0, np.float32, "component_labels"), (n, 0.05, np.float64, "component_label"), (b, 0.03, None, "component_label")):
            labels = mine[rng.random(len(mine)) < share]
            getattr(level, key).append(labels)
            for j, s in enumerate(level.stats_to_aggregate):
                x = rng.standard_normal(len(labels)) * 10.0 ** rng.integers(-2, 3, len(labels))
                x[rng.random(len(labels)) < 0.2] = np.nan
                getattr(level, s).append(x.astype(dtype or (np.float32 if j < 4 else np.float64)))
    im_info = SimpleNamespace(no_t=False, no_z=comp.ndim == 3, file_info=SimpleNamespace(filename_no_ext="plain"))
    h = SimpleNamespace(im_info=im_info, num_t=len(comp), spacing=tuple(float(s) for s in spacing), viewer=None, label_components=comp,
                        skip_nodes=skip_nodes, low_memory=False, im_obj_reassigned=reassigned, voxels=v, nodes=n, branches=b)
    return h, dict(T=len(comp), D=comp.ndim - 1, skip_nodes=skip_nodes, filename="plain")


@pytest.mark.parametrize("name", NAMES)
def test_golden(hip, name):
    g = cg.load(name)
    own = restated(cg.double_of(g))
    for low_memory in (False, True):                              # accepted and ignored: the values of the default path
        got = run_components(cg.double_of(g, low_memory=low_memory))
        cg.assert_same_components(got, g["ref"], g["base"])
        cg.assert_same_regions(got, own)
        assert len(got.kernel_ms) == g["base"]["T"] and all(set(p) == {"regions", "aggregation"} for p in got.kernel_ms)
        assert sum(len(a) for a in got.component_label) == sum(len(a) for a in g["ref"]["component_label"]) > 0


_MODES = {}


def reassigned_of(name):
    """reassigned labels 0 .. 2 for a scene's frame and their mode per region by counting; made once"""
    if name not in _MODES:
        lab = cs.frame(name)
        re = np.random.default_rng(len(name)).integers(0, 3, lab.shape).astype(np.int32)
        _MODES[name] = (re, cr.mode_of(lab, re))
    return _MODES[name]


@pytest.mark.parametrize("name", sorted(cs.FRAMES))
def test_rows_equal_the_sums_per_voxel_and_direct_sums(hip, name):
    """regions(rows=True) against regions(rows=False) on the same inputs -- labels, all F x R sums and the mode identical -- and
    both against direct summation, in every label dtype that holds the frame's labels, on a handle that never saw frame()"""
    from nellie_amd import hipnative
    lab = cs.frame(name)
    labels, sums = cs.direct(name)
    re, mode = reassigned_of(name)
    D = lab.ndim
    spacing = (0.3, 0.1, 0.1)[3 - D:]
    dtypes = [dt for dt in DTYPES if labels.max() <= np.iinfo(dt).max]
    assert len(dtypes) == (2 if name == "sparse" else 3)
    with hipnative.BranchFeatures(lab.shape, spacing) as eng:
        for dt in dtypes:
            frame = lab.astype(dt)
            for stack, want_mode in ((None, np.full(len(labels), -1, np.int64)), (re, mode)):
                got = {}
                for rows in (True, False):
                    assert eng.regions(frame, stack, rows=rows) == len(labels)
                    got[rows] = eng.fetch_regions()
                    assert eng.kernel_ms_parts()["regions"] > 0
                for a, b in zip(got[True], got[False]):
                    assert a.dtype == b.dtype == np.int64 and a.shape == b.shape and a.tobytes() == b.tobytes()
                assert np.array_equal(got[True][0], labels) and np.array_equal(got[True][1], sums) and np.array_equal(got[True][2], want_mode)
    if name in ("box", "longest_run"):
        assert np.array_equal(sums, cs.box_sums(lab.shape))
    if name == "scatter":
        assert len(np.unique(lab[0, :16][lab[0, :16] > 0])) == cs.SCATTERED + 1


@pytest.mark.parametrize("name", ["components_3d_sparse_flow", "components_2d"])
def test_reassigned_labels(hip, name):
    """with the reassigned stack (few values, so ties and zeros decide), without it, and under no_t, where the reference ignores it"""
    g = cg.load(name)
    assert not g["no_t"]
    rng = np.random.default_rng(6)
    reassigned = rng.integers(0, 3, g["base"]["comp"].shape).astype(np.uint16 if g["base"]["D"] == 2 else np.int32)
    with_re = run_components(cg.double_of(g, reassigned=reassigned))
    cg.assert_same_components(with_re, g["ref"], g["base"])
    cg.assert_same_regions(with_re, restated(cg.double_of(g, reassigned=reassigned)))
    values = np.concatenate([np.asarray(a, np.float64) for a in with_re.reassigned_label])
    assert np.isfinite(values).all() and {0.0, 1.0} <= set(values.tolist()) <= {0.0, 1.0, 2.0}
    for kw in (dict(), dict(reassigned=reassigned, no_t=True)):
        got = run_components(cg.double_of(g, **kw))
        cg.assert_same_regions(got, restated(cg.double_of(g, **kw)))
        assert all(np.isnan(a).all() for a in got.reassigned_label)
        for k in cg.REGION[:4] + ("z", "y", "x"):
            assert all(cg.same(a, b) for a, b in zip(getattr(got, k), getattr(with_re, k))), k


def test_uneven_frames_on_one_handle(hip):
    """T = 3 on one handle with plain objects as children: a large frame first (sprawling regions, 40 labels), an all-background
    frame, then a small one (two components, one without node or branch) -- nothing of a frame survives into the next"""
    shape = (6, 40, 70)
    comp = np.zeros((3,) + shape, np.uint16)
    comp[0] = cs.runs_frame(shape, 3, labels=40)
    comp[2, 1, 3:6, 60:70] = 7
    comp[2, 5, 39, 0] = 900
    reassigned = np.random.default_rng(1).integers(0, 3, comp.shape).astype(np.uint8)
    h, base = plain_hierarchy(comp, (0.3, 0.1, 0.1), 11, reassigned=reassigned)
    got = run_components(h)
    assert_same(got, restated(h), base)
    R = [len(a) for a in got.component_label]
    assert R == [40, 0, 2] and got.aggregate_voxel_metrics[1] == {} and got.aggregate_branch_metrics[1] == {} and got.organelle_area[1] == []
    assert got.component_label[0].dtype == np.uint16 and got.component_label[1].dtype == np.array([], dtype=int).dtype
    assert np.isnan(got.aggregate_branch_metrics[2]["branch_length"]["mean"][0, 1]) and got.aggregate_branch_metrics[2]["branch_length"]["sum"][0, 1] == 0
    skipped, base = plain_hierarchy(comp, (0.3, 0.1, 0.1), 11, skip_nodes=True)
    got = run_components(skipped)
    assert_same(got, restated(skipped), base)
    assert got.aggregate_node_metrics == [] and all(np.isnan(a).all() for a in got.reassigned_label if len(a))


def test_component_features_writes_the_reference_table(hip, tmp_path):
    """ComponentFeatures(im_info).run() on a stack written with the project's ImInfo: features_organelles against the text the
    restatement gives when fed this package's own Voxels, Nodes and Branches output, character for character; with and without
    the reassigned files, and with skip_nodes"""
    from nellie_amd.feature_extraction import ComponentFeatures
    from nellie_amd.im_info.verifier import ImInfo
    gc = cg.load("components_3d_integer_flow")
    gb, g = gc["branches"], gc["base"]
    dim_res = dict(zip("ZYX", (float(s) for s in g["spacing"])), T=g["dt"])
    im_info = ImInfo(g["raw"], dim_res=dim_res, output_dir=str(tmp_path), name="components")
    paths = im_info.pipeline_paths
    rng = np.random.default_rng(1)
    reassigned = rng.integers(0, 4, g["comp"].shape).astype(np.int32)
    for key, data in (("im_preprocessed", g["struct"]), ("im_distance", g["distance"]), ("im_skel", gb["skel"]), ("im_instance_label", g["comp"]),
                      ("im_skel_relabelled", g["branch"]), ("im_border", gb["border"]), ("im_pixel_class", g["pixel_class"])):
        im_info.allocate_memory(paths[key], dtype=str(data.dtype), data=data, description=key)
    np.save(paths["flow_vector_array"], g["flow"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ComponentFeatures(im_info, device="cpu")

    def check(cf, re):
        named = dict(g, filename=cf.voxels.image_name[0][0], skip_nodes=cf.skip_nodes)
        h = cg.hierarchy_double(dict(gb, base=named), voxels=cf.voxels, nodes=cf.nodes, branches=cf.branches, reassigned=re)
        own = restated(h)
        assert_same(cf.components, own, named)
        for k in cg.PER_COMPONENT:                                 # what does not depend on the interpolated vectors
            assert all(cg.same(a, b) for a, b in zip(getattr(cf.components, k), gc["ref"][k])), k
        header, want = cr.feature_table(own)
        got = open(paths["features_organelles"]).read()
        assert got == want and got.splitlines()[0] == ",".join(header) and len(header) == 2 + (0 if cf.skip_nodes else 20) + 55 + 45 + 9
        assert len(got.splitlines()) == 1 + sum(len(a) for a in gc["ref"]["component_label"])
    cf = ComponentFeatures(im_info)
    assert cf.run() is cf.components and cf.components.hierarchy is cf and cf.im_obj_reassigned is None
    assert all(np.isnan(a).all() for a in cf.components.reassigned_label)
    check(cf, None)
    assert all(os.path.exists(paths[k]) for k in ("features_voxels", "features_nodes", "features_branches"))
    for key in ("im_obj_label_reassigned", "im_branch_label_reassigned"):
        im_info.allocate_memory(paths[key], dtype="int32", data=reassigned, description=key)
    both = ComponentFeatures(im_info)
    both.run()
    assert both.im_obj_reassigned is not None and np.isfinite(np.concatenate(both.components.reassigned_label)).all()
    check(both, reassigned)
    os.remove(paths["features_organelles"])
    skipped = ComponentFeatures(im_info, skip_nodes=True)
    skipped.run()
    assert skipped.components.aggregate_node_metrics == []
    check(skipped, reassigned)


def test_two_runs_give_identical_bits(hip):
    g = cg.load("components_3d_sparse_flow")
    rng = np.random.default_rng(2)
    reassigned = rng.integers(0, 3, g["base"]["comp"].shape).astype(np.int32)
    a, b = (run_components(cg.double_of(g, reassigned=reassigned)) for _ in range(2))
    for k in cg.PER_COMPONENT + cg.REGION:
        for x, y in zip(getattr(a, k), getattr(b, k)):
            x, y = np.asarray(x), np.asarray(y)
            assert x.dtype == y.dtype and x.tobytes() == y.tobytes(), k
    for _, frames in cg.AGGREGATES:
        for fa, fb in zip(getattr(a, frames), getattr(b, frames)):
            assert list(fa) == list(fb)
            for s in fa:
                for key in cg.KEYS:
                    assert fa[s][key].tobytes() == fb[s][key].tobytes(), (s, key)
    assert sum(len(x) for x in a.component_label) > 30
    from nellie_amd import hipnative
    lab = cs.frame("scatter")                                      # hundreds of regions in one workgroup, one sprawling around them
    with hipnative.BranchFeatures(lab.shape, (0.3, 0.1, 0.1)) as eng:
        runs = []
        for _ in range(2):
            eng.regions(lab, reassigned_of("scatter")[0], rows=True)
            runs.append(b"".join(x.tobytes() for x in eng.fetch_regions()))
    assert runs[0] == runs[1]


def test_refusals(hip):
    from nellie_amd import hipnative
    from nellie_amd.feature_extraction import Components
    g = cg.load("components_3d_aniso")
    h = cg.double_of(g, voxels=bg.ng.voxels_double(g["base"]))
    h.voxels.intensity = [a[:-1] for a in h.voxels.intensity]        # a statistic shorter than its labels
    short = Components(h)
    with pytest.raises(ValueError, match="intensity"):
        short.run()
    assert short._engine is None and short._aggregator is None
    with hipnative.BranchFeatures((2, 32769), (0.1, 0.1)) as engine:   # an extent above 2^15
        for rows in (True, False):
            with pytest.raises(ValueError, match="32768"):
                engine.regions(np.ones((2, 32769), np.int32), rows=rows)
    with hipnative.BranchFeatures((4, 5, 6), (0.3, 0.1, 0.1)) as engine:
        with pytest.raises(TypeError):
            engine.regions(np.zeros((4, 5, 6), np.float32), rows=True)
        with pytest.raises(ValueError):
            engine.regions(np.zeros((4, 5, 7), np.int32), rows=True)
        with pytest.raises(ValueError):                           # a reassigned label below 0: np.bincount refuses it too
            engine.regions(np.ones((4, 5, 6), np.int32), np.full((4, 5, 6), -1, np.int32), rows=True)
        assert engine.regions(np.zeros((4, 5, 6), np.int64), rows=True) == 0 and engine.fetch_regions()[1].shape == (16, 0)
        assert engine.regions(np.ones((4, 5, 6), np.int64), rows=True) == 1 and engine.fetch_regions()[1][0, 0] == 120
