"""GPU tests of every entry point that takes a frame "in its own dtype", with every dtype of hipnative.DTYPE_CODES: the two
conversion call sites (csrc/nellie_hip.hip), Markers' intensities (csrc/nellie_markers.hip), Label's intensity mask
(csrc/nellie_label.hip), and the voxel-, node- and branch-feature handles (csrc/voxfeat.inc, nodefeat.inc, branchfeat.inc) and the
tracker, which refuses most of them.  The frames come from tests/dtype_cases.py: random bits over the type's whole range with the
values at which a cast or a predicate goes wrong at the first and last voxel, the end of the first row and the start of the last
plane.

Every comparison is for equality of bits, with NaN equal to NaN.  The references are numpy on the same arrays and the restatements
under tests/; tests/test_dtype_cases_cpu.py checks numpy's cast itself against integer arithmetic."""
import ctypes as C

import numpy as np
import pytest

import branch_features_restatement as br
import dtype_cases as dc
import node_features_restatement as nr
import voxel_features_restatement as vr
from dtype_cases import same_bits

pytestmark = pytest.mark.gpu

ALL, INTEGERS = dc.ALL, dc.INTEGERS
SMALL = (3, 5, 7)                                       # "which arm of the switch"
# grid1d caps a launch at 8192 * 256 = 2 097 152 threads: the smallest frame at which convert_kernel's stride loop makes a second trip
TWO_TRIPS = (33, 256, 257)
assert int(np.prod(TWO_TRIPS)) > 8192 * 256
FEATURE_SHAPES = [(4, 7, 129), (33, 70)]                # rows that are no multiple of a 64-bit mask word; the second one 2-D
SPACING = {2: (0.1, 0.1), 3: (0.3, 0.1, 0.1)}


@pytest.fixture(scope="module")
def hip():
    from nellie_amd import build, hipnative
    build.build(verbose=False)
    assert hipnative.load().device_count() > 0, "no HIP device"
    return hipnative


def dtype_params(dtypes=ALL):
    return pytest.mark.parametrize("dtype", list(dtypes), ids=dc.ids(dtypes))


def shape_params(shapes):
    return pytest.mark.parametrize("shape", shapes, ids=lambda s: "x".join(map(str, s)))


def as_f32(a):
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return np.ascontiguousarray(a).astype(np.float32)


# ============================================================================================ a. conversion to float32
def _conversion_paths(hip, a, shape, slot=0):
    """the converted frame by each way in: filter_load; input_load + filter_begin; input_load_async from pinned memory +
    filter_begin.  gauss_store() returns the cascade's current source, which before any gauss_step is the converted frame (for a
    float32 input read in place, the resident input itself)."""
    out = {}
    with hip.Context(shape) as ctx:
        ctx.filter_load(a)
        out["filter_load"] = ctx.gauss_store()
        ctx.input_load(a)
        ctx.filter_begin()
        out["input_load"] = ctx.gauss_store()
        c = np.ascontiguousarray(a)
        if c.dtype in hip.DTYPE_CODES:                    # the streaming upload takes the library's dtypes only
            pin = hip.PinnedArray(shape, c.dtype)
            try:
                pin.array[...] = c
                ctx.input_load_async(slot, pin)
                ctx.input_select(slot)
                ctx.filter_begin()
                out["input_load_async"] = ctx.gauss_store()
            finally:
                ctx.sync()
                pin.free()
    return out


@shape_params([SMALL, TWO_TRIPS])
@dtype_params(ALL + dc.HOST_CAST)
def test_conversion_to_float32(hip, dtype, shape):
    """frame -> float32 equals numpy's astype(float32) (the reference's xp.asarray(frame, float32)) on every path, NaN, inf and
    values that overflow or underflow float32 included; nothing here runs the filter on them."""
    a = dc.frame(dtype, shape, 1) if dtype in ALL else dc.host_cast_frame(dtype, shape, 1)
    want = as_f32(a)
    got = _conversion_paths(hip, a, shape)
    assert len(got) == (3 if dtype in ALL else 2)
    for path, g in got.items():
        assert same_bits(g, want), (path, np.flatnonzero(g.view(np.uint32).ravel() != want.view(np.uint32).ravel())[:5])


@shape_params([SMALL, TWO_TRIPS])
@dtype_params([np.dtype(np.uint16), np.dtype(np.float64), np.dtype(np.int64)])
def test_conversion_of_strided_views(hip, dtype, shape):
    a = dc.frame(dtype, shape, 2)
    want = as_f32(a)
    for name, view in dc.strided_views(a):
        assert not view.flags.c_contiguous
        for path, g in _conversion_paths(hip, view, shape, slot=1).items():
            assert same_bits(g, want), (name, path)


@pytest.mark.parametrize("copy", [False, True], ids=["in_place", "NELLIE_COPY_INPUT"])
@shape_params([SMALL, TWO_TRIPS])
def test_float32_input_in_place_and_copied(hip, monkeypatch, shape, copy):
    """a resident float32 frame is read where it lies; NELLIE_COPY_INPUT sends it through convert_kernel<float> instead"""
    if copy:
        monkeypatch.setenv("NELLIE_COPY_INPUT", "1")
    else:
        monkeypatch.delenv("NELLIE_COPY_INPUT", raising=False)
    a = dc.frame(np.float32, shape, 3)
    with hip.Context(shape) as ctx:
        ctx.input_load(a)
        ctx.filter_begin()
        assert same_bits(ctx.gauss_store(), a)


@dtype_params([np.dtype(np.int16), np.dtype(np.uint64)])
def test_filter_load_in_two_plane_ranges(hip, dtype):
    """the staging buffer is one of the context's float volumes for elements of up to 4 bytes, an allocation for 8-byte ones"""
    shape = (5, 9, 11)
    a = dc.frame(dtype, shape, 4)
    with hip.Context(shape) as ctx:
        ctx.filter_load(a[:2], 0, 2)
        ctx.filter_load(a[2:], 2, 5)
        assert same_bits(ctx.gauss_store(), as_f32(a))
        ctx.filter_load(a[::-1][1:4], 1, 4)               # and over a loaded frame: the other planes stay
        want = as_f32(a)
        want[1:4] = as_f32(a[::-1][1:4])
        assert same_bits(ctx.gauss_store(), want)


# ============================================================================================ b. Markers' intensities
MARKERS_SHAPE, MARKERS_RES = (30, 9, 140), {"X": 0.1, "Y": 0.1, "Z": 0.1, "T": 1.0}     # the smallest of test_markers_any_radius_vs_oracle


@pytest.fixture(scope="module")
def marker_labels():
    from nellie_amd.synthetic import make_volume
    vol = make_volume(MARKERS_SHAPE, 77)
    lab = (vol > np.percentile(vol, 97)).astype(np.int32)
    lab.setflags(write=False)
    return lab


def _markers(pipe, lab, intensity, resident):
    """(n, marker, distance, border): the intensities from the host (upload_convert), or left on the device by input_load
    (nellie_markers.hip's own switch)"""
    if resident:
        pipe.ctx.input_load(intensity)
    n = pipe.markers(MARKERS_RES, labels=lab, intensity=None if resident else intensity)
    return (n,) + tuple(a.copy() for a in pipe.download_markers())


@pytest.mark.parametrize("resident", [False, True], ids=["host", "resident"])
@dtype_params()
def test_markers_intensity(hip, marker_labels, dtype, resident):
    """marker, distance and border with the intensities in their own dtype are those of the same frame given as float32"""
    from nellie_amd import pipeline as pl
    a = dc.frame(dtype, MARKERS_SHAPE, 5, finite=True)
    f = as_f32(a)
    assert np.isfinite(f).all()
    pipe = pl.FramePipeline(MARKERS_SHAPE)
    try:
        want = _markers(pipe, marker_labels, f, False)
        got = _markers(pipe, marker_labels, a, resident)
    finally:
        pipe.close()
    assert want[0] > 0 and got[0] == want[0]
    for g, w in zip(got[1:], want[1:]):
        assert same_bits(g, w)


# ============================================================================================ c. Label's intensity mask
MASK_SHAPE = (4, 5, 7)


def _mask_image(dtype):
    """three planes of dtype_cases.frame (NaN among the floats) and a plane that holds the elements the thresholds are built
    around, so that `equal to an element` and `one step either side` are what they say"""
    orig = np.empty(MASK_SHAPE, dtype)
    orig[:3] = dc.frame(dtype, SMALL, 6)
    plant = []
    for _, t in dc.thresholds(dtype):
        if isinstance(t, (int, np.integer)) and dtype.kind in "iu" and np.iinfo(dtype).min <= int(t) <= np.iinfo(dtype).max:
            plant.append(int(t))
        elif isinstance(t, (float, np.floating)) and dtype.kind == "f" and np.isfinite(t):
            plant.append(float(t))
    plant = np.array(sorted(set(plant)), dtype=object).astype(dtype)
    last = orig[3].reshape(-1)
    last[:] = plant[np.arange(last.size) % len(plant)] if len(plant) <= last.size else plant[:last.size]
    return orig


def _labels_of(ctx, frangi):
    ctx.label_run(np.float32(0.25), 1, True)
    return ctx.label_store()


@dtype_params()
def test_label_intensity_mask(hip, dtype):
    """(frangi, orig, thresh) through Label._effective_threshold + label_intensity_mask + the label run = the labels of the
    pre-masked frangi * (orig > thresh) with no mask, numpy evaluating the comparison, for every threshold form; the masked
    Frangi frame itself (filter_store) is compared too."""
    from nellie_amd.segmentation.labelling import Label
    orig = _mask_image(dtype)
    rng = np.random.default_rng(7)
    frangi = rng.uniform(0.05, 1.0, MASK_SHAPE).astype(np.float32)
    forms, masks = set(), set()
    with hip.Context(MASK_SHAPE) as ctx:
        for name, t in dc.thresholds(dtype):
            keep = dc.mask_reference(orig, t)
            pre = frangi * keep
            ctx.label_load_frangi(pre)
            want = _labels_of(ctx, pre)
            ctx.label_load_frangi(frangi)
            ctx.label_intensity_mask(orig, Label._effective_threshold(orig, t))
            assert same_bits(ctx.filter_store(), pre), (name, np.flatnonzero((ctx.filter_store() != 0).ravel() != keep.ravel()))
            got = _labels_of(ctx, frangi)
            assert np.array_equal(got, want), name
            forms.add(type(t))
            masks.add(keep.tobytes())
        assert forms == set(dc.THRESHOLD_FORMS) and len(masks) > 4
        # a plane range: the other planes keep their values (nl_label_intensity_mask_planes, and its integer twin for 64-bit images)
        for name, t in dc.thresholds(dtype)[:: max(1, len(dc.thresholds(dtype)) // 6)]:
            ctx.label_load_frangi(frangi)
            ctx.label_intensity_mask(orig[1:3], Label._effective_threshold(orig, t), z0=1, z1=3)
            want = frangi.copy()
            want[1:3] *= dc.mask_reference(orig[1:3], t)
            assert same_bits(ctx.filter_store(), want), name


@dtype_params([np.dtype(np.uint64), np.dtype(np.int64)])
def test_integer_threshold_beyond_2_53_on_the_device(hip, dtype):
    """np.array([2**53 + 1]) > 2**53 is True; compared in float64 it is False"""
    from nellie_amd.segmentation.labelling import Label
    shape = (1, 1, 4)
    orig = np.array([2 ** 53 + 1, 2 ** 53, 2 ** 53 + 2, 0], dtype).reshape(shape)
    frangi = np.ones(shape, np.float32)
    with hip.Context(shape) as ctx:
        for t in (2 ** 53, np.int64(2 ** 53), 2 ** 53 + 1, float(2 ** 53), -1, 2 ** 64):
            ctx.label_load_frangi(frangi)
            ctx.label_intensity_mask(orig, Label._effective_threshold(orig, t))
            assert np.array_equal(ctx.filter_store() != 0, dc.mask_reference(orig, t)), t
        with pytest.raises(ValueError):
            ctx.label_intensity_mask(orig.astype(np.int32), 5)      # an int threshold is for 64-bit integer images


# ============================================================================================ d. VoxelFeatures
def _label_frames(shape, seed):
    rng = np.random.default_rng(seed)
    comp = (rng.random(shape) < 0.3) * rng.integers(1, 50, shape)
    comp[rng.random(shape) < 0.05] = -3                   # negative labels are background
    comp.reshape(-1)[[0, -1]] = 7
    branch = np.where(comp > 0, rng.integers(-2, 40, shape), 0)
    return comp.astype(np.int32), branch.astype(np.int32)


@shape_params(FEATURE_SHAPES)
@dtype_params()
def test_voxel_frame_values(hip, dtype, shape):
    """fetch_voxels() returns raw[comp > 0] and structure[comp > 0] exactly, in the uploaded dtype, whichever of the two it is"""
    comp, branch = _label_frames(shape, 8)
    other = ALL[(ALL.index(dtype) + 3) % len(ALL)]
    want = np.flatnonzero(comp > 0)
    with hip.VoxelFeatures(shape, SPACING[len(shape)], 1.0) as eng:
        for raw, struct in ((dc.frame(dtype, shape, 9), dc.frame(other, shape, 10)), (dc.frame(other, shape, 11), dc.frame(dtype, shape, 12))):
            assert eng.frame(comp, branch, raw, struct) == len(want)
            vox, c, b, r, s = eng.fetch_voxels()
            assert same_bits(vox, want) and same_bits(c, comp.ravel()[want]) and same_bits(b, branch.ravel()[want])
            assert same_bits(r, raw.ravel()[want]) and same_bits(s, struct.ravel()[want])


@pytest.mark.parametrize("dist_dtype", [np.float32, np.float64, np.float16], ids=["f4", "f8", "f2"])
@shape_params(FEATURE_SHAPES)
@dtype_params()
def test_voxel_nodes_pixel_class(hip, dtype, shape, dist_dtype):
    """nodes are the voxels with pixel class > 0 as numpy says it: not the negatives, -0.0 or NaN; the smallest denormal, +inf and a
    uint64 at or above 2**63 are.  Boxes and both lists equal the restatement's on the same arrays."""
    comp, branch = _label_frames(shape, 13)
    pc = dc.sparse_frame(dtype, shape, 14)
    distance = np.random.default_rng(15).uniform(0.0, 2.5, shape).astype(dist_dtype)
    with np.errstate(invalid="ignore"):
        nodes, lims = vr.node_boxes(pc, distance)
    assert 2 <= len(nodes) < pc.size // 4
    if dtype.kind == "f":
        tiny = np.nextafter(dtype.type(0), dtype.type(1))
        held = pc[tuple(nodes.T)]
        assert (held == tiny).any() and np.isinf(held).any() and np.isnan(pc).any() and (pc < 0).any()
    if dtype == np.uint64:
        assert (pc[tuple(nodes.T)] >= 2 ** 63).sum() >= 3
    (node_off, node_val), (vox_off, vox_val) = vr.node_assignment(lims, np.argwhere(comp > 0))
    raw = np.ones(shape, np.uint8)
    with hip.VoxelFeatures(shape, SPACING[len(shape)], 1.0) as eng:
        eng.frame(comp, branch, raw, raw)
        assert eng.nodes(pc, distance) == (len(nodes), len(node_val))
        got_lims, node_csr, vox_csr = eng.fetch_nodes()
    assert all(same_bits(a, b.astype(np.int64)) for a, b in zip(got_lims, lims))
    assert same_bits(node_csr[0], node_off) and same_bits(node_csr[1], node_val)
    assert same_bits(vox_csr[0], vox_off) and same_bits(vox_csr[1], vox_val)


# ============================================================================================ e. NodeFeatures
NODE_ROLES = ("pixel_class", "comp", "branch", "border")


@pytest.mark.parametrize("role", NODE_ROLES)
@shape_params(FEATURE_SHAPES)
@dtype_params()
def test_node_frame(hip, dtype, shape, role):
    """each of the four frames in every dtype, the other three held at a fixed one: nodes follow > 0, the border != 0 (a NaN border
    voxel is set, -0.0 is not), the gathered labels come back exact in their own dtype"""
    rng = np.random.default_rng(16)
    fixed = dict(pixel_class=((rng.random(shape) < 0.04) * rng.integers(1, 5, shape)).astype(np.uint8),
                 comp=rng.integers(-5, 60, shape).astype(np.int32), branch=rng.integers(-5, 900, shape).astype(np.int16),
                 border=((rng.random(shape) < 0.03) * 2).astype(np.uint8))
    fixed[role] = dc.sparse_frame(dtype, shape, 17) if role in ("pixel_class", "border") else dc.frame(dtype, shape, 17)
    pc, comp, branch, border = (fixed[k] for k in NODE_ROLES)
    with np.errstate(invalid="ignore"):
        nodes = np.argwhere(pc > 0)
    if role == "border" and dtype.kind == "f":
        assert np.isnan(border).any() and (np.signbit(border) & (border == 0)).any()
    at = tuple(nodes.T)
    sp = SPACING[len(shape)]
    with hip.NodeFeatures(shape, sp) as eng:
        assert eng.frame(pc, comp, branch, border) == len(nodes) > 1
        coords, c, b, thick = eng.fetch()
    assert same_bits(coords, nodes.astype(np.int64))
    assert same_bits(c, comp[at]) and same_bits(b, branch[at])
    assert same_bits(thick, nr.thickness(border, nodes, sp)) and np.isfinite(thick).all()


GROUP_LENGTHS = (1, 7, 8, 129, 300)
HOST_CAST_VALUES = [np.dtype(t) for t in (np.int64, np.uint64, np.float16, bool)]


def _groups(n_values, seed):
    rng = np.random.default_rng(seed)
    lengths = list(GROUP_LENGTHS) + [0, 2]
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    idx = rng.integers(0, n_values, offsets[-1]).astype(np.int64)
    idx[:5] = np.arange(5)                                # the first groups start on the extremes
    return offsets, idx


@dtype_params(ALL + [np.dtype(np.float16), np.dtype(bool)])
def test_node_aggregate_values(hip, dtype):
    """all five keys of every group equal the restatement's for values of every dtype: the eight the device converts itself and
    the four the binding converts first, with each type's extremes (a uint32 at or above 2**31, the minima of int8 and int32)"""
    from nellie_amd.hipnative import NodeFeatures
    assert set(ALL) == set(NodeFeatures.VALUE_DTYPES) | {np.dtype(np.int64), np.dtype(np.uint64)}
    rng = np.random.default_rng(18)
    if dtype in ALL:
        values = np.concatenate([dc.edge_values(dtype), dc.random_values(dtype, 400, rng)])
    else:
        values = dc.host_cast_frame(dtype, (500,), 18)
    offsets, idx = _groups(len(values), 19)
    with np.errstate(invalid="ignore"):                   # a signalling NaN among the random float32 bits
        want = nr.aggregate_values(values, offsets, idx)
    with hip.NodeFeatures() as eng:
        assert eng.groups(offsets, idx) == max(GROUP_LENGTHS)
        got = eng.aggregate(values)
    assert set(got) == set(nr.KEYS)
    for key in nr.KEYS:
        assert same_bits(got[key], want[key]), key


@dtype_params([np.dtype(np.uint64), np.dtype(np.int64)])
def test_node_aggregate_refuses_64_bit_integers_at_the_c_entry(hip, dtype):
    values = np.arange(10, dtype=dtype)
    out = np.empty((5, 1), np.float64)
    with hip.NodeFeatures() as eng:
        eng.groups(np.array([0, 3]), np.array([0, 1, 2]))
        with pytest.raises(ValueError, match="32 bits"):
            eng._call("nl_nodefeat_aggregate", values.ctypes.data_as(C.c_void_p), hip.DTYPE_CODES[dtype], values.size,
                      out.ctypes.data_as(C.c_void_p))
        assert eng.aggregate(values)["sum"][0] == 3.0     # through the binding, and on the same handle


# ============================================================================================ f. BranchFeatures
def _branch_labels(dtype, shape, seed, top=2 ** 26, runs=14, reassigned=False):
    """(frame in dtype, the int64 frame the restatement sees): runs of one label along a row, the labels up to the type's maximum
    or `top`; a few negative voxels in the signed types and, in uint64, a few at or above 2**63, which are no label"""
    rng = np.random.default_rng(seed)
    info = np.iinfo(dtype)
    hi = min(info.max, top)
    labels = sorted({1, 2, 3, hi, hi - 1, max(1, hi // 2)})
    vol = np.zeros(shape, dtype)
    rows = vol.reshape(-1, shape[-1])
    for j in range(runs):
        r, length = rng.integers(0, len(rows)), rng.integers(2, 24)
        x0 = rng.integers(0, shape[-1] - length)
        rows[r, x0:x0 + length] = labels[j % len(labels)]
    rows[0, 0] = rows[-1, -1] = 1
    seen = vol.astype(np.int64) if dtype != np.uint64 else vol.astype(object).astype(np.int64)
    free = np.flatnonzero(vol.reshape(-1) == 0)
    if not reassigned:
        spots = rng.choice(free, 6, replace=False)
        if dtype.kind == "i":
            vol.reshape(-1)[spots] = [info.min, -1, -2, info.min, -1, -7]
            seen.reshape(-1)[spots] = [info.min, -1, -2, info.min, -1, -7]
        if dtype == np.uint64:
            vol.reshape(-1)[spots] = np.array([2 ** 63, 2 ** 64 - 1, 2 ** 63 + 5, 2 ** 63, 2 ** 64 - 1, 2 ** 63 + 1], np.uint64)
    return vol, seen


def _region_sums(lab, reassigned=None):
    """what fetch_regions returns, with the restatement's own lines (region_columns): labels, the integer sums n, min and max per
    axis, S_a, Q_ab for a <= b, and the reassigned label's mode"""
    D = lab.ndim
    where = np.argwhere(lab > 0)
    of = lab[tuple(where.T)]
    labels = np.unique(of)
    sums = np.zeros((1 + 3 * D + D * (D + 1) // 2, len(labels)), np.int64)
    mode = np.full(len(labels), -1, np.int64)
    for r, l in enumerate(labels):
        c = where[of == l]
        col = [len(c)] + [int(c[:, a].min()) for a in range(D)] + [int(c[:, a].max()) for a in range(D)] + [int(c[:, a].sum()) for a in range(D)]
        col += [int((c[:, a] * c[:, b]).sum()) for a in range(D) for b in range(a, D)]
        sums[:, r] = col
        if reassigned is not None:
            mode[r] = br.reassigned_mode(np.asarray(reassigned)[tuple(c.T)])
    return labels.astype(np.int64), sums, mode


def _check_branch_frame(eng, skel, seen, comp, border, sp):
    want = br.skeleton_stats(seen, border, sp)
    counts = eng.frame(skel, comp, border)
    got = eng.fetch()
    idxs, lab = want["branch_idxs"], want["labels"]
    assert counts == (len(idxs), len(want["branch_label"]), len(want["tips"]), len(want["lone"])) and len(idxs) > 10
    assert same_bits(got["coords"], idxs.astype(np.int64)) and same_bits(got["labels"], lab.astype(np.int64))
    assert same_bits(got["branch_label"], want["branch_label"].astype(np.int64))
    assert same_bits(got["degree"], want["degree"]) and same_bits(got["radius"], want["radius"])
    assert same_bits(got["tips"], want["tips"].astype(np.int64)) and same_bits(got["lone"], want["lone"].astype(np.int64))
    assert same_bits(got["edges"], want["pair_counts"].astype(np.uint32))
    uniq, first, n = np.unique(lab, return_index=True, return_counts=True)
    assert same_bits(got["count"], n.astype(np.int32))
    assert same_bits(got["comp"], comp[tuple(idxs[first].T)])
    with np.errstate(all="ignore"):
        median = np.array([np.median((want["radius"] * 2.0)[lab == l]) for l in uniq]).astype(np.float32)
    assert same_bits(got["median"].astype(np.float32), median)


def _branch_fixed(shape, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 200, shape).astype(np.uint8), ((rng.random(shape) < 0.03) * 3).astype(np.uint8)


@pytest.mark.parametrize("role", ["skel", "comp", "border"])
@shape_params(FEATURE_SHAPES)
@dtype_params()
def test_branch_frame(hip, dtype, shape, role):
    """skeleton labels in every integer dtype, component labels and border mask in every dtype; labels up to the type's maximum or
    2**26 (an 8 MB presence table), negative labels background, a uint64 label at or above 2**63 no label"""
    sp = SPACING[len(shape)]
    comp, border = _branch_fixed(shape, 20)
    if role == "skel":
        if dtype.kind == "f":
            with hip.BranchFeatures(shape, sp) as eng:
                with pytest.raises(TypeError):
                    eng.frame(np.zeros(shape, dtype), comp, border)
                skel, seen = _branch_labels(np.dtype(np.int32), shape, 21)
                _check_branch_frame(eng, skel, seen, comp, border, sp)
            return
        skel, seen = _branch_labels(dtype, shape, 21)
        assert seen.max() == min(np.iinfo(dtype).max, 2 ** 26) and (dtype.kind == "u" or seen.min() < 0)
        if dtype == np.uint64:
            assert (skel >= 2 ** 63).sum() == 6 and (seen >= 0).all()
    else:
        skel, seen = _branch_labels(np.dtype(np.uint16), shape, 21)
        if role == "comp":
            comp = dc.frame(dtype, shape, 22)
        else:
            border = dc.sparse_frame(dtype, shape, 22)
    with hip.BranchFeatures(shape, sp) as eng:
        _check_branch_frame(eng, skel, seen, comp, border, sp)


@pytest.mark.parametrize("role", ["labels", "reassigned"])
@shape_params(FEATURE_SHAPES)
@dtype_params()
def test_branch_regions(hip, dtype, shape, role):
    sp = SPACING[len(shape)]
    with hip.BranchFeatures(shape, sp) as eng:
        if dtype.kind == "f":
            good = np.ones(shape, np.int32)
            with pytest.raises(TypeError):
                eng.regions(np.zeros(shape, dtype)) if role == "labels" else eng.regions(good, np.zeros(shape, dtype))
            dtype = np.dtype(np.int32)                        # and the handle goes on
        lab_dtype, re_dtype = (dtype, np.dtype(np.int16)) if role == "labels" else (np.dtype(np.uint16), dtype)
        lab, seen = _branch_labels(lab_dtype, shape, 23, runs=40)
        re, re_seen = _branch_labels(re_dtype, shape, 24, top=2 ** 31 - 1, runs=60, reassigned=True)
        for reassigned, ref in ((None, None), (re, re_seen)):
            labels, sums, mode = _region_sums(seen, ref)
            assert eng.regions(lab, reassigned) == len(labels) > 3
            got = eng.fetch_regions()
            assert same_bits(got[0], labels) and same_bits(got[1], sums) and same_bits(got[2], mode)
        assert role == "labels" or re_seen.max() == min(np.iinfo(re_dtype).max, 2 ** 31 - 1)


BF_MAX_LABEL = 2 ** 31 - 2
TOO_LARGE = [(np.uint32, 2 ** 32 - 1), (np.int64, 2 ** 40), (np.uint64, 2 ** 40), (np.uint32, BF_MAX_LABEL + 1)]
BAD_REASSIGNED = [(d, v) for d in INTEGERS for v in (2 ** 31, -1) if np.iinfo(d).min <= v <= np.iinfo(d).max]


def test_branch_refusals_leave_the_handle_usable(hip):
    """a label above BF_MAX_LABEL, a reassigned label above 2**31 - 1 or below 0: refused, and the same handle then runs a good frame"""
    shape = FEATURE_SHAPES[0]
    sp = SPACING[3]
    comp, border = _branch_fixed(shape, 25)
    skel, seen = _branch_labels(np.dtype(np.int32), shape, 26)
    lab, lab_seen = _branch_labels(np.dtype(np.uint16), shape, 27, runs=40)
    re, re_seen = _branch_labels(np.dtype(np.int32), shape, 28, top=2 ** 31 - 1, runs=60, reassigned=True)
    labels, sums, mode = _region_sums(lab_seen, re_seen)
    assert {np.dtype(d) for d, _ in BAD_REASSIGNED} == set(INTEGERS) - {np.dtype(t) for t in (np.uint8, np.uint16)}
    with hip.BranchFeatures(shape, sp) as eng:
        def good():
            _check_branch_frame(eng, skel, seen, comp, border, sp)
            assert eng.regions(lab, re) == len(labels)
            got = eng.fetch_regions()
            assert same_bits(got[0], labels) and same_bits(got[1], sums) and same_bits(got[2], mode)
        good()
        for dtype, value in TOO_LARGE:
            bad = skel.astype(dtype)
            bad[1, 2, 3] = value
            with pytest.raises(ValueError):
                eng.frame(bad, comp, border)
            good()
            bad = lab.astype(dtype)
            bad[1, 2, 3] = value
            with pytest.raises(ValueError):
                eng.regions(bad)
            good()
        for dtype, value in BAD_REASSIGNED:
            bad = re.astype(dtype) if np.iinfo(dtype).max >= 2 ** 31 - 1 else np.zeros(shape, dtype)
            bad[lab > 0] = np.where(bad[lab > 0] == 0, 1, bad[lab > 0])
            bad.reshape(-1)[np.flatnonzero(lab.reshape(-1) > 0)[3]] = value
            with pytest.raises(ValueError):
                eng.regions(lab, bad)
            good()


# ============================================================================================ g. Tracker
TRACKED = [np.dtype(t) for t in (np.uint8, np.uint16, np.float32)]
REFUSED = [d for d in ALL if d not in TRACKED]


def _track_inputs(shape):
    rng = np.random.default_rng(29)
    marker = np.zeros(shape, np.uint8)
    marker[(slice(2, None, 3),) * len(shape)] = 1
    return rng.integers(0, 60000, shape).astype(np.uint16), rng.random(shape).astype(np.float32), np.full(shape, 1.5, np.float32), marker


@dtype_params(REFUSED + TRACKED)
def test_tracker_intensity_dtypes(hip, dtype):
    """uint8, uint16 and float32 intensities are accepted (their values are tested in test_hip_tracking.py); each of the other
    seven raises the binding's error, and the handle then gives what a fresh handle gives"""
    shape = (6, 12, 14)
    good = _track_inputs(shape)
    with hip.Tracker(shape, SPACING[3]) as fresh:
        n = fresh.frame(*good)
        want = fresh.features(0)
    assert n == int(good[3].sum()) > 0
    with hip.Tracker(shape, SPACING[3]) as t:
        if dtype in REFUSED:
            with pytest.raises(ValueError, match="uint8, uint16 or float32"):
                t.frame(dc.frame(dtype, shape, 30), *good[1:])
            assert t.n == [0, 0]
        else:
            assert t.frame(dc.frame(dtype, shape, 30, finite=True), *good[1:]) == n
        assert t.frame(*good) == n
        for g, w in zip(t.features(0), want):
            assert same_bits(g, w)


# ============================================================================================ the binding's label casts
@dtype_params(INTEGERS + [np.dtype(np.float64), np.dtype(bool)])
def test_labels_within_int32_give_the_int32_result(hip, dtype):
    """VoxelFeatures.frame and Reassigner.frame take their labels as int32: every dtype that holds the labels gives the same"""
    shape = FEATURE_SHAPES[0]
    rng = np.random.default_rng(31)
    hi = 2 if dtype == bool else min(np.iinfo(dtype).max if dtype.kind in "iu" else 2 ** 31 - 1, 2 ** 31 - 1)
    comp = ((rng.random(shape) < 0.3) * rng.integers(1, hi, shape)).astype(np.int64)
    comp.reshape(-1)[[0, -1]] = hi - 1 if dtype == bool else hi
    if dtype.kind in "if":
        comp[rng.random(shape) < 0.05] = -(2 ** 31) if dtype.itemsize >= 4 else np.iinfo(dtype).min
    obj = np.roll(comp, 5, axis=-1)
    raw = np.ones(shape, np.uint8)
    c32, o32 = comp.astype(np.int32), obj.astype(np.int32)
    with hip.VoxelFeatures(shape, SPACING[3], 1.0) as eng:
        n = eng.frame(c32, o32, raw, raw)
        want = eng.fetch_voxels()
        assert eng.frame(comp.astype(dtype), obj.astype(dtype), raw, raw) == n == int((c32 > 0).sum())
        assert all(same_bits(g, w) for g, w in zip(eng.fetch_voxels(), want))
    with hip.Reassigner(shape, SPACING[3], 0.25) as r:
        n = r.frame(c32, o32, seed=True)
        want = r.fetch(0)[:3]
        assert r.frame(comp.astype(dtype), obj.astype(dtype), seed=True) == n == int(((c32 > 0) | (o32 > 0)).sum())
        assert all(same_bits(g, w) for g, w in zip(r.fetch(0)[:3], want))


@pytest.mark.parametrize("value,dtype", [(2 ** 31 + 5, np.uint32), (2 ** 40 + 3, np.int64), (2 ** 63 + 1, np.uint64), (1.5, np.float32),
                                         (np.nan, np.float64), (-2 ** 31 - 1, np.int64)])
def test_lossy_label_casts_are_refused(hip, value, dtype):
    """2**31 + 5 as int32 is background, 2**40 + 3 is label 3: refused before anything is uploaded; the handle goes on"""
    shape = (4, 6, 8)
    good = np.zeros(shape, np.int32)
    good[1:3, 1:3, 1:3] = 3
    bad = good.astype(dtype)
    bad[2, 2, 2] = value
    raw = np.ones(shape, np.uint8)
    with hip.VoxelFeatures(shape, SPACING[3], 1.0) as eng:
        for comp, branch in ((bad, good), (good, bad)):
            with pytest.raises(ValueError, match="label"):
                eng.frame(comp, branch, raw, raw)
        assert eng.frame(good, good, raw, raw) == 8
    with hip.Reassigner(shape, SPACING[3], 0.25) as r:
        for branch, obj in ((bad, good), (good, bad)):
            with pytest.raises(ValueError, match="frame holds"):
                r.frame(branch, obj, seed=True)
        assert r.frame(good, good, seed=True) == 8 and r.n == [8, 0]


# ============================================================================================ h. completeness
def _dtypes_of(test):
    found = set()
    for mark in getattr(test, "pytestmark", []):
        if mark.name == "parametrize":
            for value in mark.args[1]:
                for v in (value if isinstance(value, tuple) else (value,)):
                    if isinstance(v, (np.dtype, type)):
                        try:
                            found.add(np.dtype(v))
                        except TypeError:
                            pass
    return found


@pytest.mark.parametrize("test", [test_conversion_to_float32, test_markers_intensity, test_label_intensity_mask, test_voxel_frame_values,
                                  test_voxel_nodes_pixel_class, test_node_frame, test_node_aggregate_values, test_branch_frame,
                                  test_branch_regions, test_tracker_intensity_dtypes], ids=lambda t: t.__name__)
def test_every_entry_point_sees_every_dtype(test):
    """an eleventh key of DTYPE_CODES extends every test above, or this fails"""
    from nellie_amd import hipnative
    assert set(hipnative.DTYPE_CODES) <= _dtypes_of(test), set(hipnative.DTYPE_CODES) - _dtypes_of(test)
