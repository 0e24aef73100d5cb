"""GPU tests of what the four stage handles share (csrc/nl_stage.h, csrc/rank_scan.inc, hipnative._Handle): the lifecycle of every
class in 2-D and 3-D, and the shared mask / scan / compaction and query-coordinate kernels at the smallest frames whose scan
crosses a workgroup boundary; and the one device object per frame shape the stage classes hold (nellie_amd/stage.py).  Every
expectation comes from numpy or from a fresh object of the same library."""
from types import SimpleNamespace

import numpy as np
import pytest

from nellie_amd.hipnative import NL_ESTATE, NellieHipError

pytestmark = pytest.mark.gpu

# a scan workgroup covers 4096 mask words of 64 voxels: the second one starts at voxel 262144.  These frames have 4104 and 4220
# words (two workgroups, the second partly filled); the 3-D one's voxel count is no multiple of 256, so the mask kernel's last
# workgroup is partly filled too (513 * 512 is 1026 * 256: the 2-D frame ends on a full one).
BOUNDARY = 4096 * 64
SHAPES = [(513, 512), (3, 300, 300)]
assert 3 * 300 * 300 % 256 != 0
SPACING = {2: (0.1, 0.1), 3: (0.3, 0.1, 0.1)}
RADIUS = 0.25


@pytest.fixture(scope="module")
def hip():
    from nellie_amd import build, hipnative
    build.build(verbose=False)
    assert hipnative.load().device_count() > 0, "no HIP device"
    return hipnative


# ---- lifecycle -------------------------------------------------------------------------------------------------------------------
def _tracker(hip, shape):
    return hip.Tracker(shape, SPACING[len(shape)])


def _use_tracker(t, shape):
    marker = np.zeros(shape, np.uint8)
    marker[(slice(2, 6, 2),) * len(shape)] = 1
    one = np.ones(shape, np.float32)
    assert t.frame(np.full(shape, 7, np.uint16), one, one, marker) == int(marker.sum())


def _flow(hip, shape):
    return hip.FlowField(len(shape), SPACING[len(shape)], RADIUS)


def _use_flow(f, shape):
    D = len(shape)
    f.load(np.full((1, D), 2.25), np.ones((1, D)), np.array([0.5]))
    out, found = f.interpolate(np.array([[2.0] * D, [7.0] * D]))
    assert found == 1 and np.isnan(out[1]).all() and not np.isnan(out[0]).any()


def _reassigner(hip, shape):
    return hip.Reassigner(shape, SPACING[len(shape)], RADIUS)


def _use_reassigner(r, shape):
    lab = np.zeros(shape, np.int32)
    lab[(slice(1, 4),) * len(shape)] = 3
    assert r.frame(lab, lab, seed=True) == int((lab > 0).sum())


def _voxfeat(hip, shape):
    return hip.VoxelFeatures(shape, SPACING[len(shape)], 1.0)


def _use_voxfeat(v, shape):
    lab = np.zeros(shape, np.int32)
    lab[(slice(1, 4),) * len(shape)] = 3
    assert v.frame(lab, lab, np.ones(shape, np.uint16), np.ones(shape, np.float32)) == int((lab > 0).sum())


HANDLES = {"tracker": (_tracker, _use_tracker), "flow field": (_flow, _use_flow), "reassigner": (_reassigner, _use_reassigner),
           "voxel-feature object": (_voxfeat, _use_voxfeat)}


@pytest.mark.parametrize("shape", [(4, 8, 8), (8, 8)], ids=str)
@pytest.mark.parametrize("noun", list(HANDLES))
def test_lifecycle(hip, noun, shape):
    make, use = HANDLES[noun]
    a, b = make(hip, shape), make(hip, shape)              # two handles alive at once on one device
    use(a, shape)
    use(b, shape)
    a.close()
    use(b, shape)                                          # closing one leaves the other usable
    with pytest.raises(NellieHipError, match=f"{noun} is closed") as e:
        use(a, shape)
    assert e.value.code == NL_ESTATE
    b.close()
    b.close()


# ---- mask, scan, compaction --------------------------------------------------------------------------------------------------------
def _seeds(shape, rng):
    """linear indices that straddle the scan's workgroup boundary, the frame's first and last voxel and a random handful"""
    n = int(np.prod(shape))
    assert BOUNDARY < n < 2 * BOUNDARY
    fixed = [0, 63, 64, BOUNDARY - 65, BOUNDARY - 64, BOUNDARY - 1, BOUNDARY, BOUNDARY + 1, BOUNDARY + 64, n - 2, n - 1]
    return np.unique(np.concatenate([fixed, rng.choice(n, 3000, replace=False)]))


@pytest.fixture(scope="module", params=SHAPES, ids=str)
def frame(request):
    shape = request.param
    rng = np.random.default_rng(20240 + len(shape))
    idx = _seeds(shape, rng)
    n = int(np.prod(shape))
    branch, obj, comp = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    comp[idx] = 1 + idx % 50
    kind = np.arange(len(idx)) % 4                          # both labels | branch only | object only | a negative branch label
    branch[idx] = np.where(kind == 2, 0, np.where(kind == 3, -4, 1 + idx % 1000))
    obj[idx] = np.where(kind == 1, 0, 1 + idx % 77)
    extra = rng.choice(n, 500, replace=False)               # negative and zero labels alone do not label a voxel
    branch[extra] = np.where(branch[extra] == 0, -1, branch[extra])
    raw = rng.integers(0, 60000, n).astype(np.uint16)
    struct = rng.random(n).astype(np.float32)
    for a in (branch, obj, comp, raw, struct):
        a.setflags(write=False)
    return SimpleNamespace(shape=shape, branch=branch.reshape(shape), obj=obj.reshape(shape), comp=comp.reshape(shape),
                           raw=raw.reshape(shape), struct=struct.reshape(shape))


def test_reassigner_lists_the_labelled_voxels(hip, frame):
    want = np.flatnonzero((frame.branch > 0) | (frame.obj > 0))
    assert {BOUNDARY - 1, BOUNDARY, frame.branch.size - 1} <= set(want.tolist())
    with _reassigner(hip, frame.shape) as r:
        assert r.frame(frame.branch, frame.obj, seed=True) == len(want)
        vox, rb, ro, _ = r.fetch(0)
        np.testing.assert_array_equal(vox, want)
        # a seeded frame's reassigned labels are its own positive labels
        np.testing.assert_array_equal(rb, np.maximum(frame.branch.ravel()[want], 0))
        np.testing.assert_array_equal(ro, np.maximum(frame.obj.ravel()[want], 0))
        zero = np.zeros(frame.shape, np.int32)
        assert r.frame(zero, zero) == 0
        vox, rb, ro, _ = r.fetch(0)
        assert vox.size == rb.size == ro.size == 0
        vox, rb, ro, _ = r.fetch(1)                          # the frame before is still there
        np.testing.assert_array_equal(vox, want)


def test_voxel_features_list_the_labelled_voxels(hip, frame):
    comp = frame.comp
    want = np.flatnonzero(comp > 0)
    assert {BOUNDARY - 1, BOUNDARY, comp.size - 1} <= set(want.tolist())
    with _voxfeat(hip, frame.shape) as v:
        assert v.frame(comp, frame.branch, frame.raw, frame.struct) == len(want)
        vox, c, b, r, s = v.fetch_voxels()
        np.testing.assert_array_equal(vox, want)
        for got, src in ((c, comp), (b, frame.branch), (r, frame.raw), (s, frame.struct)):
            assert got.dtype == src.dtype
            np.testing.assert_array_equal(got, src.ravel()[want])
        zero = np.zeros(frame.shape, np.int32)
        assert v.frame(zero, zero, frame.raw, frame.struct) == 0
        assert all(a.size == 0 for a in v.fetch_voxels())


# ---- query coordinates ---------------------------------------------------------------------------------------------------------------
def test_query_coordinates_match_unravel_index(hip, frame):
    """The flow rows sit a quarter voxel off a handful of labelled voxels (both sides of the scan boundary and the last voxel
    among them) and carry zero vectors.  The field tells how many of numpy's coordinates of the labelled voxels find a row; the
    device-side coordinates of both users must find as many.  The reassigner reports candidates, not found voxels: with the same
    frame loaded twice a voxel with a (zero) vector lands on itself, at distance 0 < r, so the forward candidates are exactly
    the voxels that found a row, and without a backward field there are no others."""
    comp = frame.comp
    lab = np.flatnonzero(comp > 0)
    at = np.unique(np.concatenate([[BOUNDARY - 1, BOUNDARY, comp.size - 1], lab[:: len(lab) // 9]]))
    rows = np.column_stack(np.unravel_index(at, frame.shape)).astype(np.float64) + 0.25
    with _flow(hip, frame.shape) as field, _voxfeat(hip, frame.shape) as v, _reassigner(hip, frame.shape) as r:
        field.load(rows, np.zeros_like(rows), np.linspace(0.1, 0.9, len(rows)))
        _, want = field.interpolate(np.column_stack(np.unravel_index(lab, frame.shape)).astype(np.float64))
        assert want >= len(at)                               # every row is within r of the voxel it was placed at
        v.frame(comp, frame.branch, frame.raw, frame.struct)
        assert v.motility(field, field) == (want, want)
        for seed in (True, False):
            r.frame(comp, comp, seed=seed)
        assert r.pair(field, None) == want


# ---- one device object per frame shape -----------------------------------------------------------------------------------------------
def test_filter_holds_one_pipeline_per_shape(hip):
    """Asked for another shape, a stage closes the pipeline it has (its context with it) and builds the next; the new one computes
    what a pipeline of its own computes, bit for bit; after close() the stage starts over."""
    from fakes import ArrayImInfo
    from nellie_amd.pipeline import FramePipeline
    from nellie_amd.segmentation.filtering import Filter
    from nellie_amd.synthetic import make_volume
    vol = make_volume((8, 16, 24), 5)
    f = Filter(ArrayImInfo(vol[None], {"X": 0.1, "Y": 0.1, "Z": 0.1, "T": 1.0}))
    zeros = np.zeros((8, 16, 16), np.float32)
    try:
        first = f._get_pipeline((8, 16, 16))
        first.upload_frangi(zeros)
        second = f._get_pipeline((8, 16, 24))
        assert second is not first and f._get_pipeline((8, 16, 24)) is second
        with pytest.raises(NellieHipError, match="context is closed") as e:
            first.upload_frangi(zeros)
        assert e.value.code == NL_ESTATE
        second.filter(vol, f._params())
        got = second.download_frangi()
        fresh = FramePipeline((8, 16, 24))
        try:
            fresh.filter(vol, f._params())
            want = fresh.download_frangi()
        finally:
            fresh.close()
        assert got.dtype == np.float32 and got.shape == vol.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        f.close()
        with pytest.raises(NellieHipError, match="context is closed"):
            second.download_frangi()
        third = f._get_pipeline((8, 16, 24))
        assert third is not second
        third.upload_frangi(want)
    finally:
        f.close()
        f.close()


def test_network_kernels_hold_one_context_per_shape(hip):
    from nellie_amd.segmentation.networking import HipNetworkKernels
    rng = np.random.default_rng(16)
    skel2 = (rng.random((16, 16)) < 0.3).astype(np.int32)
    skel3 = (rng.random((4, 16, 16)) < 0.2).astype(np.int32)
    k = HipNetworkKernels()
    try:
        first = k._hip_context(skel2.shape)
        assert first.shape == (1, 16, 16) and k._get_pixel_class(skel2).shape == skel2.shape and k._hip_context((16, 16)) is first
        second = k._hip_context(skel3.shape)
        assert second is not first and k._hip_context((4, 16, 16)) is second
        with pytest.raises(NellieHipError, match="context is closed") as e:
            first.skel_pixel_class(skel2)
        assert e.value.code == NL_ESTATE
        got = k._get_pixel_class(skel3)
        assert k._hip_context(skel3.shape) is second
        with hip.Context((4, 16, 16)) as fresh:
            want, n = fresh.skel_pixel_class(skel3)
        assert n == int(skel3.sum()) == k.n_skeleton_voxels and got.dtype == np.uint8 and np.array_equal(got, want)
        k.close()
        with pytest.raises(NellieHipError, match="context is closed"):
            second.skel_pixel_class(skel3)
        third = k._hip_context(skel3.shape)
        assert third is not second and np.array_equal(third.skel_pixel_class(skel3)[0], want)
    finally:
        k.close()
        k.close()
