"""
GPU tests at BASELINE.json's headline size (1024^3 float32, 5-scale Frangi + Label).  The oracle needs ~45 min
and ~96 GB there, so parity at full size is shown through size-independent properties:

  * slab invariance: the volume processed as two Z-slabs (two contexts, ghost planes exchanged) equals the
    single-context result BIT FOR BIT, Frangi and labels -- every plane of one run is recomputed in the other
    with different tiling, chunking and boundary handling;
  * Frangi >= 0 and finite; the labelled set is contained in the Frangi support grown by one voxel
    (majority filter), labels are 1..K without gaps, K equals the returned count, and label ids increase with the
    raster index of each object's first voxel (scipy.ndimage.label's numbering, labelling.py:507).
"""
import os
import threading

import numpy as np
import pytest

from comms import ThreadComm, ThreadGroup

pytestmark = pytest.mark.gpu

SHAPE = (1024, 1024, 1024)
SEED = 2345


@pytest.fixture(scope="module")
def full_run(hip):
    free, _ = hip.device_mem_info(0)
    if free < 60e9:
        pytest.skip("needs ~50 GB of free HBM")
    from nellie_amd import pipeline as pl
    from nellie_amd.synthetic import ISO_01, make_volume
    vol = make_volume(SHAPE, SEED)
    p = pl.FilterParams(dim_res=ISO_01)
    pipe = pl.FramePipeline(SHAPE)
    pipe.filter(vol, p)
    fr = pipe.download_frangi()
    thr = pipe.frangi_threshold()
    n = pipe.label(thr, pl.min_area_pixels_of(ISO_01))
    lab = pipe.download_labels()
    trace = pipe.trace
    pipe.close()
    return dict(vol=vol, frangi=fr, labels=lab, n=n, thr=thr, trace=trace)


def test_properties_at_1024_cube(full_run):
    fr, lab, n = full_run["frangi"], full_run["labels"], full_run["n"]
    assert fr.dtype == np.float32 and lab.dtype == np.int32
    assert np.isfinite(fr.min()) and np.isfinite(fr.max()) and fr.min() >= 0.0
    idx = np.flatnonzero(lab)
    vals = lab.reshape(-1)[idx]
    assert n >= 10 and vals.max() == n
    counts = np.bincount(vals, minlength=n + 1)
    assert (counts[1:] > 0).all(), "label ids must be 1..K without gaps"
    # ids increase with the raster index of the first voxel
    first = np.full(n + 1, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(first, vals, idx)
    assert (np.diff(first[1:]) > 0).all()
    # after the majority filter a labelled voxel has a thresholded voxel in its 3x3x3 neighbourhood
    mask = fr > np.float32(full_run["thr"])
    z, y, x = np.unravel_index(idx[:: max(1, idx.size // 200000)], SHAPE)
    ok = np.zeros(z.size, bool)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                zz = np.clip(z + dz, 0, SHAPE[0] - 1); yy = np.clip(y + dy, 0, SHAPE[1] - 1); xx = np.clip(x + dx, 0, SHAPE[2] - 1)
                ok |= mask[zz, yy, xx]
    assert ok.all()
    assert all(0.01 < sc.mask_count / fr.size < 0.9 for sc in full_run["trace"].scales)


def test_labels_equal_the_oracle_at_1024_cube(full_run):
    """Label at the headline size against the oracle (labelling.py:467-509 restated; ~1 min of C union-find and numpy on the host)
    on the SAME Frangi frame: threshold, object count and every voxel of the int32 volume.  (This comparison found the wrong
    bit of the first majority kernel at x = nx - 1, which no smaller volume triggered.)"""
    from nellie_amd.synthetic import ISO_01
    from oracle import nellie_oracle as orc
    orc.build_c_helper()
    ref, thr = orc.label_frame(full_run["frangi"], ISO_01, return_thr=True)
    assert thr == full_run["thr"]
    assert int(ref.max()) == full_run["n"]
    assert np.array_equal(ref, full_run["labels"])


def given_scales_of(trace):
    """The volume-wide quantities of a device run, in the form the oracle's crop mode takes them."""
    return [dict(gamma=sc.gamma, max_abs=sc.max_abs, frob_thr=sc.frob_thr, skipped=sc.skipped) for sc in trace.scales]


def crop_valid_slices(box, shape, margin):
    return tuple(slice(0 if a == 0 else m, (b - a) - (0 if b == n else m)) for (a, b), n, m in zip(box, shape, margin))


def check_frangi_crops(vol, frangi, trace, shape, boxes, what):
    """Voxel-level parity of a Frangi image too large for the oracle, box by box: the oracle recomputes each box from the RAW
    voxels with the run's volume-wide thresholds (oracle.filter_frame_crop, pinned against the reference's own outputs in
    tests/test_oracle_golden.py::test_crop_mode_reproduces_the_reference_on_crop_interiors) and the device image must meet
    the usual bar -- |a - b| <= 1e-4 |ref| + 1e-6 max|ref|, identical support, capped tie zone of the percentile
    threshold -- on the part of the box no artificial face reaches."""
    from nellie_amd.synthetic import ISO_01
    from oracle import nellie_oracle as orc
    from test_hip_parity import assert_masked_close
    given = given_scales_of(trace)
    margin = orc.crop_margin(ISO_01)
    checked = 0
    for box in boxes:
        sl = tuple(slice(a, b) for a, b in box)
        valid = crop_valid_slices(box, shape, margin)
        raw = orc.filter_frame_crop(vol[sl], ISO_01, given, None)
        ref = orc.mask_volume(raw, given_thr=trace.percentile_thr)
        got = np.ascontiguousarray(frangi[sl][valid])
        assert_masked_close(got, np.ascontiguousarray(ref[valid]), np.ascontiguousarray(raw[valid]), trace.percentile_thr, f"{what} box {box}")
        checked += int(np.count_nonzero(ref[valid]))
    assert checked > 1000, f"{what}: the boxes hold only {checked} non-zero reference voxels"
    return checked


# boxes of 120 x 280 x 280 (valid interiors 72..96 x 232..256 x 232..256): a corner of the volume, a box on the X face, the
# centre, a box across the seam of the walk's 128-plane chunks (z = 128), the opposite corner in Z
CUBE_BOXES = [((0, 120), (0, 280), (0, 280)), ((452, 572), (372, 652), (744, 1024)), ((452, 572), (372, 652), (372, 652)),
              ((68, 188), (700, 980), (100, 380)), ((904, 1024), (744, 1024), (0, 280))]


def test_frangi_crops_equal_the_oracle_at_1024_cube(full_run):
    """filtering.py:806-853 at the headline size, voxel by voxel on five boxes (the walk's 128-plane chunks, the resolve kernel's
    capped grid and the automatic chunk choice only exist at this size)."""
    n = check_frangi_crops(full_run["vol"], full_run["frangi"], full_run["trace"], SHAPE, CUBE_BOXES, "1024^3")
    print(f"1024^3: {n} non-zero reference voxels compared in {len(CUBE_BOXES)} boxes")


def test_gaussian_scale_space_and_gamma_at_1024_cube(full_run, hip):
    """The cascade at the headline size: every scale's Gaussian volume BIT-equal to the oracle's on the interiors of the same
    boxes (filtering.py:816-835), and gamma = min(triangle, Otsu) of the oracle's own strided sample of the device volume
    (:365-380, :348-363) equal to the run's trace."""
    from nellie_amd import pipeline as pl
    from nellie_amd.synthetic import ISO_01
    from oracle import nellie_oracle as orc
    vol = full_run["vol"]
    margin = orc.crop_margin(ISO_01, with_mask_volume=False)
    pipe = pl.FramePipeline(SHAPE)
    try:
        pipe.ctx.filter_load(vol)
        sig = pl.default_sigmas(ISO_01)
        refs = [vol[tuple(slice(a, b) for a, b in box)].astype(np.float32) for box in CUBE_BOXES]
        for s, delta in enumerate(pl.cascade_deltas(sig, pl.z_ratio_of(ISO_01))):
            pipe.ctx.gauss_step(*[pl.gaussian_weights(d) for d in delta])
            gauss = pipe.ctx.gauss_store()
            assert orc.calculate_gamma(gauss) == full_run["trace"].scales[s].gamma, f"gamma of scale {s}"
            for k, box in enumerate(CUBE_BOXES):
                refs[k] = orc.gaussian_filter_f32(refs[k], delta, 3.0)
                # the cascade's reach grows scale by scale; the final margin covers every scale
                valid = crop_valid_slices(box, SHAPE, margin)
                sl = tuple(slice(a, b) for a, b in box)
                assert np.array_equal(gauss[sl][valid], refs[k][valid]), f"Gaussian of scale {s}, box {box}"
            del gauss
    finally:
        pipe.close()


def run_slabs(vol, shape, world, seed_dim_res=None):
    """The volume as `world` Z-slabs, one context and one thread per slab on this GPU (ghost planes and reductions
    through the host): [(o0, o1, frangi, labels, thr, n, trace)] per rank."""
    from nellie_amd.pipeline import FilterParams, min_area_pixels_of
    from nellie_amd.sharded import ShardedFramePipeline, slab_range
    from nellie_amd.synthetic import ISO_01
    group = ThreadGroup(world)
    out, errs = [None] * world, []

    def worker(rank):
        try:
            p = FilterParams(dim_res=ISO_01)
            o0, o1 = slab_range(shape[0], world, rank)
            pipe = ShardedFramePipeline(shape, rank, world, lambda ctx: ThreadComm(group, rank), p)
            pipe.filter(vol[o0:o1], p)
            thr = pipe.frangi_threshold()
            n = pipe.label(thr, min_area_pixels_of(ISO_01))
            out[rank] = (o0, o1, pipe.download_frangi(), pipe.download_labels(), thr, n, pipe.trace)
            pipe.close()
        except Exception as exc:  # noqa: BLE001
            errs.append(exc)
            group.barrier.abort()

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errs:
        raise errs[0]
    return out


def test_two_slabs_equal_one_volume_at_1024_cube(full_run):
    for o0, o1, fr, lab, thr, n, _ in run_slabs(full_run["vol"], SHAPE, 2):
        assert thr == full_run["thr"], (thr, full_run["thr"])
        assert n == full_run["n"], (n, full_run["n"])
        ref = full_run["frangi"][o0:o1]
        assert np.array_equal(fr, ref), f"slab [{o0},{o1}): {int((fr != ref).sum())} Frangi voxels differ, first at {np.argwhere(fr != ref)[:4].tolist()}"
        ref = full_run["labels"][o0:o1]
        assert np.array_equal(lab, ref), f"slab [{o0},{o1}): {int((lab != ref).sum())} label voxels differ, first at {np.argwhere(lab != ref)[:4].tolist()}"


@pytest.mark.parametrize("aniso", [False, True], ids=["iso_0.1um", "aniso_z0.3um"])
def test_c2_parity_at_its_own_size(hip, aniso):
    """BASELINE config 2 (256 x 512 x 512, seed 1234) against the oracle at its own size -- at the isotropic 0.1 um of the
    configs and, since round 4, at SURVEY 8(d)'s secondary anisotropic set (Z = 0.3 um: cascade radii 1, 1, 1, 1, 2 along Z against
    4, 3, 4, 4, 5 in the plane, min_area_pixels 22) --: Frangi within
    |a - b| <= 1e-4 |ref| + 1e-6 max|ref| with identical support (the threshold-tie relaxation of the golden tests is
    available but capped), labels bit-exact given the oracle's Frangi frame, thresholds equal."""
    from nellie_amd import pipeline as pl
    from nellie_amd.synthetic import ANISO_03, ISO_01 as ISO, make_volume
    from oracle import nellie_oracle as orc
    from test_hip_parity import assert_masked_close
    ISO_01 = ANISO_03 if aniso else ISO
    shape = (256, 512, 512)
    vol = make_volume(shape, 1234)
    run_ref = orc.run_frame(vol, ISO_01)
    ref, thr_ref = orc.mask_volume(run_ref, return_thr=True)
    p = pl.FilterParams(dim_res=ISO_01)
    pipe = pl.FramePipeline(shape)
    pipe.filter(vol, p)
    fr = pipe.download_frangi()
    assert abs(pipe.trace.percentile_thr - float(thr_ref)) <= 2e-4 * float(thr_ref)
    assert_masked_close(fr, ref, run_ref, thr_ref, "C2 256x512x512" + (" aniso" if aniso else ""))
    ref_lab, ref_lthr = orc.label_frame(ref, ISO_01, return_thr=True)
    pipe.upload_frangi(ref)
    lthr = pipe.frangi_threshold()
    assert lthr == ref_lthr
    n = pipe.label(lthr, pl.min_area_pixels_of(ISO_01))
    assert np.array_equal(pipe.download_labels(), ref_lab) and n == int(ref_lab.max()) and n >= 3
    # end to end at this size (device Frangi -> device labels), what bench.py's accuracy block reports as 1.0
    pipe.upload_frangi(fr)
    n_e2e = pipe.label(pipe.frangi_threshold(), pl.min_area_pixels_of(ISO_01))
    lab_e2e = pipe.download_labels()
    n_diff = int((lab_e2e != ref_lab).sum())
    print(f"C2 end to end: {n_diff} label voxels differ, {n_e2e} vs {int(ref_lab.max())} labels")
    if aniso:        # (exact equality end to end is a property of the seeded isotropic volumes; here: all but a tie zone's worth)
        assert n_diff <= 1e-5 * lab_e2e.size and abs(n_e2e - int(ref_lab.max())) <= 1
    else:
        assert n_diff == 0 and n_e2e == int(ref_lab.max())
    pipe.close()


def test_c5_streamed_equals_per_frame_at_its_frame_size(hip):
    """BASELINE config 5 at its own frame size (128 x 512 x 512, seeds 4567 + t), 7 frames: the double-buffered streamer
    (H2D of frame t+1 and D2H of frame t-1 on their own HIP streams while frame t computes) writes the arrays the
    frame-by-frame path writes -- with one lane, with three (the default at this frame size: three contexts of the GPU take the
    frames in turn, one upload thread feeds them), with two and with four, where the stack length is no multiple of the lane count."""
    from nellie_amd import pipeline as pl
    from nellie_amd.streaming import StreamedSegmenter, default_lanes
    from nellie_amd.synthetic import ISO_01, make_volume
    T, fs = 7, (128, 512, 512)
    frames = np.stack([make_volume(fs, 4567 + t) for t in range(T)])
    p = pl.FilterParams(dim_res=ISO_01)
    ma = pl.min_area_pixels_of(ISO_01)
    fr, lab = np.empty(frames.shape, np.float32), np.empty(frames.shape, np.int32)
    pipe = pl.FramePipeline(fs)
    counts = []
    for t in range(T):
        npos = pipe.filter(frames[t], p)
        counts.append((npos, pipe.label(pipe.frangi_threshold(), ma)))
        pipe.download_frangi(out=fr[t]); pipe.download_labels(out=lab[t])
    pipe.close()
    assert default_lanes(fs) == 3 and default_lanes((256, 512, 512)) == 2 and default_lanes((1024, 1024, 1024)) == 1
    for lanes in (None, 1, 2, 4):
        fr2, lab2 = np.full_like(fr, -1.0), np.full_like(lab, -1)
        seg = StreamedSegmenter(fs, frames.dtype, p, lanes=lanes)
        assert seg.n_lanes == (lanes or 3)
        stats = seg.run(frames, fr2, lab2, flush=False)
        if lanes is None:                   # a second stack through the same streamer: nothing of the first one lingers
            fr2[:] = -1.0; lab2[:] = -1
            stats = seg.run(frames, fr2, lab2, flush=False)
        seg.close()
        assert np.array_equal(fr, fr2) and np.array_equal(lab, lab2), f"lanes={lanes}"
        assert [tuple(int(v) for v in s_) for s_ in stats] == [tuple(int(v) for v in c) for c in counts]
    assert all(int(lab[t].max()) >= 1 for t in range(T)) and (fr >= 0).all()


def test_streamer_lanes_on_a_memory_mapped_stack_and_a_failing_frame(hip, tmp_path):
    """Two lanes fed from a file-backed stack (no page-locking in place: the upload thread stages through pinned buffers, the host copy
    of frame t + 1 beside the H2D of frame t), uint16 frames; and a stack whose third frame makes the engine raise (a +Inf voxel:
    numpy's histogram refuses the range, filtering.py:365-380 via gpu_functions.py) ends the run with that exception instead of a hang."""
    from nellie_amd import pipeline as pl
    from nellie_amd.streaming import StreamedSegmenter
    from nellie_amd.synthetic import ISO_01, make_volume
    T, fs = 5, (40, 96, 136)
    p = pl.FilterParams(dim_res=ISO_01)
    ma = pl.min_area_pixels_of(ISO_01)
    stack = np.lib.format.open_memmap(str(tmp_path / "stack.npy"), mode="w+", dtype=np.uint16, shape=(T,) + fs)
    for t in range(T):
        stack[t] = np.clip(make_volume(fs, 900 + t), 0, 65535).astype(np.uint16)
    stack.flush()
    stack = np.load(str(tmp_path / "stack.npy"), mmap_mode="r")
    fr, lab = np.empty(stack.shape, np.float32), np.empty(stack.shape, np.int32)
    pipe = pl.FramePipeline(fs)
    for t in range(T):
        pipe.filter(np.asarray(stack[t]), p)
        pipe.label(pipe.frangi_threshold(), ma)
        pipe.download_frangi(out=fr[t]); pipe.download_labels(out=lab[t])
    pipe.close()
    fr2, lab2 = np.zeros_like(fr), np.zeros_like(lab)
    seg = StreamedSegmenter(fs, stack.dtype, p, lanes=2)
    seg.run(stack, fr2, lab2, flush=False, outputs_zeroed=True)
    assert np.array_equal(fr, fr2) and np.array_equal(lab, lab2) and int(lab.max()) >= 1
    bad = np.stack([make_volume(fs, 900 + t) for t in range(T)])
    bad[2, 5, 5, 5] = np.inf
    seg2 = StreamedSegmenter(fs, bad.dtype, p, lanes=2)
    with pytest.raises(ValueError):
        seg2.run(bad, np.empty(bad.shape, np.float32), np.empty(bad.shape, np.int32), flush=False)
    fr3, lab3 = np.empty(bad.shape, np.float32), np.empty(bad.shape, np.int32)          # ... and the streamer is usable afterwards
    good = np.stack([make_volume(fs, 900 + t) for t in range(T)])
    seg2.run(good, fr3, lab3, flush=False)
    seg.close(); seg2.close()
    assert (lab3.reshape(T, -1).max(axis=1) >= 1).all()


def test_c4_volume_partition_invariance(hip):
    """BASELINE.json's 8-GPU configuration -- ONE (1024, 2048, 2048) volume, 4.29e9 voxels -- on a single MI355X: the
    eight 128-plane slabs of the 8-GPU decomposition (eight contexts on this device, 288 GB of HBM hold them all) and
    the four 256-plane slabs of a 4-GPU decomposition must give the same Frangi image and the same labels, bit for bit."""
    import json
    import time
    free, _ = hip.device_mem_info(0)
    if free < 200e9 or os.environ.get("NELLIE_TEST_C4", "1") == "0":
        pytest.skip("needs ~170 GB of free HBM (and NELLIE_TEST_C4 != 0)")
    try:
        import psutil
        if psutil.virtual_memory().available < 90e9:
            pytest.skip("needs ~80 GB of free host RAM")
    except ImportError:
        pass
    from nellie_amd.synthetic import make_volume
    shape = (1024, 2048, 2048)
    vol = make_volume(shape, 3456)
    t0 = time.perf_counter()
    a = run_slabs(vol, shape, 8)
    t8 = time.perf_counter() - t0
    fr8 = np.concatenate([r[2] for r in a]); lab8 = np.concatenate([r[3] for r in a])
    thr8, n8, trace8 = a[0][4], a[0][5], a[0][6]
    assert all(r[4] == thr8 and r[5] == n8 for r in a)
    assert all([(sc.gamma, sc.max_abs, sc.frob_thr) for sc in r[6].scales] == [(sc.gamma, sc.max_abs, sc.frob_thr) for sc in trace8.scales]
               and r[6].percentile_thr == trace8.percentile_thr for r in a)
    del a
    # voxel-level against the oracle (filtering.py:806-853) where only the slab layout computes: 2048-wide rows, 137-plane
    # contexts, planes either side of the interfaces at z = 128 and z = 896, the X / Y faces of the wide planes
    c4_boxes = [((68, 188), (0, 280), (1768, 2048)), ((836, 956), (884, 1164), (884, 1164)), ((0, 120), (1768, 2048), (0, 280))]
    n_cmp = check_frangi_crops(vol, fr8, trace8, shape, c4_boxes, "C4 as 8 slabs")
    t0 = time.perf_counter()
    b = run_slabs(vol, shape, 4)
    t4 = time.perf_counter() - t0
    assert all(r[4] == thr8 and r[5] == n8 for r in b), ([r[4] for r in b], thr8, [r[5] for r in b], n8)
    for o0, o1, fr, lab, _, _, _ in b:
        assert np.array_equal(fr, fr8[o0:o1]), f"planes [{o0},{o1}): {int((fr != fr8[o0:o1]).sum())} Frangi voxels differ"
        assert np.array_equal(lab, lab8[o0:o1]), f"planes [{o0},{o1}): {int((lab != lab8[o0:o1]).sum())} label voxels differ"
    assert fr8.min() >= 0.0 and np.isfinite(fr8.max()) and n8 >= 10 and int(lab8.max()) == n8
    report = {"shape": list(shape), "voxels": int(np.prod(shape)), "labels": int(n8), "frangi_threshold": float(thr8),
              "survival_fraction": float(np.count_nonzero(fr8) / fr8.size), "labelled_fraction": float(np.count_nonzero(lab8) / lab8.size),
              "wall_s_8_slabs_one_gpu_incl_host_io": round(t8, 2), "wall_s_4_slabs_one_gpu_incl_host_io": round(t4, 2),
              "equal_bit_for_bit": True, "voxels_compared_with_the_oracle_in_boxes": n_cmp}
    os.makedirs("gpurun_out", exist_ok=True)
    with open("gpurun_out/c4_partition_invariance.json", "w") as f:
        json.dump(report, f)
    print(json.dumps(report))


# ---------------------------------------------------------------------------------------------------------------
# Markers and Hu-moment tracking at the headline size.  The oracle's markers_frame recomputes boxes from the RAW crops
# (labels, intensities, Frangi); oracle.markers_crop_margin gives the part of a box no artificial face reaches
# (tests/test_oracle_golden.py pins both).  Host RAM: ~50 GB at the peak of the tracking test.
# ---------------------------------------------------------------------------------------------------------------
def marker_oracle_boxes(intensity, labels, frangi, outs, shape, boxes, what):
    """marker / distance / border of a device run equal the oracle's on the valid interior of every box (boxes in threads:
    numpy releases the GIL in its loops).  Returns the oracle markers compared."""
    from concurrent.futures import ThreadPoolExecutor
    from nellie_amd.synthetic import ISO_01
    from oracle import nellie_oracle as orc
    margin = orc.markers_crop_margin(ISO_01)

    def one(box):
        sl = tuple(slice(a, b) for a, b in box)
        return orc.markers_frame(intensity[sl], labels[sl], ISO_01, frangi=None if frangi is None else frangi[sl])

    with ThreadPoolExecutor(max_workers=min(8, len(boxes))) as ex:
        refs = list(ex.map(one, boxes))
    n = 0
    for box, ref in zip(boxes, refs):
        sl = tuple(slice(a, b) for a, b in box)
        valid = crop_valid_slices(box, shape, margin)
        for name, got, want in zip(("marker", "distance", "border"), outs, ref):
            g, w = got[sl][valid], want[valid]
            assert np.array_equal(g, w), f"{what} box {box}: {name} differs at {int((g != w).sum())} voxels, first {np.argwhere(g != w)[:4].tolist()}"
        n += int(ref[0][valid].sum())
    return n


def check_marker_volume(labels, n, outs, clamp=20.0):
    """Whole-volume invariants: border = dilation6(mask) ^ mask; distance 0 off the mask, in [1, clamp] on it and the float32
    root of an integer below the clamp; markers only on mask & distance > 0; the count returned equals marker.sum()."""
    from oracle import nellie_oracle as orc
    marker, dist, border = outs
    assert marker.dtype == np.uint8 and dist.dtype == np.float32 and border.dtype == np.uint8
    nz = labels.shape[0]
    for z0 in range(0, nz, 64):                     # plane blocks (plus one plane each side for the dilation)
        z1 = min(nz, z0 + 64)
        e0, e1 = max(0, z0 - 1), min(nz, z1 + 1)
        m = labels[e0:e1] > 0
        want = (orc.binary_dilation6(m) ^ m)[z0 - e0:z0 - e0 + (z1 - z0)]
        m = m[z0 - e0:z0 - e0 + (z1 - z0)]
        assert np.array_equal(border[z0:z1] > 0, want) and border[z0:z1].max(initial=0) <= 1, f"border, planes [{z0}, {z1})"
        d = dist[z0:z1]
        assert not d[~m].any(), f"distance off the mask, planes [{z0}, {z1})"
        dm = d[m]
        assert dm.size == 0 or (dm.min() >= 1.0 and dm.max() <= np.float32(clamp)), f"distance range, planes [{z0}, {z1})"
        below = dm[dm < np.float32(clamp)].astype(np.float64)
        assert np.array_equal(np.sqrt(np.round(below * below)).astype(np.float32), below.astype(np.float32)), "d^2 not integral"
        mk = marker[z0:z1] > 0
        assert not (mk & ~(m & (d > 0))).any() and marker[z0:z1].max(initial=0) <= 1, f"markers off the mask, planes [{z0}, {z1})"
    assert int(np.count_nonzero(marker)) == n


def densest_box(labels, shape, starts, size, margin):
    """the box (from candidate starts) whose valid interior holds the most mask voxels"""
    best, arg = -1, None
    for s in starts:
        box = tuple((a, a + size) for a in s)
        sl = tuple(slice(a, b) for a, b in box)
        valid = crop_valid_slices(box, shape, margin)
        c = int(np.count_nonzero(labels[sl][valid]))
        if c > best:
            best, arg = c, box
    return arg


def run_markers_resident(vol, n_labels, env):
    """Filter -> Label -> Markers on one FramePipeline, nothing leaving the device in between (use_im='distance', the float32
    input read in place)."""
    from nellie_amd import pipeline as pl
    from nellie_amd.synthetic import ISO_01
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    pipe = pl.FramePipeline(SHAPE)
    try:
        pipe.load_input(vol)                            # resident: Filter starts from it, Markers reads its intensities there
        pipe.filter(None, pl.FilterParams(dim_res=ISO_01))
        assert pipe.label(pipe.frangi_threshold(), pl.min_area_pixels_of(ISO_01)) == n_labels
        n = pipe.markers(ISO_01)
        return n, tuple(a.reshape(SHAPE) for a in pipe.download_markers())
    finally:
        pipe.close()
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def markers_run(full_run):
    n, outs = run_markers_resident(full_run["vol"], full_run["n"], {"NELLIE_MK_SPARSE": "1", "NELLIE_MK_POISON": "0"})
    return dict(n=n, marker=outs[0], distance=outs[1], border=outs[2])


def test_markers_resident_chain_at_1024_cube(full_run, markers_run):
    """Markers at the headline size (mk_edt_x_kernel and mk_nms_kernel take 8 trips of their capped grids, mk_tile_mark_kernel
    4, the sparse LoG 16 Z chunks): whole-volume invariants, the oracle on a corner box, an X-face box and the densest interior
    box, and the sparse LoG bit-identical to its NaN-poisoned form and to the dense LoG."""
    from nellie_amd.synthetic import ISO_01
    from oracle import nellie_oracle as orc
    outs = (markers_run["marker"], markers_run["distance"], markers_run["border"])
    lab = full_run["labels"]
    check_marker_volume(lab, markers_run["n"], outs)
    margin = orc.markers_crop_margin(ISO_01)
    L, nx = 256, SHAPE[2]
    mid = (128, 384, 640)
    boxes = [((0, L), (0, L), (0, L)),
             densest_box(lab, SHAPE, [(z, y, nx - L) for z in mid for y in mid], L, margin),
             densest_box(lab, SHAPE, [(z, y, x) for z in mid for y in mid for x in mid], L, margin)]
    n_cmp = marker_oracle_boxes(full_run["vol"], lab, None, outs, SHAPE, boxes, "1024^3")
    print(f"1024^3 Markers: {markers_run['n']} markers, {n_cmp} compared with the oracle in boxes {boxes}")
    assert n_cmp >= 1000
    for env in ({"NELLIE_MK_SPARSE": "1", "NELLIE_MK_POISON": "1"}, {"NELLIE_MK_SPARSE": "0", "NELLIE_MK_POISON": "0"}):
        n2, outs2 = run_markers_resident(full_run["vol"], full_run["n"], env)
        assert n2 == markers_run["n"], env
        for name, a, b in zip(("marker", "distance", "border"), outs2, outs):
            assert np.array_equal(a, b), f"{env}: {name} differs at {int((a != b).sum())} voxels"
        del outs2


def test_markers_odd_frame_above_2_30_voxels(full_run):
    """Markers from host inputs on a 1030 x 1090 x 1100 frame (1.235e9 voxels: 18-word rows with a partial last word, ny no
    multiple of the 16-row tile or the 4-row peak group, a second trip of mk_tile_list_kernel), uint16 intensities and
    use_im='frangi', with thick solids planted in the labels whose interiors reach the distance clamp: a ball of radius 45, a
    60 x 200 x 200 block across the Z chunk seam at z = 128, slabs on the x = nx - 1 and z = 0 faces."""
    from nellie_amd import pipeline as pl
    from nellie_amd.synthetic import ISO_01
    pad = ((3, 3), (33, 33), (38, 38))
    lab = np.pad(full_run["labels"], pad, mode="reflect")
    shape = lab.shape
    assert shape == (1030, 1090, 1100) and lab.size > 2 ** 30
    nz, ny, nx = shape
    zz, yy, xx = np.ogrid[:nz, :ny, :nx]
    k = int(lab.max()) + 1
    ball = (500, 300, 700)
    lab[455:546, 255:346, 655:746][((zz[455:546] - ball[0]) ** 2 + (yy[:, 255:346] - ball[1]) ** 2
                                    + (xx[:, :, 655:746] - ball[2]) ** 2) <= 45 * 45] = k
    lab[100:160, 600:800, 150:350] = k + 1
    lab[700:760, 100:220, nx - 50:] = k + 2
    lab[:50, 850:970, 850:970] = k + 3
    vol = np.clip(np.rint(np.pad(full_run["vol"], pad, mode="reflect")), 0, 65535).astype(np.uint16)
    fr = np.pad(full_run["frangi"], pad, mode="reflect")
    pipe = pl.FramePipeline(shape)
    try:
        n = pipe.markers(ISO_01, labels=lab, intensity=vol, use_image=fr)
        outs = tuple(a.reshape(shape) for a in pipe.download_markers())
    finally:
        pipe.close()
    check_marker_volume(lab, n, outs)
    dist = outs[1]
    for name, sl in (("ball", ball), ("block", (130, 700, 250)), ("x-face slab", (730, 160, nx - 21)), ("z-face slab", (20, 910, 910))):
        assert dist[sl] == np.float32(20.0), f"{name}: distance {dist[sl]} at {sl} does not reach the clamp"
    boxes = [((nz - 256, nz), (ny - 256, ny), (nx - 256, nx)),          # the far corner
             ((418, 582), (218, 382), (618, 782)),                     # the ball
             ((65, 195), (565, 835), (115, 385)),                      # the block
             ((665, 795), (65, 255), (nx - 85, nx)),                   # the slab on the x = nx - 1 face
             ((0, 85), (815, 1005), (815, 1005))]                      # the slab on the z = 0 face
    n_cmp = marker_oracle_boxes(vol, lab, fr, outs, shape, boxes, "1030x1090x1100")
    print(f"1030x1090x1100 Markers: {n} markers, {n_cmp} compared with the oracle")
    assert n_cmp >= 1000


def test_markers_as_two_z_slabs_at_1024_cube(full_run, markers_run, monkeypatch):
    """The Markers stage class with the frame cut into two Z slabs (each with its halo) writes the single-context products."""
    from fakes import ArrayImInfo
    from nellie_amd.segmentation.mocap_marking import Markers
    from nellie_amd.synthetic import ISO_01
    monkeypatch.setenv("NELLIE_FORCE_SLABS", "2")
    im = ArrayImInfo(full_run["vol"][None], ISO_01)
    im.store["labels"] = full_run["labels"][None].view(type(im.store["im"]))
    mk = Markers(im, device="gpu")
    mk.run()
    assert mk._slab_plan(SHAPE)[0] >= 2
    for key in ("marker", "distance", "border"):
        a, b = np.asarray(im.store[key])[0], markers_run[key]
        assert a.dtype == b.dtype and np.array_equal(a, b), f"{key}: {int((a != b).sum())} voxels differ"


def _radii_at(distance, coords):
    """ceil(2 * (3 x 3 x 3 maximum of the distance, faces clamped)) at the markers: the ROI radius of the tracker"""
    m = np.zeros(len(coords), np.float32)
    for off in np.ndindex(3, 3, 3):
        c = np.clip(coords + np.array(off) - 1, 0, np.array(distance.shape) - 1)
        m = np.maximum(m, distance[tuple(c.T)])
    return np.ceil(m * np.float32(2)).astype(np.int64)


def test_tracking_at_1024_cube(full_run, markers_run, tmp_path):
    """HuMomentTracking at the headline size: frame 0 is the 1024^3 intensity, Frangi and Markers products plus markers at
    linear index 0 and 2^30 - 1 and on both sides of 4096-voxel chunk and scan-segment edges; frame 1 is frame 0 rolled by
    (1, 2, -1).  (Frangi voxels where the host's float32 log10 is not the correctly rounded one are zeroed.)  Coordinates equal argwhere; features of a sample (3000 seeded markers, the planted ones, every marker whose ROI a
    face clips, the largest ROI) equal the restatement; sparse matching equals the restatement; every frame-1 marker whose
    ROI clears the rolled faces and with no other marker nearer than the shift takes its own pre-roll copy.  Host RAM ~50 GB."""
    import hu_tracking_restatement as rs
    from test_hip_tracking import assert_features, bad_rows, run_stage
    from nellie_amd import hipnative
    spacing, shift = (0.1, 0.1, 0.1), (1, 2, -1)
    n = int(np.prod(SHAPE))
    marker = markers_run["marker"].copy()
    nblk = n // 4096
    seg = (nblk + 1023) // 1024
    planted = {0, n - 1}
    for kk in (1, 2, nblk // 2, nblk - 1):
        planted |= {kk * 4096 - 1, kk * 4096}
    for t in (1, 2, 511, 512, 1023):
        planted |= {t * seg * 4096 - 1, t * seg * 4096}
    planted = np.array(sorted(planted))
    marker.flat[planted] = 1
    # Frangi voxels whose float32 log10 is not the float64 one rounded are zeroed (as test_hip_tracking.exact_log_frangi does):
    # numpy's float32 log10 depends on the host, the device's is the correctly rounded one
    fr = full_run["frangi"].copy()
    for z0 in range(0, SHAPE[0], 64):
        blk = fr[z0:z0 + 64]
        with np.errstate(divide="ignore"):
            blk[(blk > 0) & (np.log10(blk) != np.log10(blk.astype(np.float64)).astype(np.float32))] = 0
    f0 = (full_run["vol"], fr, markers_run["distance"], marker)
    f1 = tuple(np.roll(a, shift, axis=(0, 1, 2)) for a in f0)
    feats = []
    with hipnative.Tracker(SHAPE, spacing) as trk:
        trk.frame(*f0)
        c0, s0, h0 = trk.features(0)
        trk.frame(*f1)
        c1, s1, h1 = trk.features(0)
        ri, rc, ci, cc = trk.match("sparse", 1.0)
    feats = [(c0, c0 * np.asarray(spacing), s0, h0), (c1, c1 * np.asarray(spacing), s1, h1)]
    shp = np.array(SHAPE)
    rng = np.random.default_rng(77)
    for t, (fr, (c, _, s, h)) in enumerate(zip((f0, f1), feats)):
        assert np.array_equal(c, np.argwhere(fr[3]))
        r = _radii_at(fr[2], c)
        pick = np.zeros(len(c), bool)
        pick[rng.choice(len(c), 3000, replace=False)] = True
        pick |= np.isin(np.ravel_multi_index(tuple(c.T), SHAPE), np.ravel_multi_index(tuple(np.unravel_index(planted, SHAPE)), SHAPE)
                        if t == 0 else np.ravel_multi_index(tuple(((np.array(np.unravel_index(planted, SHAPE)).T + shift) % shp).T), SHAPE))
        pick |= ((c - r[:, None]) < 0).any(axis=1) | ((c + r[:, None]) >= shp).any(axis=1)
        pick[int(np.argmax(r))] = True                   # the largest ROI sets the zero-padded R^3 of the float sums
        sample = np.zeros(SHAPE, np.uint8)
        sample[tuple(c[pick].T)] = 1
        want = rs.frame_features(fr[0], fr[1], fr[2], sample, spacing)
        assert_features((c[pick], s[pick], h[pick]), want)
        print(f"tracking 1024^3 frame {t}: {len(c)} markers, {int(pick.sum())} compared with the restatement")
        del sample
    stack = tuple(np.stack([a, b]) for a, b in zip(f0, f1))
    flow = run_stage(tmp_path, stack, spacing, 1.0, "sparse")
    want = rs.track([(stack[0][t],) for t in range(2)], spacing, mode="sparse", features=feats)
    bad = bad_rows(flow, want)
    n_markers = len(c0) + len(c1)
    print(f"tracking 1024^3 sparse: {n_markers} markers, {len(want)} rows, {bad} differing")
    assert len(want) > 0 and bad <= max(2, 2 * n_markers // 10000), bad
    del stack
    # known answer: the pre-roll copy wins every row whose ROI clears the rolled faces and with no rival nearer than the shift
    pre = c1 - np.array(shift)
    r1 = _radii_at(f1[2], c1)
    ok = ((pre - r1[:, None] - 1) >= 0).all(axis=1) & ((pre + r1[:, None] + 1) < shp).all(axis=1)
    ok &= ((c1 - r1[:, None] - 1) >= 0).all(axis=1) & ((c1 + r1[:, None] + 1) < shp).all(axis=1)
    d_shift = float(np.dot(shift, shift))
    for off in np.ndindex(5, 5, 5):
        o = np.array(off) - 2
        if float(np.dot(o, o)) <= d_shift and tuple(o) != tuple(shift):
            q = np.clip(c1 - o, 0, shp - 1)
            ok &= ~((marker[tuple(q.T)] > 0) & ((c1 - o) == q).all(axis=1))
    own = np.searchsorted(np.ravel_multi_index(tuple(c0.T), SHAPE), np.ravel_multi_index(tuple(np.where(ok[:, None], pre, 0).T), SHAPE))
    hit = ok & (ri == own)
    print(f"tracking 1024^3 known answer: {int(hit.sum())} of {int(ok.sum())} eligible rows ({len(c1)} markers) take their own copy")
    assert int(ok.sum()) >= len(c1) // 2 and int(hit.sum()) == int(ok.sum())
    assert np.array_equal(s1[ok], s0[own[ok]]) and np.array_equal(h1[ok], h0[own[ok]])
