"""
GPU parity tests (-m gpu): the HIP path, called through the C-ABI, against
  (1) the golden vectors captured from the reference, and
  (2) the oracle on seeded inputs.
Bars: Gaussian scale space, every threshold, max|H|, mask counts, labels: bit-exact.
Frangi response: |a-b| <= 1e-4*|ref| + 1e-6*max|ref| (float32 `exp` differs by <= 1 ulp between
numpy and the device; SURVEY.md section 8(d) / DESIGN.md explain why plain per-voxel rtol is
unattainable for 1-exp(-x) at small x).
"""
import zlib

import os

import numpy as np
import pytest

from conftest import FILTER_2D_CASES, MARKERS_CASES, FILTER_CASES, LABEL_INTENSITY_CASES, LABEL_ONLY_CASES, load_golden
from oracle import nellie_oracle as orc

pytestmark = pytest.mark.gpu

RTOL, ATOL_REL = 1e-4, 1e-6


def assert_frangi_close(got, ref, what=""):
    assert got.dtype == np.float32 and got.shape == ref.shape
    scale = float(np.max(np.abs(ref))) if ref.size else 0.0
    tol = RTOL * np.abs(ref) + ATOL_REL * scale
    bad = np.abs(got.astype(np.float64) - ref.astype(np.float64)) > tol
    assert not bad.any(), f"{what}: {int(bad.sum())} voxels outside tolerance, max|d|={np.abs(got - ref).max()}"
    assert np.array_equal(got > 0, ref > 0), f"{what}: support differs"


TIE_ZONE_USED = {}      # what -> voxels that used the relaxation below (printed by test_tie_zone_report)


def assert_masked_close(got, ref, run_frame_ref, thr_ref, what="frangi"):
    """
    After _mask_volume (filtering.py:964-966) the frame went through `> percentile` and a binary
    opening.  A voxel whose value sits within the Frangi tolerance of the threshold may legitimately
    fall on either side, and the opening carries that decision to voxels within L1 distance 2.
    Everywhere else the usual bar applies (tolerance on values, identical support).
    """
    thr = np.float32(thr_ref)
    border = np.abs(run_frame_ref - thr) <= (2 * RTOL * abs(float(thr)) + ATOL_REL * float(run_frame_ref.max()))
    zone = border.copy()
    for _ in range(2):
        zone = orc.binary_dilation6(zone)
    if not border.any():
        assert_frangi_close(got, ref, what)
        return
    keep = ~zone
    g2, r2 = np.where(keep, got, 0).astype(np.float32), np.where(keep, ref, 0).astype(np.float32)
    assert_frangi_close(g2, r2, what + " (outside the threshold-tie zone)")
    # inside the zone a voxel is either the reference value, or zero, or the unmasked value
    inside = zone & (got != ref)
    ok = (got[inside] == 0) | (np.abs(got[inside] - run_frame_ref[inside]) <= RTOL * np.abs(run_frame_ref[inside]) + ATOL_REL * run_frame_ref.max())
    assert ok.all(), f"{what}: unexplained values inside the threshold-tie zone"
    # the relaxation is for a handful of voxels next to an exact tie; a regression that widens the zone must not pass
    # (a tie voxel reaches the 25 voxels within L1 distance 2 through the opening; symmetric inputs have exact ties by the
    # dozen without using the relaxation at all, so the bounds are: at most 25 voxels per tie, and ties a small fraction of the support
    # (measured on the goldens: 0-33 ties, 0-116 voxels using the relaxation)
    used, ties = int(inside.sum()), int(border.sum())
    TIE_ZONE_USED[what] = max(TIE_ZONE_USED.get(what, (0, 0)), (ties, used))
    cap = 64 + int(1e-3 * np.count_nonzero(ref))
    assert used <= 25 * ties and ties <= cap, f"{what}: {ties} near-tie voxels (cap {cap}), {used} voxels used the relaxation"


def _params(g):
    from nellie_amd.pipeline import FilterParams
    kw = dict(g["kwargs"])
    return FilterParams(dim_res=g["dim_res_dict"], **kw)


@pytest.fixture(scope="module")
def pipes(hip):
    from nellie_amd.pipeline import FramePipeline
    cache = {}

    def get(shape):
        shape = tuple(int(s) for s in shape)
        if shape not in cache:
            cache[shape] = FramePipeline(shape)
        return cache[shape]
    yield get
    for p in cache.values():
        p.close()


@pytest.mark.parametrize("one_pass", [True, False], ids=["one_pass", "two_pass"])
@pytest.mark.parametrize("name", FILTER_CASES)
def test_filter_golden(name, one_pass, pipes):
    g = load_golden(name)
    vol = g["input"]
    pipe = pipes(vol.shape)
    pipe.one_pass = one_pass and pipe.ctx.one_pass_available()
    p = _params(g)
    if "error_type" in g:
        with pytest.raises(ValueError, match=str(g["error_msg"])[:30]) as ei:       # (numpy.linalg.LinAlgError is a ValueError)
            pipe.filter(vol, p, mask=g["run_mask"])
        assert type(ei.value).__name__ == str(g["error_type"])
        return
    assert np.array_equal(np.array(p.resolved_sigmas()), g["sigmas"])
    pipe.compute_vesselness(vol, p, mask=g["run_mask"])
    tr = pipe.trace
    assert len(tr.scales) == len(g["gamma"])
    if not g["run_mask"]:
        # Filter.run(mask=False) (filtering.py:566-567): every voxel of every scale goes to the eigen queue.  No bracket exists to
        # speculate on, so neither the one-pass walk nor the device chain may have been used -- the known-threshold walk queues at
        # full capacity (one entry per voxel of a wave's region), which cannot overflow
        assert not any(sc.one_pass for sc in tr.scales) and all(sc.mask_count == vol.size for sc in tr.scales)
    for s, sc in enumerate(tr.scales):
        assert sc.gamma == g["gamma"][s], f"gamma scale {s}"
        assert sc.max_abs == g["max_abs"][s], f"max_abs scale {s}"
        if g["run_mask"] and not np.isnan(g["frob_thr"][s]):      # (mask=False never derives a threshold)
            assert sc.frob_thr == g["frob_thr"][s], f"frob threshold scale {s}"
        assert sc.mask_count == (0 if sc.skipped else g["mask_count"][s]), f"mask count scale {s}"
        assert sc.skipped == (g["mask_count"][s] == 0)
    run_frame = pipe.download_frangi()
    assert_frangi_close(run_frame, g["run_frame"], "run_frame")
    if tr.n_positive > 0:
        thr = pipe.mask_volume(p)
        # the percentile interpolates two order statistics of the (tolerance-equal) Frangi samples
        assert abs(float(thr) - float(g["percentile_thr"])) <= 2e-4 * float(g["percentile_thr"]) + 1e-12
        assert_masked_close(pipe.download_frangi(), g["frangi"], g["run_frame"], g["percentile_thr"])
    else:
        assert_frangi_close(pipe.download_frangi(), g["frangi"], "frangi")


@pytest.mark.parametrize("shape,aniso", [((40, 96, 80), False), ((21, 70, 131), True)])
def test_one_pass_vesselness_equals_two_pass(shape, aniso, hip):
    """nl_vesselness_spec + nl_vesselness_resolve (one walk over the Hessian per scale) against nl_hessian_stats +
    nl_vesselness_step (two walks): identical bits, identical trace; a bracket that misses falls back."""
    from nellie_amd.pipeline import FilterParams, FramePipeline
    from nellie_amd.synthetic import ANISO_03, ISO_01, make_volume
    vol = make_volume(shape, 99)
    p = FilterParams(dim_res=ANISO_03 if aniso else ISO_01)
    out = {}
    for mode in ("two", "one", "miss", "ahead"):
        pipe = FramePipeline(shape)
        assert pipe.ctx.one_pass_available()
        pipe.one_pass = mode != "two"
        if mode == "miss":
            pipe._one_pass_test_scale = 1.2
        pipe._gauss_ahead = mode == "ahead"          # cascade step of scale s+1 beside the Hessian walk of scale s
        pipe.compute_vesselness(vol, p)
        out[mode] = (pipe.download_frangi(), pipe.trace)
        pipe.close()
    f2, t2 = out["two"]
    for mode in ("one", "miss", "ahead"):
        f1, t1 = out[mode]
        assert np.array_equal(f1.view(np.uint32), f2.view(np.uint32)), mode
        assert t1.n_positive == t2.n_positive
        for a, b in zip(t1.scales, t2.scales):
            assert (a.gamma, a.max_abs, a.frob_thr, a.mask_count, a.skipped) == (b.gamma, b.max_abs, b.frob_thr, b.mask_count, b.skipped)
            assert a.one_pass == (mode in ("one", "ahead") and not a.skipped)


def test_one_pass_queue_overflow_falls_back(hip):
    """A dense texture of domes (negative Hessian trace on 60 % of the voxels of a wave's region, all of them masked) fills more
    than half of a queue region: the one-pass walk reports the overflow and the scale is redone the two-pass way -- same bits.
    (Until round 4 a sin x sin x sin texture did that; the two-sided trace test keeps its positive-trace half out of the queue.)"""
    from nellie_amd.pipeline import FilterParams, FramePipeline
    from nellie_amd.synthetic import ISO_01
    shape = (64, 64, 128)
    z, y, x = np.mgrid[:shape[0], :shape[1], :shape[2]]
    vol = np.random.default_rng(3).normal(100, 0.02, shape).astype(np.float32)
    vol += (50.0 * (np.abs(np.sin(0.15 * x)) + np.abs(np.sin(0.15 * y)) + np.abs(np.sin(0.15 * z)))).astype(np.float32)
    out = {}
    for mode in (False, True):
        pipe = FramePipeline(shape)
        pipe.one_pass = mode
        overflow = []
        spec = pipe.ctx.vesselness_spec
        pipe.ctx.vesselness_spec = lambda *a, **k: (lambda r: (overflow.append(bool(r[3])), r)[1])(spec(*a, **k))
        pipe.compute_vesselness(vol, FilterParams(dim_res=ISO_01))
        out[mode] = (pipe.download_frangi(), [s.mask_count for s in pipe.trace.scales], [s.one_pass for s in pipe.trace.scales], overflow)
        pipe.close()
    assert any(out[True][3]), "the texture was meant to overflow a queue region"
    assert [h for h, o in zip(out[True][2], out[True][3]) if o] == [False] * sum(out[True][3])
    assert out[True][1] == out[False][1]
    assert np.array_equal(out[True][0].view(np.uint32), out[False][0].view(np.uint32))


@pytest.mark.parametrize("scale", [1e15, 1e16, 3e16, 1e17, 3e17])
def test_hessians_whose_frob_sq_overflows_float32(hip, scale):
    """Intensities of 1e17 ... 1e19: from 1e16 on the squared Frobenius norm of some Hessians is +inf in float32 (filtering.py:421-426
    handles that), the one-pass walk hands those scales to the two-pass path, and the eigenvalues -- float64 from finite components --
    still give responses > 0.  The walk's queue test (trace |trace| + 0.30 frob_sq < 0) must not drop such a voxel: round 4's first
    form did, and only this probe showed it."""
    from nellie_amd.pipeline import FilterParams, FramePipeline
    from nellie_amd.synthetic import ISO_01, make_volume
    shape = (40, 96, 96)
    vol = (make_volume(shape, 5).astype(np.float64) * scale).astype(np.float32)
    with np.errstate(all="ignore"):
        ref = orc.run_frame(vol, ISO_01)
    pipe = FramePipeline(shape)
    pipe.compute_vesselness(vol, FilterParams(dim_res=ISO_01))
    got = pipe.download_frangi()
    two_pass = [not s.one_pass for s in pipe.trace.scales]
    pipe.close()
    if scale >= 1e16:
        assert any(two_pass), "these intensities were meant to overflow frob_sq"
    assert_frangi_close(got, ref, f"scale {scale:g}")


def test_two_pass_vesselness_in_several_launches(hip):
    """The two-pass path launches the Hessian kernel per block of Z chunks when the eigen queue is small
    (NELLIE_VQ_CAP is read once per process, hence the child processes): same bits as one launch."""
    import subprocess
    import sys
    code = (
        "import sys, zlib, numpy as np; sys.path.insert(0, %r)\n"
        "from nellie_amd import pipeline as pl\n"
        "from nellie_amd.synthetic import ISO_01, make_volume\n"
        "shape = (150, 40, 70); vol = make_volume(shape, 77)\n"
        "pipe = pl.FramePipeline(shape); pipe.one_pass = False\n"
        "pipe.compute_vesselness(vol, pl.FilterParams(dim_res=ISO_01))\n"
        "print(zlib.crc32(pipe.download_frangi().tobytes()), [s.mask_count for s in pipe.trace.scales])\n"
    ) % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for cap in ("", "200000"):          # default (one launch) / two Z chunks per launch at most
        env = dict(os.environ)
        env.pop("NELLIE_VQ_CAP", None)
        if cap:
            env["NELLIE_VQ_CAP"] = cap
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(r.stdout.strip().splitlines()[-1])
    assert outs[0] == outs[1]


@pytest.mark.parametrize("name", [n for n in FILTER_CASES if n.startswith(("iso", "aniso", "odd", "u16"))])
@pytest.mark.parametrize("fused", ["auto", "fused", "two_kernels"])
def test_gaussian_scale_space_bitexact(name, fused, pipes, monkeypatch):
    """The Gaussian of every scale, CRC for CRC, through each form of the cascade step: the fused Z+Y+X kernel (the default on volumes
    of 2^26 voxels and more; forced here), the Z march + the fused Y+X pass, and whatever the size rule picks."""
    from nellie_amd import pipeline as pl
    if fused != "auto":
        monkeypatch.setenv("NELLIE_GAUSS_FUSED", "1" if fused == "fused" else "0")
    g = load_golden(name)
    vol = g["input"]
    pipe = pipes(vol.shape)
    dr = g["dim_res_dict"]
    pipe.ctx.filter_load(vol)
    sig = pl.default_sigmas(dr)
    for s, delta in enumerate(pl.cascade_deltas(sig, pl.z_ratio_of(dr))):
        pipe.ctx.gauss_step(*[pl.gaussian_weights(d) for d in delta])
        gauss = pipe.ctx.gauss_store()
        assert np.uint32(zlib.crc32(gauss.tobytes())) == g["gauss_crc"][s], f"scale {s}"


@pytest.mark.parametrize("shape,dr", [((37, 70, 131), {"X": 0.1, "Y": 0.1, "Z": 0.1, "T": 1.0}),       # rows of 131: scalar stores, partial tiles both ways
                                      ((21, 48, 64), {"X": 0.1, "Y": 0.1, "Z": 0.3, "T": 1.0}),         # Z radii 1, 1, 1, 1, 2 beside in-plane 4, 3, 4, 4, 5
                                      ((150, 49, 66), {"X": 0.1, "Y": 0.1, "Z": 0.2, "T": 1.0}),        # two Z chunks, Z radii 2-3
                                      ((9, 200, 300), {"X": 0.1, "Y": 0.1, "Z": 0.1, "T": 1.0})])       # fewer planes than 2 R + 1 of the last scale
def test_fused_cascade_step_equals_two_kernels(hip, shape, dr, monkeypatch):
    """The fused Z+Y+X kernel against the Z march + Y+X pass on shapes the goldens do not have: every scale's Gaussian volume and the
    frame, bit for bit, from float32 and uint16 input."""
    from nellie_amd import pipeline as pl
    from nellie_amd.synthetic import make_volume
    for dtype in (np.float32, np.uint16):
        vol = make_volume(shape, 17, dtype=dtype)
        outs = []
        for fused in ("0", "1"):
            monkeypatch.setenv("NELLIE_GAUSS_FUSED", fused)
            pipe = pl.FramePipeline(shape)
            pipe.ctx.filter_load(vol)
            crcs = []
            sig = pl.default_sigmas(dr)
            for delta in pl.cascade_deltas(sig, pl.z_ratio_of(dr)):
                pipe.ctx.gauss_step(*[pl.gaussian_weights(d) for d in delta])
                crcs.append(zlib.crc32(pipe.ctx.gauss_store().tobytes()))
            pipe.filter(vol, pl.FilterParams(dim_res=dr))
            outs.append((crcs, pipe.download_frangi()))
            pipe.close()
        assert outs[0][0] == outs[1][0], f"{shape} {dtype}: Gaussian volumes differ"
        assert np.array_equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("name", [n for n in FILTER_CASES] + LABEL_ONLY_CASES)
def test_label_golden_bitexact(name, pipes):
    from nellie_amd import pipeline as pl
    g = load_golden(name)
    if "error_type" in g:
        pytest.skip("reference raises on this input")
    fr = g["frangi"]
    pipe = pipes(fr.shape)
    pipe.upload_frangi(fr)
    thr = pipe.frangi_threshold()
    if np.isnan(g["label_thr"]):
        assert thr is None
    else:
        assert float(thr) == float(g["label_thr"])
    n = pipe.label(thr, pl.min_area_pixels_of(g["dim_res_dict"]))
    labels = pipe.download_labels()
    assert labels.dtype == np.int32
    assert np.array_equal(labels, g["labels"])
    assert n == int(g["labels"].max())


@pytest.mark.parametrize("shape,seed,aniso", [((40, 96, 96), 21, False), ((33, 70, 130), 22, True),
                                              ((64, 128, 136), 23, False)])
def test_end_to_end_vs_oracle(shape, seed, aniso, pipes):
    """Seeded volumes the oracle finishes in seconds (the largest exceeds 1e6 voxels: strided sampling)."""
    from nellie_amd import pipeline as pl
    from nellie_amd.synthetic import ANISO_03, ISO_01, make_volume
    dr = ANISO_03 if aniso else ISO_01
    vol = make_volume(shape, seed)
    ref_fr = orc.filter_frame(vol, dr)
    ref_lab = orc.label_frame(ref_fr, dr)
    pipe = pipes(shape)
    pipe.filter(vol, pl.FilterParams(dim_res=dr))
    fr = pipe.download_frangi()
    assert_frangi_close(fr, ref_fr, "frangi")
    # Label on the oracle's own Frangi image: bit-exact
    pipe.upload_frangi(ref_fr)
    thr = pipe.frangi_threshold()
    pipe.label(thr, pl.min_area_pixels_of(dr))
    assert np.array_equal(pipe.download_labels(), ref_lab)
    # end to end (device Frangi -> device labels): report, and require the same objects
    pipe.upload_frangi(fr)
    pipe.label(pipe.frangi_threshold(), pl.min_area_pixels_of(dr))
    lab = pipe.download_labels()
    match = float(np.mean(lab == ref_lab))
    n_diff = int((lab != ref_lab).sum())
    print(f"E2E {shape} seed {seed}: end-to-end label match fraction {match:.8f} ({n_diff} voxels), labels {lab.max()} vs {ref_lab.max()}")
    # measured on these seeded volumes (MI355X, round 3): identical labellings
    assert n_diff == 0 and int(lab.max()) == int(ref_lab.max())


@pytest.mark.parametrize("name", FILTER_2D_CASES)
def test_filter_and_label_2d_golden(name, hip):
    """2-D images (im_info.no_z) against the reference's own outputs: thresholds / statistics / mask counts equal,
    Gaussian scale space bit-exact, Frangi + blob response within the Frangi tolerance, Label bit-exact."""
    from nellie_amd import pipeline as pl
    g = load_golden(name)
    img, dr = g["input"], g["dim_res_dict"]
    kw = dict(g["kwargs"])
    rm = bool(kw.pop("remove_edges", False))
    p = pl.FilterParams(dim_res=dr, **kw)
    pipe = pl.FramePipeline(img.shape)
    try:
        assert pipe.two_d and np.array_equal(np.array(p.resolved_sigmas()), g["sigmas"])
        pipe.compute_vesselness(img, p, mask=g["run_mask"])
        tr = pipe.trace
        assert len(tr.scales) == len(g["gamma"])
        for s, sc in enumerate(tr.scales):
            assert sc.gamma == g["gamma"][s] and sc.max_abs == g["max_abs"][s]
            if g["run_mask"] and not np.isnan(g["frob_thr"][s]):      # (mask=False never derives a threshold)
                assert sc.frob_thr == g["frob_thr"][s]
            assert sc.mask_count == (0 if sc.skipped else g["mask_count"][s])
        run_frame = pipe.download_frangi()[0]
        if rm:
            run_frame = orc.remove_edges_2d(run_frame)
            pipe.upload_frangi(run_frame)
        assert_frangi_close(run_frame, g["run_frame"], "run_frame")
        if float(run_frame.sum()) > 0:
            thr = pipe.mask_volume(p)
            assert abs(float(thr) - float(g["percentile_thr"])) <= 2e-4 * float(g["percentile_thr"]) + 1e-12
            fr = pipe.download_frangi()[0]
            assert_masked_close(fr[None], g["frangi"][None], g["run_frame"][None], g["percentile_thr"])
        # Label on the reference's Frangi image: bit-exact
        pipe.upload_frangi(g["frangi"])
        thr = pipe.frangi_threshold()
        if np.isnan(g["label_thr"]):
            assert thr is None
        else:
            assert float(thr) == float(g["label_thr"])
        assert pl.min_area_pixels_of(dr, no_z=True) == int(g["min_area_pixels"])
        pipe.label(thr, int(g["min_area_pixels"]), fill_holes=False)
        assert np.array_equal(pipe.download_labels()[0], g["labels"])
    finally:
        pipe.close()


def test_stage_api_2d(hip):
    """Filter / Label stage classes on a (T, Y, X) stack (im_info.no_z)."""
    from fakes import ArrayImInfo
    from nellie_amd.segmentation.filtering import Filter
    from nellie_amd.segmentation.labelling import Label
    from nellie_amd.synthetic import make_image_2d
    dr = {"X": 0.1, "Y": 0.1, "Z": None, "T": 1.0}
    stack = np.stack([make_image_2d((80, 96), 40 + t) for t in range(2)])
    im_info = ArrayImInfo(stack, dr, no_z=True)
    before = stack.copy()
    Filter(im_info).run()
    Label(im_info).run()
    assert np.array_equal(im_info.store["im"], before), "input was modified"
    for t in range(2):
        ref_fr = orc.filter_frame_2d(stack[t], dr)
        fr = np.asarray(im_info.store["frangi"][t])
        assert fr.shape == ref_fr.shape
        assert_frangi_close(fr, ref_fr, f"t={t}")
        ref_lab = orc.label_frame_2d(fr, dr)
        assert np.array_equal(np.asarray(im_info.store["labels"][t]), ref_lab)


@pytest.mark.parametrize("name", MARKERS_CASES)
@pytest.mark.parametrize("mode", ["sparse", "sparse+poison", "dense"])
def test_markers_golden_bitexact(name, mode, hip, monkeypatch):
    """Markers stage against the reference's own outputs: marker, distance and border images bit for bit -- 3-D and
    2-D images, use_im='distance' and use_im='frangi'.  The LoG only computes the tiles somebody reads (default); with the scratch
    volumes poisoned by NaNs first a value taken from a skipped tile would show; NELLIE_MK_SPARSE=0 is the dense form."""
    from nellie_amd import pipeline as pl
    monkeypatch.setenv("NELLIE_MK_SPARSE", "0" if mode == "dense" else "1")
    monkeypatch.setenv("NELLIE_MK_POISON", "1" if mode == "sparse+poison" else "0")
    g = load_golden(name)
    dr = g["dim_res_dict"]
    kw = {k: (int(v) if k in ("peak_min_distance", "num_sigma") else v) for k, v in g["kwargs"].items()}
    vol, lab, fr = g["input"], g["labels_in"], g.get("frangi_in")
    pipe = pl.FramePipeline(vol.shape)
    try:
        sig, _ = pl.marker_sigmas(dr, num_sigma=kw.get("num_sigma", 5))
        assert np.array_equal(np.array(sig), g["sigmas"])
        n = pipe.markers(dr, labels=lab, intensity=vol, use_image=fr, **kw)
        marker, dist, border = (a.reshape(vol.shape) for a in pipe.download_markers())
        assert np.array_equal(dist, g["distance"])
        assert np.array_equal(border, g["border"])
        assert np.array_equal(marker, g["marker"]) and n == int(g["marker"].sum())
        if vol.ndim == 3 and fr is None:
            # the same from device-resident labels and input (Filter -> Label -> Markers without leaving the GPU)
            pipe.load_input(vol)
            pipe.upload_frangi(np.where(lab > 0, 1.0, 0.0).astype(np.float32))
            pipe.label(np.float32(0.5), 1, fill_holes=False)
            if np.array_equal(pipe.download_labels() > 0, lab > 0):          # same object mask (ids do not matter)
                pipe.markers(dr, **kw)
                m2, d2, b2 = pipe.download_markers()
                assert np.array_equal(m2, g["marker"]) and np.array_equal(d2, g["distance"]) and np.array_equal(b2, g["border"])
    finally:
        pipe.close()


def test_markers_sparse_log_equals_dense_on_scattered_objects(hip, monkeypatch):
    """The tile list and the Z-march map of the sparse LoG on a volume with skipped tiles in every pass (160 x 300 x 520: 19 x 9 in-plane
    tiles, 3 Z chunks): objects in corners, on faces, across tile and chunk seams -- dense, sparse and sparse over NaN-poisoned
    scratch give the same three products."""
    from nellie_amd import pipeline as pl
    from nellie_amd.synthetic import ISO_01
    rng = np.random.default_rng(5)
    shape = (160, 300, 520)
    lab = np.zeros(shape, np.int32)
    zz, yy, xx = np.ogrid[:shape[0], :shape[1], :shape[2]]
    centres = [(0, 0, 0), (159, 299, 519), (80, 31, 255), (80, 32, 256), (63, 150, 300), (64, 150, 40), (10, 290, 500), (150, 5, 258)]
    centres += [tuple(int(rng.integers(0, s)) for s in shape) for _ in range(10)]
    for k, (cz, cy, cx) in enumerate(centres):
        r = 3 + (k % 5)
        lab[(zz - cz) ** 2 + (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = k + 1
    vol = rng.normal(100, 5, shape).astype(np.float32)
    outs = []
    for sparse, poison in (("0", "0"), ("1", "0"), ("1", "1")):
        monkeypatch.setenv("NELLIE_MK_SPARSE", sparse)
        monkeypatch.setenv("NELLIE_MK_POISON", poison)
        pipe = pl.FramePipeline(shape)
        n = pipe.markers(ISO_01, labels=lab, intensity=vol)
        outs.append((n,) + tuple(a.copy() for a in pipe.download_markers()))
        pipe.close()
    assert outs[0][0] > 0
    for o in outs[1:]:
        assert o[0] == outs[0][0]
        for a, b in zip(o[1:], outs[0][1:]):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("shape,dr", [((20, 60, 70), {"X": 0.065, "Y": 0.065, "Z": 0.25, "T": 1.0}),      # LoG radii up to 21 in-plane
                                      ((30, 9, 140), {"X": 0.1, "Y": 0.1, "Z": 0.1, "T": 1.0}),           # Y shorter than the kernel radius
                                      ((24, 50, 66), {"X": 0.05, "Y": 0.05, "Z": 0.05, "T": 1.0})])       # radii 27 on all three axes
def test_markers_any_radius_vs_oracle(hip, shape, dr):
    """Pixel sizes below 0.1 um make LoG kernels wider than the tiled in-plane kernels hold (GM_MAX_R = 12), thin images make them
    longer than an axis (scipy reflects several times): nl_markers_log_step then takes the one-thread-per-voxel passes.  Found by
    tools/fuzz_stages.py (the library used to refuse such radii).  All three products equal the oracle's."""
    from nellie_amd import pipeline as pl
    from nellie_amd.synthetic import make_volume
    vol = make_volume(shape, 77)
    lab = (vol > np.percentile(vol, 97)).astype(np.int32)
    ref = orc.markers_frame(vol, lab, dr)
    pipe = pl.FramePipeline(shape)
    try:
        n = pipe.markers(dr, labels=lab, intensity=vol)
        marker, dist, border = (a.reshape(shape) for a in pipe.download_markers())
        assert np.array_equal(dist, ref[1]) and np.array_equal(border, ref[2])
        assert np.array_equal(marker, ref[0]) and n == int(ref[0].sum()) and n > 0
    finally:
        pipe.close()


def test_stage_api_markers(hip):
    """Filter -> Label -> Markers through the drop-in stage classes; products equal the oracle's on the same labels."""
    from fakes import ArrayImInfo
    from nellie_amd.segmentation.filtering import Filter
    from nellie_amd.segmentation.labelling import Label
    from nellie_amd.segmentation.mocap_marking import Markers
    from nellie_amd.synthetic import ISO_01, make_volume
    vols = np.stack([make_volume((24, 48, 48), 50 + t) for t in range(2)])
    im_info = ArrayImInfo(vols, ISO_01)
    Filter(im_info).run()
    Label(im_info).run()
    Markers(im_info).run()
    for t in range(2):
        lab = np.asarray(im_info.store["labels"][t])
        marker, dist, border = orc.markers_frame(vols[t], lab, ISO_01)
        assert np.array_equal(np.asarray(im_info.store["distance"][t]), dist)
        assert np.array_equal(np.asarray(im_info.store["border"][t]), border)
        assert np.array_equal(np.asarray(im_info.store["marker"][t]), marker)
        assert im_info.store["marker"].dtype == np.uint8 and im_info.store["distance"].dtype == np.float32


def test_stage_api_markers_2d_and_frangi(hip):
    """Markers on a 2-D (no_z) stack and with use_im='frangi': products equal the oracle's on the same labels / Frangi."""
    from fakes import ArrayImInfo
    from nellie_amd.segmentation.filtering import Filter
    from nellie_amd.segmentation.labelling import Label
    from nellie_amd.segmentation.mocap_marking import Markers
    from nellie_amd.synthetic import ISO_01, make_image_2d, make_volume
    iso2 = {"X": 0.1, "Y": 0.1, "Z": None, "T": 1.0}
    imgs = np.stack([make_image_2d((96, 80), 60 + t) for t in range(2)])
    info2 = ArrayImInfo(imgs, iso2, no_z=True)
    Filter(info2).run(); Label(info2).run(); Markers(info2).run()
    for t in range(2):
        marker, dist, border = orc.markers_frame(imgs[t], np.asarray(info2.store["labels"][t]), iso2)
        assert np.array_equal(np.asarray(info2.store["distance"][t]), dist)
        assert np.array_equal(np.asarray(info2.store["border"][t]), border)
        assert np.array_equal(np.asarray(info2.store["marker"][t]), marker)
    vols = np.stack([make_volume((24, 48, 48), 70)])
    info3 = ArrayImInfo(vols, ISO_01)
    Filter(info3).run(); Label(info3).run(); Markers(info3, use_im="frangi").run()
    marker, dist, border = orc.markers_frame(vols[0], np.asarray(info3.store["labels"][0]), ISO_01,
                                             frangi=np.asarray(info3.store["frangi"][0]))
    assert np.array_equal(np.asarray(info3.store["marker"][0]), marker) and marker.sum() > 0
    assert np.array_equal(np.asarray(info3.store["distance"][0]), dist)
    with pytest.raises(ValueError):
        m = Markers(info3, use_im="nonsense"); m._get_t(); m._allocate_memory(); m._set_default_sigmas(); m._run_frame(0)


def test_reference_mocap_tests_on_the_hip_class(hip):
    """The reference's own tests for this stage (tests/test_mocap_marking.py:34-71) run against the HIP class: the
    `low_memory` call equals the full-frame call, and the border shell never overlaps the mask."""
    from types import SimpleNamespace
    from nellie_amd.segmentation.mocap_marking import Markers
    info = SimpleNamespace(no_t=True, no_z=True, shape=(1, 9, 9), axes="TYX", dim_res={"X": 0.2, "Y": 0.2, "Z": None, "T": 1.0})
    intensity = np.zeros((1, 9, 9), dtype=np.float32); intensity[0, 4, 4] = 10.0
    labels = np.zeros((1, 9, 9), dtype=np.uint8); labels[0, 2:7, 2:7] = 1

    def setup(**kw):
        m = Markers(info, num_t=1, **kw)
        m.im_memmap, m.label_memmap, m.shape = intensity, labels, labels.shape
        m._set_default_sigmas()
        return m

    full = setup(num_sigma=3, low_memory=False)
    low = setup(num_sigma=3, low_memory=True, max_chunk_voxels=20)
    try:
        a = full._run_frame_impl(0, low_memory=False)
        b = low._run_frame_impl(0, low_memory=True, chunk_voxels=20)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)
        g = load_golden("markers2d_reftest_9x9")                  # the reference's outputs for exactly this input
        assert np.array_equal(a[0], g["marker"]) and np.array_equal(a[1], g["distance"]) and np.array_equal(a[2], g["border"])
        mask = np.zeros((7, 7), dtype=bool); mask[2:5, 2:5] = True
        dist, border = full._distance_im(mask)
        assert border.shape == mask.shape and border.dtype == bool and not np.any(border & mask) and border.sum() == 12
        assert dist.dtype == np.float32 and dist[3, 3] == 2.0 and dist[0, 0] == 0.0
    finally:
        full.close(); low.close()


def test_label_sparse_support_equals_dense(pipes):
    """Label right after Filter reads the Frangi frame only inside the opened mask the fused epilogue left behind;
    the same frame uploaded from the host (no support known) must give the same labels -- and an entry point that
    changes the frame in between must switch the shortcut off."""
    from nellie_amd import pipeline as pl
    from nellie_amd.synthetic import ISO_01, make_volume
    shape = (40, 96, 130)
    vol = make_volume(shape, 77)
    pipe = pipes(shape)
    p = pl.FilterParams(dim_res=ISO_01)
    pipe.filter(vol, p)
    fr = pipe.download_frangi()                      # read-only: the support stays valid
    thr = pipe.frangi_threshold()
    n1 = pipe.label(thr, pl.min_area_pixels_of(ISO_01))
    lab1 = pipe.download_labels()
    pipe.upload_frangi(fr)
    n2 = pipe.label(thr, pl.min_area_pixels_of(ISO_01))
    assert n1 == n2 and n1 > 0 and np.array_equal(lab1, pipe.download_labels())
    _, ref = orc.get_labels(fr, np.float32(thr), pl.min_area_pixels_of(ISO_01))
    assert np.array_equal(lab1, ref)
    # a different frame uploaded after Filter: the stale support must not be used
    pipe.filter(vol, p)
    other = np.roll(fr, 7, axis=2)
    pipe.upload_frangi(other)
    pipe.label(thr, pl.min_area_pixels_of(ISO_01))
    _, ref2 = orc.get_labels(other, np.float32(thr), pl.min_area_pixels_of(ISO_01))
    assert np.array_equal(pipe.download_labels(), ref2)


def test_ccl_random_masks_vs_oracle(pipes):
    """Random dense masks stress the union-find far harder than Frangi output does."""
    rng = np.random.default_rng(5)
    for shape, p in (((9, 14, 13), 0.3), ((20, 33, 70), 0.5), ((16, 64, 130), 0.62), ((7, 5, 200), 0.8)):
        fr = (rng.random(shape) < p).astype(np.float32) * rng.uniform(0.5, 1.0, shape).astype(np.float32)
        pipe = pipes(shape)
        for min_area in (1, 5):
            pipe.upload_frangi(fr)
            pipe.label(np.float32(0.25), min_area)
            _, ref = orc.get_labels(fr, np.float32(0.25), min_area)
            assert np.array_equal(pipe.download_labels(), ref), (shape, p, min_area)


def test_ccl_two_level_paths_vs_oracle(pipes):
    """The union-find's two levels on the inputs that leave the common path: planes with more runs than the in-plane LDS
    array (they fall to the global pass, next to sparse planes that do not), rows wider than the LDS-staged run emission
    handles (> 30 words), and a single plane (nz = 1)."""
    rng = np.random.default_rng(11)
    cases = []
    dense = (rng.random((5, 300, 410)) < 0.5)
    dense[1] = rng.random((300, 410)) < 0.01                      # a sparse plane between planes of ~30 000 runs
    dense[3] &= rng.random((300, 410)) < 0.3
    cases.append(dense)
    cases.append(rng.random((3, 40, 2100)) < 0.4)                  # 33 words per row
    cases.append(rng.random((1, 200, 333)) < 0.55)                 # one plane
    for m in cases:
        fr = m.astype(np.float32) * rng.uniform(0.5, 1.0, m.shape).astype(np.float32)
        pipe = pipes(m.shape)
        for min_area, fill in ((1, True), (4, False)):
            pipe.upload_frangi(fr)
            pipe.ctx.label_run(np.float32(0.25), min_area, fill)
            if fill:
                _, ref = orc.get_labels(fr, np.float32(0.25), min_area)
            else:
                mk = orc._label(orc.majority3(_area_filter(orc._label(fr > 0.25, 26), min_area)), 26)
                ref = mk
            assert np.array_equal(pipe.download_labels(), ref), (m.shape, min_area, fill)


def _area_filter(lab, min_area):
    counts = np.bincount(lab.ravel())
    keep = counts >= min_area
    keep[0] = False
    return keep[lab]


def test_stage_api_filter_then_label(hip):
    """The drop-in classes behind the reference's stage API, T = 2 frames, uint16 input."""
    from fakes import ArrayImInfo
    from nellie_amd.segmentation.filtering import Filter
    from nellie_amd.segmentation.labelling import Label
    from nellie_amd.synthetic import ISO_01, make_volume
    vols = np.stack([make_volume((24, 48, 48), 30 + t, dtype=np.uint16) for t in range(2)])
    im_info = ArrayImInfo(vols, ISO_01)
    before = vols.copy()
    status = type("V", (), {"status": ""})()
    Filter(im_info, viewer=status).run()
    Label(im_info, viewer=status).run()
    assert np.array_equal(im_info.store["im"], before), "input was modified"
    assert "Frame: 2 of 2" in status.status
    for t in range(2):
        ref_fr = orc.filter_frame(vols[t], ISO_01)
        assert_frangi_close(np.asarray(im_info.store["frangi"][t]), ref_fr, f"t={t}")
        ref_lab = orc.label_frame(np.asarray(im_info.store["frangi"][t]), ISO_01)
        assert np.array_equal(np.asarray(im_info.store["labels"][t]), ref_lab)
        assert im_info.store["labels"].dtype == np.int32


def test_stage_api_filter_run_mask_false(hip):
    """Filter.run(mask=False) (filtering.py:1033 -> 841 -> 566-567) through the drop-in class: every voxel of every scale is
    eigen-solved, the product with the (all-ones) masks changes nothing, _mask_volume still applies."""
    from fakes import ArrayImInfo
    from nellie_amd.segmentation.filtering import Filter
    from nellie_amd.synthetic import ANISO_03, make_volume
    vols = np.stack([make_volume((18, 40, 52), 40 + t) for t in range(2)])
    im_info = ArrayImInfo(vols, ANISO_03)
    Filter(im_info).run(mask=False)
    for t in range(2):
        vess, masks = orc.compute_vesselness(vols[t], ANISO_03, mask=False)
        assert masks.all()
        ref_run = vess * masks
        assert float(ref_run.sum()) > 0
        ref, thr = orc.mask_volume(ref_run, return_thr=True)
        assert_masked_close(np.asarray(im_info.store["frangi"][t]), ref, ref_run, thr)


@pytest.mark.parametrize("mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("shape", [(20, 40, 40), (40, 96, 80)])
def test_nonfinite_voxels_follow_the_reference(hip, shape, mask):
    """NaN / -Inf / +Inf voxels in the input.  The reference has defined behaviour there: NaN > 0 is False, so such voxels leave the
    threshold samples; an infinite Frobenius norm is replaced by the largest finite one (filtering.py:421-426); NaN / Inf responses
    become 0 (:764-766); a +Inf that reaches a histogram makes numpy raise ValueError("... range ... is not finite"), which the
    reference lets through; with mask=False a NaN Hessian reaches LAPACK, which raises LinAlgError.  The device follows all of it:
    same support, responses within the Frangi tolerance, the same exceptions -- and it neither hangs nor leaves a NaN / Inf in the
    frame (the device chain hands such frames to the synchronous path)."""
    import warnings
    from nellie_amd import pipeline as pl
    from nellie_amd.synthetic import ISO_01, make_volume
    pipe = pl.FramePipeline(shape)
    try:
        for val, where in ((np.nan, "one"), (-np.inf, "one"), (np.nan, "plane"), (np.nan, "all"), (np.inf, "one")):
            vol = make_volume(shape, 9)
            if where == "one":
                vol[shape[0] // 2, shape[1] // 2, shape[2] // 2] = val
            elif where == "plane":
                vol[shape[0] // 2] = val
            else:
                vol[:] = val
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                if val == np.inf:
                    with pytest.raises(ValueError):
                        orc.filter_frame(vol.copy(), ISO_01, mask=mask)
                    with pytest.raises(ValueError, match="is not finite"):
                        pipe.filter(vol.copy(), pl.FilterParams(dim_res=ISO_01), mask=mask)
                    continue
                if not mask:
                    # every Hessian goes to numpy.linalg.eigvalsh then, and LAPACK gives up on one with a NaN entry: the reference's
                    # run ends in LinAlgError (pinned by the goldens nomask_nan_* / nomask_neginf_*); oracle and device raise the same
                    with pytest.raises(np.linalg.LinAlgError, match="did not converge"):
                        orc.filter_frame(vol.copy(), ISO_01, mask=False)
                    with pytest.raises(np.linalg.LinAlgError, match="did not converge"):
                        pipe.filter(vol.copy(), pl.FilterParams(dim_res=ISO_01), mask=False)
                    continue
                ref_run = orc.run_frame(vol.copy(), ISO_01, mask=mask)
                pipe.filter(vol.copy(), pl.FilterParams(dim_res=ISO_01), mask=mask)
            out = pipe.download_frangi()
            assert np.isfinite(out).all(), f"{val} {where}: the frame holds NaN / Inf"
            if float(ref_run.sum()) > 0:
                ref, thr = orc.mask_volume(ref_run, return_thr=True)
                assert_masked_close(out, ref, ref_run, thr)
            else:
                assert not out.any()
        # the context is usable afterwards
        vol = make_volume(shape, 10)
        pipe.filter(vol, pl.FilterParams(dim_res=ISO_01), mask=mask)
        assert_frangi_close(pipe.download_frangi(), orc.filter_frame(vol, ISO_01, mask=mask), "after the non-finite frames")
    finally:
        pipe.close()


def test_reference_label_tests_on_the_hip_backend(hip):
    """The reference's own two Label tests (tests/test_labelling.py:25-77), run against the drop-in."""
    from types import SimpleNamespace
    from nellie_amd.segmentation.labelling import Label
    im_info = SimpleNamespace(no_t=True, no_z=True, shape=(1, 5, 5), axes="TYX",
                              dim_res={"X": 1.0, "Y": 1.0, "Z": None, "T": 1.0})
    labeler = Label(im_info, num_t=2, device="gpu")
    original = np.zeros((5, 5), dtype=np.float32)
    original[1:4, 1:4] = 1.0
    frangi = original.copy()
    for t in range(2):
        labels = labeler._run_frame_full_volume(t, original, frangi, intensity_thresh=None, frangi_thresh=0.5)
        assert labels is not None and labels.max() == 1 and set(np.unique(labels)) <= {0, 1}
    oc, fc = original.copy(), frangi.copy()
    labels = labeler._run_frame_full_volume(0, original, frangi, intensity_thresh=0.5, frangi_thresh=0.5)
    assert labels is not None
    assert np.array_equal(original, oc) and np.array_equal(frangi, fc)
    labeler.close()


def test_eigen_frangi_known_answers(pipes):
    """Device eigen-solve + Frangi on explicit Hessians vs numpy.linalg.eigvalsh / the oracle formula."""
    rng = np.random.default_rng(11)
    m = 400000
    scales = rng.choice([1.0, 30.0, 3000.0], size=(m, 1))
    h = (rng.normal(0, 1, (m, 6)) * scales * np.array([3, 1, 1, 2, 1, 1.5])).astype(np.float32)
    h[:2000, [1, 2, 4]] = 0                       # diagonal matrices
    h[2000:4000] = np.repeat(h[2000:4000, :1], 6, axis=1) * np.array([1, 0, 0, 1, 0, 1], np.float32)  # multiples of I
    h[4000:6000, 3] = h[4000:6000, 0]; h[4000:6000, [1, 2, 4]] *= 1e-4        # near-degenerate pairs
    h[6000:6100] = 0
    H = np.stack([np.stack([h[:, 0], h[:, 1], h[:, 2]], -1), np.stack([h[:, 1], h[:, 3], h[:, 4]], -1),
                  np.stack([h[:, 2], h[:, 4], h[:, 5]], -1)], -2)
    ev = np.linalg.eigvalsh(H)
    ref = np.take_along_axis(ev, np.argsort(np.abs(ev), axis=1, kind="stable"), axis=1)
    gamma_sq = 2.0 * 40.0 ** 2
    pipe = pipes((40, 256, 256))
    for impl in (0, 1):
        out = pipe.ctx.debug_eig_frangi(h, 0.5, 0.5, gamma_sq, impl=impl)
        norm = np.abs(ref).max(axis=1, keepdims=True) + 1e-30
        rel = np.abs(out[:, :3] - ref) / norm
        exact = float(np.mean(out[:, :3] == ref))
        print(f"impl {impl}: eigenvalues bit-equal to LAPACK {exact * 100:.4f}%, max err/||A|| {rel.max():.2e}")
        assert rel.max() < 2e-7
        assert exact == 1.0           # measured: every one of the 4e5 matrices, both solvers
        v_ref = orc.frangi_response(ref.copy(), 0.5, 0.5, gamma_sq)
        tol = 1e-4 * np.abs(v_ref) + 1e-6
        ok = np.abs(out[:, 3] - v_ref) <= tol
        # a 1-ulp eigenvalue difference may flip the sign tests only at |lambda| ~ 0
        assert ok.mean() > 0.9999, ok.mean()


def test_run_on_disk_layout(hip, tmp_path):
    """nellie_amd.run.run() on files: re-saved input + im_preprocessed (float32) + im_instance_label (int32)
    under nellie_output/nellie_necessities/, reopened through the memory maps, equal to the oracle."""
    import os
    from nellie_amd.im_info.verifier import ImInfo
    from nellie_amd.run import run
    from nellie_amd.synthetic import ISO_01, make_volume
    vols = np.stack([make_volume((24, 48, 48), 40 + t) for t in range(2)])
    im_info = ImInfo(vols, dim_res=ISO_01, output_dir=str(tmp_path), name="stack")
    run(im_info, device="gpu", markers=True)
    fr_path, lab_path = im_info.pipeline_paths["im_preprocessed"], im_info.pipeline_paths["im_instance_label"]
    assert os.path.dirname(fr_path).endswith(os.path.join("nellie_output", "nellie_necessities"))
    fr = im_info.get_memmap(fr_path, read_mode="r")
    lab = im_info.get_memmap(lab_path, read_mode="r")
    assert fr.dtype == np.float32 and lab.dtype == np.int32 and fr.shape == vols.shape == lab.shape
    assert np.array_equal(im_info.get_memmap(im_info.im_path, read_mode="r"), vols), "input file was modified"
    mk = im_info.get_memmap(im_info.pipeline_paths["im_marker"], read_mode="r")
    di = im_info.get_memmap(im_info.pipeline_paths["im_distance"], read_mode="r")
    bo = im_info.get_memmap(im_info.pipeline_paths["im_border"], read_mode="r")
    assert mk.dtype == np.uint8 and di.dtype == np.float32 and bo.dtype == np.uint8 and mk.shape == vols.shape
    for t in range(2):
        assert_frangi_close(np.asarray(fr[t]), orc.filter_frame(vols[t], ISO_01), f"t={t}")
        assert np.array_equal(np.asarray(lab[t]), orc.label_frame(np.asarray(fr[t]), ISO_01))
        m, d, b = orc.markers_frame(vols[t], np.asarray(lab[t]), ISO_01)
        assert np.array_equal(np.asarray(mk[t]), m) and np.array_equal(np.asarray(di[t]), d) and np.array_equal(np.asarray(bo[t]), b)


def test_c1_ome_tiff_file_through_the_stage_api(hip, tmp_path):
    """BASELINE config 1 as SURVEY 8(d) scopes it (the sample file is absent: a generated small OME-TIFF): uint16 ZYX
    OME-TIFF on disk -> FileInfo -> ImInfo -> Filter(max_radius_um=0.375).run() -> Label().run(), i.e. a SINGLE sigma
    (sigma = [1.25] at 0.1 um), outputs reopened from the files and compared with the oracle; then the default run(file_info)
    on the same file."""
    import os
    from nellie_amd.im_info import ome_tiff
    from nellie_amd.im_info.verifier import FileInfo, ImInfo
    from nellie_amd.run import run
    from nellie_amd.segmentation.filtering import Filter
    from nellie_amd.segmentation.labelling import Label
    from nellie_amd.synthetic import ISO_01, make_volume
    vol = make_volume((24, 56, 64), 77, dtype=np.uint16)
    src = str(tmp_path / "yeast_like.ome.tif")
    ome_tiff.create(src, (1,) + vol.shape, np.uint16, ISO_01, "raw", data=vol[None])
    fi = FileInfo(src, output_dir=str(tmp_path / "out"))
    fi.find_metadata(); fi.load_metadata()
    assert fi.good_axes and fi.good_dims and fi.dim_res["Z"] == ISO_01["Z"]
    im_info = ImInfo(fi)
    assert os.path.basename(im_info.im_path).startswith("yeast_like.ome-")
    flt = Filter(im_info, max_radius_um=0.375, device="gpu")
    flt.run()
    assert [float(s) for s in flt.sigmas] == [1.25] == orc.default_sigmas(ISO_01, 0.25, 0.375)
    Label(im_info, device="gpu").run()
    fr = np.asarray(im_info.get_memmap(im_info.pipeline_paths["im_preprocessed"], read_mode="r"))[0]
    lab = np.asarray(im_info.get_memmap(im_info.pipeline_paths["im_instance_label"], read_mode="r"))[0]
    ref = orc.filter_frame(vol, ISO_01, sigmas=[1.25])
    assert (ref > 0).any()
    assert_frangi_close(fr, ref, "single sigma")
    assert np.array_equal(lab, orc.label_frame(fr, ISO_01)) and lab.max() >= 1
    assert np.array_equal(np.asarray(im_info.get_memmap(im_info.im_path, read_mode="r"))[0], vol), "input file was modified"
    # the default five-scale run(file_info) on the same source (a second output directory)
    fi2 = FileInfo(src, output_dir=str(tmp_path / "out5"))
    im2 = run(fi2, device="gpu")
    fr5 = np.asarray(im2.get_memmap(im2.pipeline_paths["im_preprocessed"], read_mode="r"))[0]
    lab5 = np.asarray(im2.get_memmap(im2.pipeline_paths["im_instance_label"], read_mode="r"))[0]
    assert_frangi_close(fr5, orc.filter_frame(vol, ISO_01), "five sigmas")
    assert np.array_equal(lab5, orc.label_frame(fr5, ISO_01))


def test_streamed_stack_equals_per_stage_run(hip, tmp_path):
    """BASELINE config 5 in miniature: a T-stack streamed with overlapped H2D / compute / D2H gives exactly the
    files the stage-by-stage run() writes (uint16 input, 5 frames)."""
    from nellie_amd.im_info.verifier import ImInfo
    from nellie_amd.run import run, run_streamed
    from nellie_amd.synthetic import ISO_01, make_volume
    vols = np.stack([make_volume((20, 40, 56), 60 + t, dtype=np.uint16) for t in range(5)])
    a = ImInfo(vols, dim_res=ISO_01, output_dir=str(tmp_path / "a"), name="s")
    b = ImInfo(vols, dim_res=ISO_01, output_dir=str(tmp_path / "b"), name="s")
    run(a, device="gpu")
    run_streamed(b)
    for key in ("im_preprocessed", "im_instance_label"):
        x = a.get_memmap(a.pipeline_paths[key], read_mode="r")
        y = b.get_memmap(b.pipeline_paths[key], read_mode="r")
        assert x.dtype == y.dtype and np.array_equal(x, y), key
    assert np.asarray(b.get_memmap(b.pipeline_paths["im_instance_label"], read_mode="r")).max() >= 1


@pytest.mark.parametrize("aniso,how", [(False, "force3"), (True, "force4"), (False, "devices00")])
def test_markers_as_z_slabs_equal_the_whole_volume(hip, aniso, how, monkeypatch):
    """Markers(...).run() with the frame cut into Z slabs (each slab computed with its halo of labels and intensities from the
    maps, nothing exchanged: nellie_amd/segmentation/mocap_marking.py) writes the three products of the whole-volume run --
    and of the oracle.  Tall enough in Z for slabs whose halos do NOT reach the far faces."""
    from fakes import ArrayImInfo
    from nellie_amd.segmentation.mocap_marking import Markers
    from nellie_amd.synthetic import ANISO_03, ISO_01, make_volume
    dr = ANISO_03 if aniso else ISO_01
    shape = (150, 40, 48) if not aniso else (96, 48, 56)
    vol = make_volume(shape, 51)
    lab = orc.label_frame(orc.filter_frame(vol, dr), dr)
    assert lab.max() >= 1
    outs = []
    for sharded in (False, True):
        im = ArrayImInfo(vol[None], dr)
        im.store["labels"] = np.ascontiguousarray(lab[None]).view(type(im.store["im"]))
        kw = {}
        if sharded and how.startswith("force"):
            monkeypatch.setenv("NELLIE_FORCE_SLABS", how[5:])
        elif sharded:
            kw["devices"] = [0, 0]
        mk = Markers(im, device="gpu", **kw)
        mk.run()
        if sharded:
            assert mk._slab_halo() < shape[0] // 2, "the test volume must be taller than two halos"
        outs.append([np.asarray(im.store[k]) for k in ("marker", "distance", "border")])
        monkeypatch.delenv("NELLIE_FORCE_SLABS", raising=False)
    for a, b, name in zip(outs[0], outs[1], ("marker", "distance", "border")):
        assert a.dtype == b.dtype and np.array_equal(a, b), f"{name}: {int((a != b).sum())} voxels differ"
    m, d, b = orc.markers_frame(vol, lab, dr)
    assert np.array_equal(outs[1][0][0], m) and np.array_equal(outs[1][1][0], d) and np.array_equal(outs[1][2][0], b) and m.sum() >= 1


def test_streamed_stack_frame_parallel_lanes(hip, tmp_path):
    """run_streamed(devices=[...]): one streamer per GPU, GPU k takes frames k, k + N, ... (here two lanes on device 0) --
    the files of the single-lane run."""
    from nellie_amd.im_info.verifier import ImInfo
    from nellie_amd.run import run_streamed
    from nellie_amd.synthetic import ISO_01, make_volume
    vols = np.stack([make_volume((20, 40, 56), 80 + t, dtype=np.uint16) for t in range(5)])
    a = ImInfo(vols, dim_res=ISO_01, output_dir=str(tmp_path / "a"), name="s")
    b = ImInfo(vols, dim_res=ISO_01, output_dir=str(tmp_path / "b"), name="s")
    run_streamed(a)
    run_streamed(b, devices=[0, 0])
    for key in ("im_preprocessed", "im_instance_label"):
        x = a.get_memmap(a.pipeline_paths[key], read_mode="r")
        y = b.get_memmap(b.pipeline_paths[key], read_mode="r")
        assert x.dtype == y.dtype and np.array_equal(x, y), key
    assert all(np.asarray(y[t]).max() >= 1 for t in range(5))


def test_remove_edges_golden(hip):
    """Filter(remove_edges=True) behind the stage API (filtering.py:931-932, 969-1000)."""
    from fakes import ArrayImInfo
    from nellie_amd.segmentation.filtering import Filter
    g = load_golden("removeedges_16x96x40_s8")
    im_info = ArrayImInfo(g["input"][None], g["dim_res_dict"])
    Filter(im_info, remove_edges=True).run()
    assert_masked_close(np.asarray(im_info.store["frangi"][0]), g["frangi"], g["run_frame"], g["percentile_thr"])


def test_remove_edges_device_vs_oracle(hip):
    """nl_remove_edges against the oracle's restatement of filtering.py:969-1000: random sparse frames (3-D, 2-D),
    spans shorter than the margin (overlapping stretches), empty planes, a single non-zero row, negative values."""
    from types import SimpleNamespace
    from nellie_amd.segmentation.filtering import Filter
    rng = np.random.default_rng(3)
    iso = {"X": 0.1, "Y": 0.1, "Z": 0.1, "T": 1.0}
    vol = np.zeros((9, 70, 45), np.float32)
    vol[0, 20:60] = (rng.random((40, 45)) < 0.2) * rng.random((40, 45))       # ordinary plane
    vol[1, 30:38, 5] = 1.0                                                   # span of 8 rows < margin: all zeroed
    vol[2, 10:35, 7] = 2.0                                                   # span of 25: the two stretches overlap
    vol[3, 33, 40] = 5.0                                                     # one row
    vol[5, 0, 0] = 1.0; vol[5, 69, 44] = 1.0                                 # first and last row
    vol[6, 12:50, 3] = -1.0                                                  # non-zero but not positive
    vol[7] = rng.random((70, 45)).astype(np.float32)                         # dense
    f3 = Filter(SimpleNamespace(no_t=True, no_z=False, shape=vol.shape, axes="ZYX", dim_res=iso, im_path="im", pipeline_paths={}),
                remove_edges=True)
    try:
        out = f3._remove_edges(vol.copy())
        assert np.array_equal(out, orc.remove_edges(vol))
        pipe = f3._get_pipeline(vol.shape)
        pipe.upload_frangi(vol)
        assert pipe.ctx.remove_edges(15) == int((orc.remove_edges(vol) > 0).sum())      # the count that gates _mask_volume
        assert f3._bbox(vol[0]) == (20, 59, int(np.flatnonzero(vol[0].any(0))[0]), int(np.flatnonzero(vol[0].any(0))[-1]))
        assert f3._bbox(np.zeros((4, 5))) == (0, 0, 0, 0) and f3._bbox(np.zeros((2, 3, 4))) == (0,) * 6
    finally:
        f3.close()
    img = vol[0].copy()
    f2 = Filter(SimpleNamespace(no_t=True, no_z=True, shape=img.shape, axes="YX", dim_res={"X": 0.1, "Y": 0.1, "Z": None, "T": 1.0},
                                im_path="im", pipeline_paths={}), remove_edges=True)
    try:
        assert np.array_equal(f2._remove_edges(img.copy()), orc.remove_edges_2d(img))
        assert np.array_equal(f2._remove_edges(vol[1].copy()), orc.remove_edges_2d(vol[1]))
    finally:
        f2.close()


@pytest.mark.parametrize("name", LABEL_INTENSITY_CASES)
def test_label_intensity_threshold_golden(name, hip):
    """Label(otsu_thresh_intensity=True) / Label(threshold=...) behind the stage API (labelling.py:511-532, 550-552)."""
    from fakes import ArrayImInfo
    from nellie_amd.segmentation.labelling import Label
    g = load_golden(name)
    im_info = ArrayImInfo(g["input"][None], g["dim_res_dict"])
    im_info.store["frangi"] = g["frangi"][None]
    kw = dict(otsu_thresh_intensity=True) if int(g["otsu"]) else dict(threshold=float(g["threshold"]))
    Label(im_info, **kw).run()
    assert np.array_equal(np.asarray(im_info.store["labels"][0]), g["labels"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", __import__("conftest").NETWORK_CASES)
def test_network_steps_golden_bitexact(name, hip):
    """Network's two dense steps against the reference's own outputs, through the mixin a maintainer would use."""
    from nellie_amd.segmentation.networking import HipNetworkKernels, pixel_class, branch_skel_labels
    g = load_golden(name)
    k = HipNetworkKernels()
    try:
        pc = k._get_pixel_class(g["skel"])
        assert pc.dtype == np.uint8 and pc.shape == g["skel"].shape and np.array_equal(pc, g["pixel_class"])
        assert k.n_skeleton_voxels == int((g["skel"] > 0).sum())
        bl = k._get_branch_skel_labels(pc)                       # device-resident classes
        assert bl.dtype == np.int32 and np.array_equal(bl, g["branch_labels"])
        assert k.n_branches == int(g["branch_labels"].max())
        bl2 = k._get_branch_skel_labels(g["pixel_class"].copy())   # classes handed over by the host (e.g. after _clean_junctions)
        assert np.array_equal(bl2, g["branch_labels"])
    finally:
        k.close()
    assert np.array_equal(pixel_class((g["skel"] > 0).astype(np.uint16)), g["pixel_class"])
    assert np.array_equal(branch_skel_labels(g["pixel_class"]), g["branch_labels"])


@pytest.mark.gpu
def test_network_steps_large_vs_oracle(hip):
    """A 96x200x330 skeleton image (rows of 6 words, ~30k skeleton voxels): both steps equal the oracle's."""
    from nellie_amd.synthetic import make_skeleton
    from nellie_amd.segmentation.networking import HipNetworkKernels
    skel = make_skeleton((96, 200, 330), 21, n_walks=400)
    k = HipNetworkKernels()
    try:
        pc = k._get_pixel_class(skel)
        ref = orc.network_pixel_class(skel)
        assert np.array_equal(pc, ref)
        assert np.array_equal(k._get_branch_skel_labels(pc), orc.network_branch_skel_labels(ref))
        with pytest.raises(RuntimeError):
            k._get_pixel_class(skel, force_cpu=True)
    finally:
        k.close()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(40, 300, 1000), (24, 200, 1024), (12, 70, 960), (20, 64, 130)])
def test_label_dense_structure_on_the_x_faces(hip, shape):
    """Dense specks, shells and blobs hugging x = 0 and x = nx-1 (rows of 15-16 mask words, with and without a partial last
    word), three runs: bit-exact against the oracle every time.  Found at 1024^3: the first majority-filter kernel gave
    nondeterministic bits in the column x = nx-1 for some volume sizes (right inputs, right source, wrong code: it passed
    when compiled for other shapes of the same test) -- the kernel was rewritten with 32-bit indexing and an explicit
    last-word clamp, and this test pins the faces."""
    from nellie_amd import pipeline as pl
    rng = np.random.default_rng(shape[2])
    fr = np.zeros(shape, np.float32)
    m = rng.random((shape[0], shape[1], 8)) < 0.25
    fr[:, :, -8:][m] = 1.0
    fr[:, :, :8][m[:, :, ::-1]] = 1.0
    zz, yy, xx = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij", sparse=True)
    for _ in range(25):
        c = [rng.uniform(0, shape[0]), rng.uniform(0, shape[1]), rng.choice([abs(rng.normal(0, 3)), shape[2] - 1 - abs(rng.normal(0, 3))])]
        r = rng.uniform(2.0, 8.0)
        d = np.sqrt((zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2)
        fr[(d < r) & (d > r - rng.uniform(1.0, 3.0))] = 1.0
    for fill, min_area in ((True, 12), (False, 1)):
        if fill:
            ref = orc.get_labels(fr, 0.5, min_area)[1]
        else:
            ref = orc.label26(orc.majority3(fr > 0.5))            # area filter off, no hole filling: the majority filter alone
        for rep in range(3):
            pipe = pl.FramePipeline(shape)
            pipe.upload_frangi(fr)
            n = pipe.label(0.5, min_area, fill_holes=fill)
            lab = pipe.download_labels()
            pipe.close()
            bad = np.argwhere(lab != ref)
            assert bad.size == 0, f"fill={fill} run {rep}: {len(bad)} voxels differ, x in {sorted(set(bad[:, 2].tolist()))[:6]}"
            assert n == int(ref.max())


# ---------------------------------------------------------------------------------------------------------------------
# Device-resident threshold chain (csrc/chain.inc, nl_chain_*): the scale loop without a host round trip
# ---------------------------------------------------------------------------------------------------------------------
def _run_both_ways(vol, dr, **kw):
    from nellie_amd import pipeline as pl
    out = []
    for chain in (True, False):
        pipe = pl.FramePipeline(vol.shape)
        pipe._device_chain = chain
        for k, v in kw.items():
            setattr(pipe, k, v)
        pipe.filter(vol, pl.FilterParams(dim_res=dr))
        tr = [(s.sigma, s.gamma, s.max_abs, s.frob_thr, s.mask_count, s.skipped) for s in pipe.trace.scales]
        out.append((pipe.download_frangi(), tr, pipe.trace.n_positive, pipe.trace.percentile_thr, pipe.chain_fallbacks,
                    getattr(pipe, "last_chain_flags", None)))
        pipe.close()
    return out


@pytest.mark.parametrize("shape,seed,aniso", [((40, 96, 96), 21, False), ((33, 70, 130), 22, True), ((64, 128, 136), 23, False),
                                              ((96, 160, 200), 24, False)])
def test_device_chain_equals_the_synchronous_path(hip, shape, seed, aniso):
    """Thresholds decided by kernels (gamma, bracket, max |H|, Frobenius threshold, mask test) and read by the walk and the
    resolve kernel from device memory: same trace, same Frangi frame as the path that takes every histogram to the host --
    and the chain stood (no flag, nothing redone), i.e. the host's repetition of the arithmetic agreed bit for bit."""
    from nellie_amd.synthetic import ANISO_03, ISO_01, make_volume
    vol = make_volume(shape, seed)
    (fr_c, tr_c, np_c, pt_c, fb_c, flags), (fr_s, tr_s, np_s, pt_s, fb_s, _) = _run_both_ways(vol, ANISO_03 if aniso else ISO_01)
    if flags is None and fb_c == 0:
        pytest.skip("the device chain is not offered in this configuration (NELLIE_HV_RS=0 / NELLIE_DEVICE_CHAIN=0)")
    assert fb_c == 0 and flags == [0] * len(tr_c), f"the chain fell back: flags {flags}"
    assert fb_s == 0
    assert tr_c == tr_s
    assert np_c == np_s and pt_c == pt_s
    assert np.array_equal(fr_c, fr_s) and (fr_c > 0).any()


@pytest.mark.parametrize("shape,seed", [((96, 80), 41), ((257, 513), 42), ((64, 1000), 43), ((700, 33), 44)])
def test_device_chain_on_images(hip, shape, seed):
    """Round 6: 2-D images (im_info.no_z; filtering.py:675-690, 732-741) go through the device-resident threshold chain too -- two passes per
    scale, no walk: the statistics kernel and the vesselness kernel read / write the scale's record.  Same trace, same frame as the synchronous
    path, and the chain stood (no flag), frame after frame on one context."""
    from nellie_amd import pipeline as pl
    from nellie_amd.synthetic import make_image_2d
    img = make_image_2d(shape, seed)
    dr = {"X": 0.1, "Y": 0.1, "Z": None, "T": 1.0}
    out = []
    for chain in (True, False):
        pipe = pl.FramePipeline(img.shape)
        assert pipe.two_d
        pipe._device_chain = chain
        assert pipe._chain_usable(pl.FilterParams(dim_res=dr), True) == chain
        for _ in range(2):
            n = pipe.filter(img, pl.FilterParams(dim_res=dr))
        tr = [(s.sigma, s.gamma, s.max_abs, s.frob_thr, s.mask_count, s.skipped) for s in pipe.trace.scales]
        out.append((pipe.download_frangi(), tr, n, pipe.chain_fallbacks, getattr(pipe, "last_chain_flags", None)))
        pipe.close()
    (fa, ta, na, fba, flags), (fb, tb, nb, _, _) = out
    assert fba == 0 and flags == [0] * len(ta), f"the chain fell back: {flags}"
    assert ta == tb and na == nb and np.array_equal(fa, fb) and (fa > 0).any()


@pytest.mark.parametrize("shape,seed,aniso", [((40, 96, 96), 21, False), ((33, 70, 130), 22, True), ((70, 150, 200), 25, False), ((9, 61, 121), 26, False),
                                              ((130, 64, 61), 27, True), ((24, 7, 300), 28, False)])
def test_wave_autonomous_walk_is_bit_identical(hip, shape, seed, aniso, monkeypatch):
    """NELLIE_HV_DPP=1 (round 6, csrc/hessian_dpp.inc; profiles/r06_walk_dpp_*.txt): the one-pass walk without LDS and without the barrier --
    strips of 4 rows x 60 columns per wave, Y neighbours in registers, X neighbours through DPP, mask words shared by two strips OR-ed in with
    atomics.  Measured equal to the pair walk at 1024^3 (the mask / queue logic bounds both), hence opt-in -- but the same bits: trace, frame,
    chain and synchronous path, on shapes whose strips stick out of the volume in X and Y, one strip wide or high, with planes that are no
    multiple of a group of four, and with a cumulative mask from the earlier scales."""
    from nellie_amd.synthetic import ANISO_03, ISO_01, make_volume
    vol = make_volume(shape, seed)
    dr = ANISO_03 if aniso else ISO_01
    monkeypatch.setenv("NELLIE_HV_DPP", "0")
    ref = _run_both_ways(vol, dr)
    monkeypatch.setenv("NELLIE_HV_DPP", "1")
    got = _run_both_ways(vol, dr)
    for (fr_a, tr_a, np_a, pt_a, _, _), (fr_b, tr_b, np_b, pt_b, fb_b, _) in zip(ref, got):
        assert tr_a == tr_b and np_a == np_b and pt_a == pt_b
        assert np.array_equal(fr_a, fr_b)
    assert (ref[0][0] > 0).any() or shape[1] < 16


@pytest.mark.parametrize("shape,seed,aniso", [((40, 96, 96), 21, False), ((33, 70, 130), 22, True), ((70, 150, 200), 25, False)])
def test_walk_with_four_voxels_per_lane_is_bit_identical(hip, shape, seed, aniso, monkeypatch):
    """NELLIE_HV_NP=2 (round 5, profiles/r05_walk_variants_1024cube.txt block 4): the pair walk with two pair-rows per lane -- measured
    26 % slower and therefore off, but the same bits: trace, frame (chain and synchronous path, which also runs the two-pass modes)."""
    from nellie_amd import pipeline as pl
    from nellie_amd.synthetic import ANISO_03, ISO_01, make_volume
    probe = pl.FramePipeline((8, 16, 64))
    try:
        built = probe.ctx.info("hv_variants")
    finally:
        probe.close()
    if not built:
        pytest.skip("the shipping library no longer carries the rejected walk variants (tools/build_variant.sh hv_all -DNL_HV_VARIANTS=1)")
    vol = make_volume(shape, seed)
    dr = ANISO_03 if aniso else ISO_01
    ref = _run_both_ways(vol, dr)
    monkeypatch.setenv("NELLIE_HV_NP", "2")
    got = _run_both_ways(vol, dr)
    for (fr_a, tr_a, np_a, pt_a, _, _), (fr_b, tr_b, np_b, pt_b, _, _) in zip(ref, got):
        assert tr_a == tr_b and np_a == np_b and pt_a == pt_b
        assert np.array_equal(fr_a, fr_b) and (fr_a > 0).any()
    two = _run_both_ways(vol, dr, one_pass=False)[1]          # statistics walk + known-threshold walk (MODE 0 / MODE 1) of the same kernel
    assert two[1] == ref[1][1] and np.array_equal(two[0], ref[1][0])


@pytest.mark.parametrize("fused", ["0", "1"])
def test_device_chain_with_the_next_cascade_step_running_ahead(hip, fused, monkeypatch):
    """Round 5: on frames below 2^26 voxels the chain enqueues the cascade step of scale s+1 on the side stream beside the
    threshold kernels and the walk of scale s (pipeline._chain_ahead).  Forced on and off, with the two-kernel and the fused
    cascade step (which may not zero the scale maximum in passing from the side stream): same trace, same frame, same labels."""
    from nellie_amd import pipeline as pl
    from nellie_amd.synthetic import ISO_01, make_volume
    monkeypatch.setenv("NELLIE_GAUSS_FUSED", fused)
    vol = make_volume((72, 136, 200), 31)
    p = pl.FilterParams(dim_res=ISO_01)
    got = []
    for ahead in ("1", "0"):
        pipe = pl.FramePipeline(vol.shape)
        pipe._chain_ahead_env = ahead
        for _ in range(2):                       # the second frame starts from the state the first one left
            pipe.filter(vol, p)
        tr = [(s.sigma, s.gamma, s.max_abs, s.frob_thr, s.mask_count, s.skipped) for s in pipe.trace.scales]
        fr = pipe.download_frangi()
        n = pipe.label(pipe.frangi_threshold(), pl.min_area_pixels_of(ISO_01))
        got.append((fr, tr, pipe.trace.n_positive, n, pipe.download_labels(), pipe.chain_fallbacks))
        pipe.close()
    (fa, ta, pa, na, la, fba), (fb, tb, pb, nb, lb, fbb) = got
    assert fba == 0 and fbb == 0
    assert ta == tb and pa == pb and na == nb
    assert np.array_equal(fa, fb) and (fa > 0).any() and np.array_equal(la, lb)


@pytest.mark.parametrize("mode", ["2"])
@pytest.mark.parametrize("ahead", ["0", "1"])
@pytest.mark.parametrize("shape,seed,aniso", [((40, 96, 96), 21, False), ((33, 70, 130), 22, True), ((96, 160, 200), 24, False)])
def test_device_chain_with_the_resolve_kernel_held_back(hip, shape, seed, aniso, ahead, mode, monkeypatch):
    """Round 5: on volumes of 2^26 voxels and more the chain starts the resolve kernel of scale s only behind the cascade step of scale
    s+1, on the side stream, beside that scale's threshold kernels (nl_chain_scale).  Forced here on small volumes (NELLIE_RESOLVE_DEFER=2),
    with and without the cascade step running ahead on the same side stream: the chain stands, same trace and frame as the synchronous path,
    frame after frame on one context."""
    from nellie_amd import pipeline as pl
    from nellie_amd.synthetic import ANISO_03, ISO_01, make_volume
    dr = ANISO_03 if aniso else ISO_01
    vol = make_volume(shape, seed)
    ref = _run_both_ways(vol, dr)[1]
    monkeypatch.setenv("NELLIE_RESOLVE_DEFER", mode)
    pipe = pl.FramePipeline(shape)
    pipe._chain_ahead_env = ahead
    for rep in range(3):
        pipe.filter(vol, pl.FilterParams(dim_res=dr))
        tr = [(s.sigma, s.gamma, s.max_abs, s.frob_thr, s.mask_count, s.skipped) for s in pipe.trace.scales]
        assert pipe.chain_fallbacks == 0 and pipe.last_chain_flags == [0] * len(tr)
        assert tr == ref[1] and pipe.trace.n_positive == ref[2] and pipe.trace.percentile_thr == ref[3]
        assert np.array_equal(pipe.download_frangi(), ref[0])
    pipe.close()


def test_cascade_steps_of_three_passes_never_run_ahead(hip):
    """A cascade step whose in-plane radius has no fused Y+X kernel (> 12) makes three passes, and the third lands in the volume the step
    started from -- the Gaussian the current scale still reads when the step runs ahead (found by the fuzz slice's explicit sigma lists,
    round 5).  The library refuses such a step ahead, the pipeline runs it in order: sigma lists with radius-13 / radius-21 steps give the
    frame the chain gives without running ahead, and the one the synchronous path gives."""
    from nellie_amd import hipnative
    from nellie_amd import pipeline as pl
    from nellie_amd.synthetic import ISO_01, make_volume
    vol = make_volume((48, 96, 120), 33)
    pipe = pl.FramePipeline(vol.shape)
    assert pipe._yx_max_r == 12
    w1, w4, w13 = pl.gaussian_weights(0.4), pl.gaussian_weights(1.3), pl.gaussian_weights(4.3)
    assert (len(w4) - 1) // 2 == 4 and (len(w13) - 1) // 2 == 13
    assert pipe._step_fits_ahead([w1, w4, w4]) and pipe._step_fits_ahead([None, w4, w4]) and pipe._step_fits_ahead([w1, w13, None])
    assert not pipe._step_fits_ahead([w1, w13, w13]) and not pipe._step_fits_ahead([w1, w4, w13])
    pipe.ctx.filter_load(vol)
    pipe.ctx.gauss_step(w1, w4, w4, z0=0, z1=vol.shape[0])
    with pytest.raises(hipnative.NellieHipError, match="cannot run ahead"):
        pipe.ctx.gauss_step(w1, w13, w13, z0=0, z1=vol.shape[0], ahead=True)
    pipe.close()
    for sig in ([0.936, 1.629, 1.638, 4.673], [2.238, 7.372]):
        p = pl.FilterParams(dim_res=ISO_01, sigmas=sig)
        got = []
        for ahead, chain in (("1", True), ("0", True), ("0", False)):
            pipe = pl.FramePipeline(vol.shape)
            pipe._chain_ahead_env = ahead
            pipe._device_chain = chain
            pipe.filter(vol, p)
            got.append((pipe.download_frangi(), [(s.gamma, s.max_abs, s.frob_thr, s.mask_count) for s in pipe.trace.scales]))
            pipe.close()
        for fr, tr in got[1:]:
            assert tr == got[0][1] and np.array_equal(fr, got[0][0])
        assert (got[0][0] > 0).any()


def test_device_chain_falls_back_on_a_bracket_miss(hip):
    """A prediction pushed off by 50 % misses the bracket: the chain flags it (NL_CF_MISS = 128), the frame is redone the
    synchronous way (which goes two-pass) and the result is the one-pass result."""
    from nellie_amd.synthetic import ISO_01, make_volume
    vol = make_volume((40, 96, 96), 21)
    (fr_c, tr_c, _, _, fb_c, flags), (fr_s, tr_s, _, _, _, _) = _run_both_ways(vol, ISO_01, _one_pass_test_scale=1.5)
    if flags is None and fb_c == 0:
        pytest.skip("the device chain is not offered in this configuration (NELLIE_HV_RS=0 / NELLIE_DEVICE_CHAIN=0)")
    assert fb_c == 1 and all(f & 128 for f in flags), flags
    assert tr_c == tr_s and np.array_equal(fr_c, fr_s)
    ref = _run_both_ways(vol, ISO_01)[0][0]
    assert np.array_equal(fr_c, ref)


@pytest.mark.parametrize("name", FILTER_CASES)
def test_device_chain_on_the_golden_cases(name, hip):
    """Every golden Filter case through the default pipeline (chain on): the frames the synchronous path gives -- including
    the cases the chain hands back (zeros, constant, single voxel, empty scales, fixed thresholds)."""
    from nellie_amd import pipeline as pl
    g = load_golden(name)
    vol, dr, kw = g["input"], g["dim_res_dict"], dict(g["kwargs"])
    frames = []
    for chain in (True, False):
        pipe = pl.FramePipeline(vol.shape)
        pipe._device_chain = chain
        try:
            pipe.filter(vol, pl.FilterParams(dim_res=dr, **kw), mask=g["run_mask"])
            frames.append((pipe.download_frangi(), [(s.gamma, s.max_abs, s.frob_thr, s.mask_count, s.skipped) for s in pipe.trace.scales]))
        except ValueError as exc:
            frames.append(("raised", str(exc)))
        pipe.close()
    if isinstance(frames[0][0], str) or isinstance(frames[1][0], str):
        assert isinstance(frames[0][0], str) and isinstance(frames[1][0], str)
    else:
        assert frames[0][1] == frames[1][1] and np.array_equal(frames[0][0], frames[1][0])


def test_positive_gather_in_two_halves_and_under_the_chain_wait(hip):
    """nl_sample_gather_positive_begin / _end give the one-call result; _end without _begin is a state error; and the frame's
    percentile threshold is the same whether its samples are compacted under the chain's wait (default) or afterwards."""
    from nellie_amd import hipnative, pipeline as pl
    from nellie_amd.synthetic import ISO_01, make_volume
    vol = make_volume((48, 112, 120), 31)
    res = []
    for tail in (True, False):
        pipe = pl.FramePipeline(vol.shape)
        pipe._tail_ok = tail
        pipe.filter(vol, pl.FilterParams(dim_res=ISO_01))
        assert pipe.chain_fallbacks == 0
        res.append((pipe.trace.percentile_thr, pipe.trace.n_positive, pipe.download_frangi()))
        if tail:
            ctx = pipe.ctx
            strides = pipe._strides(1_000_000)
            one = np.sort(ctx.sample_gather_positive(pl.FIELD_FRANGI, strides))
            ctx.sample_gather_positive_begin(pl.FIELD_FRANGI, strides)
            two = np.sort(ctx.sample_gather_positive_end())
            assert one.size > 0 and np.array_equal(one, two)
            with pytest.raises(hipnative.NellieHipError):
                ctx.sample_gather_positive_end()
        pipe.close()
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1] and np.array_equal(res[0][2], res[1][2])


def test_fused_pair_sampling_equals_two_separate_sequences(hip, tmp_path):
    """sample_minmax2 / edges2 / hist2 (one pass for the Gaussian and the Frobenius samples of a scale) against the two separate
    range + histogram sequences (NELLIE_CHAIN_UNFUSED_SAMPLING=1, read once per process: a child process), chain and synchronous."""
    import json, subprocess, sys
    code = r'''
import json, sys, zlib
import numpy as np
from nellie_amd import pipeline as pl
from nellie_amd.synthetic import ANISO_03, make_volume
vol = make_volume((40, 100, 132), 77)
out = {}
for chain in (True, False):
    pipe = pl.FramePipeline(vol.shape)
    pipe._device_chain = chain
    pipe.filter(vol, pl.FilterParams(dim_res=ANISO_03))
    tr = [(s.sigma, s.gamma, s.max_abs, s.frob_thr, s.mask_count) for s in pipe.trace.scales]
    out[str(chain)] = [tr, pipe.trace.percentile_thr, zlib.crc32(pipe.download_frangi().tobytes()), pipe.chain_fallbacks]
    pipe.close()
print(json.dumps(out))
'''
    got = []
    for unfused in ("0", "1"):
        env = dict(os.environ, NELLIE_CHAIN_UNFUSED_SAMPLING=unfused, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        got.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert got[0] == got[1]
    assert got[0]["True"][:3] == got[0]["False"][:3] and got[0]["True"][3] == 0


def test_three_forms_of_the_constant_division_agree(hip):
    """The walk divides by float32(h) / float32(2h) in one of three ways (csrc/walk_common.h: Dv<2> two instructions, Dv<1> three,
    Dv<0> through float64), the short ones only after a proof by exhaustion for the divisors in use: same Frangi frame, same
    trace, on an isotropic and an anisotropic spacing (NELLIE_EXACT_DIV is read per context, a child process per setting)."""
    import json, subprocess, sys
    code = r'''
import json, zlib
from nellie_amd import pipeline as pl
from nellie_amd.synthetic import ANISO_03, ISO_01, make_volume
out = []
for dr, seed in ((ISO_01, 5), (ANISO_03, 6), ({"X": 0.065, "Y": 0.065, "Z": 0.29, "T": 1.0}, 7)):
    vol = make_volume((40, 72, 136), seed)
    pipe = pl.FramePipeline(vol.shape)
    pipe.filter(vol, pl.FilterParams(dim_res=dr))
    tr = [(s.gamma, s.max_abs, s.frob_thr, s.mask_count) for s in pipe.trace.scales]
    out.append([int(pipe.ctx.info("fast_div")), tr, zlib.crc32(pipe.download_frangi().tobytes()), pipe.trace.n_positive])
    pipe.close()
print(json.dumps(out))
'''
    got = {}
    for setting in ("0", "3", "1"):
        env = dict(os.environ, NELLIE_EXACT_DIV=setting, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        got[setting] = json.loads(r.stdout.strip().splitlines()[-1])
    assert [g[0] for g in got["1"]] == [0, 0, 0] and all(g[0] <= 1 for g in got["3"])
    assert any(g[0] == 2 for g in got["0"]), "the two-instruction division was not selected for any of the spacings"
    for a, b, c in zip(got["0"], got["3"], got["1"]):
        assert a[1:] == b[1:] == c[1:] and a[3] > 0


def test_chain_is_skipped_where_the_pair_walk_is_unavailable(hip):
    """NELLIE_HV_RS=0 (what a plane of >= 2^30 voxels selects by itself) leaves the one-voxel walk and nl_chain_begin's
    precondition unmet: the default pipeline (chain on) must then take the synchronous path instead of raising, and give the
    frame the pair walk gives (the switch is read once per process: child processes)."""
    import json, subprocess, sys
    code = r'''
import json, zlib
from nellie_amd import pipeline as pl
from nellie_amd.synthetic import ISO_01, make_volume
vol = make_volume((40, 96, 104), 31)
pipe = pl.FramePipeline(vol.shape)
usable = pipe._chain_usable(pl.FilterParams(dim_res=ISO_01), True)
pipe.filter(vol, pl.FilterParams(dim_res=ISO_01))
tr = [(s.gamma, s.max_abs, s.frob_thr, s.mask_count) for s in pipe.trace.scales]
print(json.dumps([bool(pipe.ctx.chain_available()), bool(usable), tr, zlib.crc32(pipe.download_frangi().tobytes()), pipe.trace.n_positive]))
pipe.close()
'''
    got = {}
    for rs in ("8", "0"):
        env = dict(os.environ, NELLIE_HV_RS=rs, NELLIE_DEVICE_CHAIN="1", PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        got[rs] = json.loads(r.stdout.strip().splitlines()[-1])
    assert got["8"][:2] == [True, True] and got["0"][:2] == [False, False]
    assert got["8"][2:] == got["0"][2:] and got["8"][4] > 0


def test_every_launch_branch_of_the_walk_gives_the_same_frame(hip):
    """The walk's launch plan (csrc/walk_plan.h) has branches only switches reach on frames of test size: the forced 128-plane chunk, the
    one-voxel kernel at both tile heights (what a plane too large for one buffer resource selects by itself), its known-threshold mode in
    several launches, the wave-autonomous walk at a forced chunk.  70 x 37 x 130: two 64-plane chunks or three 32-plane ones, rows that are
    no multiple of 4, 8 or 16, columns that overhang the 64-column tile and the 60-column strip.  Per setting (cached switches: a child
    process each) the chain, the synchronous one-pass path and the two-pass path -- MODE 2, and MODE 0 + 1 -- must give the default's
    per-scale trace, Frangi frame and labels bit for bit."""
    import json, subprocess, sys
    code = r'''
import json, zlib
from nellie_amd import pipeline as pl
from nellie_amd.synthetic import ISO_01, make_volume
vol = make_volume((70, 37, 130), 91)
out = []
for chain, one_pass in ((True, True), (False, True), (False, False)):
    pipe = pl.FramePipeline(vol.shape)
    pipe._device_chain = chain
    pipe.one_pass = one_pass
    pipe.filter(vol, pl.FilterParams(dim_res=ISO_01))
    tr = [(s.gamma, s.max_abs, s.frob_thr, s.mask_count) for s in pipe.trace.scales]
    fr = pipe.download_frangi()
    pipe.label(pipe.frangi_threshold(), pl.min_area_pixels_of(ISO_01))
    lab = pipe.download_labels()
    out.append([tr, zlib.crc32(fr.tobytes()), int((fr > 0).sum()), zlib.crc32(lab.tobytes()), int(lab.max()), int(pipe.ctx.info("hessian_tile_rows"))])
    pipe.close()
print(json.dumps(out))
'''
    one_chunk = 192 * 64 * 64          # queue entries of one 64-plane chunk of this frame: its padded plane is 64 rows x 192 columns
    settings = {"default": {},
                "zchunk128": {"NELLIE_HV_ZCHUNK": "128"},
                "one_voxel": {"NELLIE_HV_RS": "0"},
                "one_voxel_ty16": {"NELLIE_HV_RS": "0", "NELLIE_HM_TY": "16"},
                "one_voxel_launches": {"NELLIE_HV_RS": "0", "NELLIE_VQ_CAP": str(one_chunk)},
                "dpp_zchunk64": {"NELLIE_HV_DPP": "1", "NELLIE_HV_ZCHUNK": "64"}}
    switches = ("NELLIE_HV_RS", "NELLIE_HV_NP", "NELLIE_HV_DPP", "NELLIE_HM_TY", "NELLIE_HV_ZCHUNK", "NELLIE_VQ_CAP", "NELLIE_SPEC_MAX_GB")
    got = {}
    for name, sw in settings.items():
        env = {k: v for k, v in os.environ.items() if k not in switches}
        env.update(sw, PYTHONPATH=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, f"{name}: {r.stderr[-2000:]}"
        got[name] = json.loads(r.stdout.strip().splitlines()[-1])
    ref = got["default"]
    assert all(way[2] > 0 and way[4] > 0 for way in ref), "the default run gave an empty frame"
    assert [way[5] for way in ref] == [16] * 3 and [way[5] for way in got["one_voxel"]] == [8] * 3 and [way[5] for way in got["one_voxel_ty16"]] == [16] * 3
    for name, ways in got.items():
        for way, ref_way, how in zip(ways, ref, ("chain", "one pass", "two passes")):
            assert way[:5] == ref_way[:5], f"{name}, {how}: differs from the default run"


def test_device_percentile_equals_numpy(hip):
    """The radix select of csrc/percentile.inc (three levels, both order statistics at once, numpy's float32 'linear'
    interpolation on the device) against np.percentile itself -- filtering.py:963 takes the 1st percentile; other q, tiny arrays,
    ties and values spread over many binades are covered too."""
    from nellie_amd import pipeline as pl
    rng = np.random.default_rng(99)
    pipe = pl.FramePipeline((16, 256, 256))
    try:
        cases = []
        for n in (1, 2, 3, 7, 100, 101, 4097, 65536, 830584):
            cases.append((rng.random(n, dtype=np.float32) * np.float32(1e-3) + np.float32(1e-9)).astype(np.float32))
        cases.append(np.exp(rng.normal(0, 8, 50000)).astype(np.float32))                    # many binades
        cases.append(np.repeat(np.float32([0.25, 0.5, 0.75]), 3333))                        # ties
        cases.append(np.full(1000, np.float32(3.0e-5)))                                     # all equal
        cases.append(np.float32([1e-38, 1e-38, 3.4e38, 1.0]))                               # extremes
        for v in cases:
            for q in (1, 50, 99, 100, 0):
                want = np.percentile(v, q)
                thr, a, b = pipe.ctx.debug_percentile(v, q)
                assert type(want) is np.float32 and thr == want, (v.size, q, thr, want, a, b)
    finally:
        pipe.close()


def test_device_tail_equals_the_host_epilogue(hip):
    """filter() with the epilogue enqueued on the device (nl_tail_enqueue: percentile selected by kernels, threshold read from
    device memory) against the round-3 epilogue (samples to the host, np.partition there): same threshold, same count, same frame,
    with the chain and on the synchronous path."""
    from nellie_amd import pipeline as pl
    from nellie_amd.synthetic import ANISO_03, ISO_01, make_volume
    for shape, seed, dr in (((40, 96, 104), 41, ISO_01), ((33, 70, 130), 42, ANISO_03), ((64, 128, 136), 43, ISO_01)):
        vol = make_volume(shape, seed)
        res = []
        for chain in (True, False):
            for dev in (True, False):
                pipe = pl.FramePipeline(shape)
                pipe._device_chain, pipe._device_tail = chain, dev
                assert pipe._device_tail_usable() == dev
                pipe.filter(vol, pl.FilterParams(dim_res=dr))
                res.append((pipe.trace.percentile_thr, pipe.trace.n_positive, zlib.crc32(pipe.download_frangi().tobytes())))
                pipe.close()
        assert all(r == res[0] for r in res), res
        assert res[0][1] > 0
