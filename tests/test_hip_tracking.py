"""GPU tests of Hu-moment tracking (nellie_amd.tracking.hu_tracking.HuMomentTracking, csrc/track.inc): the reference's goldens end
to end, the device features against them, the dense float16 costs against the numpy restatement given the device's own
features, a fixed-seed fuzz slice, determinism, and one file-level run through run(markers=True, tracking=True).  Beyond the
goldens: a sweep of ROI radii up to the tile limit and its rejection above it, frames above 4096 * 1024 voxels, a long stack whose
marker buffers grow and shrink, and float32 intensities on a background offset."""
import glob
import os
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN_DIR
import hu_tracking_restatement as rs

pytestmark = pytest.mark.gpu
GOLDENS = sorted(glob.glob(os.path.join(GOLDEN_DIR, "tracking", "tracking_*.npz")))


@pytest.fixture(scope="module")
def hip():
    from nellie_amd import build, hipnative
    build.build(verbose=False)
    lib = hipnative.load()
    assert lib.device_count() > 0, "no HIP device"
    return lib


def im_double(tmp_path, intensity, frangi, distance, marker, spacing, dt):
    two_d = intensity.ndim == 3
    axes = "TYX" if two_d else "TZYX"
    arrays = {"im": intensity, "fr": frangi, "mk": marker, "dist": distance}
    dim_res = dict(zip(axes[1:], (float(s) for s in spacing)))
    dim_res["T"] = float(dt)
    paths = {"im_preprocessed": "fr", "im_marker": "mk", "im_distance": "dist",
             "flow_vector_array": str(tmp_path / f"flow_{len(os.listdir(tmp_path))}.npy")}
    return SimpleNamespace(no_t=False, no_z=two_d, shape=intensity.shape, axes=axes, dim_res=dim_res, pipeline_paths=paths,
                           im_path="im", get_memmap=lambda p: arrays[p])


def run_stage(tmp_path, stack, spacing, dt, mode, max_dense_pairs=int(1e7), max_distance_um=1.0):
    from nellie_amd.tracking.hu_tracking import HuMomentTracking
    im = im_double(tmp_path, *stack, spacing, dt)
    HuMomentTracking(im, mode=mode, max_dense_pairs=max_dense_pairs, max_distance_um=max_distance_um).run()
    return np.load(im.pipeline_paths["flow_vector_array"])


def device_features(stack, spacing):
    from nellie_amd import hipnative
    out = []
    with hipnative.Tracker(stack[0].shape[1:], spacing) as trk:
        for t in range(stack[0].shape[0]):
            trk.frame(*(a[t] for a in stack))
            c, s, h = trk.features(0)
            out.append((c, c * np.asarray(spacing, float), s, h))
    return out


def assert_flow(flow, want, exact_cost, cost_tol=None):
    """index columns exact; costs exact, within cost_tol, or within 4 float32 ulp (the float64 statistics of the sparse
    matcher are sums in another order than numpy's)"""
    assert flow.shape == want.shape, (flow.shape, want.shape)
    assert np.array_equal(flow[:, :-1], want[:, :-1])
    c, w = flow[:, -1].astype(np.float32), want[:, -1].astype(np.float32)
    if exact_cost:
        assert np.array_equal(c, w)
    elif cost_tol is not None:
        assert np.all(np.abs(c - w) <= cost_tol * np.maximum(1.0, np.abs(w))), np.abs(c - w).max()
    else:
        assert np.all(np.abs(c - w) <= 4 * np.spacing(np.abs(w))), (np.abs(c - w) / np.spacing(np.abs(w))).max()


def golden(path):
    z = np.load(path)
    stack = (z["intensity"], z["frangi"], z["distance"], z["marker"])
    return z, stack


@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(p)[:-4] for p in GOLDENS])
def test_golden_end_to_end(hip, tmp_path, path):
    z, stack = golden(path)
    mode = str(z["mode"])
    flow = run_stage(tmp_path, stack, z["spacing"], z["dt"], mode, int(z["max_dense_pairs"]))
    # dense pairs: float16 costs with a margin -> exact; sparse pairs: the same pairs, float64 costs from features that
    # differ from the reference's in the last bits (its float32 log10 of the Frangi values is numpy's host routine; DESIGN.md
    # "Tracking") -> 1e-5
    dense_only = mode == "dense" or (mode == "auto" and int(z["max_dense_pairs"]) >= 10 ** 6)
    assert_flow(flow, z["flow"], exact_cost=dense_only, cost_tol=None if dense_only else 1e-5)
    # the other two modes against the restatement on the device's own features
    feats = device_features(stack, z["spacing"])
    frames = [(z["intensity"][t],) for t in range(z["intensity"].shape[0])]
    for m in ("dense", "sparse"):
        f = run_stage(tmp_path, stack, z["spacing"], z["dt"], m)
        want = rs.track(frames, z["spacing"], dt=float(z["dt"]), mode=m, features=feats)
        assert_flow(f, want, exact_cost=m == "dense")


@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(p)[:-4] for p in GOLDENS])
def test_features_against_golden(hip, path):
    z, stack = golden(path)
    off = np.concatenate([[0], np.cumsum(z["counts"])])
    for t, (c, _, s, h) in enumerate(device_features(stack, z["spacing"])):
        a, b = off[t], off[t + 1]
        assert np.array_equal(c, z["coords"][a:b])
        # intensity stats exact for every dtype (float32: numpy's summation order); the Frangi columns within 1e-5, as the
        # golden's Frangi values went through the capture host's float32 log10 (DESIGN.md "Tracking")
        assert np.array_equal(s[:, :2], z["stats"][a:b, :2])
        assert np.allclose(s, z["stats"][a:b], rtol=1e-5, atol=0)
        d = np.abs(h - z["hu"][a:b])
        assert np.all((d <= 1e-5 * np.abs(z["hu"][a:b])) | (d <= 1e-6))


def random_stack(rng, shape, T, dtype, density):
    n = int(np.prod(shape))
    out = []
    for t in range(T):
        if dtype == np.float32:
            im = (rng.gamma(2.0, 300.0, shape) - 100.0).astype(np.float32)
        elif dtype == np.uint8:
            im = rng.integers(0, 256, shape).astype(np.uint8)
        else:
            im = rng.integers(0, int(rng.choice([5000, 65536])), shape).astype(np.uint16)
        im[rng.random(shape) < 0.1] = 0
        fr = (rng.gamma(1.5, 2.0, shape) * (rng.random(shape) < 0.7)).astype(np.float32)
        dist = np.sqrt(rng.integers(0, 12, shape)).astype(np.float32)
        mk = (rng.random(shape) < density).astype(np.uint8)
        out.append((im, fr, dist, mk))
    return tuple(np.stack([o[k] for o in out]) for k in range(4))


FUZZ = []
_r = np.random.default_rng(2024)
for _k in range(30):
    _two_d = _k % 4 == 3
    _shape = (int(_r.choice([31, 48, 61, 97])), int(_r.choice([29, 53, 64, 101]))) if _two_d else \
        (int(_r.choice([1, 2, 5, 7, 13])), int(_r.choice([17, 23, 40])), int(_r.choice([19, 31, 44])))
    FUZZ.append(dict(seed=_k, shape=_shape, dtype=[np.uint8, np.uint16, np.float32][_k % 3],
                     spacing=(0.1, 0.1) if _two_d else (float(_r.choice([0.1, 0.2, 0.35])), 0.1, 0.1),
                     maxd=float(_r.choice([0.3, 0.8, 1.5])), density=float(_r.choice([0.002, 0.01, 0.03])),
                     max_dense_pairs=int(_r.choice([int(1e7), 2000])), mode=["auto", "dense", "sparse"][_k % 3 if _k % 5 else 0]))


@pytest.mark.parametrize("case", FUZZ, ids=[f"fuzz{c['seed']}" for c in FUZZ])
def test_fuzz_against_restatement(hip, tmp_path, case):
    rng = np.random.default_rng(case["seed"])
    stack = random_stack(rng, case["shape"], 3, case["dtype"], case["density"])
    feats = device_features(stack, case["spacing"])
    for t, (c, p, s, h) in enumerate(feats):
        rc, _, rst, rh = rs.frame_features(*(a[t] for a in stack), case["spacing"])
        assert np.array_equal(c, rc)
        assert np.array_equal(s[:, :2], rst[:, :2])                # Frangi columns: the host's float32 log10, as above
        assert np.allclose(s, rst, rtol=1e-5, atol=1e-30)
        d = np.abs(h - rh)
        assert np.all((d <= 1e-5 * np.abs(rh)) | (d <= 1e-6))
    flow = run_stage(tmp_path, stack, case["spacing"], 1.0, case["mode"], case["max_dense_pairs"], case["maxd"])
    frames = [(stack[0][t],) for t in range(3)]
    want = rs.track(frames, case["spacing"], dt=1.0, max_distance_um=case["maxd"], mode=case["mode"],
                    max_dense_pairs=case["max_dense_pairs"], features=feats)
    n_markers = sum(len(f[0]) for f in feats)
    if flow.shape == want.shape:
        bad = int(np.sum(np.any(flow[:, :-1] != want[:, :-1], axis=1)))
        c, w = flow[:, -1].astype(np.float32), want[:, -1].astype(np.float32)
        bad += int(np.sum(np.abs(c - w) > np.spacing(np.abs(w))))
    else:
        bad = abs(len(flow) - len(want)) + 1
    print(f"fuzz {case['seed']}: {n_markers} markers, {len(want)} rows, {bad} differing")
    # the device's float64 z-score statistics are sums in another order than numpy's: a z-score that lands on a float16
    # rounding boundary can move one half ulp and flip a near tie (DESIGN.md "Tracking").  Measured: 2 rows in the 30 cases.
    assert bad <= max(2, 2 * n_markers // 10000), bad


def test_dense_costs_against_restatement(hip):
    """float16 costs and row / column minima of the device equal the restatement's bit for bit, given the device's features"""
    from nellie_amd import hipnative
    for seed, (shape, dtype, spacing) in enumerate([((9, 30, 33), np.uint16, (0.2, 0.1, 0.1)), ((64, 70), np.float32, (0.1, 0.1)),
                                                   ((6, 40, 41), np.uint8, (0.1, 0.1, 0.1))]):
        rng = np.random.default_rng(100 + seed)
        stack = random_stack(rng, shape, 2, dtype, 0.02)
        with hipnative.Tracker(shape, spacing) as trk:
            for t in range(2):
                trk.frame(*(a[t] for a in stack))
            post, pre = trk.features(0), trk.features(1)
            ri, rc, ci, cc, full = trk.match("dense", 1.0, full=True)
        P = [(c, c * np.asarray(spacing, float), s, h) for c, s, h in (post, pre)]
        want = rs.dense_costs(P[0][1], P[1][1], P[0][2], P[1][2], P[0][3], P[1][3], 1.0)
        assert np.array_equal(full.view(np.uint16), want.view(np.uint16))
        wri, wrv, wci, wcv = rs.best_of(want)
        assert np.array_equal(ri, wri) and np.array_equal(ci, wci)
        assert np.array_equal(rc, wrv) and np.array_equal(cc, wcv)


def test_deterministic(hip, tmp_path):
    rng = np.random.default_rng(77)
    stack = random_stack(rng, (12, 60, 64), 3, np.float32, 0.01)
    a = run_stage(tmp_path, stack, (0.2, 0.1, 0.1), 1.0, "dense")
    b = run_stage(tmp_path, stack, (0.2, 0.1, 0.1), 1.0, "dense")
    c = run_stage(tmp_path, stack, (0.2, 0.1, 0.1), 1.0, "sparse")
    d = run_stage(tmp_path, stack, (0.2, 0.1, 0.1), 1.0, "sparse")
    assert len(a) > 0 and a.tobytes() == b.tobytes() and c.tobytes() == d.tobytes()


def test_run_markers_and_tracking_on_files(hip, tmp_path):
    from nellie_amd.im_info.verifier import ImInfo
    from nellie_amd.run import run
    from nellie_amd.synthetic import ISO_01, make_volume
    vols = np.stack([make_volume((24, 48, 48), 60 + t) for t in range(3)])
    im_info = ImInfo(vols, dim_res=ISO_01, output_dir=str(tmp_path), name="trk")
    run(im_info, device="gpu", markers=True, tracking=True)
    flow = np.load(im_info.pipeline_paths["flow_vector_array"])
    get = lambda k: np.asarray(im_info.get_memmap(im_info.pipeline_paths[k], read_mode="r"))   # noqa: E731
    im, fr, mk, di = np.asarray(im_info.get_memmap(im_info.im_path, read_mode="r")), get("im_preprocessed"), get("im_marker"), \
        get("im_distance")
    sp = (im_info.dim_res["Z"], im_info.dim_res["Y"], im_info.dim_res["X"])
    feats = device_features((im, fr, di, mk), sp)
    dt = im_info.dim_res.get("T") or 1.0
    want = rs.track([(im[t],) for t in range(3)], sp, dt=dt, features=feats)
    assert flow.shape[1] == 8 and mk.any()
    assert_flow(flow, want, exact_cost=True)


# ---------------------------------------------------------------------------------------------------------------------------
# Radii, frame sizes and stack lengths beyond the goldens.  The Frangi inputs of these tests keep only values whose float32
# log10 on this host equals the correctly rounded one the device computes, so that all four stats columns compare bit for bit.

def exact_log_frangi(rng, shape):
    fr = (rng.gamma(1.5, 2.0, shape) * (rng.random(shape) < 0.7)).astype(np.float32)
    with np.errstate(divide="ignore"):
        ok = np.log10(fr) == np.log10(fr.astype(np.float64)).astype(np.float32)
    fr[~ok] = 0
    return fr


def intensity(rng, shape, kind):
    if kind == "u8":
        im = rng.integers(0, 256, shape).astype(np.uint8)
    elif kind == "u16":
        im = rng.integers(0, 5000, shape).astype(np.uint16)
    elif kind == "u16_bright":
        im = rng.integers(40000, 65536, shape).astype(np.uint16)
    elif kind == "f32_gamma":
        im = (rng.gamma(2.0, 300.0, shape) - 100.0).astype(np.float32)
    else:                                                          # "f32_low": a camera offset, 1000 +- 10
        im = rng.uniform(990.0, 1010.0, shape).astype(np.float32)
    im[rng.random(shape) < 0.15] = 0
    return im


def edge_markers(rng, shape, n_random):
    """every corner, the centre of every face and n_random voxels"""
    mk = np.zeros(shape, np.uint8)
    for corner in np.ndindex(*(2,) * len(shape)):
        mk[tuple(c * (s - 1) for c, s in zip(corner, shape))] = 1
    for ax in range(len(shape)):
        for end in (0, shape[ax] - 1):
            p = [s // 2 for s in shape]
            p[ax] = end
            mk[tuple(p)] = 1
    mk.flat[rng.choice(mk.size, n_random, replace=False)] = 1
    return mk


def assert_features(dev, want):
    c, s, h = dev
    rc, _, rst, rh = want
    assert np.array_equal(c, rc)
    assert np.array_equal(s, rst), (np.argwhere(s != rst)[:5], s[s != rst][:5], rst[s != rst][:5])
    d = np.abs(h - rh)
    assert np.all((d <= 1e-5 * np.abs(rh)) | (d <= 1e-6))


KINDS = ["u8", "u16", "u16_bright", "f32_gamma", "f32_low"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rmax", [8, 20, 40, 62])
@pytest.mark.parametrize("ndim", [2, 3])
def test_radius_sweep(hip, ndim, rmax, kind):
    """ROI tiles R = 17 .. 125 (the strided tile loops' second passes, several 8192-item blocks of the float sums), markers
    on every corner and face: coordinates exact, all four stats columns bit-exact, log-Hu within the golden bound"""
    from nellie_amd import hipnative
    rng = np.random.default_rng(1000 * ndim + 10 * rmax + KINDS.index(kind))
    shape = (150, 160) if ndim == 2 else (30, 60, 64)
    spacing = (0.1,) * ndim
    mk = edge_markers(rng, shape, 10 if ndim == 3 else 16)
    dist = np.sqrt(rng.integers(0, 4, shape)).astype(np.float32)
    pts = np.argwhere(mk)
    dist[tuple(pts.T)] = rng.uniform(0.0, rmax / 2.0, len(pts)).astype(np.float32)
    dist[tuple(pts[len(pts) // 2])] = np.float32(rmax / 2.0 - 0.05)      # ceil(2 * d) = rmax
    im, fr = intensity(rng, shape, kind), exact_log_frangi(rng, shape)
    want = rs.frame_features(im, fr, dist, mk, spacing)
    R = int(np.ceil((rs._max3(dist) * np.float32(2))[mk > 0].max())) * 2 + 1
    assert R == 2 * rmax + 1
    with hipnative.Tracker(shape, spacing) as trk:
        trk.frame(im, fr, dist, mk)
        assert_features(trk.features(0), want)


@pytest.mark.parametrize("ndim", [2, 3])
def test_radius_above_tile_raises(hip, tmp_path, ndim):
    """a distance that gives radius 63 (R = 127 > 125) is refused with the radius named, and no flow file is written"""
    from nellie_amd.tracking.hu_tracking import HuMomentTracking
    rng = np.random.default_rng(63 + ndim)
    shape = (40, 44) if ndim == 2 else (6, 20, 22)
    stack = random_stack(rng, shape, 2, np.uint16, 0.02)
    stack[2][0][stack[3][0] > 0] = 31.4                                 # ceil(2 * 31.4) = 63 at the first frame's markers
    im = im_double(tmp_path, *stack, (0.1,) * ndim, 1.0)
    with pytest.raises(ValueError, match="radius 63"):
        HuMomentTracking(im).run()
    assert not os.path.exists(im.pipeline_paths["flow_vector_array"])


def large_frame(rng, shape, n_random):
    n = int(np.prod(shape))
    nblk = (n + 4095) // 4096
    seg = (nblk + 1023) // 1024                                          # chunks per lane of the one-workgroup scan
    assert seg >= 2
    flat = {0, n - 1}
    for k in (1, 2, nblk // 2, nblk - 1):
        flat |= {k * 4096 - 1, k * 4096}
    for t in (1, 2, 511, 512, (nblk - 1) // seg):
        flat |= {t * seg * 4096 - 1, t * seg * 4096}
    flat = np.array(sorted(f for f in flat if 0 <= f < n))
    mk = np.zeros(shape, np.uint8)
    mk.flat[flat] = 1
    mk.flat[rng.choice(n, n_random, replace=False)] = 1
    im = (rng.gamma(2.0, 300.0, shape) - 100.0).astype(np.float32)
    fr = exact_log_frangi(rng, shape)
    dist = np.sqrt(rng.integers(0, 8, shape)).astype(np.float32)
    return im, fr, dist, mk


def bad_rows(flow, want):
    if flow.shape != want.shape:
        return abs(len(flow) - len(want)) + 1
    bad = int(np.sum(np.any(flow[:, :-1] != want[:, :-1], axis=1)))
    c, w = flow[:, -1].astype(np.float32), want[:, -1].astype(np.float32)
    return bad + int(np.sum(np.abs(c - w) > np.spacing(np.abs(w))))


@pytest.mark.parametrize("shape", [(40, 320, 340), (2100, 2100)], ids=["3d_4.35M", "2d_4.41M"])
def test_large_frames(hip, tmp_path, shape):
    """frames above 4096 * 1024 voxels (the scan's multi-chunk lanes): markers at the first and last voxel, at chunk and scan
    segment boundaries and ~2000 random ones; coordinates equal np.argwhere, features and matching equal the restatement
    (sparse at the full count, dense against a frame of 200 markers, where the restatement's pair cube fits)"""
    rng = np.random.default_rng(len(shape))
    spacing = (0.1,) * len(shape)
    f0 = large_frame(rng, shape, 200)
    f1 = large_frame(rng, shape, 2000)
    stack = tuple(np.stack([a, b]) for a, b in zip(f0, f1))
    feats = device_features(stack, spacing)
    for t in range(2):
        assert np.array_equal(feats[t][0], np.argwhere(stack[3][t]))
        assert_features((feats[t][0], feats[t][2], feats[t][3]), rs.frame_features(*(a[t] for a in stack), spacing))
    frames = [(stack[0][t],) for t in range(2)]
    n_markers = sum(len(f[0]) for f in feats)
    for mode in ("sparse", "dense"):
        flow = run_stage(tmp_path, stack, spacing, 1.0, mode)
        want = rs.track(frames, spacing, mode=mode, features=feats)
        bad = bad_rows(flow, want)
        print(f"large {shape} {mode}: {n_markers} markers, {len(want)} rows, {bad} differing")
        assert len(want) > 0 and bad <= max(2, 2 * n_markers // 10000), bad


def test_long_stack_buffers(hip, tmp_path):
    """T = 6 with marker counts [300, 2500, 0, 40, 3000, 3000]: the tracker's marker, partial-sum and result buffers grow,
    shrink and regrow.  Every frame's features equal the restatement; every pair's dense (where the restatement's pair cube
    fits) and sparse matches too; auto switches to sparse exactly above n_post * n_pre == max_dense_pairs."""
    counts = [300, 2500, 0, 40, 3000, 3000]
    rng = np.random.default_rng(6)
    shape, spacing = (16, 90, 96), (0.2, 0.1, 0.1)
    frames = []
    for n in counts:
        mk = np.zeros(shape, np.uint8)
        mk.flat[rng.choice(mk.size, n, replace=False)] = 1
        frames.append((intensity(rng, shape, "f32_low"), exact_log_frangi(rng, shape),
                       np.sqrt(rng.integers(0, 8, shape)).astype(np.float32), mk))
    stack = tuple(np.stack([f[k] for f in frames]) for k in range(4))
    feats = device_features(stack, spacing)
    for t, n in enumerate(counts):
        assert len(feats[t][0]) == n
        assert_features((feats[t][0], feats[t][2], feats[t][3]), rs.frame_features(*frames[t], spacing))
    im_frames = [(stack[0][t],) for t in range(len(counts))]
    for mode in ("sparse", "dense"):
        flow = run_stage(tmp_path, stack, spacing, 1.0, mode)
        # the restatement's dense matcher holds (n_post, n_pre, 23) float64 arrays: the 3000 x 3000 pair is left out of the
        # dense comparison (its rows are dropped on both sides) and compared in sparse mode only
        want = rs.track(im_frames, spacing, mode="auto" if mode == "dense" else "sparse", max_dense_pairs=int(1e6),
                        features=feats)
        if mode == "dense":
            big = [t for t in range(1, len(counts)) if counts[t] * counts[t - 1] > int(1e6)]
            flow = flow[~np.isin(flow[:, 0], [t - 1 for t in big])]
            want = want[~np.isin(want[:, 0], [t - 1 for t in big])]
        bad = bad_rows(flow, want)
        print(f"long stack {mode}: {len(want)} rows, {bad} differing")
        assert len(want) > 0 and bad <= max(2, 2 * sum(counts) // 10000), bad
    # auto at the switch: frames 0 and 1 (300 x 2500 pairs)
    two = tuple(a[:2] for a in stack)
    P = counts[0] * counts[1]
    dense, sparse = run_stage(tmp_path, two, spacing, 1.0, "dense"), run_stage(tmp_path, two, spacing, 1.0, "sparse")
    assert dense.tobytes() != sparse.tobytes()
    assert run_stage(tmp_path, two, spacing, 1.0, "auto", max_dense_pairs=P).tobytes() == dense.tobytes()
    assert run_stage(tmp_path, two, spacing, 1.0, "auto", max_dense_pairs=P - 1).tobytes() == sparse.tobytes()


def offset_stack(rng, shape, T, density):
    out = []
    for t in range(T):
        im = (rng.uniform(-10.0, 10.0, shape) + rng.choice([100.0, 1000.0, 4000.0])).astype(np.float32)
        im[rng.random(shape) < 0.1] = 0
        out.append((im, exact_log_frangi(rng, shape), np.sqrt(rng.integers(0, 12, shape)).astype(np.float32),
                    (rng.random(shape) < density).astype(np.uint8)))
    return tuple(np.stack([o[k] for o in out]) for k in range(4))


FUZZ_OFFSET = []
_r = np.random.default_rng(4048)
for _k in range(8):
    _two_d = _k % 4 == 3
    _shape = (int(_r.choice([48, 61, 97])), int(_r.choice([53, 64, 101]))) if _two_d else \
        (int(_r.choice([2, 5, 7, 13])), int(_r.choice([23, 40])), int(_r.choice([31, 44])))
    FUZZ_OFFSET.append(dict(seed=500 + _k, shape=_shape, spacing=(0.1, 0.1) if _two_d else (float(_r.choice([0.1, 0.2])), 0.1, 0.1),
                            maxd=float(_r.choice([0.8, 1.5])), density=float(_r.choice([0.01, 0.03])),
                            mode=["auto", "dense", "sparse"][_k % 3]))


@pytest.mark.parametrize("case", FUZZ_OFFSET, ids=[f"offset{c['seed']}" for c in FUZZ_OFFSET])
def test_fuzz_offset_against_restatement(hip, tmp_path, case):
    """float32 intensities on a background offset (100, 1000 or 4000 +- 10): stats bit-exact, flows within the fuzz bound"""
    rng = np.random.default_rng(case["seed"])
    stack = offset_stack(rng, case["shape"], 3, case["density"])
    feats = device_features(stack, case["spacing"])
    for t, (c, p, s, h) in enumerate(feats):
        assert_features((c, s, h), rs.frame_features(*(a[t] for a in stack), case["spacing"]))
    flow = run_stage(tmp_path, stack, case["spacing"], 1.0, case["mode"], max_distance_um=case["maxd"])
    want = rs.track([(stack[0][t],) for t in range(3)], case["spacing"], max_distance_um=case["maxd"], mode=case["mode"],
                    features=feats)
    n_markers = sum(len(f[0]) for f in feats)
    bad = bad_rows(flow, want)
    print(f"offset fuzz {case['seed']}: {n_markers} markers, {len(want)} rows, {bad} differing")
    assert bad <= max(2, 2 * n_markers // 10000), bad
