"""CPU tests of Hu-moment tracking: the numpy restatement against the reference's goldens (tests/golden/tracking_*.npz), the
float16 helpers the device matcher uses against numpy, and the stage's behaviour where no GPU is needed."""
import glob
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN_DIR
import hu_tracking_restatement as rs

GOLDENS = sorted(glob.glob(os.path.join(GOLDEN_DIR, "tracking", "tracking_*.npz")))


def load_golden(path):
    z = np.load(path)
    off = np.concatenate([[0], np.cumsum(z["counts"])])
    T = z["intensity"].shape[0]
    ref = [(z["coords"][off[t]:off[t + 1]], z["stats"][off[t]:off[t + 1]], z["hu"][off[t]:off[t + 1]]) for t in range(T)]
    return z, ref


def hu_close(a, b):
    return np.all((np.abs(a - b) <= 1e-5 * np.abs(b)) | (np.abs(a - b) <= 1e-6))


def test_goldens_cover_the_cases():
    names = {os.path.basename(p) for p in GOLDENS}
    assert len(names) >= 8
    kinds = [np.load(p) for p in GOLDENS]
    assert {z["intensity"].ndim for z in kinds} == {3, 4}                        # 2-D and 3-D stacks
    assert {z["intensity"].dtype for z in kinds} >= {np.dtype(np.uint16), np.dtype(np.float32), np.dtype(np.uint8)}
    assert {str(z["mode"]) for z in kinds} == {"auto", "dense", "sparse"}
    assert any(z["counts"][0] == 0 for z in kinds) and any(0 in z["counts"][1:-1] for z in kinds)
    assert any(float(z["dt"]) != 1.0 for z in kinds)
    assert all(os.path.getsize(p) < 300_000 for p in GOLDENS)


@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(p)[:-4] for p in GOLDENS])
def test_restatement_reproduces_golden(path):
    z, ref = load_golden(path)
    T = z["intensity"].shape[0]
    feats = []
    for t in range(T):
        c, p, s, h = rs.frame_features(z["intensity"][t], z["frangi"][t], z["distance"][t], z["marker"][t], z["spacing"])
        rc, rst, rh = ref[t]
        assert np.array_equal(c, rc), "coordinates / marker order"
        assert np.array_equal(s, rst), "stats (integer, float32 intensity and Frangi) are exact"
        assert hu_close(h, rh), "log-Hu"
        feats.append((c, p, s, h))
    frames = [(z["intensity"][t],) for t in range(T)]
    kw = dict(dt=float(z["dt"]), mode=str(z["mode"]), max_dense_pairs=int(z["max_dense_pairs"]))
    # matching given the reference's own features: exact
    ref_feats = [(c, c * z["spacing"], s, h) for c, s, h in ref]
    assert np.array_equal(rs.track(frames, z["spacing"], features=ref_feats, **kw), z["flow"])
    # end to end: integer columns exact; the cost column too on dense pairs (float16 margin), within 1e-5 on sparse ones
    # (numpy's float32 log10 of the Frangi values is host-specific, DESIGN.md "Tracking")
    flow = rs.track(frames, z["spacing"], features=feats, **kw)
    g = z["flow"]
    assert flow.shape == g.shape
    assert np.array_equal(flow[:, :-1], g[:, :-1])
    c, gc = flow[:, -1].astype(np.float32), g[:, -1].astype(np.float32)
    assert np.all(np.abs(c - gc) <= 1e-5 * np.maximum(1.0, np.abs(gc)))


def test_empty_flow_layout():
    f3 = rs.track([(np.zeros((4, 5, 6), np.uint16),) * 4] * 2, (1, 1, 1), features=[
        (np.zeros((0, 3), np.int64), np.zeros((0, 3)), np.zeros((0, 4), np.float32), np.zeros((0, 18)))] * 2)
    assert f3.shape == (0, 8) and f3.dtype == np.float32


@pytest.fixture(scope="module")
def lib():
    from nellie_amd import build, hipnative
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        if not os.path.exists(hipnative.LIB_PATH):
            pytest.skip("no hipcc and no prebuilt libnellie_hip.so")
    else:
        build.build(verbose=False)
    return hipnative.load()


def test_half_round_matches_numpy(lib):
    from nellie_amd import hipnative
    rng = np.random.default_rng(7)
    n = 3_000_000
    x = rng.standard_normal(n) * 10.0 ** rng.uniform(-9, 5.5, n)
    edge = [0.0, -0.0, np.inf, -np.inf, np.nan, 65504.0, 65519.999, 65520.0, 1e6, -1e300, 2.0 ** -24, 2.0 ** -25,
            2.0 ** -25 * (1 + 2 ** -40), 3 * 2.0 ** -26, 1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 2.0 ** -14 * (1 - 2 ** -11), 5e-324]
    halves = np.arange(0, 0x7c00, dtype=np.uint16).view(np.float16).astype(np.float64)
    ties = (halves[:-1] + halves[1:]) / 2                                         # every tie between neighbouring halves
    x = np.concatenate([x, edge, ties, -ties, np.nextafter(ties, 0), np.nextafter(ties, np.inf)])
    got = hipnative.host_half_round(x)
    with np.errstate(over="ignore"):
        want = x.astype(np.float16)
    assert np.array_equal(got.view(np.uint16), want.view(np.uint16))


@pytest.mark.parametrize("k", [23, 11, 7, 1])
def test_half_nansum_matches_numpy(lib, k):
    from nellie_amd import hipnative
    rng = np.random.default_rng(k)
    rows = 400_000
    z = (rng.standard_normal((rows, k)) * 10.0 ** rng.uniform(-7, 4.5, (rows, 1))).astype(np.float16)
    z[rng.random(z.shape) < 0.02] = np.nan
    z[rng.random(z.shape) < 0.005] = np.inf
    z[rng.random(z.shape) < 0.002] = -np.inf
    z[rng.random(z.shape) < 0.01] = np.float16(6e-8)                             # subnormal
    z[:1000] = np.float16(30000.0)                                                # overflow to inf in the half result
    got = hipnative.host_half_nansum(z)
    with np.errstate(invalid="ignore", over="ignore"):
        want = np.nansum(z, axis=1)
    same = (got.view(np.uint16) == want.view(np.uint16)) | (np.isnan(got) & np.isnan(want))
    assert same.all(), int((~same).sum())
    assert np.array_equal(rs.half_nansum(z).view(np.uint16)[~np.isnan(want)], want.view(np.uint16)[~np.isnan(want)])


def _im_info(tmp_path, no_t=False, no_z=False):
    paths = {k: str(tmp_path / f"{k}.npy") for k in ("im_marker", "im_distance", "im_preprocessed", "im_instance_label",
                                                      "flow_vector_array")}
    return SimpleNamespace(no_t=no_t, no_z=no_z, shape=(3, 4, 8, 8), axes="TZYX", im_path=str(tmp_path / "im.npy"),
                           dim_res={"X": .1, "Y": .1, "Z": .1, "T": 1.0}, pipeline_paths=paths,
                           get_memmap=lambda p: np.load(p))


def test_stage_cpu_device_raises(tmp_path):
    from nellie_amd.tracking.hu_tracking import HuMomentTracking
    with pytest.raises(RuntimeError, match="HIP backend only"):
        HuMomentTracking(_im_info(tmp_path), device="cpu")
    with pytest.raises(ValueError):
        HuMomentTracking(_im_info(tmp_path), device="tpu")


def test_stage_no_t_writes_nothing(tmp_path):
    from nellie_amd.tracking.hu_tracking import HuMomentTracking
    im = _im_info(tmp_path, no_t=True)
    HuMomentTracking(im).run()
    assert not os.path.exists(im.pipeline_paths["flow_vector_array"])


def test_run_tracking_without_markers_files_raises(tmp_path):
    from nellie_amd.run import run
    with pytest.raises(FileNotFoundError, match="im_marker"):
        run(_im_info(tmp_path), tracking=True)


def _np_sum_lengths():
    ns = list(range(1, 301)) + [8191, 8192, 8193, 16384, 16385]
    for R in (13, 21, 41, 63, 125):
        ns += [R * R, R * R * R]
    return ns


@pytest.mark.parametrize("data", ["offset", "zero_runs", "gamma"])
def test_host_np_sum_matches_numpy(lib, data):
    """the order of the feature kernel's float stats (nl_host_np_sum_f32) equals np.sum of float32 bit for bit, for the value
    and for the float32 square, at every length up to 300, around the 8192-item blocks and at R^2 / R^3 of real ROI tiles"""
    from nellie_amd import hipnative
    rng = np.random.default_rng({"offset": 1, "zero_runs": 2, "gamma": 3}[data])
    for n in _np_sum_lengths():
        if data == "offset":                                        # camera offset: the variance's sumsq - s^2/c cancels
            a = (1000.0 + 10.0 * rng.standard_normal(n)).astype(np.float32)
            a[rng.random(n) < 0.2] = 0
        elif data == "zero_runs":                                   # a zero-padded ROI: runs of data between runs of zeros
            a = np.zeros(n, np.float32)
            step = int(rng.integers(3, 40))
            for s in range(0, n, 2 * step):
                a[s:s + step] = rng.uniform(0.5, 3.0, len(a[s:s + step])).astype(np.float32) * 10.0 ** rng.integers(-3, 4)
        else:
            a = (rng.gamma(2.0, 300.0, n) - 100.0).astype(np.float32)
        for x in (a, a * a):
            got, want = hipnative.host_np_sum_f32(x), np.sum(x)
            assert got.view(np.uint32) == want.view(np.uint32), (n, got, want)
