"""GPU tests of flow-vector interpolation (nellie_amd.tracking.flow_interpolation.FlowInterpolator, csrc/flow.inc): the reference's
goldens through the public class, the (0, D) cases, a fixed-seed fuzz slice against the numpy restatement, caching of a time
point's rows, determinism, one call of 2 * 10^7 queries and one file-level run behind run(markers=True, tracking=True).

Bound (tests/flow_interpolation_restatement.py: tolerance): NaN rows identical, values within 16 * k * 2^-52 * max(1, max|v|) per
row, k the row's neighbour count."""
import glob
import os
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN_DIR
import flow_interpolation_restatement as rs
from test_flow_cpu import compare_with_reference, radius

pytestmark = pytest.mark.gpu
GOLDENS = sorted(glob.glob(os.path.join(GOLDEN_DIR, "flow", "flow_*.npz")))
POINT = [p for p in GOLDENS if "tracks" not in os.path.basename(p)]
TRACKS = [p for p in GOLDENS if "tracks" in os.path.basename(p)]
ids = lambda paths: [os.path.basename(p)[:-4] for p in paths]   # noqa: E731


@pytest.fixture(scope="module")
def hip():
    from nellie_amd import build, hipnative
    build.build(verbose=False)
    lib = hipnative.load()
    assert lib.device_count() > 0, "no HIP device"
    return lib


def im_double(tmp_path, flow, spacing, dt, T=4):
    D = len(spacing)
    path = str(tmp_path / f"flow_{len(os.listdir(tmp_path))}.npy")
    np.save(path, flow)
    axes = "TYX" if D == 2 else "TZYX"
    dim_res = dict(zip(axes[1:], (float(s) for s in spacing)))
    dim_res["T"] = float(dt)
    stack = np.zeros((T,) + (4,) * D, np.uint8)
    return SimpleNamespace(no_t=False, no_z=D == 2, shape=stack.shape, axes=axes, dim_res=dim_res, im_path="im",
                           pipeline_paths={"flow_vector_array": path}, get_memmap=lambda p: stack)


def interpolator(tmp_path, flow, spacing, dt=1.0, max_distance_um=0.5, forward=True):
    from nellie_amd.tracking.flow_interpolation import FlowInterpolator
    return FlowInterpolator(im_double(tmp_path, flow, spacing, dt), max_distance_um=max_distance_um, forward=forward)


@pytest.mark.parametrize("path", POINT, ids=ids(POINT))
def test_golden(hip, tmp_path, path):
    z = np.load(path)
    name = os.path.basename(path)[:-4]
    fi = interpolator(tmp_path, z["flow"], z["spacing"], float(z["dt"]), float(z["max_distance_um"]), bool(z["forward"]))
    assert fi.max_distance_um == radius(z)
    got = fi.interpolate_coord(z["queries"].copy(), int(z["t"]))
    want, k, vmax, _ = rs.interpolate_coord(z["flow"], z["spacing"], radius(z), z["queries"], int(z["t"]), bool(z["forward"]))
    assert got.shape == want.shape and got.dtype == np.float64
    if len(want):
        rs.assert_close(got, want, k, vmax, name + " against the restatement")
    compare_with_reference(got, z, k, vmax, name + " against the reference")
    rows, cc = rs.select_rows(z["flow"], int(z["t"]), bool(z["forward"]), len(z["spacing"]))
    assert fi.current_t == int(z["t"]) and np.array_equal(fi.check_rows, rows) and np.array_equal(fi.check_coords, cc)
    fi.close()


@pytest.mark.parametrize("path", TRACKS, ids=ids(TRACKS))
def test_golden_tracks(hip, tmp_path, path):
    from nellie_amd.tracking.flow_interpolation import interpolate_all_backward, interpolate_all_forward
    z = np.load(path)
    for key, fn in (("forward", interpolate_all_forward), ("backward", interpolate_all_backward)):
        coords = z["start"].copy()
        a, b = (int(v) for v in z[f"range_{key}"])
        im = im_double(tmp_path, z["flow"], z["spacing"], float(z["dt"]))
        tracks, props = fn(coords, a, b, im, min_track_num=7, max_distance_um=float(z["max_distance_um"]))
        want = z[f"tracks_{key}"]
        tracks = np.asarray(tracks, float)
        assert tracks.shape == want.shape and np.array_equal(tracks[:, :2], want[:, :2])
        assert list(props) == ["frame_num"] and np.array_equal(np.asarray(props["frame_num"]), z[f"frame_num_{key}"])
        err = np.abs(tracks[:, 2:] - want[:, 2:]).max()
        print(f"{os.path.basename(path)} {key}: {len(tracks)} track rows, max err {err:.3g}")
        # three steps of vectors of at most 4 voxels: the per-step bound with k = 100 (above every neighbour count of the fixture)
        assert err <= 3 * rs.tolerance(100, 4.0)
        assert np.array_equal(np.isnan(coords), np.isnan(z[f"coords_{key}"]))               # coords updated in place
        assert np.allclose(coords[:-5], z[f"coords_{key}"][:-5], rtol=0, atol=3 * rs.tolerance(100, 4.0))


def test_zero_row_results(hip, tmp_path):
    """(0, D), not (n, D) of NaN: a t without rows, queries all out of reach, all-NaN queries, an empty query array"""
    rng = np.random.default_rng(0)
    for D in (2, 3):
        flow = random_flow(rng, D, (20,) * D, [30, 0, 30], 4)
        for forward in (True, False):
            fi = interpolator(tmp_path, flow, (0.107,) * D, forward=forward)
            t_none, t_rows = (1, 0) if forward else (2, 1)
            q = rng.integers(0, 20, (50, D)).astype(float)
            assert fi.interpolate_coord(q, t_none).shape == (0, D)
            assert fi.interpolate_coord(q, 17).shape == (0, D)
            assert fi.interpolate_coord(q, t_rows).shape == (50, D)
            assert fi.interpolate_coord(q + 1000.0, t_rows).shape == (0, D)
            assert fi.interpolate_coord(np.full((7, D), np.nan), t_rows).shape == (0, D)
            assert fi.interpolate_coord(np.zeros((0, D)), t_rows).shape == (0, D)
            assert fi.interpolate_coord(np.argwhere(np.ones((3,) * D)), t_rows).shape == (27 if D == 3 else 9, D)   # int64 in
            fi.close()


def random_flow(rng, D, shape, rows_per_t, vmax, integer=True):
    out = []
    for t, n in enumerate(rows_per_t):
        if integer:
            pos = np.column_stack([rng.integers(0, s, n) for s in shape]).astype(float)
            vec = rng.integers(-vmax, vmax + 1, (n, D)).astype(float)
        else:
            pos = np.column_stack([rng.uniform(0, s, n) for s in shape])
            vec = rng.uniform(-vmax, vmax, (n, D))
        if n > 10:                                                   # repeated positions, as row- and column-based candidates give
            dup = rng.choice(n, n // 6, replace=False)
            pos[dup] = pos[(dup + 1) % n]
        cost = rng.random(n).astype(np.float32).astype(float)
        if n > 3:
            cost[:2] = (0.0, 1.0)
        out.append(np.column_stack([np.full(n, float(t)), pos, vec, cost]))
    return np.concatenate(out) if out else np.zeros((0, 2 * D + 2))


SPACINGS3 = [(0.107,) * 3, (0.29, 0.0973, 0.0973), (0.211, 0.083, 0.083), (0.1, 0.1, 0.1), (0.3, 0.1, 0.1)]
SPACINGS2 = [(0.107, 0.107), (0.107, 0.083), (0.1, 0.1)]
FUZZ = []
_r = np.random.default_rng(2025)
for _k in range(36):
    _D = 2 if _k % 3 == 2 else 3
    _shape = tuple(int(_r.choice([40, 97, 256, 700])) for _ in range(2)) if _D == 2 else \
        (int(_r.choice([6, 20, 64])), int(_r.choice([40, 128, 300])), int(_r.choice([40, 128, 300])))
    FUZZ.append(dict(seed=_k, D=_D, shape=_shape, forward=_k % 2 == 0,
                     spacing=(SPACINGS2 if _D == 2 else SPACINGS3)[int(_r.integers(0, 3 if _D == 2 else 5))],
                     rows=int([0, 1, 2, 37, 500, 2000, 5000][int(_r.integers(0, 7))]) if _k >= 4 else [0, 1, 5000, 5000][_k],
                     queries=int([0, 1, 63, 1000, 40000, 250000][int(_r.integers(0, 6))]) if _k >= 4 else 1_000_000,
                     maxd=float(_r.choice([0.5, 0.5, 0.8, 1.3])), vmax=int(_r.choice([1, 4, 20])),
                     integer=bool(_k % 5 != 4), nan_rows=bool(_k % 7 == 3)))
    if FUZZ[-1]["queries"] >= 40000:                                 # many queries on a large frame: the restatement's pair lists stay small
        FUZZ[-1]["shape"] = (700, 700) if _D == 2 else (64, 300, 300)


@pytest.mark.parametrize("case", FUZZ, ids=[f"fuzz{c['seed']}" for c in FUZZ])
def test_fuzz_against_restatement(hip, tmp_path, case):
    """2-D / 3-D, both directions, 0 .. 5 000 rows per time point, up to 10^6 queries, vectors up to +-20 voxels, costs in
    [0, 1] (0 and 1 included), integer and fractional coordinates, round spacings too: on the radius the device and numpy
    form the same float64 d2 from the same operations, so membership stays identical"""
    rng = np.random.default_rng(case["seed"])
    D, shape = case["D"], case["shape"]
    flow = random_flow(rng, D, shape, [case["rows"]] * 3, case["vmax"], case["integer"])
    n = case["queries"]
    if case["integer"]:
        q = np.column_stack([rng.integers(-2, s + 2, n) for s in shape]).astype(float).reshape(n, D)
    else:
        q = np.column_stack([rng.uniform(-2, s + 2, n) for s in shape]).reshape(n, D)
    if case["rows"] and n > 10:                                      # some queries on check coordinates (d == 0)
        _, cc = rs.select_rows(flow, 1, case["forward"], D)
        q[:min(n // 4, len(cc))] = cc[:min(n // 4, len(cc))]
    if case["nan_rows"] and n > 3:
        q[rng.choice(n, max(1, n // 50), replace=False)] = np.nan
        q[n // 2, D - 1] = np.nan                                    # NaN in the last column only
    fi = interpolator(tmp_path, flow, case["spacing"], max_distance_um=case["maxd"], forward=case["forward"])
    got = fi.interpolate_coord(q.copy(), 1)
    want, k, vmax, _ = rs.interpolate_coord(flow, case["spacing"], max(case["maxd"], 0.5), q, 1, case["forward"])
    assert got.shape == want.shape, (got.shape, want.shape)
    if len(want):
        rs.assert_close(got, want, k, vmax, f"fuzz {case['seed']} ({case['rows']} rows)")
    fi.close()


def test_cached_rows_and_determinism(hip, tmp_path):
    """t, then t + 1, then t again gives the first answer bit for bit; so does a second interpolator; rows stay on the device
    while t does not change"""
    rng = np.random.default_rng(5)
    flow = random_flow(rng, 3, (30, 100, 100), [3000, 3000, 3000], 6)
    q = np.argwhere(rng.random((30, 100, 100)) < 0.3).astype(float)
    for forward in (True, False):
        fi = interpolator(tmp_path, flow, (0.29, 0.0973, 0.0973), forward=forward)
        a = fi.interpolate_coord(q, 1)
        rows_id = id(fi.check_rows)
        a2 = fi.interpolate_coord(q, 1)
        assert id(fi.check_rows) == rows_id                           # no reload for the same t
        b = fi.interpolate_coord(q, 2)
        c = fi.interpolate_coord(q, 1)
        fi.close()
        fj = interpolator(tmp_path, flow, (0.29, 0.0973, 0.0973), forward=forward)
        d = fj.interpolate_coord(q, 1)
        fj.close()
        assert np.isfinite(a).any() and a.tobytes() != b.tobytes()
        assert a.tobytes() == a2.tobytes() == c.tobytes() == d.tobytes()


def test_twenty_million_queries(hip, tmp_path):
    """one call with 2 * 10^7 query rows (several chunks inside the library), checked on 200 000 random rows"""
    rng = np.random.default_rng(20)
    shape = (128, 512, 512)
    flow = random_flow(rng, 3, shape, [3000, 3000], 5)
    n = 20_000_000
    q = np.empty((n, 3))
    for a, s in enumerate(shape):
        q[:, a] = rng.integers(0, s, n)
    fi = interpolator(tmp_path, flow, (0.29, 0.0973, 0.0973), max_distance_um=2.0)
    got = fi.interpolate_coord(q, 1)
    fi.close()
    assert got.shape == (n, 3)
    pick = np.sort(rng.choice(n, 200_000, replace=False))
    pick[-1] = n - 1                                                  # the last row of the last chunk
    want, k, vmax, _ = rs.interpolate_coord(flow, (0.29, 0.0973, 0.0973), 2.0, q[pick], 1, True)
    rs.assert_close(got[pick], want, k, vmax, "2e7 queries, subset")
    assert int((k > 0).sum()) > 1000
    # and the number of rows with a neighbour in all 2 * 10^7 is plausible against the subset's share
    share = float(np.isfinite(got[:, 0]).mean())
    assert abs(share - float((k > 0).mean())) < 0.01


def test_run_tracking_then_interpolate_on_files(hip, tmp_path):
    """run(markers=True, tracking=True) on a small synthetic T stack, then the flow at every labelled voxel, forward and
    backward, from the flow_vector_array it wrote"""
    from nellie_amd.im_info.verifier import ImInfo
    from nellie_amd.run import run
    from nellie_amd.synthetic import ISO_01, make_volume
    from nellie_amd.tracking.flow_interpolation import FlowInterpolator
    vols = np.stack([make_volume((24, 48, 48), 60 + t) for t in range(3)])
    im_info = ImInfo(vols, dim_res=ISO_01, output_dir=str(tmp_path), name="flow")
    run(im_info, device="gpu", markers=True, tracking=True)
    flow = np.load(im_info.pipeline_paths["flow_vector_array"])
    labels = np.asarray(im_info.get_memmap(im_info.pipeline_paths["im_instance_label"], read_mode="r"))
    sp = (im_info.dim_res["Z"], im_info.dim_res["Y"], im_info.dim_res["X"])
    r = max(0.5 * (im_info.dim_res.get("T") or 1.0), 0.5)
    assert len(flow) > 0 and labels.any()
    found = 0
    for forward, ts in ((True, (0, 1)), (False, (1, 2))):
        fi = FlowInterpolator(im_info, forward=forward)
        assert fi.scaling == sp and fi.max_distance_um == r and np.array_equal(fi.flow_vector_array, flow)
        for t in ts:
            q = np.argwhere(labels[t] > 0)
            got = fi.interpolate_coord(q, t)
            want, k, vmax, _ = rs.interpolate_coord(flow.astype(np.float64), sp, r, q, t, forward)
            assert got.shape == want.shape
            if len(want):
                rs.assert_close(got, want, k, vmax, f"files, forward={forward}, t={t}")
            found += int((k > 0).sum())
        fi.close()
    assert found > 0
