"""CPU tests of LabelTracks: the numpy restatement against the reference's goldens (tests/golden/label_tracks/*.npz), its row
building against flow_interpolation_restatement.interpolate_all, its defined order against a hand-written expectation, the
scenes the GPU tests run (margins, exact cases) and the public class where no GPU is needed."""
import glob
import os
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN_DIR
import flow_interpolation_restatement as rs
import label_tracks_restatement as lrs
import label_tracks_scenes as sc

GOLDENS = sorted(glob.glob(os.path.join(GOLDEN_DIR, "label_tracks", "label_tracks_*.npz")))
ids = lambda paths: [os.path.basename(p)[:-4] for p in paths]   # noqa: E731


def golden_kw(z):
    return {k[3:]: int(z[k]) for k in z.files if k.startswith("kw_")}


def golden_bound(z, steps):
    """the flow bound per step (rs.tolerance with the fixture's largest neighbour count and largest |vector component|) times the
    number of steps behind a coordinate"""
    D = len(z["spacing"])
    return steps * rs.tolerance(int(z["kmax"]), float(np.abs(z["flow"][:, 1 + D:1 + 2 * D]).max()))


def compare_with_reference(rows, frame_num, z, steps, what):
    """rows against the captured reference: both sides in the stable (id, frame) order (the reference's order within an id is
    not defined), ids and frames exactly, coordinates within golden_bound; frame_num is column 1"""
    rows = np.asarray(rows, np.float64).reshape(len(rows), -1)
    want = z["tracks"]
    assert rows.shape == want.shape, (what, rows.shape, want.shape)
    assert np.array_equal(np.asarray(frame_num), rows[:, 1]), what
    assert np.array_equal(z["frame_num"], want[:, 1]), what
    a, b = lrs.sort_rows(rows), lrs.sort_rows(want)
    assert np.array_equal(a[:, :2], b[:, :2]), what
    err = float(np.abs(a[:, 2:] - b[:, 2:]).max())
    print(f"{what}: {len(rows)} rows, max err {err:.3g}, bound {golden_bound(z, steps):.3g}")
    assert err <= golden_bound(z, steps), (what, err)


def test_goldens_cover_the_cases():
    zs = {os.path.basename(p)[len("label_tracks_"):-4]: np.load(p) for p in GOLDENS}
    assert len(zs) == 12
    for dim in ("3d", "2d"):
        assert golden_kw(zs[f"{dim}_forward_only"])["start_frame"] == 0
        assert golden_kw(zs[f"{dim}_backward_only"])["start_frame"] == zs[f"{dim}_backward_only"]["labels"].shape[0] - 1
        assert 0 < golden_kw(zs[f"{dim}_both_directions"])["start_frame"] < 3
        assert golden_kw(zs[f"{dim}_label_num"])["label_num"] > 0
        assert golden_kw(zs[f"{dim}_skip_3"])["skip_coords"] == 3
        assert golden_kw(zs[f"{dim}_min_track_num_7"])["min_track_num"] == 7
    for name, z in zs.items():
        assert z["labels"].shape[0] == 4 and float(z["max_distance_um"]) == 1.0
        assert all(round(float(s), 1) != float(s) for s in z["spacing"])                           # non-round spacings
        assert float(z["radius_margin"]) > 1e-9 and float(z["half_margin"]) > 1e-9 and int(z["kmax"]) > 1
        assert os.path.getsize(os.path.join(GOLDEN_DIR, "label_tracks", f"label_tracks_{name}.npz")) < 100_000
    both = zs["3d_both_directions"]["tracks"]                                                      # the duplicated start rows
    start = golden_kw(zs["3d_both_directions"])["start_frame"]
    assert len(np.unique(both[both[:, 1] == start], axis=0)) * 2 == int((both[:, 1] == start).sum())


@pytest.mark.parametrize("path", GOLDENS, ids=ids(GOLDENS))
def test_restatement_reproduces_golden(path):
    z = np.load(path)
    kw = golden_kw(z)
    r = sc.radius(float(z["max_distance_um"]), float(z["dt"]))
    rows, frame_num, info = lrs.label_tracks(z["labels"], z["flow"], z["spacing"], r, **kw)
    assert info["ran"] and info["radius_margin"] > 1e-9 and info["half_margin"] > 1e-9 and info["kmax"] == int(z["kmax"])
    n_seeds = len(lrs.seeds(z["labels"], kw["start_frame"], kw.get("label_num"), kw.get("skip_coords", 1)))
    assert not np.isnan(info["raw"]).any() and len(info["raw"]) % n_seeds == 0                     # no coordinate is lost
    kept = len(rows) / len(info["raw"])
    assert 0.1 <= kept <= 0.9                                                                      # the filter keeps and drops
    compare_with_reference(rows, frame_num, z, info["steps"], os.path.basename(path)[:-4])
    assert rows[:, 0].min() >= kw.get("min_track_num", 0)
    # the defined order: the backward rows by id and frame, then the forward rows as emitted
    n_back = int(lrs.keep_rows(z["labels"], info["raw"][:info["n_back"]]).sum())
    assert np.array_equal(rows[:n_back], lrs.sort_rows(rows[:n_back])) and (kw["start_frame"] == 0) == (n_back == 0)
    assert np.all(rows[:n_back, 1] <= kw["start_frame"]) and np.all(rows[n_back:, 1] >= kw["start_frame"])


@pytest.mark.parametrize("path", GOLDENS, ids=ids(GOLDENS))
def test_follow_is_interpolate_all(path):
    """label_tracks_restatement.follow builds array-wise, row for row and bit for bit, what interpolate_all builds in its loop"""
    z = np.load(path)
    kw = golden_kw(z)
    r = sc.radius(float(z["max_distance_um"]), float(z["dt"]))
    start = lrs.seeds(z["labels"], kw["start_frame"], kw.get("label_num"), kw.get("skip_coords", 1))
    for forward, (a, b) in ((True, (kw["start_frame"], 4)), (False, (kw["start_frame"], 0))):
        c1, c2 = start.copy(), start.copy()
        tracks, frame_num, margin = rs.interpolate_all(z["flow"], z["spacing"], r, c1, a, b, forward, min_track_num=kw.get("min_track_num", 0))
        rows, margin2, _ = lrs.follow(z["flow"], z["spacing"], r, c2, a, b, forward, min_track_num=kw.get("min_track_num", 0))
        assert np.array_equal(np.asarray(tracks, float).reshape(-1, rows.shape[1]), rows) and margin == margin2
        assert np.array_equal(np.asarray(frame_num, float), rows[:, 1]) and np.array_equal(c1, c2, equal_nan=True)


def test_restatement_order_beyond_16_backward_rows():
    """Six seeds followed back over three frames are 24 backward rows, more than the 16 up to which numpy's default argsort is
    stable.  Every vector is (0, +1) at one isolated flow row per seed and frame, so a track steps one voxel to the left per
    frame backward; the third seed has no row at the last step and ends early.  Expected by hand: by id, within an id by
    ascending frame."""
    shape = (4, 60)
    labels = np.ones((4,) + shape, np.int32)
    labels[3] = 0
    xs = [10, 18, 26, 34, 42, 50]
    for x in xs:
        labels[3][1, x] = 1
    flow = []
    for t in (2, 1, 0):                                       # backward at t + 1 uses the rows of t at pos + vec
        for n, x in enumerate(xs):
            if t == 0 and n == 2:
                continue
            at = x - (3 - t)                                  # where the track is after the step
            flow.append([float(t), 1.0, float(at), 0.0, 1.0, 0.5])
    rows, frame_num, info = lrs.label_tracks(labels, np.array(flow), (0.25, 0.25), 0.5, start_frame=3, min_track_num=5)
    want = []
    for n, x in enumerate(xs):
        frames = [3, 2, 1, 0] if n != 2 else [3, 2, 1]
        want += [[5 + n, f, 1.0, float(x - (3 - f))] for f in sorted(frames)]
    assert len(info["raw"]) == 23 and np.array_equal(rows, np.array(want, float)) and np.array_equal(frame_num, rows[:, 1])


def test_exact_scenes_decide_by_half_to_even():
    """the exact cases of the GPU file: the restatement keeps exactly the rows the table says, and every landing coordinate is
    a multiple of 0.5, bit for bit"""
    for D in (2, 3):
        for forward in (True, False):
            labels, flow, spacing, start, keep = sc.exact_scene(D, forward)
            rows, frame_num, info = lrs.label_tracks(labels, flow, spacing, 0.5, start_frame=start)
            raw = info["raw"]
            assert len(raw) == 2 * len(keep) and info["kmax"] == 1 and np.array_equal(raw[:, 2:] * 2, np.round(raw[:, 2:] * 2))
            landed = raw[raw[:, 1] != start]
            assert np.array_equal(landed[:, 0], np.arange(len(keep)))
            assert lrs.keep_rows(labels, landed).tolist() == keep, (D, forward)
            assert len(rows) == len(keep) + sum(keep)                     # every start row stays
            assert np.any(landed[:, 2:] == -0.5) and np.any(landed[:, -1] == labels.shape[-1] - 0.5)


@pytest.mark.parametrize("k", range(sc.N_FUZZ))
def test_fuzz_cases_clear_the_margins(k):
    """every fuzz case of test_hip_label_tracks.py: no squared distance within 1e-9 (relative) of r*r, no track coordinate within
    1e-9 of a half-integer -- the GPU run skips nothing"""
    case = sc.fuzz_case(k)
    info = case["want"][2]
    assert info["radius_margin"] > sc.MARGIN and info["half_margin"] > sc.MARGIN
    assert np.array_equal(case["want"][1], case["want"][0][:, 1])


def test_fuzz_cases_cover_the_list():
    cases = [sc.fuzz_case(k) for k in range(sc.N_FUZZ)]
    specs = [c["spec"] for c in cases]
    assert {s["D"] for s in specs} == {2, 3} and {s["start"] for s in specs} == {0, 1, 2, 3}
    assert {s["skip"] for s in specs} >= {1, 3, 100, 10 ** 6} and {s["label"] for s in specs} == {None, 2, 99}
    assert any(s["end"] is not None and s["end"] < sc.T for s in specs) and any(s["end"] is not None and s["end"] > sc.T for s in specs)
    assert max(s["vmax"] for s in specs) == 6
    assert any(c["want"][2]["ran"] and len(c["want"][0]) == 0 for c in cases) or any(not c["want"][2]["ran"] for c in cases)
    lost_mid = tracks_leave = frame_T = 0
    for c in cases:
        raw, labels = c["want"][2]["raw"], c["labels"]
        if len(raw) == 0:
            continue
        ids_per_frame = [set(raw[raw[:, 1] == f, 0].tolist()) for f in range(-1, sc.T + 1)]
        full = max(len(s) for s in ids_per_frame)
        lost_mid += any(0 < len(s) < full for s in ids_per_frame)
        pos = raw[:, 2:]
        tracks_leave += bool(np.any((pos < -0.5) | (pos > np.asarray(labels.shape[1:]) - 0.5)))
        frame_T += bool(np.any(raw[:, 1] == sc.T))
    assert lost_mid >= 3 and tracks_leave >= 3 and frame_T >= 1
    for k, first in ((4, True), (9, False), (14, True), (19, False)):                  # a time point without rows
        c = cases[k]
        raw, start = c["want"][2]["raw"], c["spec"]["start"]
        assert len(raw) > 0, k
        starts = raw[raw[:, 1] == start]
        assert (len(starts) == 0) == first, (k, "the start rows are emitted only when the first frame has rows")


def _im_info(axes="TZYX", shape=(3, 4, 8, 8)):
    return SimpleNamespace(no_t="T" not in axes, no_z="Z" not in axes, shape=shape, axes=axes, im_path="im",
                           dim_res={"X": .1, "Y": .1, "Z": .3, "T": 1.0},
                           pipeline_paths={"im_instance_label": "instance", "im_obj_label_reassigned": "reassigned"},
                           get_memmap=lambda p: np.zeros(shape, np.int32))


def test_constructor_attributes_need_no_gpu(monkeypatch):
    from nellie_amd.tracking.all_tracks_for_label import LabelTracks
    from nellie_amd.utils import adaptive_run
    monkeypatch.setattr(adaptive_run, "gpu_available", lambda: False)
    im = _im_info()
    lt = LabelTracks(im)
    assert lt.im_info is im and lt.num_t == 3 and lt.label_im_path == "instance" and lt.im_memmap is None and lt.label_memmap is None
    lt = LabelTracks(im, num_t=2, label_im_path="reassigned")
    assert lt.num_t == 2 and lt.label_im_path == "reassigned"
    with pytest.raises(RuntimeError, match="GPU backend requested but"):
        lt.initialize()
    lt.close()
    lt.close()
    with LabelTracks(im) as held:
        assert held.label_memmap is None


def test_stack_without_t_raises():
    from nellie_amd.tracking.all_tracks_for_label import LabelTracks
    with pytest.raises(ValueError, match="without T"):
        LabelTracks(_im_info(axes="ZYX", shape=(4, 8, 8)))
    with pytest.raises(ValueError, match="without T"):
        LabelTracks(_im_info(axes="YX", shape=(8, 8)), num_t=1)


def test_tracking_package_exports_nothing():
    import nellie_amd.tracking as pkg
    assert open(pkg.__file__).read().strip() == ""
