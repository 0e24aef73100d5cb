"""CPU tests of flow-vector interpolation: the numpy restatement against the reference's goldens (tests/golden/flow/flow_*.npz,
the two situations in which the port deliberately differs stated exactly), and the public class where no GPU is needed."""
import glob
import os
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN_DIR
import flow_interpolation_restatement as rs

GOLDENS = sorted(glob.glob(os.path.join(GOLDEN_DIR, "flow", "flow_*.npz")))
POINT = [p for p in GOLDENS if "tracks" not in os.path.basename(p)]
TRACKS = [p for p in GOLDENS if "tracks" in os.path.basename(p)]
ids = lambda paths: [os.path.basename(p)[:-4] for p in paths]   # noqa: E731


def radius(z):
    return max(float(z["max_distance_um"]) * float(z["dt"]), 0.5)


def compare_with_reference(got, z, k, vmax, what):
    """got against the golden's `ref` under the issue's rule.  Two reference accidents are stated exactly: with no query above
    one neighbour it fills row 0 only, and after a NaN query row it leaves the last good rows NaN.  There `got` equals the
    reference on the rows the reference filled, and holds the rule's value (k >= 1, finite) where the reference left NaN."""
    ref = z["ref"]
    if ref.shape[0] == 0:
        assert got.shape == ref.shape and not k.any(), what
        return 0
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    quirk = (k.max() == 1) or bool(np.isnan(z["queries"]).any())
    filled = ~np.isnan(ref).any(axis=1)
    if not quirk:
        rs.assert_close(got, ref, k, vmax, what)
        return 0
    assert np.all(k[filled] > 0), what                               # the reference fills no row the rule leaves NaN
    dropped = ~filled & (k > 0)
    assert dropped.any(), (what, "the fixture does not show the reference's accident")
    assert np.all(np.isfinite(got[dropped])) and np.all(np.isnan(got[k == 0])), what
    rs.assert_close(got[filled], ref[filled], k[filled], vmax[filled], what + " (rows the reference filled)")
    return int(dropped.sum())


def test_goldens_cover_the_cases():
    zs = {os.path.basename(p)[:-4]: np.load(p) for p in POINT}
    assert len(zs) >= 14 and len(TRACKS) >= 2
    assert {len(z["spacing"]) for z in zs.values()} == {2, 3}
    assert {bool(z["forward"]) for z in zs.values()} == {True, False}
    assert any(len(set(z["spacing"].tolist())) > 1 for z in zs.values())                       # anisotropic
    assert any(z["ref"].shape[0] == 0 and len(z["queries"]) > 0 for z in zs.values())            # a t without rows
    assert any(len(z["queries"]) == 0 for z in zs.values())                                      # an empty query array
    assert any(float(z["max_distance_um"]) * float(z["dt"]) > 0.5 for z in zs.values())
    assert any(np.isnan(z["queries"]).any() for z in zs.values())
    assert any(np.any(z["queries"] != np.round(z["queries"])) for z in zs.values())              # fractional coordinates
    assert all(float(np.load(p)["margin"]) > 1e-9 for p in GOLDENS)                              # nothing on the radius
    assert all(round(float(s), 1) != float(s) for z in zs.values() for s in z["spacing"])        # non-round spacings
    assert all(os.path.getsize(p) < 300_000 for p in GOLDENS)
    # queries on the check coordinates themselves, two rows at one position among them
    z = zs["flow_3d_marker_queries"]
    _, cc = rs.select_rows(z["flow"], int(z["t"]), bool(z["forward"]), 3)
    assert len(np.unique(cc, axis=0)) < len(cc) and np.array_equal(z["queries"][:len(cc)], cc)


@pytest.mark.parametrize("path", POINT, ids=ids(POINT))
def test_restatement_reproduces_golden(path):
    z = np.load(path)
    name = os.path.basename(path)[:-4]
    got, k, vmax, margin = rs.interpolate_coord(z["flow"], z["spacing"], radius(z), z["queries"], int(z["t"]), bool(z["forward"]))
    assert margin > 1e-9
    dropped = compare_with_reference(got, z, k, vmax, name)
    if name == "flow_3d_max_k_1":
        assert k.max() == 1 and dropped == int((k > 0).sum()) - int(k[0] > 0)                    # the reference fills row 0 only
        _, cc = rs.select_rows(z["flow"], int(z["t"]), True, 3)
        rows = z["flow"][z["flow"][:, 0] == int(z["t"])]
        for n in np.nonzero(k > 0)[0][:50]:                                                      # one neighbour gives its vector
            near = np.argmin((((z["queries"][n] - cc) * z["spacing"]) ** 2).sum(axis=1))
            assert np.array_equal(got[n], rows[near, 4:7])
    if name == "flow_3d_nan_rows":
        n_nan = int(np.isnan(z["queries"]).any(axis=1).sum())
        assert n_nan == 4 and dropped > 0 and np.all(np.isnan(got[np.isnan(z["queries"]).any(axis=1)]))


@pytest.mark.parametrize("path", TRACKS, ids=ids(TRACKS))
def test_restatement_reproduces_tracks(path):
    z = np.load(path)
    for key, fwd in (("forward", True), ("backward", False)):
        coords = z["start"].copy()
        a, b = (int(v) for v in z[f"range_{key}"])
        tracks, frame_num, margin = rs.interpolate_all(z["flow"], z["spacing"], radius(z), coords, a, b, fwd, min_track_num=7)
        want = z[f"tracks_{key}"]
        assert margin > 1e-9 and len(want) > 0
        tracks = np.asarray(tracks, float)
        assert tracks.shape == want.shape and np.array_equal(tracks[:, :2], want[:, :2])
        assert np.array_equal(np.asarray(frame_num), z[f"frame_num_{key}"])
        # three steps of vectors of at most 4 voxels, up to 24 * 3 neighbours in all: the issue's bound with k = 100 per step
        assert np.all(np.abs(tracks[:, 2:] - want[:, 2:]) <= 3 * rs.tolerance(100, 4.0))
        assert np.array_equal(np.isnan(coords), np.isnan(z[f"coords_{key}"]))


def _im_info(tmp_path, no_t=False, no_z=False, dt=1.0):
    paths = {"flow_vector_array": str(tmp_path / "flow.npy")}
    dim_res = {"X": .107, "Y": .107, "Z": .29}
    if dt is not None:
        dim_res["T"] = dt
    return SimpleNamespace(no_t=no_t, no_z=no_z, shape=(3, 4, 8, 8), axes="TZYX", im_path=str(tmp_path / "im.npy"),
                           dim_res=dim_res, pipeline_paths=paths, get_memmap=lambda p: np.load(p))


def test_class_without_gpu_raises(tmp_path, monkeypatch):
    from nellie_amd.tracking.flow_interpolation import FlowInterpolator, interpolate_all_forward
    from nellie_amd.utils import adaptive_run
    monkeypatch.setattr(adaptive_run, "gpu_available", lambda: False)
    with pytest.raises(RuntimeError, match="GPU backend requested but"):
        FlowInterpolator(_im_info(tmp_path))
    with pytest.raises(RuntimeError, match="GPU backend requested but"):
        interpolate_all_forward(np.zeros((2, 3)), 0, 2, _im_info(tmp_path))


def test_class_no_t_returns_early(tmp_path):
    from nellie_amd.tracking.flow_interpolation import FlowInterpolator

    def boom(p):
        raise AssertionError("a no_t image must not touch files")
    im = _im_info(tmp_path, no_t=True)
    im.get_memmap = boom
    fi = FlowInterpolator(im)
    assert fi.im_info is im and not hasattr(fi, "flow_vector_array")
    assert not os.listdir(tmp_path)


def test_class_attributes_before_the_device_check(tmp_path, monkeypatch):
    """scaling, the radius (dt applied, 0.5 um at least, 1.0 s with a warning when T is missing) and the direction are those of
    the reference's constructor"""
    from nellie_amd.tracking import flow_interpolation as fl
    from nellie_amd.utils import adaptive_run
    monkeypatch.setattr(adaptive_run, "gpu_available", lambda: False)
    seen = {}

    class Probe(fl.FlowInterpolator):
        def __init__(self, *a, **kw):
            try:
                super().__init__(*a, **kw)
            except RuntimeError:
                seen.update(self.__dict__)
    Probe(_im_info(tmp_path, dt=2.0), max_distance_um=0.4, forward=False)
    assert seen["scaling"] == (.29, .107, .107) and seen["max_distance_um"] == 0.8 and seen["forward"] is False
    assert seen["num_t"] == 3 and seen["current_t"] is None and seen["check_rows"] is None and seen["check_coords"] is None
    Probe(_im_info(tmp_path, no_z=True, dt=None), max_distance_um=0.3)
    assert seen["scaling"] == (.107, .107) and seen["max_distance_um"] == 0.5
