"""The Network stage behind the thinning, the part that needs no GPU: the numpy restatement (tests/network_steps_restatement.py)
against the reference's recorded steps and against scipy's feature transform, and the host-side refusals of `Network` and `run()`."""
import glob
import inspect
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN_DIR

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import network_scenes as scenes  # noqa: E402
import network_steps_restatement as rs  # noqa: E402

STEP_CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "network_steps", "*.npz")))
SPACINGS = {3: [(1, 1, 1), (0.3, 0.1, 0.1), (2.5, 1, 1), (0.29, 0.11, 0.11)], 2: [(1, 1), (0.1, 0.1), (2.5, 1), (0.29, 0.11)]}


def load_steps(name):
    return dict(np.load(os.path.join(GOLDEN_DIR, "network_steps", name + ".npz"), allow_pickle=False))


def test_the_fixtures_cover_the_cases():
    assert len(STEP_CASES) >= 8
    g = {n: load_steps(n) for n in STEP_CASES}
    assert any(v["labels"].ndim == 2 for v in g.values()) and any(v["labels"].ndim == 3 for v in g.values())
    assert any(not v["labels"].any() for v in g.values())
    assert any(int(v["n_seedless"]) > 0 for v in g.values())
    assert any(int(v["n_seeded"]) > 0 for v in g.values())
    assert any(int(v["n_removed"]) > 0 for v in g.values())
    for want in ((1.0, 1.0, 1.0), (0.3, 0.1, 0.1), (0.29, 0.11, 0.11)):
        assert any(tuple(v["spacing"]) == want for v in g.values()), want


@pytest.mark.parametrize("name", STEP_CASES)
def test_restatement_equals_the_reference_bit_for_bit(name):
    g = load_steps(name)
    assert rs.unique_maxima(g["labels"], g["frangi"])
    mine = rs.frame(g["labels"], g["skel_mask"], g["frangi"], tuple(g["spacing"]))
    for key in ("skel", "skel_clean", "skel_seeded", "pixel_class", "branch", "relabelled"):
        assert mine[key].dtype == g[key].dtype and np.array_equal(mine[key], g[key]), key
    for key in ("branch", "pixel_class", "relabelled"):
        assert np.array_equal(mine[key], g["frame_" + key]), key
    assert mine["n_seeded"] == int(g["n_seeded"])
    assert int(((mine["skel"] > 0) & (mine["skel_clean"] == 0)).sum()) == int(g["n_removed"])


def test_feature_transform_equals_scipy_index_for_index():
    rng = np.random.default_rng(20240611)
    checked = 0
    for k in range(240):
        rank = 2 + k % 2
        shape = tuple(int(v) for v in rng.integers(1, 13, rank))
        seeds = rng.random(shape) < rng.uniform(0.02, 0.5)
        if not seeds.any():
            seeds.flat[int(rng.integers(seeds.size))] = True
        sp = SPACINGS[rank][(k // 2) % 4]
        mine, ref = rs.feature_transform(seeds, sp), rs.scipy_transform(seeds, sp)
        assert mine.shape == ref.shape and np.array_equal(mine, ref), (k, shape, sp)
        checked += 1
    assert checked >= 200


def test_feature_transform_without_a_seed_finds_nothing():
    assert (rs.feature_transform(np.zeros((3, 4), bool), (1, 1)) == -1).all()


def test_network_refuses_the_cpu():
    from nellie_amd.segmentation import Network
    from nellie_amd.segmentation.networking import Network as same
    assert Network is same
    info = scenes.network_im_info(np.zeros((1, 4, 5, 6), np.int32), np.zeros((1, 4, 5, 6), np.float32), (0.3, 0.1, 0.1))
    with pytest.raises(RuntimeError, match="device='cpu' is not available"):
        Network(info, device="cpu")
    with pytest.raises(ValueError, match="Unsupported device"):
        Network(info, device="tpu")
    assert info.created == []


def test_network_keeps_the_reference_signature():
    from nellie_amd.segmentation.networking import Network
    p = inspect.signature(Network.__init__).parameters
    assert list(p)[1:9] == ["im_info", "num_t", "min_radius_um", "max_radius_um", "viewer", "device", "low_memory", "max_chunk_voxels"]
    assert (p["num_t"].default, p["min_radius_um"].default, p["max_radius_um"].default, p["viewer"].default, p["device"].default,
            p["low_memory"].default, p["max_chunk_voxels"].default) == (None, 0.20, 1, None, "auto", False, int(1e6))
    assert (p["device_index"].default, p["skeletonize"].default, p["scratch_voxels"].default) == (0, None, None)
    info3 = scenes.network_im_info(np.zeros((2, 4, 5, 6), np.int32), np.zeros((2, 4, 5, 6), np.float32), (0.3, 0.1, 0.2))
    info2 = scenes.network_im_info(np.zeros((2, 5, 6), np.int32), np.zeros((2, 5, 6), np.float32), (0.1, 0.2))
    assert Network(info3).scaling == (0.3, 0.1, 0.2) and Network(info2).scaling == (0.1, 0.2)
    assert Network(info3).num_t == 2 and Network(info3, num_t=1).num_t == 1


def test_network_without_a_thinning_raises_before_any_file(monkeypatch):
    from nellie_amd.segmentation.networking import Network
    for mod in ("skimage", "skimage.morphology"):
        monkeypatch.setitem(sys.modules, mod, None)
    info = scenes.network_im_info(np.zeros((1, 4, 5, 6), np.int32), np.zeros((1, 4, 5, 6), np.float32), (0.3, 0.1, 0.1))
    with pytest.raises(ImportError, match="skeletonize="):
        Network(info).run()
    assert info.created == []
    from nellie_amd import run as run_mod
    monkeypatch.setattr(run_mod, "Filter", None)            # run() must not get as far as building a stage
    with pytest.raises(ImportError, match="skeletonize="):
        run_mod.run(info, network=True)
    assert info.created == []


class _Stage:
    log = []

    def __init__(self, im_info, **kw):
        self.kw = kw

    def run(self):
        type(self).log.append((type(self).__name__, self.kw))


def _fake_stages(monkeypatch):
    from nellie_amd import run as run_mod
    from nellie_amd.segmentation import mocap_marking, networking
    _Stage.log = []
    names = {}
    for name in ("Filter", "Label", "Network", "Markers"):
        names[name] = type(name, (_Stage,), {})
    monkeypatch.setattr(run_mod, "Filter", names["Filter"])
    monkeypatch.setattr(run_mod, "Label", names["Label"])
    monkeypatch.setattr(networking, "Network", names["Network"])
    monkeypatch.setattr(mocap_marking, "Markers", names["Markers"])
    return run_mod


def test_run_without_network_is_unchanged(monkeypatch, capsys):
    run_mod = _fake_stages(monkeypatch)
    p = inspect.signature(run_mod.run).parameters
    assert p["network"].default is False and p["skeletonize"].default is None
    assert list(p)[:11] == ["file_info", "remove_edges", "otsu_thresh_intensity", "threshold", "timeit", "device", "low_memory", "markers",
                            "devices", "shard", "tracking"]
    info = scenes.network_im_info(np.zeros((1, 4, 5, 6), np.int32), np.zeros((1, 4, 5, 6), np.float32), (0.3, 0.1, 0.1))
    assert run_mod.run(info, timeit=True, markers=True) is info
    assert [n for n, _ in _Stage.log] == ["Filter", "Label", "Markers"]
    out = capsys.readouterr().out
    assert [line.split(":")[0] for line in out.splitlines()] == ["[timeit] Filter", "[timeit] Label", "[timeit] Markers", "[timeit] Total"]


def test_run_with_network_runs_it_between_label_and_markers(monkeypatch, capsys):
    run_mod = _fake_stages(monkeypatch)
    info = scenes.network_im_info(np.zeros((1, 4, 5, 6), np.int32), np.zeros((1, 4, 5, 6), np.float32), (0.3, 0.1, 0.1))

    def thin(mask):
        return mask
    run_mod.run(info, timeit=True, markers=True, network=True, skeletonize=thin, device="gpu")
    assert [n for n, _ in _Stage.log] == ["Filter", "Label", "Network", "Markers"]
    assert _Stage.log[2][1]["skeletonize"] is thin and _Stage.log[2][1]["device"] == "gpu"
    out = capsys.readouterr().out
    assert [line.split(":")[0] for line in out.splitlines()] == ["[timeit] Filter", "[timeit] Label", "[timeit] Network", "[timeit] Markers",
                                                                "[timeit] Total"]
