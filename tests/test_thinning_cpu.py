"""The 3-D thinning, the part that needs no GPU: both forms of the numpy restatement (tests/thinning_restatement.py) against the
recorded results of skimage.morphology.skeletonize (tests/golden/thinning, made by tests/golden/make_golden_thinning.py), the library's
decision functions on the host against the restatement's definitions, and the host-side refusals of `Network`, `run()` and
`skeletonize`."""
import glob
import inspect
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN_DIR

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import network_scenes as scenes  # noqa: E402
import thinning_restatement as rs  # noqa: E402

THIN_CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "thinning", "*.npz")))
NETWORK_CASES = [n for n in THIN_CASES if n.startswith("net_3d_")]
COUNTS = ("outer", "subiters", "candidates", "removed", "max_candidates", "rounds", "max_rounds")
# the restatement takes most of a minute on the large case: the recording script has held it against skimage there, the suite does not
SMALL_CASES = [n for n in THIN_CASES if not n.startswith("large_")]
LAUNCH_THREADS = 1024 * 256            # csrc/thin.inc: THIN_MAX_GRID workgroups of 256


def load_thinning(name):
    """-> dict: mask and skel (bool volumes), the restatement's counts as ints, skimage_version."""
    with np.load(os.path.join(GOLDEN_DIR, "thinning", name + ".npz"), allow_pickle=False) as f:
        shape = tuple(int(s) for s in f["shape"])
        n = int(np.prod(shape))
        out = {k: int(f[k]) for k in COUNTS}
        out["mask"] = np.unpackbits(f["mask_bits"], count=n).astype(bool).reshape(shape)
        out["skel"] = np.unpackbits(f["skel_bits"], count=n).astype(bool).reshape(shape)
        out["skimage_version"] = str(f["skimage_version"])
    return out


def test_the_fixtures_are_the_cases_of_the_design():
    want = {"box", "ball", "bar_x", "bar_y", "bar_z", "plate", "full", "plane", "one", "two", "empty", "hollow", "noise", "tubes_r2", "tubes_r4",
            "odd"}
    assert want <= set(THIN_CASES)
    scenes_3d = [os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN_DIR, "network_steps", "*.npz")) if np.load(p)["labels"].ndim == 3]
    assert sorted(scenes_3d) == NETWORK_CASES and len(NETWORK_CASES) >= 6
    g = {n: load_thinning(n) for n in THIN_CASES}
    assert all(v["skimage_version"] == "0.18.3" for v in g.values())
    assert all(not (v["skel"] & ~v["mask"]).any() for v in g.values())
    # the conditions each case is there for
    assert g["box"]["mask"].shape == (12, 36, 40) and g["box"]["mask"].sum() == 6 * 30 * 34
    assert (g["box"]["skel"].sum(), g["box"]["outer"]) == (0, 8)
    assert (g["ball"]["skel"].sum(), g["ball"]["outer"]) == (2, 9)
    assert g["bar_x"]["max_rounds"] == 204 and g["bar_x"]["mask"].shape[2] > 3 * 64
    assert g["bar_z"]["max_rounds"] == 241
    assert g["full"]["mask"].all() and g["full"]["skel"].sum() == 3
    assert g["plane"]["mask"].shape[0] == 1 and g["plane"]["subiters"] == 4 * g["plane"]["outer"]      # one plane: four directions
    for name in ("one", "two"):
        assert g[name]["removed"] == 0 and np.array_equal(g[name]["skel"], g[name]["mask"]) and g[name]["mask"].all()
    assert not g["empty"]["mask"].any()
    cavity = ~g["hollow"]["mask"][1:-1, 1:-1, 1:-1]
    assert g["hollow"]["skel"].sum() == 382 and cavity.sum() == 5 * 6 * 7 and not g["hollow"]["skel"][1:-1, 1:-1, 1:-1][cavity].any()
    assert g["noise"]["mask"].shape == (9, 10, 70) and g["noise"]["skel"].sum() > 1000
    large = g["large_tiled_noise"]
    assert large["mask"].sum() > LAUNCH_THREADS and large["max_candidates"] > LAUNCH_THREADS      # every stride loop takes a second trip
    assert all(g[n]["mask"].sum() < LAUNCH_THREADS for n in SMALL_CASES)
    for name in NETWORK_CASES:
        labels = np.load(os.path.join(GOLDEN_DIR, "network_steps", name + ".npz"))["labels"]
        assert np.array_equal(g[name]["mask"], labels > 0)


@pytest.mark.parametrize("name", SMALL_CASES)
def test_both_forms_of_the_restatement_equal_skimage(name):
    g = load_thinning(name)
    seq, s_seq = rs.thin_sequential(g["mask"])
    par, s_par = rs.thin_rounds(g["mask"])
    assert np.array_equal(seq, g["skel"]) and np.array_equal(par, g["skel"])
    assert all(s_seq[k] == g[k] for k in s_seq) and all(s_par[k] == g[k] for k in COUNTS)


def test_the_restatements_definitions_agree_with_each_other():
    """The scalar forms are the definitions (a flood; the Euler characteristic of the cell complex counted cell by cell); the vector
    forms are what the restatement runs."""
    words = np.concatenate([rs.all_words_up_to(2), np.random.default_rng(94).integers(0, 1 << 27, 1500).astype(np.uint32) | np.uint32(1 << 13)])
    assert np.array_equal(rs.simple_v(words), [rs.simple(int(w)) for w in words])
    assert np.array_equal(rs.euler_invariant_v(words), [rs.euler_invariant(int(w)) for w in words])


@pytest.fixture(scope="module")
def lib():
    from nellie_amd import build, hipnative
    build.build(verbose=False)
    return hipnative.load()


def _flags_of_the_restatement(words):
    return ((rs.popcount(words) == 2).astype(np.uint8) | rs.euler_invariant_v(words).astype(np.uint8) << 1 | rs.simple_v(words).astype(np.uint8) << 2)


def test_host_decisions_on_every_sparse_neighbourhood(lib):
    from nellie_amd import hipnative
    words = rs.all_words_up_to(4)
    assert len(words) == 17902
    assert np.array_equal(hipnative.thin_decide_host(words), _flags_of_the_restatement(words))


def test_host_decisions_on_random_neighbourhoods(lib):
    from nellie_amd import hipnative
    words = np.random.default_rng(1994).integers(0, 1 << 27, 100000).astype(np.uint32)
    flags = hipnative.thin_decide_host(words)
    assert np.array_equal(flags, _flags_of_the_restatement(words))
    assert 0 < (flags & 2).astype(bool).sum() < len(words) and 0 < (flags & 4).astype(bool).sum() < len(words)
    assert hipnative.thin_decide_host(np.zeros(0, np.uint32)).size == 0


def test_signatures_and_defaults():
    from nellie_amd import run as run_mod
    from nellie_amd import segmentation
    from nellie_amd.segmentation import thinning
    from nellie_amd.segmentation.networking import Network
    p = inspect.signature(Network.__init__).parameters
    assert p["skeletonize"].default is None and p["rounds_per_sync"].default is None
    assert inspect.signature(run_mod.run).parameters["skeletonize"].default is None
    assert segmentation.skeletonize is thinning.skeletonize
    q = inspect.signature(thinning.skeletonize).parameters
    assert list(q)[:2] == ["mask", "device"] and q["device"].default == 0 and q["rounds_per_sync"].default is None


def _infos():
    info3 = scenes.network_im_info(np.zeros((1, 4, 5, 6), np.int32), np.zeros((1, 4, 5, 6), np.float32), (0.3, 0.1, 0.1))
    info2 = scenes.network_im_info(np.zeros((1, 5, 6), np.int32), np.zeros((1, 5, 6), np.float32), (0.1, 0.1))
    return info3, info2


def test_hip_thinning_of_a_2d_image_raises_before_any_file(monkeypatch):
    from nellie_amd import run as run_mod
    from nellie_amd.segmentation.networking import Network
    _, info2 = _infos()
    with pytest.raises(NotImplementedError, match="skeletonize=None"):
        Network(info2, skeletonize="hip").run()
    assert info2.created == []
    monkeypatch.setattr(run_mod, "Filter", None)            # run() must not get as far as building a stage
    with pytest.raises(NotImplementedError, match="skeletonize=None"):
        run_mod.run(info2, network=True, skeletonize="hip")
    assert info2.created == []


def test_an_unknown_thinning_name_raises_before_any_file(monkeypatch):
    from nellie_amd import run as run_mod
    from nellie_amd.segmentation.networking import Network
    info3, info2 = _infos()
    monkeypatch.setattr(run_mod, "Filter", None)
    for info in (info3, info2):
        for name in ("lee", "HIP", ""):
            with pytest.raises(ValueError, match="skeletonize="):
                Network(info, skeletonize=name).run()
            with pytest.raises(ValueError, match="skeletonize="):
                run_mod.run(info, network=True, skeletonize=name)
        assert info.created == []


def test_hip_thinning_needs_no_skimage(monkeypatch):
    """With skimage unimportable the default still raises ImportError, and "hip" gets past the keyword's check (to the device's)."""
    from nellie_amd.segmentation import networking
    for mod in ("skimage", "skimage.morphology"):
        monkeypatch.setitem(sys.modules, mod, None)
    info3, _ = _infos()
    networking._check_thinning("hip", info3)
    with pytest.raises(ImportError, match="skeletonize="):
        networking.Network(info3).run()


def test_function_form_refuses_what_it_cannot_thin():
    from nellie_amd.segmentation.thinning import skeletonize
    with pytest.raises(NotImplementedError, match="3-D"):
        skeletonize(np.ones((5, 6), bool))
    with pytest.raises(NotImplementedError, match="3-D"):
        skeletonize(np.ones((2, 3, 4, 5), bool))
    with pytest.raises(TypeError, match="bool or integer"):
        skeletonize(np.ones((3, 4, 5), np.float32))
