"""The 3-D thinning on the MI355X (nellie_amd.segmentation.thinning.skeletonize, Network(skeletonize="hip")): every result is compared
for equality with what skimage.morphology.skeletonize recorded (tests/golden/thinning) and, through the Network stage, with the run that
is handed the recorded mask."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import network_scenes as scenes  # noqa: E402
import thinning_restatement as rs  # noqa: E402
from test_network_steps_cpu import load_steps  # noqa: E402
from test_thinning_cpu import NETWORK_CASES, THIN_CASES, load_thinning  # noqa: E402

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def golden(name):
    return load_thinning(name)


def _check_counts(info, g):
    assert info["n_in"] == int(g["mask"].sum()) and info["n_out"] == int(g["skel"].sum())
    for key in ("outer", "subiters", "rounds", "candidates", "removed"):
        assert info[key] == g[key], key


@pytest.mark.parametrize("name", THIN_CASES)
def test_every_fixture(name):
    from nellie_amd.segmentation import skeletonize
    g = golden(name)
    got, info = skeletonize(g["mask"], with_info=True)
    assert got.dtype == np.bool_ and got.shape == g["mask"].shape
    assert np.array_equal(got, g["skel"])
    assert info["outer"] == g["outer"]
    _check_counts(info, g)


@pytest.mark.parametrize("name", ["bar_z", "box", "noise"])
def test_the_batch_of_rounds_changes_nothing(name):
    from nellie_amd.segmentation import skeletonize
    g = golden(name)
    for rounds_per_sync in (1, 3, None):
        got, info = skeletonize(g["mask"], rounds_per_sync=rounds_per_sync, with_info=True)
        assert np.array_equal(got, g["skel"]), rounds_per_sync
        _check_counts(info, g)
        if name == "bar_z":
            assert info["rounds"] >= 241


def test_one_context_many_frames():
    """Frames of different content through one context: nothing of a frame -- image, state volume, lists, counters -- reaches the next."""
    from nellie_amd import hipnative
    shape = (40, 40, 40)
    frames = []
    for name in ("tubes_r2", "empty", "ball", "tubes_r4", "tubes_r2"):
        g = golden(name)
        mask, skel = np.zeros(shape, bool), np.zeros(shape, bool)
        sl = tuple(slice(0, s) for s in g["mask"].shape)
        mask[sl], skel[sl] = g["mask"], g["skel"]
        frames.append((name, mask, skel, g))
    with hipnative.Context(shape) as ctx:
        for name, mask, skel, g in frames:
            assert np.array_equal(ctx.thin(mask), skel), name
            counts, ms = ctx.thin_info()
            assert counts["n_out"] == int(skel.sum()) and counts["removed"] == g["removed"] and ms > 0
            assert np.array_equal(ctx.network_fetch_mask(), skel), name


def test_padding_a_frame_with_background_changes_nothing():
    """`empty` and `ball` (above) sit in a corner of a larger frame; here every fixture that fits is moved off the faces."""
    from nellie_amd import hipnative
    shape = (16, 40, 50)
    with hipnative.Context(shape) as ctx:
        for name in ("full", "hollow", "odd", "net_3d_iso"):
            g = golden(name)
            mask, skel = np.zeros(shape, bool), np.zeros(shape, bool)
            sl = tuple(slice(2, 2 + s) for s in g["mask"].shape)
            mask[sl], skel[sl] = g["mask"], g["skel"]
            assert np.array_equal(ctx.thin(mask), skel), name


def test_integer_and_bool_inputs():
    from nellie_amd.segmentation import skeletonize
    g = golden("odd")
    for dtype, value in ((np.uint8, 255), (np.int32, 7), (np.uint16, 2), (np.int64, -3)):
        mask = g["mask"].astype(dtype) * dtype(value)
        before = mask.copy()
        assert np.array_equal(skeletonize(mask), g["skel"]), dtype
        assert np.array_equal(mask, before)
    strided = np.zeros(g["mask"].shape + (2,), bool)
    strided[..., 1] = g["mask"]
    assert np.array_equal(skeletonize(strided[..., 1]), g["skel"])           # not contiguous
    frozen = g["mask"].copy()
    frozen.setflags(write=False)
    assert np.array_equal(skeletonize(frozen), g["skel"])


def test_refusals():
    from nellie_amd import hipnative
    with hipnative.Context((4, 5, 6)) as ctx:
        with pytest.raises(ValueError, match="shape"):
            ctx.thin(np.ones((4, 5, 7), bool))
        with pytest.raises(hipnative.NellieHipError, match="first"):
            ctx.network_fetch_mask()
        with pytest.raises(hipnative.NellieHipError, match="first"):
            ctx.thin_info()
        full = np.ones((4, 5, 6), bool)
        assert np.array_equal(ctx.thin(full), rs.thin_rounds(full)[0])       # the context still works
    with hipnative.Context((1, 5, 6)) as ctx:
        with pytest.raises(NotImplementedError):
            ctx.network_load_thin(np.ones((5, 6), np.int32), np.ones((5, 6), np.float32))


# ---- through the Network stage --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NETWORK_CASES)
def test_network_with_the_thinning_on_the_device(name):
    from nellie_amd.segmentation.networking import Network
    steps, g = load_steps(name), golden(name)
    spacing = tuple(steps["spacing"])
    info = scenes.network_im_info(steps["labels"][None], steps["frangi"][None], spacing)
    host = Network(info, skeletonize=lambda m: g["skel"].copy())
    want = host.frame(steps["labels"], steps["frangi"])
    host.close()
    assert "thin" not in host.kernel_ms[-1]
    net = Network(info, skeletonize="hip")
    got = net.frame(steps["labels"], steps["frangi"])
    for a, b, key in zip(got, want, ("branch", "pixel_class", "relabelled")):
        assert a.dtype == b.dtype and np.array_equal(a, b), key
    assert "thin" in net.kernel_ms[-1] and net.kernel_ms[-1]["thin"] > 0          # the path without a mask upload
    assert set(net.kernel_ms[-1]) == {"clean", "seed", "classes", "relabel", "thin"}
    stats = net.frame_stats[-1]
    assert stats["thin_outer"] == g["outer"] and stats["thin_n_out"] == int(g["skel"].sum()) and stats["thin_rounds"] == g["rounds"]
    assert {k: v for k, v in stats.items() if not k.startswith("thin_")} == host.frame_stats[-1]
    ctx = net._held.obj
    assert np.array_equal(ctx.network_fetch_mask(steps["labels"].shape), g["skel"])
    again = net.frame(steps["labels"], steps["frangi"], skel_mask=g["skel"])      # a mask handed in still takes the upload path
    assert "thin" not in net.kernel_ms[-1] and all(np.array_equal(a, b) for a, b in zip(again, want))
    net.close()


def test_run_on_a_file_with_the_thinning_on_the_device(tmp_path):
    """run(file, network=True, skeletonize="hip") on a small 3-D + T file writes the three files of the run whose thinning is the
    restatement on the host (which equals skimage on every fixture)."""
    from nellie_amd.im_info import ome_tiff
    from nellie_amd.im_info.verifier import FileInfo
    from nellie_amd.run import run
    from nellie_amd.synthetic import ISO_01, make_volume
    vols = np.stack([make_volume((10, 40, 48), seed, dtype=np.uint16) for seed in (5, 6)])
    src = str(tmp_path / "stack.ome.tif")
    ome_tiff.create(src, vols.shape, np.uint16, ISO_01, "raw", data=vols)
    outs = []
    for how, thin in (("host", lambda m: rs.thin_rounds(m)[0]), ("hip", "hip")):
        im = run(FileInfo(src, output_dir=str(tmp_path / how)), device="gpu", network=True, skeletonize=thin)
        outs.append([np.array(im.get_memmap(im.pipeline_paths[k], read_mode="r")) for k in ("im_skel", "im_pixel_class", "im_skel_relabelled")])
    for a, b in zip(*outs):
        assert a.shape == (2, 10, 40, 48) and a.dtype == b.dtype and np.array_equal(a, b)
    assert all(outs[0][0][t].any() for t in range(2))
