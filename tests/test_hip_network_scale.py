"""The Network stage behind the thinning on the MI355X at the sizes its small exact tests do not reach: frames above 2 097 152 voxels,
where every stride loop takes a later trip; 3-D and 2-D rows of several mask words with a partial last one; the seeding rule at ties,
NaNs, signed zeros and infinities; per-label tables that grow and serve a small frame again; batches of many objects of mixed box
shapes; and the thinning on the device composed with the rest.  Everything is compared for equality of whole arrays, dtype included,
with the numpy/scipy restatement (tests/network_steps_restatement.py); tests/test_network_scale_cpu.py holds the scenes to their
properties."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import network_scenes as scenes  # noqa: E402
from network_scenes import TRIP_8192  # noqa: E402
from test_hip_network_steps import device_relabel, network  # noqa: E402
from test_network_scale_cpu import (ANISO_029, PRODUCTS, expected_stats, greedy_batches, seed_rule, seed_rule_expected, seeded_boxes,  # noqa: E402
                                    table_growth, wide, wide_expected)

pytestmark = pytest.mark.gpu

DTYPES = (np.int32, np.uint8, np.uint32)
STATS = ("max_label", "n_removed", "n_seeded", "n_skel", "n_branches", "n_objects", "box_volume")


def _assert_products(got, want, what=""):
    for out, key, dtype in zip(got, PRODUCTS, DTYPES):
        assert out.dtype == dtype and out.shape == want[key].shape, (what, key, out.dtype, out.shape)
        assert np.array_equal(out, want[key]), (what, key, int((out != want[key]).sum()), np.argwhere(out != want[key])[:5].tolist())


def _assert_stats(stats, labels, want, what=""):
    exp = expected_stats(labels, want)
    assert {k: stats[k] for k in STATS} == exp, (what, stats, exp)


# ---- 1. the wide scenes through the whole stage ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(scenes.WIDE))
def test_wide_scene_through_frame(name):
    labels, mask, frangi, spacing, _ = wide(name)
    want = wide_expected(name)
    net = network(spacing, scratch_voxels=1)                            # the floor, one frame: several batches of many objects
    try:
        got = net.frame(labels, frangi, skel_mask=mask)
        _assert_products(got, want, name)
        _assert_stats(net.frame_stats[-1], labels, want, name)
        assert net.frame_stats[-1]["n_batches"] == len(greedy_batches(seeded_boxes(labels, want["branch"]), labels.size)) >= 3
    finally:
        net.close()


def test_negative_label_in_the_last_trip_is_refused_and_the_handle_goes_on():
    labels, mask, frangi, spacing, ids = wide("wide_3d")
    want = wide_expected("wide_3d")
    bad = labels.copy()
    at = np.flatnonzero(labels.ravel() == ids["largest"])[-1]
    assert at >= TRIP_8192 and (labels >= 0).all()
    bad.reshape(-1)[at] = -5                                            # the only negative label, seen in the last trip alone
    net = network(spacing)
    try:
        with pytest.raises(ValueError, match="not negative"):
            net.frame(bad, frangi, skel_mask=mask)
        got = net.frame(labels, frangi, skel_mask=mask)
        _assert_products(got, want)
        _assert_stats(net.frame_stats[-1], labels, want)
    finally:
        net.close()


# ---- 2. the relabelling alone, in three, two and one batch --------------------------------------------------------------------------------
def test_wide_3d_relabel_alone_in_three_or_more_two_and_one_batch():
    labels, _, _, spacing, _ = wide("wide_3d")
    want = wide_expected("wide_3d")
    branch, rel = want["branch"], want["relabelled"]
    boxes = seeded_boxes(labels, branch)
    vol = sum(int(np.prod(b)) for b in boxes)
    assert len(boxes) == want["n_objects"] and vol == want["box_volume"] >= 3 * labels.size
    two = next(b for b in range(vol // 2, vol + 1, max(1, vol // 400)) if len(greedy_batches(boxes, b)) == 2)
    for budget, batches in ((1, len(greedy_batches(boxes, labels.size))), (two, 2), (vol, 1)):
        got, (n_obj, box_volume, n_batches) = device_relabel(labels, branch, spacing, scratch_voxels=budget)
        assert got.dtype == np.uint32 and np.array_equal(got, rel), (budget, int((got != rel).sum()))
        assert (n_obj, box_volume, n_batches) == (len(boxes), vol, batches), budget
    assert len(greedy_batches(boxes, labels.size)) >= 3


# ---- 3. the seeding rule ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, as_shape, runs", [(scenes.SEED_RULE_SMALL, None, 1), (scenes.SEED_RULE_SMALL, (15, 70), 1), (scenes.SEED_RULE_LARGE, None, 2)],
                         ids=["small_3d", "small_2d", "large_3d_twice"])
def test_seed_rule(shape, as_shape, runs):
    labels, frangi, which = seed_rule(shape)
    want = seed_rule_expected(shape, as_shape)
    as_shape = as_shape or shape
    labels, frangi = labels.reshape(as_shape), frangi.reshape(as_shape)
    empty = np.zeros(as_shape, bool)
    planted_want = np.flatnonzero(want["skel_seeded"].ravel())
    assert planted_want.size == want["n_seeded"] == len(which)
    net = network(ANISO_029[3 - len(as_shape):])
    try:
        outs = [net.frame(labels, frangi, skel_mask=empty) for _ in range(runs)]
        for t, got in enumerate(outs):
            planted = np.flatnonzero(got[1].ravel())                   # an empty mask: the skeleton is the planted voxels
            assert np.array_equal(planted, planted_want), (t, dict(zip(labels.ravel()[planted].tolist(), planted.tolist())),
                                                           dict(zip(labels.ravel()[planted_want].tolist(), planted_want.tolist())), which)
            assert net.frame_stats[t]["n_seeded"] == want["n_seeded"]
            _assert_products(got, want, t)
            _assert_stats(net.frame_stats[t], labels, want, t)
        for a, b in zip(outs[0], outs[-1]):
            assert np.array_equal(a, b)
    finally:
        net.close()


# ---- 4. the per-label table across frames ------------------------------------------------------------------------------------------------
def test_table_grows_shrinks_and_grows_on_one_handle():
    frames, wants = table_growth()
    net = network(ANISO_029)
    try:
        for t, ((labels, mask, frangi), want) in enumerate(zip(frames, wants)):
            got = net.frame(labels, frangi, skel_mask=mask)
            _assert_products(got, want, t)
            _assert_stats(net.frame_stats[t], labels, want, t)
            if t == 2:
                third = got
    finally:
        net.close()
    fresh = network(ANISO_029)
    try:
        labels, mask, frangi = frames[2]
        for a, b in zip(fresh.frame(labels, frangi, skel_mask=mask), third):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        assert {k: fresh.frame_stats[0][k] for k in STATS} == expected_stats(labels, wants[2])
    finally:
        fresh.close()


# ---- 5. the thinning on the device, composed with the rest at size --------------------------------------------------------------------
def test_device_thinning_composed_with_the_stage_on_wide_3d():
    from nellie_amd.segmentation import skeletonize
    labels, _, frangi, spacing, _ = wide("wide_3d")
    mask = skeletonize(labels > 0)                                      # the stand-alone entry point, held against skimage by its own tests
    assert mask.dtype == np.bool_ and mask.shape == labels.shape and mask.any() and not mask[labels == 0].any()
    host = network(spacing)
    dev = network(spacing, skeletonize="hip")
    try:
        want = host.frame(labels, frangi, skel_mask=mask)
        got = dev.frame(labels, frangi)
        for a, b, key in zip(got, want, PRODUCTS):
            assert a.dtype == b.dtype and np.array_equal(a, b), key
        a, b = dev.frame_stats[-1], host.frame_stats[-1]
        assert {k: v for k, v in a.items() if not k.startswith("thin_")} == b and set(b) >= set(STATS)
        assert a["thin_n_out"] == int(mask.sum()) and a["thin_n_in"] == int((labels > 0).sum())
    finally:
        host.close()
        dev.close()
