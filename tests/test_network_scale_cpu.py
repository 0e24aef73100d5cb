"""The scenes of tests/test_hip_network_scale.py, checked without a device: each wide scene really has the properties that make it reach
a second trip of the Network kernels' stride loops, rows of several mask words and batches of many objects; restatement variants that
get exactly those places wrong are told apart by it; the seeding scene tells three other tie rules from the device's; and the frames
of the table-growth sequence really reuse ids with the other status.  The scenes and their expectations are cached here for both files."""
import functools
import os
import sys

import numpy as np
import pytest
from scipy import ndimage as ndi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import network_scenes as scenes  # noqa: E402
import network_steps_restatement as rs  # noqa: E402
from network_scenes import TRIP_2048, TRIP_8192  # noqa: E402

ANISO_029 = (0.29, 0.11, 0.11)
PRODUCTS = ("branch", "pixel_class", "relabelled")


def _freeze(*arrays):
    for a in arrays:
        a.setflags(write=False)


@functools.lru_cache(maxsize=None)
def wide(name):
    """labels, mask, frangi, spacing, {planted name: label}"""
    kw = dict(scenes.WIDE[name])
    spacing = kw.pop("spacing")
    labels, mask, frangi, ids = scenes.wide_scene(**kw)
    _freeze(labels, mask, frangi)
    return labels, mask, frangi, spacing, ids


@functools.lru_cache(maxsize=None)
def wide_expected(name):
    labels, mask, frangi, spacing, _ = wide(name)
    want = rs.frame(labels, mask, frangi, spacing, transform=rs.scipy_transform)
    _freeze(*[v for v in want.values() if isinstance(v, np.ndarray)])
    return want


def expected_stats(labels, want):
    """What Network.frame_stats must hold for a frame, from the restatement's intermediates."""
    return dict(max_label=int(labels.max()), n_removed=int(((want["skel"] > 0) & (want["skel_clean"] == 0)).sum()), n_seeded=want["n_seeded"],
                n_skel=int((want["skel_seeded"] > 0).sum()), n_branches=int(want["branch"].max()), n_objects=want["n_objects"],
                box_volume=want["box_volume"])


def seeded_boxes(labels, branch):
    """(dz, dy, dx) of every object with a seed, in label order: the objects the relabelling batches, as its host code lists them."""
    out = []
    for k, sl in enumerate(ndi.find_objects(labels)):
        if sl is not None and ((branch[sl] > 0) & (labels[sl] == k + 1)).any():
            out.append((1,) * (3 - labels.ndim) + tuple(s.stop - s.start for s in sl))
    return out


def greedy_batches(boxes, budget):
    """The relabelling's batches: lists of boxes, a new one whenever the next box would pass the budget."""
    batches, used = [], None
    for b in boxes:
        v = int(np.prod(b))
        if used is None or used + v > budget:
            batches.append([])
            used = 0
        batches[-1].append(b)
        used += v
    return batches


@functools.lru_cache(maxsize=None)
def seed_rule(shape):
    labels, frangi, which = scenes.seed_rule_scene(shape)
    _freeze(labels, frangi)
    return labels, frangi, which


@functools.lru_cache(maxsize=None)
def seed_rule_expected(shape, as_shape=None):
    labels, frangi, _ = seed_rule(shape)
    as_shape = as_shape or shape
    labels, frangi = labels.reshape(as_shape), frangi.reshape(as_shape)
    want = rs.frame(labels, np.zeros(as_shape, bool), frangi, ANISO_029[3 - len(as_shape):], transform=rs.scipy_transform)
    _freeze(*[v for v in want.values() if isinstance(v, np.ndarray)])
    return want


@functools.lru_cache(maxsize=None)
def table_growth():
    frames = scenes.table_growth_frames()
    wants = []
    for labels, mask, frangi in frames:
        _freeze(labels, mask, frangi)
        wants.append(rs.frame(labels, mask, frangi, ANISO_029, transform=rs.scipy_transform))
    return frames, wants


# ---- 1. the properties of the wide scenes ---------------------------------------------------------------------------------------------
def _shifted(a, shift):
    """a moved by `shift` (one entry per axis), False where nothing moves in: out[p] = a[p + shift]."""
    out = np.zeros_like(a)
    src = tuple(slice(max(s, 0), a.shape[k] + min(s, 0)) for k, s in enumerate(shift))
    dst = tuple(slice(max(-s, 0), a.shape[k] + min(-s, 0)) for k, s in enumerate(shift))
    out[dst] = a[src]
    return out


def _neighbour_at(skel, dx, other_plane):
    """Voxels with a skeleton voxel at x + dx: in the same row, or (other_plane) in another plane (2-D: there is none)."""
    ndim = skel.ndim
    if not other_plane:
        return _shifted(skel, (0,) * (ndim - 1) + (dx,))
    out = np.zeros_like(skel)
    if ndim == 3:
        for dz in (-1, 1):
            for dy in (-1, 0, 1):
                out |= _shifted(skel, (dz, dy, dx))
    return out


def wide_properties(name):
    """The counts behind properties (a)-(n) of a wide scene -> dict."""
    labels, mask, frangi, spacing, ids = wide(name)
    want = wide_expected(name)
    ndim, nx, n = labels.ndim, labels.shape[-1], labels.size
    lin = np.arange(n, dtype=np.int64).reshape(labels.shape)
    x = np.broadcast_to(np.arange(nx), labels.shape)
    all_ids = np.unique(labels)
    all_ids = all_ids[all_ids > 0]
    first, last = ndi.minimum(lin, labels, all_ids).astype(np.int64), ndi.maximum(lin, labels, all_ids).astype(np.int64)
    best = np.array([np.ravel_multi_index(p, labels.shape) for p in ndi.maximum_position(frangi, labels, all_ids)])
    no_mask = ~np.isin(all_ids, np.unique(labels[mask]))
    skel = want["skel_seeded"] > 0
    planted = np.flatnonzero((want["skel_seeded"] != want["skel_clean"]).ravel())
    removed = np.flatnonzero(((want["skel"] > 0) & (want["skel_clean"] == 0)).ravel())
    p = dict(n=n, n_labels=int(all_ids.size), max_label=int(all_ids[-1]), n_no_mask=int(no_mask.sum()), n_seeded=want["n_seeded"])
    p["planted_id_span"] = int(np.ptp(labels.ravel()[planted]))
    p["a_largest_first_index"] = int(first[-1])
    p["b_no_mask_wholly_in_last_trip"] = int((no_mask & (first >= TRIP_8192)).sum())
    p["b_seeds_in_last_trip"] = int((planted >= TRIP_8192).sum())
    p["c_spanning_with_late_maximum"] = int((no_mask & (first < TRIP_2048) & (last >= TRIP_8192) & (best >= TRIP_8192)).sum())
    p["d_removed_in_last_trip"] = int((removed >= TRIP_8192).sum())
    p["e_x63_neighbour_right"] = int((skel & (x % 64 == 63) & _neighbour_at(skel, 1, False)).sum())
    p["f_x0_neighbour_left"] = int((skel & (x % 64 == 0) & (x > 0) & _neighbour_at(skel, -1, False)).sum())
    p["g_x63_neighbour_right_other_plane"] = int((skel & (x % 64 == 63) & _neighbour_at(skel, 1, True)).sum())
    p["g_x0_neighbour_left_other_plane"] = int((skel & (x % 64 == 0) & (x > 0) & _neighbour_at(skel, -1, True)).sum())
    # (h): a class is min(4, voxels in the neighbourhood), so losing one neighbour changes it exactly where the count is <= 4
    count = ndi.convolve(skel.astype(np.uint8), np.ones((3,) * ndim, np.uint8), mode="constant", cval=0)
    across = np.zeros_like(skel)
    for d in np.ndindex(*(3,) * (ndim - 1)):
        across |= _shifted(skel, tuple(v - 1 for v in d) + (1,))
    deciding = skel & (x % 64 == 63) & across & (count <= 4)
    p["h_deciding_pairs"] = int(deciding.sum())
    p["h_example"] = tuple(int(v) for v in np.argwhere(deciding)[0]) if deciding.any() else None
    p["i_x_first"], p["i_x_last"] = int(skel[..., 0].sum()), int(skel[..., -1].sum())
    p["j_z_first"], p["j_z_last"] = (int(skel[0].sum()), int(skel[-1].sum())) if ndim == 3 else (None, None)
    boxes = seeded_boxes(labels, want["branch"])
    p["k_widest_box"] = max(b[2] for b in boxes)
    batches = greedy_batches(boxes, n)                                  # scratch_voxels=1 floors at one frame
    p["box_volume_over_frame"] = sum(int(np.prod(b)) for b in boxes) / n
    p["batch_objects"] = [len(b) for b in batches]
    lines = [[sum(b[1] * b[2] for b in bt), sum(b[0] * b[2] for b in bt), sum(b[0] * b[1] for b in bt)] for bt in batches]
    p["l_lines_per_pass"] = lines
    starts = lambda f: [tuple(np.cumsum([0] + [f(b) for b in bt[:-1]])) for bt in batches]      # noqa: E731
    seqs = [starts(lambda b: b[0] * b[1] * b[2]), starts(lambda b: b[1] * b[2]), starts(lambda b: b[0] * b[2]), starts(lambda b: b[0] * b[1])]
    if ndim == 2:
        seqs.pop(1)            # one plane: pass 0 does not run, and its line starts (dy * dx each) are the slot offsets themselves
    p["m_different_start_sequences"] = min(len({s[k] for s in seqs}) for k in range(len(batches)))
    p["m_sequences"] = len(seqs)
    p["n_unique_maxima"] = rs.unique_maxima(labels, frangi)
    return p


@functools.lru_cache(maxsize=None)
def _properties(name):
    return wide_properties(name)


@pytest.mark.parametrize("name", sorted(scenes.WIDE))
def test_wide_scene_has_its_properties(name):
    labels, mask, frangi, spacing, ids = wide(name)
    p = _properties(name)
    print(name, p)
    ndim = labels.ndim
    assert TRIP_8192 < p["n"] < 1 << 24, p
    assert labels.dtype == np.int32 and mask.dtype == np.bool_ and frangi.dtype == np.float32
    assert 300 <= p["n_labels"] <= 600 and p["max_label"] > 1024, p
    assert 0.4 * p["n_labels"] <= p["n_no_mask"] <= 0.6 * p["n_labels"] and p["planted_id_span"] > 256, p
    assert p["a_largest_first_index"] >= TRIP_8192 and p["max_label"] == ids["largest"], p                        # (a)
    assert p["b_no_mask_wholly_in_last_trip"] >= 1 and p["b_seeds_in_last_trip"] >= 1, p                           # (b)
    assert p["c_spanning_with_late_maximum"] >= 1, p                                                               # (c)
    assert p["d_removed_in_last_trip"] >= 1, p                                                                     # (d)
    assert p["e_x63_neighbour_right"] >= 1 and p["f_x0_neighbour_left"] >= 1, p                                    # (e) (f)
    if ndim == 3:
        assert p["g_x63_neighbour_right_other_plane"] >= 1 and p["g_x0_neighbour_left_other_plane"] >= 1, p        # (g)
        assert p["j_z_first"] >= 1 and p["j_z_last"] >= 1, p                                                       # (j)
    assert p["h_deciding_pairs"] >= 1, p                                                                           # (h)
    assert p["i_x_first"] >= 1 and p["i_x_last"] >= 1, p                                                           # (i)
    assert p["k_widest_box"] > 64, p                                                                               # (k)
    assert p["box_volume_over_frame"] >= 3 and len(p["batch_objects"]) >= 3 and min(p["batch_objects"][:-1]) >= 20, p
    passes = range(3 - ndim, 3)
    assert all(max(lines[d] for lines in p["l_lines_per_pass"]) > 256 for d in passes), p                          # (l)
    assert p["m_different_start_sequences"] == p["m_sequences"] == ndim + 1, p                                     # (m)
    assert p["n_unique_maxima"], p                                                                                 # (n)


@pytest.mark.parametrize("name", sorted(scenes.WIDE))
def test_the_deciding_neighbour_across_a_word_boundary_decides(name):
    """(h) literally: take the neighbours at x + 1 of one such voxel away and its class changes."""
    want = wide_expected(name)
    at = _properties(name)["h_example"]
    assert at is not None and at[-1] % 64 == 63
    crop = tuple(slice(max(v - 2, 0), v + 3) for v in at)
    inside = tuple(v - s.start for v, s in zip(at, crop))
    pre = np.array(want["skel_pre"][crop])
    before = rs.pixel_class(pre, pre.ndim)[inside]
    assert before == want["pixel_class"][at]
    pre[..., inside[-1] + 1] = 0
    assert rs.pixel_class(pre, pre.ndim)[inside] != before


# ---- 2. the wide scenes tell restatements apart that go wrong where the kernels could ------------------------------------------------------
def _from_clean(labels, skel_clean, frangi, spacing, pixel_class=rs.pixel_class, relabel_labels=None):
    """rs.frame from the cleaned skeleton on, with the class step and the labels the relabelling sees open to a variant."""
    ndim = labels.ndim
    seeded, _ = rs.seed(skel_clean, labels, frangi)
    pc = pixel_class((seeded > 0) * labels, ndim)
    branch = rs.branch_skel_labels(pc, ndim)
    rel = rs.relabel(branch, labels if relabel_labels is None else relabel_labels, spacing, rs.scipy_transform)[0]
    return dict(pixel_class=pc, branch=branch, relabelled=rel)


def _differing(got, want):
    return [k for k in PRODUCTS if not np.array_equal(got[k], want[k])]


@pytest.mark.parametrize("name", sorted(scenes.WIDE))
def test_wide_scene_notices_a_clean_step_that_stops_after_one_trip(name):
    labels, mask, frangi, spacing, _ = wide(name)
    want = wide_expected(name)
    lin = np.arange(labels.size).reshape(labels.shape)
    half_clean = np.where(lin < TRIP_8192, want["skel_clean"], want["skel"])
    assert _differing(_from_clean(labels, half_clean, frangi, spacing), want)


@pytest.mark.parametrize("name", sorted(scenes.WIDE))
def test_wide_scene_notices_a_largest_label_taken_from_the_first_trip(name):
    """Labels above the (too small) largest label have no table entry, so the relabelling never lists them."""
    labels, mask, frangi, spacing, _ = wide(name)
    want = wide_expected(name)
    short = int(labels.ravel()[:TRIP_2048].max())
    assert short < labels.max()
    known = np.where(labels <= short, labels, 0)
    got = _from_clean(labels, want["skel_clean"], frangi, spacing, relabel_labels=known)
    assert "relabelled" in _differing(got, want)


def _pixel_class_without_carry(skel, ndim):
    out = np.zeros(skel.shape, np.uint8)
    for x0 in range(0, skel.shape[-1], 64):
        out[..., x0:x0 + 64] = rs.pixel_class(skel[..., x0:x0 + 64], ndim)
    return out


@pytest.mark.parametrize("name", sorted(scenes.WIDE))
def test_wide_scene_notices_classes_without_a_carry_between_mask_words(name):
    labels, mask, frangi, spacing, _ = wide(name)
    want = wide_expected(name)
    pc = _pixel_class_without_carry(want["skel_pre"], labels.ndim)
    differ = np.argwhere(pc != want["pixel_class"])
    assert differ.size and set(differ[:, -1] % 64) <= {0, 63}
    assert {0, 63} <= set(differ[:, -1] % 64)


# ---- 3. the seeding rule ---------------------------------------------------------------------------------------------------------------------
def _seed_positions(labels, frangi, **rule):
    seeded, n = rs.seed(np.zeros(labels.shape, np.int32), labels, frangi, **rule)
    flat = seeded.ravel()
    at = np.flatnonzero(flat)
    assert n == at.size
    return dict(zip(flat[at].tolist(), at.tolist()))


@pytest.mark.parametrize("shape", [scenes.SEED_RULE_SMALL, scenes.SEED_RULE_LARGE], ids=["small", "large"])
def test_seed_rule_scene_and_the_rule_it_states(shape):
    labels, frangi, which = seed_rule(shape)
    lab, fr = labels.ravel(), frangi.ravel()
    got = _seed_positions(labels, frangi)
    assert sorted(got) == sorted(which.values()) and len(which) == 11
    own = {case: np.flatnonzero(lab == L) for case, L in which.items()}
    val = {case: fr[p] for case, p in own.items()}
    for case in ("tie3_late", "tie3_span"):
        ties = own[case][val[case] == val[case].max()]
        assert ties.size == 3 and got[which[case]] == ties[0]
    if labels.size > TRIP_8192:
        ties = own["tie3_span"][val["tie3_span"] == val["tie3_span"].max()]
        assert ties[0] < TRIP_2048 and ties[-1] >= TRIP_8192
        assert own["tie3_late"][val["tie3_late"] == val["tie3_late"].max()].min() >= TRIP_8192
    nans = own["nan_among_larger"][np.isnan(val["nan_among_larger"])]
    assert nans.size == 1 and np.nanmin(val["nan_among_larger"]) > 1 and got[which["nan_among_larger"]] == nans[0]
    nans = own["two_nans"][np.isnan(val["two_nans"])]
    assert nans.size == 2 and got[which["two_nans"]] == nans[0]
    assert len(set(fr[nans].view(np.uint32).tolist())) == 2                        # two bit patterns
    for case, first_sign in (("minus_zero_first", True), ("plus_zero_first", False)):
        zeros = own[case][val[case] == 0]
        assert zeros.size == 2 and (val[case] <= 0).all() and got[which[case]] == zeros[0]
        assert bool(np.signbit(fr[zeros[0]])) == first_sign and bool(np.signbit(fr[zeros[1]])) != first_sign
    assert (val["all_negative"] < 0).all() and got[which["all_negative"]] == own["all_negative"][np.argmax(val["all_negative"])]
    assert np.isposinf(val["plus_inf"]).sum() == 1 and got[which["plus_inf"]] == own["plus_inf"][np.argmax(val["plus_inf"])]
    assert np.isneginf(val["only_minus_inf"]).all() and got[which["only_minus_inf"]] == own["only_minus_inf"][0]
    sub = val["subnormals"]
    assert (np.abs(sub) < np.finfo(np.float32).tiny).all() and (sub > 0).any() and (sub < 0).any() and int((sub == sub.max()).sum()) == 1
    assert got[which["subnormals"]] == own["subnormals"][np.argmax(sub)] != own["subnormals"][0]
    assert own["one_voxel"].size == 1 and got[which["one_voxel"]] == own["one_voxel"][0]


@pytest.mark.parametrize("shape", [scenes.SEED_RULE_SMALL, scenes.SEED_RULE_LARGE], ids=["small", "large"])
@pytest.mark.parametrize("mutant, cases", [(dict(lowest_index=False), {"tie3_late", "tie3_span", "two_nans", "minus_zero_first", "plus_zero_first", "only_minus_inf"}),
                                           (dict(nan_highest=False), {"nan_among_larger", "two_nans"}),
                                           (dict(zeros_equal=False), {"minus_zero_first"})],
                         ids=["highest_index", "nan_lowest", "minus_zero_below"])
def test_seed_rule_scene_detects_another_rule(shape, mutant, cases):
    labels, frangi, which = seed_rule(shape)
    want, got = _seed_positions(labels, frangi), _seed_positions(labels, frangi, **mutant)
    assert {case for case, L in which.items() if got[L] != want[L]} == cases


def test_seeds_of_the_wide_scene_are_scipys_maximum_positions():
    """Where every maximum is unique and finite the rule is scipy.ndimage.maximum_position, the call the reference makes."""
    labels, mask, frangi, spacing, _ = wide("wide_3d")
    want = wide_expected("wide_3d")
    assert rs.unique_maxima(labels, frangi)
    flat = want["skel_seeded"].ravel()
    planted = np.flatnonzero(flat != want["skel_clean"].ravel())
    planted = planted[np.argsort(flat[planted])]
    missing = flat[planted]
    assert missing.size == want["n_seeded"] == np.unique(missing).size > 100
    at = ndi.maximum_position(frangi, labels, missing)
    assert np.array_equal(planted, [np.ravel_multi_index(p, labels.shape) for p in at])


# ---- 4. the table-growth frames --------------------------------------------------------------------------------------------------------------
def test_table_growth_frames_reuse_ids_with_the_other_status():
    frames, wants = table_growth()
    tops = [int(f[0].max()) for f in frames]
    assert tops == [40, 5000, 40, 70000]
    seeded = []
    for (labels, mask, frangi), want in zip(frames, wants):
        assert rs.unique_maxima(labels, frangi) and len(np.unique(labels)) - 1 >= 6
        seeded.append(set(want["skel_seeded"][want["skel_seeded"] != want["skel_clean"]].tolist()))
        assert len(seeded[-1]) == want["n_seeded"]
    present = [set(np.unique(f[0]).tolist()) - {0} for f in frames]
    assert {3, 12} <= seeded[1] and {7, 20} <= present[1] - seeded[1]
    assert {7, 20} <= seeded[2] and {3, 12} <= present[2] - seeded[2]
    assert max(seeded[1]) > 1024 and max(seeded[3]) > 65536 and len(seeded[3]) >= 4
