"""CPU tests of voxel reassignment: the numpy restatement against the reference's goldens (tests/golden/reassign/reassign_*.npz),
the margins the goldens were captured under, the public class where no GPU is needed, and the decisive scenes of
tests/reassign_scenes.py: every case brings the margins it is built for to exactly 0, and each rule turned into its opposite shows."""
import glob
import os
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN_DIR
import voxel_reassignment_restatement as rs

GOLDENS = sorted(glob.glob(os.path.join(GOLDEN_DIR, "reassign", "reassign_*.npz")))
ids = lambda paths: [os.path.basename(p)[:-4] for p in paths]   # noqa: E731
TAINTED_CAP = 0.05


def radius(z):
    return max(float(z["max_distance_um"]) * float(z["dt"]), 0.5)


def golden_matches(z):
    return [[z[f"match_{t}_prev"], z[f"match_{t}_next"]] for t in range(int(z["n_matches"]))]


def tainted_of(z):
    """(T - 1, ...) bool: the targets of the fixture that rest on a tie of the nearest-voxel step (none but in the integer-flow one)"""
    return z["tainted"] if "tainted" in z.files else np.zeros((z["obj"].shape[0] - 1,) + z["obj"].shape[1:], bool)


def assert_equals_reference(z, re_branch, re_obj, matches, what):
    """both stacks and every running_matches array (dtype included) equal the golden; on tainted targets anything goes"""
    keep = np.concatenate([np.ones((1,) + z["obj"].shape[1:], bool), ~tainted_of(z)])
    assert re_branch.dtype == np.int32 and re_obj.dtype == np.int32, what
    assert np.array_equal(np.asarray(re_branch)[keep], z["ref_branch"][keep]), (what, "branch")
    assert np.array_equal(np.asarray(re_obj)[keep], z["ref_obj"][keep]), (what, "obj")
    want = golden_matches(z)
    if not bool(z["kw_store_running_matches"]):
        assert not want and not matches, what
        return
    assert len(matches) == len(want), (what, len(matches), len(want))
    taint = tainted_of(z)
    for t, ((p, n), (p2, n2)) in enumerate(zip(matches, want)):
        assert p.dtype == p2.dtype and n.dtype == n2.dtype, (what, p.dtype, p2.dtype)
        ok, ok2 = ~taint[t][tuple(n.T.astype(np.int64))], ~taint[t][tuple(n2.T.astype(np.int64))]
        assert np.array_equal(p[ok], p2[ok2]) and np.array_equal(n[ok], n2[ok2]), (what, "matches of pair", t)


def test_goldens_cover_the_cases():
    zs = {os.path.basename(p)[:-4]: np.load(p) for p in GOLDENS}
    assert len(zs) >= 10
    assert {len(z["spacing"]) for z in zs.values()} == {2, 3}
    assert any(len(set(z["spacing"].tolist())) > 1 for z in zs.values())
    assert all(round(float(s), 1) != float(s) for z in zs.values() for s in z["spacing"])
    assert all(os.path.getsize(p) < 200_000 for p in GOLDENS)
    assert any(not bool(z["kw_store_running_matches"]) for z in zs.values())
    assert any(radius(z) > 0.5 for z in zs.values())
    for name, z in zs.items():
        assert z["branch"].dtype == np.int32 and z["obj"].dtype == np.int32
        assert not np.any((z["branch"] > 0) & (z["obj"] == 0)) and (z["branch"] > 0).sum() < (z["obj"] > 0).sum()   # a strict subset
        assert np.any(z["flow"][:, 1 + len(z["spacing"]):-1] != np.round(z["flow"][:, 1 + len(z["spacing"]):-1])) or "integer" in name
        # ids are permuted per frame: a copy of the input labels is not the answer
        if z["ref_obj"][1:].any():
            assert not np.array_equal(z["ref_obj"][1:], z["obj"][1:]), name
    z = zs["reassign_3d_appearing"]                      # an object far from any flow row stays 0
    new = (z["obj"][1] > 0) & (z["ref_obj"][1] == 0)
    half = z["obj"].shape[-1] // 2
    assert new[..., half:].sum() > 50                    # the appearing object, unassigned ...
    assert not (z["obj"][0][..., half:] > 0).any() and (z["obj"][1][..., half:] > 0).any()      # ... in a half no other object enters
    assert not np.any(z["flow"][:, 3] + np.abs(z["flow"][:, 6]) >= half - 6)                     # and no flow row comes near
    z = zs["reassign_3d_vanishing"]
    assert len(np.unique(z["obj"][0])) > len(np.unique(z["obj"][-1]))
    z = zs["reassign_3d_converging"]                     # two labels of frame 1 end in one object of frame 2
    assert len(np.unique(z["obj"][1])) > len(np.unique(z["obj"][2]))
    z = zs["reassign_3d_empty_frame"]
    assert not z["obj"][2].any() and z["obj"][3].any() and not z["ref_obj"][2:].any() and z["ref_obj"][1].any()
    z = zs["reassign_2d_pair_without_flow"]
    assert not np.any(z["flow"][:, 0] == 1) and z["obj"][2].any() and not z["ref_obj"][2:].any() and z["ref_obj"][1].any()
    z = zs["reassign_3d_integer_flow"]
    vec = z["flow"][:, 4:7]
    assert z["obj"].shape[0] == 2 and np.array_equal(vec, np.round(vec))


@pytest.mark.parametrize("path", GOLDENS, ids=ids(GOLDENS))
def test_stored_margins_meet_the_bounds(path):
    z = np.load(path)
    k = int(z["min_max_k"])
    assert k == 0 or k >= 2                              # below 2 the reference's interpolator loses rows
    assert float(z["margin_b"]) > 1e-6
    if "tainted" in z.files:
        share = z["tainted"].sum() / ((z["branch"][1:] > 0) | (z["obj"][1:] > 0)).sum()
        assert 0 < share <= TAINTED_CAP
        return
    assert float(z["margin_a"]) > 1e-9
    assert float(z["margin_c"]) > 1e-6 and float(z["margin_d"]) > 1e-6


@pytest.mark.parametrize("path", GOLDENS, ids=ids(GOLDENS))
def test_restatement_reproduces_golden(path):
    z = np.load(path)
    name = os.path.basename(path)[:-4]
    store = bool(z["kw_store_running_matches"])
    got = rs.reassign(z["branch"], z["obj"], z["flow"], z["spacing"], radius(z), store_running_matches=store,
                      max_refine_iterations=int(z["kw_max_refine_iterations"]))
    taint = np.stack(got["tainted"]) if got["tainted"] else np.zeros((0,) + z["obj"].shape[1:], bool)
    if "tainted" in z.files:
        assert np.array_equal(taint, z["tainted"])
        share = taint.sum() / ((z["branch"][1:] > 0) | (z["obj"][1:] > 0)).sum()
        print(f"{name}: tainted share {share:.4f}")
        assert share <= TAINTED_CAP
    else:
        assert not taint.any() and got["margin_a"] > 1e-9
        assert got["margin_b"] == float(z["margin_b"]) and got["margin_c"] == float(z["margin_c"])
    assert_equals_reference(z, got["reassigned_branch"], got["reassigned_obj"], got["running_matches"] or [], name)
    if store:                                            # and the saved object array has the reference's shape
        import io
        buf = io.BytesIO()
        rs.save_matches(buf, got["running_matches"])
        buf.seek(0)
        assert np.load(buf, allow_pickle=True).shape == tuple(z["saved_shape"])


@pytest.mark.parametrize("path", GOLDENS, ids=ids(GOLDENS))
def test_one_vote_pass_equals_three(path):
    """every target with a candidate is labelled by the first pass, so a second finds nothing unassigned"""
    z = np.load(path)
    a = rs.reassign(z["branch"], z["obj"], z["flow"], z["spacing"], radius(z), max_refine_iterations=1)
    b = rs.reassign(z["branch"], z["obj"], z["flow"], z["spacing"], radius(z), max_refine_iterations=3)
    assert np.array_equal(a["reassigned_branch"], b["reassigned_branch"]) and np.array_equal(a["reassigned_obj"], b["reassigned_obj"])
    assert a["reassigned_obj"][1].any()


def test_error_distance_is_numpys_norm():
    """the restated order of the three squares is the one np.linalg.norm uses over an axis of 3 (and of 2)"""
    rng = np.random.default_rng(0)
    for D in (2, 3):
        s = np.array((0.29, 0.0973, 0.0973)[3 - D:])
        c = rng.uniform(0, 60, (50000, D))
        m = np.round(c + rng.uniform(-3, 3, c.shape))
        want = np.linalg.norm((c - m).astype(np.float32) * s, axis=1).astype(np.float32)
        assert np.array_equal(rs.error_distance(c, m, s), want)


def test_select_match_coord_dtype():
    from nellie_amd.tracking.voxel_reassignment import VoxelReassigner, select_match_coord_dtype
    for fn in (select_match_coord_dtype, rs.select_match_coord_dtype):
        assert fn((4, 65536, 10)) is np.uint16
        assert fn((65537, 4)) is np.uint32
        assert fn((1, 2 ** 32, 7)) is np.uint32
        assert fn((2 ** 32 + 1, 4, 4)) is np.uint64
        assert fn(None) is np.uint16 and fn(()) is np.uint16
    vr = VoxelReassigner(_im_info(None, no_t=True))
    vr.spatial_shape = (3, 65537, 2)
    assert vr._select_match_coord_dtype() is np.uint32


def _im_info(tmp_path, no_t=False):
    names = ("flow_vector_array", "voxel_matches", "im_skel_relabelled", "im_instance_label", "im_branch_label_reassigned",
             "im_obj_label_reassigned")
    paths = {k: str(tmp_path / (k + ".npy")) if tmp_path is not None else k for k in names}

    def boom(*a, **kw):
        raise AssertionError("must not touch files")
    return SimpleNamespace(no_t=no_t, no_z=False, shape=(3, 4, 8, 8), axes="TZYX", im_path="im", dim_res={"X": .107, "Y": .107, "Z": .29, "T": 1.0},
                           pipeline_paths=paths, get_memmap=boom, allocate_memory=boom)


def test_class_device_errors(tmp_path):
    from nellie_amd.tracking.voxel_reassignment import VoxelReassigner
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VoxelReassigner(_im_info(tmp_path), device="cpu")
    with pytest.raises(ValueError, match="Unsupported device"):
        VoxelReassigner(_im_info(tmp_path), device="tpu")


def test_class_without_gpu_raises(tmp_path, monkeypatch):
    from nellie_amd.tracking.voxel_reassignment import VoxelReassigner
    from nellie_amd.utils import adaptive_run
    monkeypatch.setattr(adaptive_run, "gpu_available", lambda: False)
    vr = VoxelReassigner(_im_info(tmp_path), store_running_matches=False, max_refine_iterations=2)
    assert vr.num_t == 3 and vr.running_matches == [] and vr.store_running_matches is False and vr.max_refine_iterations == 2
    with pytest.raises(RuntimeError, match="GPU backend requested but"):
        vr.run()
    assert not os.listdir(tmp_path)


def test_class_no_t_returns_early(tmp_path):
    from nellie_amd.tracking.voxel_reassignment import VoxelReassigner
    vr = VoxelReassigner(_im_info(tmp_path, no_t=True), num_t=5)
    assert vr.num_t == 1 and vr.flow_interpolator_fw is None and vr.flow_interpolator_bw is None and vr.running_matches == []
    for name in ("voxel_matches_path", "branch_label_memmap", "obj_label_memmap", "reassigned_branch_memmap", "reassigned_obj_memmap",
                 "shape", "spatial_shape", "match_coord_dtype"):
        assert getattr(vr, name) is None
    assert vr.run() is None
    vr.close()
    assert not os.listdir(tmp_path)


# ---- decisive scenes (tests/reassign_scenes.py): every case brings the margins it is built for to exactly 0 --------------------
import reassign_scenes as scenes   # noqa: E402

CASES = scenes.decisive_cases()
_runs = {}


def restated(case, **rules):
    """the restatement of a decisive case on its numpy flow restatement, computed once per (case, rules) and left unchanged"""
    key = (case["id"],) + tuple(sorted(rules))
    if key not in _runs:
        branch, obj, flow = case["make"]()
        _runs[key] = rs.reassign(branch, obj, flow, case["spacing"], case["r"], **rules)
    return _runs[key]


def assert_margins_zero(case, res, what):
    """the margins a case is built for are exactly 0, and a half-voxel lattice case has at least 100 tie sets"""
    for letter in case["zero"]:
        assert res["margin_" + letter] == 0.0, (what, case["id"], letter, res["margin_" + letter])
    if case["scene"] == "lattice_holes" and case["half_voxel"]:
        assert res["tie_sets"] >= 100, (what, case["id"], res["tie_sets"])


def test_decisive_cases_are_what_the_issue_lists():
    ids = [c["id"] for c in CASES]
    assert len(set(ids)) == len(ids) == 2 * 4 * 6 + 1 + 2
    lattice = [c for c in CASES if c["scene"] == "lattice_holes"]
    assert all("a" in c["zero"] and "d" in c["zero"] for c in lattice)
    assert sum(c["dt"] == 1.4 and c["r"] == 0.7 for c in lattice) == 1
    assert sum("b" in c["zero"] for c in lattice) == 2 * 2 * 2 and sum("c" in c["zero"] for c in lattice) == 2 * 4 + 1
    for c in CASES:
        branch, obj, flow = c["make"]()
        assert branch.dtype == np.int32 and obj.dtype == np.int32 and branch.shape == obj.shape and branch.shape[0] == 2
        assert flow.shape[1] == 2 * c["D"] + 2 and len(flow) < 2000 and np.all(flow[:, 0] == 0)
        assert obj[0].size <= {"lattice_holes": 5 * 12 * 70, "crowd": 15 ** 3, "faces_and_outside": 8 * 40 * 70}[c["scene"]]
    branch, obj, _ = scenes.lattice_holes(3, (0.0, 0.0, 0.0))
    assert obj[0][2, 5, 30] != obj[0][2, 5, 31] != obj[0][2, 6, 31] and (obj[1] > 0).sum() == (obj[0] > 0).sum() // 2
    assert 0 < (branch[1] > 0).sum() < (obj[1] > 0).sum()


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_decisive_case_decides(case):
    res = restated(case)
    print(f"{case['id']}: margins a {res['margin_a']:.3g} b {res['margin_b']:.3g} c {res['margin_c']:.3g} d {res['margin_d']:.3g}, "
          f"{res['tie_sets']} tie sets, longest candidate list {res['max_candidates']}")
    assert res["pairs"] == 1 and len(res["running_matches"]) == 1
    assert_margins_zero(case, res, "flow restatement")


def test_lattice_vectors_survive_a_few_ulps():
    """the flow vectors arrive as a weighted mean of equal vectors, which need not be bit-exact: the float32 roundings of the
    centroid and of c - m restore the lattice point, so a vector that is off by a few ulps gives the same result and the same
    zero margins"""
    import flow_interpolation_restatement as fr
    rng = np.random.default_rng(5)
    for case in CASES:
        if case["scene"] != "lattice_holes":
            continue
        branch, obj, flow = case["make"]()

        def interp(coords, t, forward):
            out = fr.interpolate_coord(flow, np.asarray(case["spacing"]), case["r"], coords, t, forward)[0]
            return out * (1.0 + rng.integers(-4, 5, out.shape) * 2.0 ** -52)
        got, want = rs.reassign(branch, obj, None, case["spacing"], case["r"], interp=interp), restated(case)
        assert_margins_zero(case, got, "vectors off by up to 4 ulps")
        for key in ("reassigned_branch", "reassigned_obj"):
            assert np.array_equal(got[key], want[key]), (case["id"], key)
        assert all(np.array_equal(a, b) for x, y in zip(got["running_matches"], want["running_matches"]) for a, b in zip(x, y)), case["id"]


def crowd_labels(res):
    return [(int(res["reassigned_obj"][1][t]), int(res["reassigned_branch"][1][t])) for t in scenes.CROWD_TARGETS]


def test_crowd_ties_the_vote_over_a_long_list():
    case = next(c for c in CASES if c["scene"] == "crowd")
    res = restated(case)
    # the interior target's list: every lattice offset whose float32 length is below r (the voxel under the target included), and
    # its own backward candidate
    k = np.arange(-6, 7)
    off = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3)
    within = rs.error_distance(off.astype(np.float64), np.zeros_like(off, np.float64), np.asarray(case["spacing"])).astype(np.float64) < case["r"]
    assert res["max_candidates"] == int(within.sum()) + 1 and res["max_candidates"] > 300
    assert res["margin_c"] == 0.0
    (A, B, _), (A2, B2, _) = scenes.CROWD_LABELS
    assert A < B and A2 < B2
    assert crowd_labels(res) == [(A, 50), (A2, 51)]          # the smaller of the two tied labels; the voxel under the target wins the branch vote
    assert [o for o, _ in crowd_labels(restated(case, vote_larger=True))] == [B, B2]


def test_faces_and_outside_on_the_restatement():
    import flow_interpolation_restatement as fr
    case = next(c for c in CASES if c["scene"] == "faces_and_outside")
    branch, obj, flow = case["make"]()
    res = restated(case)
    for face in range(3):                                # labelled voxels on every face and corner of both frames
        for side in (0, -1):
            assert np.take(obj[0], side, axis=face).any() and np.take(obj[1], side, axis=face).any()
    for corner in np.ndindex(2, 2, 2):
        at = tuple(-c for c in corner)
        assert obj[0][at] > 0 and obj[1][at] > 0
    for name in scenes.FACES_REGIONS:
        m = scenes.faces_region(name)
        assert (obj[0][m] > 0).all() and (obj[1][m] > 0).all()
        got = res["reassigned_obj"][1][m]
        if name in scenes.FACES_STAY_ZERO:
            assert not got.any() and not res["reassigned_branch"][1][m].any(), name
        else:
            assert (got > 0).all() and set(got.tolist()) <= set(obj[0][m].tolist()), name
    nan = np.argwhere(scenes.faces_region("inner_nan")).astype(np.float64)
    vec = fr.interpolate_coord(flow, np.asarray(case["spacing"]), case["r"], nan, 0, True)[0]
    assert vec.shape == nan.shape and np.isnan(vec).all()
    far = fr.interpolate_coord(flow, np.asarray(case["spacing"]), case["r"], np.argwhere(scenes.faces_region("face_x69_1e12")).astype(np.float64), 0, True)[0]
    assert np.all(far[:, 2] == 1e12)
    # the eight-fold tie around (3.5, 27.5, 43.5) goes to the lowest index, a whole voxel diagonal from the point it rounds to
    vox_next, s = np.argwhere(obj[1] > 0), np.asarray(case["spacing"])
    c = np.asarray([scenes.FACES_DIAGONAL_TIE], np.float64) + 0.5
    idx, gap, ties = rs.nearest(vox_next, c, s, case["r"])
    assert tuple(vox_next[idx[0]]) == scenes.FACES_DIAGONAL_TIE and gap[0] == 0.0 and len(ties[0]) == 8
    assert np.array_equal(np.rint(c[0]) - vox_next[idx[0]], [1, 1, 1])
    high = restated(case, nearest_highest=True)
    m = scenes.faces_region("inner_half")
    assert not np.array_equal(high["reassigned_obj"][1][m], res["reassigned_obj"][1][m])
    # d == r exactly: the strict test drops the two regions that the inclusive one keeps
    inc = restated(case, radius_inclusive=True)
    for name in ("corner_out_exact", "corner_out_exact_z"):
        assert inc["reassigned_obj"][1][scenes.faces_region(name)].all()


def changed(a, b):
    """(voxels of the two reassigned stacks that differ, rows of the running matches that differ)"""
    vox = int((a["reassigned_branch"] != b["reassigned_branch"]).sum() + (a["reassigned_obj"] != b["reassigned_obj"]).sum())
    rows = 0
    for (p, n), (p2, n2) in zip(a["running_matches"], b["running_matches"]):
        rows += abs(len(p) - len(p2)) if len(p) != len(p2) else int(((p != p2).any(axis=1) | (n != n2).any(axis=1)).sum())
    return vox, rows


MUTANT_COUNTS = {}


@pytest.mark.parametrize("rule", rs.RULES)
def test_every_rule_is_observable(rule):
    """each rule turned into its opposite changes the result of the scenes (cases changed, voxels of the two reassigned stacks,
    rows of the running matches, over the 51 cases):
      nearest_highest   (a tie of the nearest voxel goes to the highest index)   38 cases, 5791 voxels, 3288 rows
      radius_inclusive  (d <= r is kept)                                         5 cases, 189 voxels, 146 rows
      best_later        (the later candidate on equal d)                         16 cases, 0 voxels, 5577 rows
      vote_larger       (a vote tie goes to the larger label)                    21 cases, 3837 voxels, 0 rows
    The half-voxel vectors carry the nearest rule ((0, 0, 0) changes no label under it: the backward candidates at d = 0 win);
    the counts are printed, and the least a rule must do is change one case."""
    cases = vox = rows = 0
    for case in CASES:
        v, r = changed(restated(case), restated(case, **{rule: True}))
        cases += bool(v or r)
        vox += v
        rows += r
        if rule == "nearest_highest" and case["scene"] == "lattice_holes" and case["dt"] == 1.0:
            labels = int((restated(case)["reassigned_obj"][1] != restated(case, **{rule: True})["reassigned_obj"][1]).sum())
            assert labels >= (100 if case["D"] == 3 else 1) or not case["half_voxel"], (case["id"], labels)
            if case["vector"] == (0.0, 0.0, 0.0):
                assert labels == 0, (case["id"], labels)
    print(f"{rule}: {cases} cases, {vox} voxels, {rows} rows")
    assert cases >= 1 and vox + rows >= 1
    if rule in ("nearest_highest", "radius_inclusive", "vote_larger"):
        assert vox >= 1                                  # these three show in the labels, the best pair only in the matches
