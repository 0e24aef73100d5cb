"""GPU tests of voxel reassignment (nellie_amd.tracking.voxel_reassignment.VoxelReassigner, csrc/reassign.inc): the reference's
goldens through the public class on files, the decisive scenes (tests/reassign_scenes.py: ties of the nearest voxel, d == r, equal
vote sums, long candidate lists, centroids outside the frame), a fixed-seed fuzz slice against the numpy restatement with no seed
left out, an analytic shift at 128 x 512 x 512, determinism, residency of the previous frame, and one file-level run behind run(markers=True, tracking=True).

Everything is compared exactly: the restatement is run on the vectors of the project's own FlowInterpolator, and from there on the
device and numpy make the same IEEE operations on the same bits in the same order."""
import glob
import os
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN_DIR
import reassign_scenes as scenes
import voxel_reassignment_restatement as rs
from test_reassign_cpu import CASES, assert_equals_reference, assert_margins_zero, radius

pytestmark = pytest.mark.gpu
GOLDENS = sorted(glob.glob(os.path.join(GOLDEN_DIR, "reassign", "reassign_*.npz")))
ids = lambda paths: [os.path.basename(p)[:-4] for p in paths]   # noqa: E731
NAMES = ("flow_vector_array", "voxel_matches", "im_skel_relabelled", "im_instance_label", "im_branch_label_reassigned", "im_obj_label_reassigned")


@pytest.fixture(scope="module")
def hip():
    from nellie_amd import build, hipnative
    build.build(verbose=False)
    lib = hipnative.load()
    assert lib.device_count() > 0, "no HIP device"
    return lib


def im_files(tmp_path, branch, obj, flow, spacing, dt=1.0):
    """an ImInfo double whose stacks are .npy files under a fresh directory of tmp_path"""
    D = branch.ndim - 1
    root = tmp_path / f"run{len(os.listdir(tmp_path))}"
    root.mkdir()
    paths = {k: str(root / (k + ".npy")) for k in NAMES}
    np.save(paths["flow_vector_array"], flow)
    np.save(paths["im_skel_relabelled"], np.asarray(branch, np.int32))
    np.save(paths["im_instance_label"], np.asarray(obj, np.int32))
    axes = "TYX" if D == 2 else "TZYX"
    dim_res = dict(zip(axes[1:], (float(s) for s in spacing)))
    dim_res["T"] = float(dt)
    stack = np.zeros((branch.shape[0],) + (4,) * D, np.uint8)

    def allocate_memory(path, dtype="float", data=None, description="", return_memmap=False, read_mode="r+"):
        mm = np.lib.format.open_memmap(path, mode="w+", dtype=np.dtype(dtype), shape=branch.shape)
        return mm if return_memmap else None
    return SimpleNamespace(no_t=False, no_z=D == 2, shape=branch.shape, axes=axes, dim_res=dim_res, im_path="im", pipeline_paths=paths,
                           get_memmap=lambda p, read_mode="r+": stack if p == "im" else np.load(p, mmap_mode=read_mode),
                           allocate_memory=allocate_memory)


def run_class(im, **kw):
    """-> (reassigned branch, reassigned obj, running_matches, the saved voxel_matches array or None)"""
    from nellie_amd.tracking.voxel_reassignment import VoxelReassigner
    vr = VoxelReassigner(im, **kw)
    vr.run()
    vr.close()
    saved = None
    if kw.get("store_running_matches", True):
        saved = np.load(im.pipeline_paths["voxel_matches"], allow_pickle=True)
    else:
        assert not os.path.exists(im.pipeline_paths["voxel_matches"])
    return (np.load(im.pipeline_paths["im_branch_label_reassigned"]), np.load(im.pipeline_paths["im_obj_label_reassigned"]),
            vr.running_matches, saved)


def restate(im, branch, obj, r, **kw):
    """the restatement on the vectors of the project's own FlowInterpolator"""
    from nellie_amd.tracking.flow_interpolation import FlowInterpolator
    fi = {True: FlowInterpolator(im), False: FlowInterpolator(im, forward=False)}
    try:
        return rs.reassign(branch, obj, None, fi[True].scaling, r,
                           interp=lambda c, t, forward: fi[forward].interpolate_coord(c.astype(np.float64), t), **kw)
    finally:
        fi[True].close()
        fi[False].close()


def assert_same(got, want, what):
    b, o, matches, _ = got
    assert np.array_equal(b, want["reassigned_branch"]), (what, "branch", int((b != want["reassigned_branch"]).sum()))
    assert np.array_equal(o, want["reassigned_obj"]), (what, "obj", int((o != want["reassigned_obj"]).sum()))
    if want["running_matches"] is not None:
        assert len(matches) == len(want["running_matches"]), what
        for (p, n), (p2, n2) in zip(matches, want["running_matches"]):
            assert p.dtype == p2.dtype and n.dtype == n2.dtype and np.array_equal(p, p2) and np.array_equal(n, n2), (what, "matches")


@pytest.mark.parametrize("path", GOLDENS, ids=ids(GOLDENS))
def test_golden(hip, tmp_path, path):
    z = np.load(path)
    name = os.path.basename(path)[:-4]
    store = bool(z["kw_store_running_matches"])
    kw = dict(store_running_matches=store, max_refine_iterations=int(z["kw_max_refine_iterations"]))
    im = im_files(tmp_path, z["branch"], z["obj"], z["flow"], z["spacing"], float(z["dt"]))
    got = run_class(im, **kw)
    assert_equals_reference(z, got[0], got[1], got[2], name + " against the reference")
    if store:
        saved = got[3]
        assert saved.shape == tuple(z["saved_shape"]) and saved.dtype == object
        assert len(saved) == int(z["n_matches"]) == len(got[2])
        for t, (p, n) in enumerate(got[2]):
            assert np.array_equal(np.asarray(saved[t][0], p.dtype), p) and np.array_equal(np.asarray(saved[t][1], n.dtype), n)
    want = restate(im, z["branch"], z["obj"], radius(z), **kw)
    assert_same(got, want, name + " against the restatement")
    print(f"{name}: {int((got[1] > 0).sum())} object and {int((got[0] > 0).sum())} branch voxels assigned, {len(got[2])} match pairs")


SPACINGS3 = [(0.107,) * 3, (0.29, 0.0973, 0.0973), (0.211, 0.083, 0.083), (0.13, 0.13, 0.13)]
SPACINGS2 = [(0.0973, 0.0973), (0.107, 0.083), (0.13, 0.11)]
FUZZ_SEEDS = range(30)


def fuzz_case(seed):
    r = np.random.default_rng([seed, 77])
    D = 2 if seed % 3 == 2 else 3
    shape = (int(r.choice([64, 90, 120])), int(r.choice([64, 100]))) if D == 2 else \
        (int(r.choice([8, 12, 16])), int(r.choice([40, 56])), int(r.choice([40, 64])))
    spacing = (SPACINGS2 if D == 2 else SPACINGS3)[int(r.integers(0, 3 if D == 2 else 4))]
    scene = dict(n_obj=int(r.integers(3, 10)), drift_um=float(r.choice([0.08, 0.16, 0.3])), rows_per_obj=int(r.choice([10, 16, 24])),
                 noise=float(r.choice([0.1, 0.4])), vanish=bool(r.integers(0, 2)), converge=bool(r.integers(0, 2)))
    if seed % 15 == 3:
        scene["empty_t"] = 2
    if seed % 15 == 8:
        scene["no_flow_t"] = 1
    return dict(D=D, shape=shape, spacing=spacing, T=int(r.integers(2, 5)), dt=float(r.choice([1.0, 1.0, 1.4])), scene=scene,
                kw=dict(store_running_matches=bool(seed % 4 != 1), max_refine_iterations=int(r.integers(1, 4))))


def test_fuzz_against_restatement(hip, tmp_path):
    """2-D and 3-D, random spacings, T, radius and keywords; every seed is compared, whatever its margins (seeds 7 and 16 have a
    best-pair tie at d = 0): both sides state the same float64 operations in the same order on the same vectors"""
    for seed in FUZZ_SEEDS:
        c = fuzz_case(seed)
        branch, obj, flow = scenes.make_scene(np.random.default_rng([seed, 78]), c["shape"], c["T"], c["spacing"], **c["scene"])
        im = im_files(tmp_path, branch, obj, flow, c["spacing"], c["dt"])
        r = max(0.5 * c["dt"], 0.5)
        want = restate(im, branch, obj, r, **dict(c["kw"], store_running_matches=True))
        print(f"fuzz {seed}: margins a {want['margin_a']:.3g} b {want['margin_b']:.3g} c {want['margin_c']:.3g} d {want['margin_d']:.3g}")
        if not c["kw"]["store_running_matches"]:
            want["running_matches"] = None
        got = run_class(im, **c["kw"])
        assert_same(got, want, f"fuzz {seed} {c}")
        print(f"fuzz {seed}: D {c['D']} T {c['T']} pairs {want['pairs']}, {int((got[1] > 0).sum())} object voxels assigned")


@pytest.mark.parametrize("case", CASES, ids=[c["id"] for c in CASES])
def test_decisive_scene(hip, tmp_path, case):
    """every scene x spacing x vector through the public class on files against the restatement on the device's own vectors: both
    stacks and every running_matches array, dtypes included, with no taint mask and no margin filter; the margins the scene is
    built for are still exactly 0 with those vectors"""
    branch, obj, flow = case["make"]()
    im = im_files(tmp_path, branch, obj, flow, case["spacing"], case["dt"])
    got = run_class(im)
    want = restate(im, branch, obj, case["r"])
    print(f"{case['id']}: margins a {want['margin_a']:.3g} b {want['margin_b']:.3g} c {want['margin_c']:.3g} d {want['margin_d']:.3g}, "
          f"{want['tie_sets']} tie sets, longest candidate list {want['max_candidates']}, {int((got[1][1] > 0).sum())} object voxels assigned")
    assert_margins_zero(case, want, "device vectors")
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and want["pairs"] == 1
    assert_same(got, want, case["id"])
    assert np.array_equal(got[0][0], branch[0]) and np.array_equal(got[1][0], obj[0])
    if case["scene"] == "crowd":
        assert want["max_candidates"] > 300
        for target, (A, B, _) in zip(scenes.CROWD_TARGETS, scenes.CROWD_LABELS):
            assert got[1][1][target] == A and got[1][1][target] != B, (target, int(got[1][1][target]))
    if case["scene"] == "faces_and_outside":             # the class came back with the 3e9 and 1e12 rows present
        assert flow[:, 4:7].max() == 1e12
        for name in scenes.FACES_REGIONS:
            m = scenes.faces_region(name)
            if name in scenes.FACES_STAY_ZERO:
                assert not got[1][1][m].any() and not got[0][1][m].any(), name
            else:
                assert got[1][1][m].all(), name


@pytest.mark.parametrize("vector", [(0.0, 0.0, 0.0), (0.0, 1.0, 2.0)], ids=["still", "whole_voxels"])
def test_handle_best_pairs_on_zero_distance_ties(hip, vector):
    """hipnative.Reassigner itself -- frame, pair, fetch(best=True) -- on lattice_holes with whole-voxel vectors.  The flow fields
    are the test's own: one row of cost 0 and a reach that spans the frame, so every query has that one neighbour and gets the
    vector exactly.  A target whose source voxel exists then has a forward and a backward candidate at d = 0, and the best pair
    is the earlier one."""
    from nellie_amd import hipnative
    branch, obj, flow = scenes.lattice_holes(3, vector)
    flow = flow[len(flow) // 2:len(flow) // 2 + 1].copy()
    flow[:, -1] = 0.0
    sp, r = (0.29, 0.0973, 0.0973), 0.5
    fw, bw, ra = hipnative.FlowField(3, sp, 64.0), hipnative.FlowField(3, sp, 64.0), hipnative.Reassigner(branch.shape[1:], sp, r)
    try:
        fw.load(flow[:, 1:4], flow[:, 4:7], flow[:, -1])
        bw.load(flow[:, 1:4] + flow[:, 4:7], flow[:, 4:7], flow[:, -1])

        def interp(coords, t, forward):
            out, found = (fw if forward else bw).interpolate(coords.astype(np.float64))
            return out if found else np.zeros((0, 3))
        want = rs.reassign(branch, obj, None, sp, r, interp=interp)
        assert ra.frame(branch[0], obj[0], seed=True) == int((obj[0] > 0).sum())
        vox_prev = ra.fetch(0)[0]
        assert ra.frame(branch[1], obj[1]) == int((obj[1] > 0).sum())
        assert ra.pair(fw, bw) > 0
        vox_next, re_b, re_o, best = ra.fetch(0, best=True)
    finally:
        for h in (fw, bw, ra):
            h.close()
    shape = branch.shape[1:]
    assert np.array_equal(vox_prev, np.flatnonzero(obj[0] > 0)) and np.array_equal(vox_next, np.flatnonzero(obj[1] > 0))
    hit = np.nonzero(best >= 0)[0]
    got_prev = np.column_stack(np.unravel_index(vox_prev[best[hit]], shape))
    got_next = np.column_stack(np.unravel_index(vox_next[hit], shape))
    (want_prev, want_next), = want["running_matches"]
    tied = want["zero_ties"][0][tuple(got_next.T)]
    moved = np.zeros(shape, bool)                        # the voxels of frame 0, moved by the vector
    moved[tuple((np.argwhere(obj[0] > 0) + np.asarray(vector, int)).T)] = True
    assert tied.sum() == int((moved & (obj[1] > 0)).sum()) >= 500 and want["margin_d"] == 0.0
    assert np.array_equal(got_next, want_next) and np.array_equal(got_prev[tied], want_prev[tied]) and np.array_equal(got_prev, want_prev)
    assert np.array_equal(re_o, want["reassigned_obj"][1].ravel()[vox_next]) and np.array_equal(re_b, want["reassigned_branch"][1].ravel()[vox_next])


def big_scene(seed, T=2, shape=(24, 96, 96), n_obj=40, **kw):
    rng = np.random.default_rng([seed, 79])
    sp = (0.211, 0.083, 0.083)
    return scenes.make_scene(rng, shape, T, sp, n_obj=n_obj, rows_per_obj=14, **kw) + (sp,)


def test_two_runs_give_identical_bits(hip, tmp_path):
    branch, obj, flow, sp = big_scene(1, T=3, converge=True)
    a = run_class(im_files(tmp_path, branch, obj, flow, sp))
    b = run_class(im_files(tmp_path, branch, obj, flow, sp))
    assert a[1][1:].any() and a[0][1:].any()
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and len(a[2]) == len(b[2]) == 2
    for (p, n), (p2, n2) in zip(a[2], b[2]):
        assert p.tobytes() == p2.tobytes() and n.tobytes() == n2.tobytes()


def test_previous_frame_stays_resident(hip, tmp_path):
    """a T = 4 run equals three T = 2 runs chained through the files: run k's first frame is what run k - 1 wrote for it.  The
    masks of the chained runs are those of the long run when every object voxel was assigned (branch labels lie inside objects),
    which the test demands of its scene."""
    for seed in range(10):
        branch, obj, flow, sp = big_scene(seed, T=4, shape=(16, 72, 72), n_obj=16, drift_um=0.1, noise=0.1)
        long = run_class(im_files(tmp_path, branch, obj, flow, sp), store_running_matches=False)
        if np.array_equal(long[1] > 0, obj > 0):
            break
    else:
        pytest.fail("no scene in which every object voxel is assigned")
    prev_b, prev_o = branch[0], obj[0]
    for t in range(3):
        rows = flow[flow[:, 0] == t].copy()
        rows[:, 0] = 0
        pair = run_class(im_files(tmp_path, np.stack([prev_b, branch[t + 1]]), np.stack([prev_o, obj[t + 1]]), rows, sp), store_running_matches=False)
        assert np.array_equal(pair[0][1], long[0][t + 1]) and np.array_equal(pair[1][1], long[1][t + 1]), t
        prev_b, prev_o = pair[0][1], pair[1][1]
    assert long[1][3].any() and long[0][3].any()


def test_analytic_shift_128x512x512(hip):
    """frame 1 is frame 0 moved by a whole-voxel vector, ids permuted, every flow row carries the vector: every centroid lands on
    a voxel at distance 0, so reassigned[1] is the moved frame 0 where a flow row is in reach and 0 elsewhere"""
    from nellie_amd.tracking.voxel_reassignment import VoxelReassigner
    rng = np.random.default_rng(3)
    shape, B, shift, sp = (128, 512, 512), 8, (2, -3, 5), (0.29, 0.107, 0.107)
    coarse = rng.random(tuple(s // B for s in shape)) < 0.07
    coarse[[0, -1]] = False; coarse[:, [0, -1]] = False; coarse[:, :, [0, -1]] = False      # images stay inside the frame
    ids_ = (np.arange(coarse.size, dtype=np.int32).reshape(coarse.shape) + 1) * coarse
    obj0 = np.kron(ids_, np.ones((B,) * 3, np.int32))
    inner = np.zeros((B,) * 3, np.int32)
    inner[2:6, 2:6, 2:6] = 1
    branch0 = np.kron(ids_, inner) * 3
    move = lambda a: np.roll(a, shift, axis=(0, 1, 2))   # noqa: E731  (nothing wraps: the border blocks are empty)
    perm = rng.permutation(coarse.size + 1).astype(np.int32) + 7
    obj1 = np.where(move(obj0) > 0, perm[move(obj0)], 0).astype(np.int32)
    branch1 = np.where(move(branch0) > 0, perm[move(obj0)] + 11, 0).astype(np.int32)
    # flow rows at the centre of every block of the lower three quarters in z, labelled or not
    cz, cy, cx = (np.arange(n // B) * B + B // 2 for n in shape)
    cz = cz[: len(cz) * 3 // 4]
    pos = np.stack(np.meshgrid(cz, cy, cx, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.float64)
    flow = np.column_stack([np.zeros(len(pos)), pos, np.tile(np.asarray(shift, float), (len(pos), 1)), rng.random(len(pos)).astype(np.float32)])
    r2 = 0.25
    near = lambda n, c, s: ((np.abs(np.arange(n)[:, None] - c[None, :]).min(axis=1)) * s) ** 2   # noqa: E731
    d2 = near(shape[0], cz, sp[0])[:, None, None] + near(shape[1], cy, sp[1])[None, :, None] + near(shape[2], cx, sp[2])[None, None, :]
    assert np.abs(d2 - r2).min() / r2 > 1e-9                                                    # nothing on the radius
    reach = d2 <= r2
    stacks = {"im_skel_relabelled": np.stack([branch0, branch1]), "im_instance_label": np.stack([obj0, obj1])}
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        paths = {k: k for k in NAMES}
        paths["flow_vector_array"] = os.path.join(tmp, "flow.npy")
        paths["voxel_matches"] = os.path.join(tmp, "matches.npy")
        np.save(paths["flow_vector_array"], flow)

        def allocate_memory(path, dtype="float", data=None, description="", return_memmap=False, read_mode="r+"):
            stacks[path] = np.zeros((2,) + shape, dtype)
            return stacks[path]
        im = SimpleNamespace(no_t=False, no_z=False, shape=(2,) + shape, axes="TZYX", dim_res=dict(Z=sp[0], Y=sp[1], X=sp[2], T=1.0), im_path="im",
                             pipeline_paths=paths, get_memmap=lambda p, read_mode="r+": stacks.get(p, np.zeros((2, 4, 4, 4), np.uint8)),
                             allocate_memory=allocate_memory)
        status = SimpleNamespace(status="")
        vr = VoxelReassigner(im, viewer=status)
        vr.run()
        vr.close()
    assert status.status == "Reassigning voxels. Frame: 1 of 2."
    for key, lab0, lab1 in (("im_obj_label_reassigned", obj0, obj1), ("im_branch_label_reassigned", branch0, branch1)):
        got = stacks[key]
        assert np.array_equal(got[0], lab0)
        want = np.where(move(reach) & (lab1 > 0), move(lab0), 0)
        assert np.array_equal(got[1], want), (key, int((got[1] != want).sum()))
        assert (want > 0).sum() > 100_000 and ((lab1 > 0) & (want == 0)).sum() > 100_000
    nvox = int((obj0 > 0).sum())
    (p, n), = vr.running_matches
    assert p.dtype == np.uint16 and np.array_equal(n.astype(np.int64) - p.astype(np.int64), np.tile(shift, (len(p), 1)))
    assert len(p) == int((move(reach) & (obj1 > 0)).sum())
    print(f"analytic: {nvox} labelled voxels per frame, {len(flow)} flow rows, device {vr.kernel_ms[0]:.2f} ms")


def test_run_tracking_then_reassign_on_files(hip, tmp_path):
    """run(markers=True, tracking=True) on a small synthetic T stack, a synthetic im_skel_relabelled (a strict subset of the
    instance labels) written by the test, then VoxelReassigner(im_info).run() against the restatement"""
    from nellie_amd.im_info.verifier import ImInfo
    from nellie_amd.run import run
    from nellie_amd.synthetic import ISO_01, make_volume
    from nellie_amd.tracking.voxel_reassignment import VoxelReassigner
    vols = np.stack([make_volume((24, 48, 48), 60 + t) for t in range(3)])
    im_info = ImInfo(vols, dim_res=ISO_01, output_dir=str(tmp_path), name="reassign")
    run(im_info, device="gpu", markers=True, tracking=True)
    paths = im_info.pipeline_paths
    obj = np.asarray(im_info.get_memmap(paths["im_instance_label"], read_mode="r")).astype(np.int32)
    zz, yy, xx = np.meshgrid(*[np.arange(n) for n in obj.shape[1:]], indexing="ij")
    branch = np.where((zz + yy + xx) % 3 == 0, obj * 2, 0).astype(np.int32)
    assert 0 < (branch > 0).sum() < (obj > 0).sum()
    im_info.allocate_memory(paths["im_skel_relabelled"], dtype="int32", data=branch, description="synthetic branch labels")
    vr = VoxelReassigner(im_info)
    vr.run()
    assert vr.shape == obj.shape and vr.spatial_shape == obj.shape[1:] and vr.match_coord_dtype is np.uint16
    assert vr.voxel_matches_path == paths["voxel_matches"] and vr.flow_interpolator_fw.forward and not vr.flow_interpolator_bw.forward
    vr.close()
    got_b = np.asarray(im_info.get_memmap(paths["im_branch_label_reassigned"], read_mode="r"))
    got_o = np.asarray(im_info.get_memmap(paths["im_obj_label_reassigned"], read_mode="r"))
    assert got_b.dtype == np.int32 and got_o.dtype == np.int32
    r = max(0.5 * (im_info.dim_res.get("T") or 1.0), 0.5)
    want = restate(im_info, branch, obj, r)
    assert_same((got_b, got_o, vr.running_matches, None), want, "files")
    saved = np.load(paths["voxel_matches"], allow_pickle=True)
    assert len(saved) == len(vr.running_matches) == want["pairs"] and want["pairs"] >= 1
    assert got_o[1].any()
