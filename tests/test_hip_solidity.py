"""GPU tests of the solidity columns (csrc/convex.inc, csrc/convex_hull.h): the convex counts of
`nellie_amd.feature_extraction.convex_counts` and of `Branches` / `Components` under `Hierarchy(..., solidity=True)`.

Every comparison is for equality: counts as integers, solidity bit for bit.  The reference is the exact restatement (b) of
tests/solidity_restatement.py, which equals the float rule through scipy on every fixture (tests/test_solidity_cpu.py); neither scipy
nor the reference is needed here."""
import glob
import os
import warnings

import numpy as np
import pytest

import branch_goldens as bg
import component_features_restatement as cr
import component_goldens as cg
import image_features_restatement as ir
import image_goldens as ig
import solidity_restatement as sr

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(HERE, "golden", "solidity", "*.npz")))
NETWORK = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(HERE, "golden", "network_steps", "*.npz")))
DTYPES = (np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.uint64, np.int64)


@pytest.fixture(scope="module")
def hip():
    from nellie_amd import build, hipnative
    build.build(verbose=False)
    lib = hipnative.load()
    assert lib.device_count() > 0, "no HIP device"
    return lib


_EXACT = {}


def exact(labels, spacing=None):
    """restatement (b) of a frame; a region shape met before (the lattice of blobs repeats a few) is counted once"""
    regs = sr.regions_of(labels)
    count = []
    for _, c, e in regs:
        key = (c.shape, c.tobytes())
        if key not in _EXACT:
            _EXACT[key] = sr.count_exact(c, e)
        count.append(_EXACT[key])
    lab, n, count = np.array([r[0] for r in regs], np.int64), np.array([len(r[1]) for r in regs], np.int64), np.array(count, np.int64)
    sp = np.ones(np.ndim(labels)) if spacing is None else np.asarray(spacing, np.float64)
    return lab, n, count, sr.solidity_of(n, count, sp)


def assert_frame(labels, spacing=None):
    """convex_counts of a frame against (b); returns the restatement's (labels, n, count, solidity)"""
    from nellie_amd.feature_extraction import convex_counts
    got, want = convex_counts(labels, spacing), exact(labels, spacing)
    for a, b, name in zip(got, want, ("labels", "n", "count", "solidity")):
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert a.tobytes() == b.tobytes(), (name, a, b)
    return want


def ball(shape, centre, radius):
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1)
    return ((g - np.asarray(centre)) ** 2).sum(axis=-1) <= radius * radius


# ---- 1. the fixtures ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_fixture(hip, name):
    from nellie_amd.feature_extraction import convex_counts
    z = np.load(os.path.join(HERE, "golden", "solidity", name + ".npz"))
    labels, n, count, solidity = convex_counts(z["labels"], z["spacing"])
    assert np.array_equal(labels, z["region_labels"]) and np.array_equal(n, z["n"]) and np.array_equal(count, z["convex_count"])
    assert count.dtype == np.int64 and solidity.dtype == np.float64 and solidity.tobytes() == z["solidity"].tobytes()


# ---- 2. the network scenes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NETWORK)
def test_network_scene(hip, name):
    z = np.load(os.path.join(HERE, "golden", "network_steps", name + ".npz"))
    for key in ("labels", "relabelled"):
        assert_frame(z[key], z["spacing"])


# ---- 3. shapes at which a kernel can go wrong ---------------------------------------------------------------------------------------
def small_shapes(D):
    """label 1 a voxel, 2 a pair, 3 a collinear triple, 4 a 2 x 2 plate, 5 a plate in an oblique plane, 6 the tetrahedron (in 2-D:
    its projection, an L of three pixels)"""
    lab = np.zeros((9, 12, 14)[3 - D:], np.int32)
    v = lab if D == 3 else lab[None]
    v[0, 0, 0] = 1
    v[0, 2, 2:4] = 2
    v[0, 4, 4:7] = 3
    v[0, 6:8, 8:10] = 4
    for k in range(4):
        v[k if D == 3 else 0, 9:12, k] = 5                             # z = x: rank 2 in 3-D
    v[-1, 0, 12] = v[-1, 1, 12] = v[-1, 0, 13] = 6
    if D == 3:
        v[-2, 0, 12] = 6
    return lab


def test_small_shapes_3d(hip):
    labels, n, count, solidity = assert_frame(small_shapes(3), (0.3, 0.1, 0.1))
    assert list(labels) == [1, 2, 3, 4, 5, 6] and list(n) == [1, 2, 3, 4, 12, 4]
    assert not count[:5].any() and np.isinf(solidity[:5]).all()
    assert count[5] >= 4 and np.isfinite(solidity[5])                  # the smallest finite 3-D case


def test_small_shapes_2d(hip):
    labels, n, count, solidity = assert_frame(small_shapes(2), (0.2, 0.1))
    assert np.isfinite(solidity).all() and (count >= n).all()
    assert solidity[0] == 1.0 and count[0] == 1                        # one pixel: its diamond holds its own centre only
    assert solidity[1] == 1.0 and solidity[3] == 1.0                   # a pair and a 2 x 2 plate are convex


def test_region_touching_all_six_faces(hip):
    lab = np.zeros((5, 6, 7), np.int16)
    lab[2, 3, :] = lab[2, :, 3] = lab[:, 3, 3] = 4                     # doubled box-relative coordinates reach -1 and 2 ext - 1
    lab[0, 0, 0] = lab[4, 5, 6] = 4
    _, _, count, _ = assert_frame(lab)
    assert 0 < count[0] < lab.size
    assert_frame(np.full((4, 5, 6), 3, np.uint8))                      # the whole frame: every lattice point
    assert exact(np.full((4, 5, 6), 3, np.uint8))[2][0] == 120


def test_c_shape_and_hollow_shell(hip):
    lab = np.zeros((12, 14, 30), np.int32)
    lab[1:11, 1:13, 1:12] = 1
    lab[2:10, 2:12, 2:11] = 0                                          # a shell: two runs of label 1 in most rows
    lab[1:6, 1:13, 14:29] = 2
    lab[1:6, 4:10, 17:29] = 0                                          # a C
    lab[3, 6, 5] = 3                                                   # a voxel inside the shell
    _, _, _, solidity = assert_frame(lab, (0.2, 0.1, 0.1))
    assert solidity[0] < 0.6 and solidity[1] < 0.8 and np.isinf(solidity[2])
    flat = np.zeros((16, 30), np.int32)
    flat[1:15, 1:14] = 1
    flat[3:13, 3:14] = 0
    flat[2:14, 16:29] = 2
    flat[4:12, 18:27] = 0                                              # a ring
    _, _, _, solidity = assert_frame(flat)
    assert (solidity < 0.8).all()


def test_ball_has_more_facets_than_a_chunk_and_more_rows_than_a_workgroup(hip):
    from nellie_amd import hipnative
    lab = ball((32, 32, 32), (15.5, 15.5, 15.5), 13.2).astype(np.int32) * 7
    want = assert_frame(lab, (0.15, 0.1, 0.1))
    limits = hipnative.convex_limits()
    with hipnative.BranchFeatures(lab.shape, (0.15, 0.1, 0.1)) as eng:
        assert eng.regions(lab, rows=True) == 1
        eng.convex()
        count, facets, rows = eng.fetch_convex(sizes=True)
        ms = eng.convex_ms_parts()
    assert count[0] == want[2][0] and want[3][0] < 1.0
    assert facets[0] > 2 * limits["facets_per_chunk"] and rows[0] > 2 * limits["rows_per_workgroup"], (facets, rows, limits)
    assert set(ms) == {"extremes", "planes", "count", "hull"} and ms["extremes"] > 0 and ms["planes"] > 0 and ms["count"] > 0


def test_wide_frame_with_a_run_longer_than_a_workgroup(hip):
    lab = np.zeros((3, 4, 300), np.int32)
    lab[1, 1, 2:299] = 5                                               # one run of 297 voxels
    lab[1, 2, 140:160] = 5
    lab[0, 1, 150] = lab[2, 2, 7] = 5
    lab[0, 3, 280:300] = 9
    lab[1, 3, 299] = lab[0, 2, 290] = 9
    assert_frame(lab, (0.3, 0.1, 0.1))


def blob_lattice():
    rng = np.random.default_rng(31)
    shapes = [rng.random((3, 3)) < p for p in (0.3, 0.5, 0.7, 0.9) for _ in range(3)]
    lab = np.zeros((4 * 50, 4 * 70), np.int32)
    k = 0
    for i in range(50):
        for j in range(70):
            k += 1
            m = shapes[rng.integers(len(shapes))].copy()
            m[1, 1] = True
            lab[4 * i:4 * i + 3, 4 * j:4 * j + 3][m] = k
    return lab


def test_more_regions_than_one_launch_covers(hip):
    from nellie_amd import hipnative
    lab = blob_lattice()
    labels, n, count, _ = assert_frame(lab, (0.1, 0.1))
    assert len(labels) == 3500 > 3 * hipnative.convex_limits()["workgroups_per_launch"] and (count >= n).all()


def test_non_consecutive_labels(hip):
    lab = small_shapes(3).astype(np.int64)
    values = np.array([0, 7, 8, 1000, 70000, 70001, 5_000_000])
    labels, *_ = assert_frame(values[lab])
    assert list(labels) == list(values[1:])


def test_empty_frame_and_one_region(hip):
    from nellie_amd.feature_extraction import convex_counts
    for shape in ((4, 5, 6), (7, 9)):
        labels, n, count, solidity = convex_counts(np.zeros(shape, np.int32))
        assert labels.shape == n.shape == count.shape == solidity.shape == (0,)
        assert count.dtype == np.int64 and solidity.dtype == np.float64
        one = np.zeros(shape, np.int32)
        one[tuple(slice(1, s - 1) for s in shape)] = 2
        _, n, count, solidity = assert_frame(one)
        assert n[0] == count[0] and solidity[0] == 1.0                 # a box is its own hull


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_every_label_dtype(hip, dtype):
    for D in (3, 2):
        lab = small_shapes(D)
        got = assert_frame(lab.astype(dtype), (0.3, 0.2, 0.1)[3 - D:])
        want = exact(lab, (0.3, 0.2, 0.1)[3 - D:])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))


def test_float_labels_are_refused(hip):
    from nellie_amd.feature_extraction import convex_counts
    with pytest.raises(TypeError):
        convex_counts(np.zeros((4, 4), np.float32))


def test_convex_needs_the_regions_frame(hip):
    from nellie_amd import hipnative
    lab = small_shapes(3)
    with hipnative.BranchFeatures(lab.shape, (0.3, 0.1, 0.1)) as eng:
        with pytest.raises(hipnative.NellieHipError):
            eng.convex()                                               # no regions yet
        eng.regions(lab)
        with pytest.raises(hipnative.NellieHipError):
            eng.fetch_convex()                                         # not taken yet
        eng.frame(lab, lab, lab)                                       # the skeleton replaces the regions' frame on the device
        with pytest.raises(hipnative.NellieHipError):
            eng.convex()


# ---- 4. arithmetic bounds -----------------------------------------------------------------------------------------------------------
def test_widest_frame(hip):
    """a region over the whole X extent the engine accepts: doubled differences near 2^16, normals near 2^33, N . p near 2^50 --
    compared with (b) only, whose integers are exact; the float rule's 1e-10 tolerance is not to be trusted at this width"""
    lab = np.zeros((3, 5, 32767), np.int32)
    for p in ((0, 0, 0), (2, 4, 32766), (0, 4, 1), (2, 0, 32765), (1, 2, 16000), (0, 3, 32766), (2, 1, 0)):
        lab[p] = 1
    lab[0:2, 0:2, 32760:32767] = 2
    lab[1, 1, 32763] = 0
    labels, n, count, solidity = assert_frame(lab, (0.3, 0.1, 0.1))
    assert list(n) == [7, 27] and count[0] > 32767 and np.isfinite(solidity).all()


# ---- 5. through the classes ---------------------------------------------------------------------------------------------------------
def run_level(cls, h):
    level = cls(h)
    level.run()
    return level


def quiet(fn):
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return fn()


@pytest.mark.parametrize("case", ["3d_aniso", "2d"])
def test_branches_components_and_image_with_solidity(hip, case):
    from nellie_amd.feature_extraction import Branches, Components, Image
    gc = cg.load("components_" + case)
    gb, base = gc["branches"], gc["base"]
    T, spacing = base["T"], base["spacing"]
    on, off = run_level(Branches, bg.double_of(gb, solidity=True)), run_level(Branches, bg.double_of(gb))
    bg.assert_same_skeleton(on, off, base)
    seen_inf = False
    for t in range(T):
        if len(off.branch_label[t]) == 0:
            assert on.branch_solidity[t] == []
            continue
        labels, _, _, want = exact(base["branch"][t], spacing)
        assert np.array_equal(on.region_label[t], labels) and on.branch_solidity[t].tobytes() == want.tobytes()
        assert np.isnan(off.branch_solidity[t]).all()
        for k in bg.REGION:
            if k != "branch_solidity":
                assert np.asarray(getattr(on, k)[t]).tobytes() == np.asarray(getattr(off, k)[t]).tobytes(), (k, t)
        assert set(on.kernel_ms[t]) == set(off.kernel_ms[t]) | {"convex", "convex_hull_host"}
        seen_inf |= bool(np.isinf(want).any())
    assert seen_inf == (base["D"] == 3)                                # a 2-D region is never flat
    # organelles: the aggregates of the branch columns, inf included, against numpy's
    h_on, h_off = cg.double_of(gc, branches=on, solidity=True), cg.double_of(gc, branches=on)
    got, plain = run_level(Components, h_on), run_level(Components, h_off)
    own = cr.Components(cg.double_of(gc, branches=on))
    quiet(own.run)
    cg.assert_same_components(got, own, base)
    cg.assert_same_components(plain, own, base)
    finite_and_inf = 0
    for t in range(T):
        if len(own.component_label[t]) == 0:
            continue
        _, _, _, want = exact(base["comp"][t], spacing)
        assert got.organelle_solidity[t].tobytes() == want.tobytes() and np.isnan(plain.organelle_solidity[t]).all()
        for k in cg.REGION:
            a, b = np.asarray(getattr(got, k)[t]), np.asarray(getattr(plain, k)[t])
            assert k == "organelle_solidity" or (a.tobytes() == b.tobytes() and cg.same(a, np.asarray(getattr(own, k)[t]))), (k, t)
        agg = got.aggregate_branch_metrics[t]["branch_solidity"]
        finite_and_inf += int(np.isinf(agg["mean"]).any() and np.isfinite(agg["max"]).any())
        assert (np.isnan(agg["std_dev"][0]) >= np.isinf(agg["mean"][0])).all()
    assert finite_and_inf > 0 or base["D"] == 2
    # the image level
    hi = ig.hierarchy_double(gc, components=got, branches=on)
    image = run_level(Image, hi)
    own_image = ir.Image(hi)
    quiet(own_image.run)
    ig.assert_same_image(image, own_image, base)
    assert any(np.isfinite(image.aggregate_component_metrics[t]["organelle_solidity"]["min"]).all() for t in range(T))


def test_run_writes_the_solidity_columns(hip, tmp_path):
    import pandas as pd
    from nellie_amd.im_info.verifier import ImInfo
    from nellie_amd.run import run
    from nellie_amd.synthetic import ISO_01, make_volume
    vols = np.stack([make_volume((16, 48, 48), 60 + t) for t in range(2)])
    im_info = ImInfo(vols, dim_res=ISO_01, output_dir=str(tmp_path), name="solid")
    run(im_info, full=True, skeletonize="hip", solidity=True)
    paths = im_info.pipeline_paths
    organelles, branches = (pd.read_csv(paths[k], float_precision="round_trip") for k in ("features_organelles", "features_branches"))
    assert len(organelles) > 0 and not organelles["organelle_solidity_raw"].isna().any()
    assert len(branches) > 0 and not branches["branch_solidity_raw"].isna().any()
    labels = np.asarray(im_info.get_memmap(paths["im_instance_label"]))
    from nellie_amd.stage import spacing_of
    want = np.concatenate([exact(labels[t], spacing_of(im_info))[3] for t in range(2)])
    assert np.array_equal(organelles["organelle_solidity_raw"].to_numpy(), want)
    for k in ("features_organelles", "features_branches"):
        os.remove(paths[k])
    from nellie_amd.feature_extraction import Hierarchy
    Hierarchy(im_info, skip_nodes=False, enable_adjacency=False).run()   # the default stays NaN
    assert pd.read_csv(paths["features_organelles"])["organelle_solidity_raw"].isna().all()


# ---- 6. repeatability ---------------------------------------------------------------------------------------------------------------
def test_one_handle_repeats_itself_and_keeps_no_stale_tables(hip):
    from nellie_amd import hipnative
    z = np.load(os.path.join(HERE, "golden", "solidity", "random_3d.npz"))
    a, b = z["labels"], small_shapes(3).astype(z["labels"].dtype)
    big = np.zeros(a.shape, a.dtype)
    big[:b.shape[0], :b.shape[1], :b.shape[2]] = b                   # fewer regions, other boxes, on the same handle
    want = {0: exact(a)[2], 1: exact(big)[2]}
    with hipnative.BranchFeatures(a.shape, z["spacing"]) as eng:
        got = []
        for k in (0, 0, 1, 0, 1):
            eng.regions((a, big)[k], rows=bool(len(got) % 2))
            eng.convex()
            got.append(eng.fetch_convex(sizes=True))
            assert np.array_equal(got[-1][0], want[k]), k
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got[0], got[1]))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got[0], got[3]))
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got[2], got[4]))
    from nellie_amd.feature_extraction import convex_counts
    first = convex_counts(a, z["spacing"])
    other = convex_counts(np.zeros((5, 40, 11), np.int32))             # a handle of another size in between
    again = convex_counts(a, z["spacing"])
    assert len(other[0]) == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(first, again))
