"""GPU tests of LabelTracks (nellie_amd.tracking.all_tracks_for_label.LabelTracks, csrc/tracks.inc): the reference's goldens
through the public class, a fixed-seed fuzz slice and bit-exact cases against the numpy restatement, the sizes at which the kernels
change wave, workgroup or scan chunk, the mask cache, determinism and one run on the files run(full=True) leaves.

Bound: ids, frames and the row order identical; coordinates within the flow bound per step (flow_interpolation_restatement.tolerance
with the scene's largest neighbour count and largest |vector component|) times the number of steps behind a coordinate.  The scenes
clear 1e-9 of the radius and of every half-integer (test_label_tracks_cpu.py), so both sides lose and drop the same rows."""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN_DIR
import flow_interpolation_restatement as rs
import label_tracks_restatement as lrs
import label_tracks_scenes as sc
from test_label_tracks_cpu import compare_with_reference, golden_bound, golden_kw

pytestmark = pytest.mark.gpu
GOLDENS = sorted(glob.glob(os.path.join(GOLDEN_DIR, "label_tracks", "label_tracks_*.npz")))
ids = lambda paths: [os.path.basename(p)[:-4] for p in paths]   # noqa: E731


@pytest.fixture(scope="module")
def hip():
    from nellie_amd import build, hipnative
    build.build(verbose=False)
    lib = hipnative.load()
    assert lib.device_count() > 0, "no HIP device"
    return lib


def tracker(tmp_path, flow, labels, spacing, **kw):
    from nellie_amd.tracking.all_tracks_for_label import LabelTracks
    lt = LabelTracks(sc.im_double(tmp_path, flow, labels, spacing), **kw)
    lt.initialize()
    return lt


def assert_rows(got, frame_num, want, bound, what):
    """got against the restatement's (rows, frame_num, info) in exact row order"""
    rows, fn, _ = want
    assert got.dtype == np.float64 and frame_num.dtype == np.int64 and got.shape == rows.shape, (what, got.shape, rows.shape)
    assert np.array_equal(frame_num, got[:, 1]), (what, "frame_num is not column 1")
    assert np.array_equal(got[:, :2], rows[:, :2]) and np.array_equal(frame_num, fn), (what, "ids, frames or order differ")
    err = float(np.abs(got[:, 2:] - rows[:, 2:]).max(initial=0.0))
    print(f"{what}: {len(got)} rows, max err {err:.3g}, bound {bound:.3g}")
    assert err <= bound, (what, err, bound)


def assert_rows_off_the_edges(got, frame_num, want, bound, what):
    """For a scene that the pipeline made, where integer vectors on a round spacing put squared distances on the radius and
    coordinates on half-integers: a track that comes within 1e-9 of a half-integer may be decided either way from there on, so its
    id is left out on both sides; every other row is held to assert_rows' rule, order included.  Such ids stay a small share."""
    rows, _, info = want
    raw = info["raw"]
    pos = raw[:, 2:]
    near = np.abs(pos - np.floor(pos) - 0.5).min(axis=1) <= sc.MARGIN
    edge_ids = np.unique(raw[near, 0])
    assert len(edge_ids) <= 0.05 * len(np.unique(raw[:, 0])) + 1, (what, len(edge_ids))
    keep_got, keep_want = ~np.isin(got[:, 0], edge_ids), ~np.isin(rows[:, 0], edge_ids)
    print(f"{what}: {len(edge_ids)} ids on an edge left out, radius margin {info['radius_margin']:.3g}, half margin {info['half_margin']:.3g}")
    assert_rows(got[keep_got], frame_num[keep_got], (rows[keep_want], want[1][keep_want], info), bound, what)


@pytest.mark.parametrize("path", GOLDENS, ids=ids(GOLDENS))
def test_golden(hip, tmp_path, path):
    z = np.load(path)
    name, kw = os.path.basename(path)[:-4], golden_kw(z)
    maxd = float(z["max_distance_um"])
    want = lrs.label_tracks(z["labels"], z["flow"], z["spacing"], sc.radius(maxd, float(z["dt"])), **kw)
    bound = golden_bound(z, want[2]["steps"])
    with tracker(tmp_path, z["flow"], z["labels"], z["spacing"]) as lt:
        rows, frame_num = lt.run_arrays(max_distance_um=maxd, **kw)
        tracks, props = lt.run(max_distance_um=maxd, **kw)
    compare_with_reference(rows, frame_num, z, want[2]["steps"], name + " run_arrays against the reference")
    assert_rows(rows, frame_num, want, bound, name + " run_arrays against the restatement")
    assert isinstance(tracks, list) and list(props) == ["frame_num"] and isinstance(props["frame_num"], list)
    assert all(type(v) is int for v in tracks[0][:2]) and all(type(v) is float for v in tracks[0][2:]) and type(props["frame_num"][0]) is int
    assert np.array_equal(np.asarray(tracks, float), rows) and np.array_equal(props["frame_num"], frame_num)
    compare_with_reference(tracks, props["frame_num"], z, want[2]["steps"], name + " run against the reference")


@pytest.mark.parametrize("k", range(sc.N_FUZZ))
def test_fuzz_against_restatement(hip, tmp_path, k):
    case = sc.fuzz_case(k)
    want, kw = case["want"], case["kw"]
    assert want[2]["radius_margin"] > sc.MARGIN and want[2]["half_margin"] > sc.MARGIN
    bound = max(1, want[2]["steps"]) * rs.tolerance(max(1, want[2]["kmax"]), case["vmax"])
    with tracker(tmp_path, case["flow"], case["labels"], case["spacing"]) as lt:
        rows, frame_num = lt.run_arrays(max_distance_um=case["maxd"], **kw)
        tracks, props = lt.run(max_distance_um=case["maxd"], **kw)
    assert_rows(rows, frame_num, want, bound, f"fuzz {k} (seed {case['seed']}, {len(want[2]['raw'])} rows tracked)")
    if not want[2]["ran"]:
        assert (tracks, props) == ([], {})
    else:
        assert props == {"frame_num": frame_num.tolist()} and np.array_equal(np.asarray(tracks, float).reshape(rows.shape), rows)


@pytest.mark.parametrize("D", (2, 3))
@pytest.mark.parametrize("forward", (True, False), ids=("forward", "backward"))
def test_exact_cases_bit_for_bit(hip, tmp_path, D, forward):
    """one neighbour of weight exactly 1, vectors that are multiples of 0.5, integer seeds: x.5 between a labelled and an
    unlabelled voxel for even and odd x, -0.5 at the lower faces, shape - 0.5 at the upper ones (label_tracks_scenes.EXACT_2D)"""
    labels, flow, spacing, start, keep = sc.exact_scene(D, forward)
    want = lrs.label_tracks(labels, flow, spacing, 0.5, start_frame=start)
    with tracker(tmp_path, flow, labels, spacing) as lt:
        rows, frame_num = lt.run_arrays(start_frame=start)
    assert rows.tobytes() == want[0].tobytes() and np.array_equal(frame_num, want[1])
    landed = rows[rows[:, 1] != start]
    assert landed[:, 0].astype(int).tolist() == [n for n, stays in enumerate(keep) if stays]


@pytest.mark.parametrize("n", sc.BOUNDARY_COUNTS)
def test_kernel_boundaries(hip, tmp_path, n):
    """A frame of 8 x 192 x 192 voxels (4 608 mask words: two scan workgroups) with n seeds, one below, at and one above the
    ballot word (64), the block of the seed, update, emit, filter and compaction kernels (256 lanes each) and one scan workgroup
    of kept-words (4096 x 64); 100 and 1000 leave a partial last ballot word.  Sparse flow: coordinates are lost in mid-array
    and the rows of a step are fewer than the seeds."""
    labels, flow, want = sc.boundary_case(n)
    info = want[2]
    assert info["half_margin"] > sc.MARGIN and len(lrs.seeds(labels, 1)) == n
    with tracker(tmp_path, flow, labels, sc.BOUNDARY_SPACING) as lt:
        rows, frame_num = lt.run_arrays(start_frame=1)
    # one step from integer seeds in each direction: the device forms the same float64 distances, so membership is identical
    assert_rows(rows, frame_num, want, rs.tolerance(max(1, info["kmax"]), 5.0), f"{n} seeds, {len(info['raw'])} rows tracked")
    assert 0 < len(rows) < len(info["raw"]) < 4 * n


def all_starts(lt, **kw):
    out = []
    for start in range(sc.T):
        rows, frame_num = lt.run_arrays(start_frame=start, **kw)
        out.append(rows.tobytes() + frame_num.tobytes())
    return out


def test_mask_cache_sizes_give_the_same_bytes(hip, tmp_path):
    """max_masks of 1 and 2 over runs from every start frame, twice round, give the bytes of an unbounded cache"""
    case = sc.fuzz_case(2)
    results = {}
    for max_masks in (None, 1, 2):
        with tracker(tmp_path, case["flow"], case["labels"], case["spacing"], max_masks=max_masks) as lt:
            results[max_masks] = all_starts(lt, max_distance_um=case["maxd"]) + all_starts(lt, max_distance_um=case["maxd"], label_num=1)
            assert len(lt._masks) <= (max_masks or sc.T)
    assert any(len(b) > 0 for b in results[None])
    assert results[1] == results[None] and results[2] == results[None]
    assert results[None][:sc.T] != results[None][sc.T:]


def test_determinism_and_cleanup(hip, tmp_path):
    """two objects and two runs of one object give identical bytes; close() twice is harmless; a closed object runs again"""
    case = sc.fuzz_case(5)
    a = tracker(tmp_path, case["flow"], case["labels"], case["spacing"])
    b = tracker(tmp_path, case["flow"], case["labels"], case["spacing"])
    first, second, other = all_starts(a, skip_coords=2), all_starts(a, skip_coords=2), all_starts(b, skip_coords=2)
    assert first == second == other and any(len(x) > 0 for x in first)
    assert set(a.kernel_ms) == {"mask", "seed", "flow", "step", "filter", "compact"}
    a.close()
    a.close()
    b.close()
    assert all_starts(a, skip_coords=2) == first
    a.close()


def test_empty_results(hip, tmp_path):
    """([], {}) exactly where the reference returns it, (0, 2 + D) arrays everywhere nothing is left"""
    case = sc.fuzz_case(0)
    D = case["labels"].ndim - 1
    with tracker(tmp_path, case["flow"], case["labels"], case["spacing"]) as lt:
        for kw in (dict(start_frame=sc.T), dict(label_num=12345), dict(label_num=2.5), dict(label_num=2 ** 40), dict(start_frame=0, end_frame=0)):
            assert lt.run(**kw) == ([], {}), kw
            rows, frame_num = lt.run_arrays(**kw)
            assert rows.shape == (0, 2 + D) and rows.dtype == np.float64 and frame_num.shape == (0,) and frame_num.dtype == np.int64
        empty = np.zeros_like(case["flow"][:0])
    with tracker(tmp_path, empty, case["labels"], case["spacing"]) as lt:      # both directions run, nothing is tracked
        assert lt.run(start_frame=1) == ([], {"frame_num": []})
        with pytest.raises(ValueError):
            lt.run(skip_coords=0)
        with pytest.raises(ValueError):
            lt.run(start_frame=-1)


def test_row_buffers_that_do_not_fit_name_skip_coords(hip, tmp_path, monkeypatch):
    """the row buffers are sized before any step: what cannot fit raises MemoryError naming skip_coords"""
    from nellie_amd.utils import adaptive_run
    case = sc.fuzz_case(2)
    with tracker(tmp_path, case["flow"], case["labels"], case["spacing"]) as lt:
        want = lt.run_arrays(start_frame=2)[0]
        monkeypatch.setattr(adaptive_run, "get_gpu_free_bytes", lambda device=0: 4096)
        with pytest.raises(MemoryError, match="skip_coords"):
            lt.run_arrays(start_frame=2)
        monkeypatch.undo()
        assert np.array_equal(lt.run_arrays(start_frame=2)[0], want) and len(want) > 0


def test_label_dtypes(hip, tmp_path):
    """label stacks of other integer types run through exact casts; a lossy cast is refused"""
    case = sc.fuzz_case(2)
    got = {}
    for dtype in (np.int32, np.uint8, np.uint16, np.int64, np.float32):
        with tracker(tmp_path, case["flow"], case["labels"].astype(dtype), case["spacing"]) as lt:
            got[dtype] = lt.run_arrays(start_frame=1, max_distance_um=case["maxd"])[0].tobytes()
    assert len(set(got.values())) == 1 and len(got[np.int32]) > 0
    with tracker(tmp_path, case["flow"], case["labels"] + 2.0 ** 40, case["spacing"]) as lt:
        with pytest.raises(ValueError, match="refusing a cast"):
            lt.run_arrays(start_frame=1)


def test_handle_refuses_calls_out_of_order(hip):
    from nellie_amd import hipnative
    with hipnative.LabelTrackSet((4, 8, 8), mask_slots=2) as ts:
        labels = np.zeros((4, 8, 8), np.int32)
        labels[1, 2, 3] = 4
        with pytest.raises(hipnative.NellieHipError):
            ts.seed(0)                                              # the slot holds no frame
        with pytest.raises(ValueError):
            ts.mask(2, labels)                                      # no such slot
        with pytest.raises(ValueError):
            ts.seed(0, label=4)                                     # seeding by label needs the frame
        assert ts.seed(0, labels=labels) == 1 and ts.seed(0) == 1 and ts.seed(0, labels=labels, label=3) == 0
        with pytest.raises(hipnative.NellieHipError):
            ts.begin(1, 1)                                          # no seeds
        assert ts.seed(1, labels=labels, label=4, skip=7) == 1
        with pytest.raises(hipnative.NellieHipError):
            ts.step(None, False, True, 0, 1)                        # before begin
        ts.begin(1, 0, id0=3)
        assert ts.step(None, False, True, 0, 1) == 0 and ts.finish() == 0 and ts.fetch().shape == (0, 5)
    ts.close()


def test_on_the_files_of_a_full_run(hip, tmp_path):
    """run(full=True) on a small synthetic T stack, then LabelTracks on im_instance_label and on im_obj_label_reassigned, against
    the restatement fed from the same files"""
    from nellie_amd.im_info.verifier import ImInfo
    from nellie_amd.run import run
    from nellie_amd.synthetic import ISO_01, make_volume
    from nellie_amd.tracking.all_tracks_for_label import LabelTracks
    vols = np.stack([make_volume((24, 48, 48), 60 + t) for t in range(3)])
    im_info = ImInfo(vols, dim_res=ISO_01, output_dir=str(tmp_path), name="tracks")
    run(im_info, device="gpu", full=True, skeletonize="hip")
    flow = np.load(im_info.pipeline_paths["flow_vector_array"]).astype(np.float64)
    sp = (im_info.dim_res["Z"], im_info.dim_res["Y"], im_info.dim_res["X"])
    r = max(0.5 * (im_info.dim_res.get("T") or 1.0), 0.5)
    vmax = float(np.abs(flow[:, 4:7]).max())
    total = 0
    for key in ("im_instance_label", "im_obj_label_reassigned"):
        labels = np.asarray(im_info.get_memmap(im_info.pipeline_paths[key], read_mode="r"))
        assert labels.any()
        with LabelTracks(im_info, label_im_path=None if key == "im_instance_label" else im_info.pipeline_paths[key]) as lt:
            lt.initialize()
            assert lt.label_im_path == im_info.pipeline_paths[key] and lt.num_t == 3 and lt.label_memmap.shape == labels.shape
            for kw in (dict(start_frame=1, skip_coords=5), dict(start_frame=0, label_num=int(labels[0].max()))):
                want = lrs.label_tracks(labels, flow, sp, r, **kw)
                rows, frame_num = lt.run_arrays(**kw)
                bound = want[2]["steps"] * rs.tolerance(max(1, want[2]["kmax"]), max(1.0, vmax))
                if want[2]["radius_margin"] > sc.MARGIN and want[2]["half_margin"] > sc.MARGIN:
                    assert_rows(rows, frame_num, want, bound, f"{key} {kw}")
                else:
                    assert_rows_off_the_edges(rows, frame_num, want, bound, f"{key} {kw}")
                total += len(rows)
    assert total > 0
