"""GPU tests of the label transitions (nellie_amd.tracking.match_transitions, hipnative.Transitions, csrc/transitions.inc; DESIGN.md
section 26).  Everything is an integer and every comparison is equality, dtype and shape included, with the numpy restatement
(tests/match_transitions_restatement.py): run heads inside and across waves and workgroups, the table at its limits and through
regrowth, chunked launches, every element type, the refusals, the drops, the relabelled frame with and without a scalar tail, a
300 000-row pair, the reference-made matches of the reassign goldens through the public function and the class on files, and
run(transitions="branch") end to end."""
import os
import pickle

import numpy as np
import pytest

import match_transitions_restatement as mr
from test_hip_reassign import im_files
from test_transitions_cpu import REASSIGN, reassign_golden

pytestmark = pytest.mark.gpu
SHAPE = (3, 5, 7)                                        # 105 voxels
V = int(np.prod(SHAPE))


@pytest.fixture(scope="module")
def hip():
    from nellie_amd import build, hipnative
    build.build(verbose=False)
    lib = hipnative.load()
    assert lib.device_count() > 0, "no HIP device"
    return lib


def coords(vox, shape=SHAPE, dtype=np.uint16):
    return np.column_stack(np.unravel_index(np.asarray(vox, np.int64), shape)).astype(dtype)


def own_labels(shape=SHAPE, dtype=np.int32, first=1):
    """every voxel its own label: a row's key is then chosen by its two voxels"""
    return (np.arange(int(np.prod(shape))).reshape(shape) + first).astype(dtype)


def counted(tr, prev, nxt, A, B, **kw):
    """frames and rows through a hipnative.Transitions -> (table, n_dropped)"""
    tr.frame(A)
    tr.frame(B)
    return tr.count(prev, nxt, **kw)


def assert_same(got, want, what):
    (table, dropped), (wtable, wdropped) = got, want
    assert table.dtype == np.int64 and table.shape == wtable.shape and np.array_equal(table, wtable), (what, table.shape, wtable.shape)
    assert dropped == wdropped, (what, dropped, wdropped)


def patterns(n):
    """name -> (prev voxels, next voxels) of n rows on SHAPE under own_labels"""
    k = np.arange(n)
    rng = np.random.default_rng(n)
    lengths = rng.choice([1, 2, 3, 30, 63, 64, 65, 100, 190, 256, 300], n)
    runs = np.repeat(np.arange(len(lengths)) % 11, lengths)[:n]           # runs that straddle waves (64) and workgroups (256)
    return {"one_key": (np.full(n, 17), np.full(n, 4)), "distinct": (k % V, k // V), "alternating": (k % 2 * 9, 50 - k % 2),
            "runs": (runs * 3, 104 - runs)}


@pytest.mark.parametrize("n", (1, 63, 64, 65, 257, 4099))
def test_wave_runs(hip, n):
    from nellie_amd import hipnative
    A, B = own_labels(), own_labels(first=1000)
    with hipnative.Transitions(SHAPE) as tr:
        tr.frame(A)
        tr.frame(B)
        for name, (pv, nv) in patterns(n).items():
            prev, nxt = coords(pv), coords(nv)
            got = tr.count(prev, nxt)
            assert_same(got, mr.transition_counts(prev, nxt, A, B), (n, name))
            assert tr.n_rows == n and tr.regrown == 0 and got[0][:, 2].sum() == n
            if name == "one_key":
                assert got[0].tolist() == [[18, 1004, n]]
                assert tr.n_heads == -(-n // 64)                     # one insertion per wave, whatever its rows
            if name in ("distinct", "alternating"):
                assert tr.n_heads == n and len(got[0]) == (n if name == "distinct" else min(n, 2))
            if name == "runs":
                assert tr.n_heads < n or n < 3


def distinct_rows(m):
    k = np.arange(m)
    return coords(k % V), coords(k // V)


def test_table_regrows_from_toy_sizes(hip):
    from nellie_amd import hipnative
    A, B = own_labels(), own_labels(dtype=np.int64, first=7)
    prev, nxt = distinct_rows(100)
    want = mr.transition_counts(prev, nxt, A, B)
    with hipnative.Transitions(SHAPE) as tr:
        assert_same(counted(tr, prev, nxt, A, B, table_slots=8), want, "100 keys from 8 slots")
        assert tr.regrown == 4 and tr.table_slots == 128             # 8, 16, 32 and 64 slots cannot hold 100 keys
        assert_same(tr.count(prev, nxt, table_slots=128), want, "100 keys in 128 slots")
        assert tr.regrown == 0
        assert_same(tr.count(prev, nxt, table_slots=2, rows_per_launch=7), want, "regrowth with chunks")
        assert tr.regrown == 6
        assert_same(tr.count(prev, nxt), want, "default slots")
        assert tr.regrown == 0 and tr.table_slots == 256
        with pytest.raises(ValueError, match="power of two"):
            tr.count(prev, nxt, table_slots=100)
        prev, nxt = distinct_rows(1000)
        assert_same(tr.count(prev, nxt, table_slots=2048), mr.transition_counts(prev, nxt, A, B), "1000 keys at load 0.5")
        assert tr.regrown == 0 and tr.table_slots == 2048
        assert_same(tr.count(prev, nxt, table_slots=1024), mr.transition_counts(prev, nxt, A, B), "1000 keys in 1024 slots")
        assert tr.regrown == 0


def test_largest_key_beside_small_ones(hip):
    from nellie_amd import hipnative
    top = 2 ** 31 - 1
    for dtype in (np.int32, np.int64):
        A, B = own_labels(dtype=dtype), own_labels(dtype=dtype)
        A[2, 4, 6] = B[0, 0, 0] = top
        pv, nv = np.array([104, 104, 0, 1, 104, 5, 104]), np.array([0, 0, 0, 1, 3, 0, 0])
        prev, nxt = coords(pv), coords(nv)
        with hipnative.Transitions(SHAPE) as tr:
            got = counted(tr, prev, nxt, A, B, table_slots=8)
        assert_same(got, mr.transition_counts(prev, nxt, A, B), dtype)
        assert got[0].tolist() == [[1, top, 1], [2, 2, 1], [6, top, 1], [top, 4, 1], [top, top, 3]]


def test_chunks_count_into_one_table(hip):
    from nellie_amd import hipnative
    A, B = own_labels(), own_labels()
    A[0, 0, :3] = 0
    pv, nv = patterns(257)["runs"]
    prev, nxt = coords(pv), coords(nv)
    with hipnative.Transitions(SHAPE) as tr:
        one = counted(tr, prev, nxt, A, B)
        for step in (100, 1, 64, 256, 257, 1000):
            assert_same(tr.count(prev, nxt, rows_per_launch=step), one, f"rows_per_launch={step}")
        with pytest.raises(ValueError):
            tr.count(prev, nxt, rows_per_launch=0)
    assert_same(one, mr.transition_counts(prev, nxt, A, B), "one launch")
    assert one[1] > 0


@pytest.mark.parametrize("D", (2, 3))
def test_element_types(hip, D):
    from nellie_amd.tracking.match_transitions import transition_counts
    shape = (5, 7, 9)[3 - D:]
    rng = np.random.default_rng(D)
    n = 300
    for ldtype in (np.int32, np.int64):
        A, B = rng.integers(0, 9, shape).astype(ldtype), rng.integers(0, 9, shape).astype(ldtype)
        pv, nv = np.repeat(rng.integers(0, A.size, n // 3), 3), np.repeat(rng.integers(0, A.size, n // 3), 3)
        want = mr.transition_counts(coords(pv, shape), coords(nv, shape), A, B)
        for cdtype in (np.uint16, np.uint32, np.uint64, np.int64, np.uint8):
            got = transition_counts(coords(pv, shape, cdtype), coords(nv, shape, cdtype), A, B)
            assert_same(got, want, (D, ldtype, cdtype))
        assert_same(transition_counts(coords(pv, shape, np.uint16), coords(nv, shape, np.uint64), A.astype(np.uint8), B.astype(np.uint16)), want, "mixed")
    with pytest.raises(ValueError):
        transition_counts(coords(pv, shape), coords(nv, shape)[:-1], A, B)
    with pytest.raises(ValueError):
        transition_counts(coords(pv, shape)[:, :1], coords(nv, shape)[:, :1], A, B)
    with pytest.raises(TypeError):
        transition_counts(coords(pv, shape, np.float64), coords(nv, shape, np.float64), A, B)
    with pytest.raises(ValueError):
        transition_counts(coords(pv, shape), coords(nv, shape), A, B[..., :-1])


def test_refusals_leave_the_handle_usable(hip):
    from nellie_amd import hipnative
    A, B = own_labels(dtype=np.int64), own_labels(dtype=np.int64)
    n = 300
    pv, nv = np.arange(n) % V, (np.arange(n) * 2) % V
    prev, nxt = coords(pv), coords(nv)
    want = mr.transition_counts(prev, nxt, A, B)
    with hipnative.Transitions(SHAPE) as tr:
        for value in (2 ** 31, -1, -2 ** 40):
            for which in (0, 1):
                frames = [A.copy(), B.copy()]
                frames[which][1, 2, 3] = value                       # voxel 52: first gathered by row 52 (prev) and row 26 (next)
                with pytest.raises(ValueError, match=f"row {(52, 26)[which]} gathers a label"):
                    mr.transition_counts(prev, nxt, *frames)
                with pytest.raises(ValueError, match=f"row {(52, 26)[which]} gathers a label"):
                    counted(tr, prev, nxt, *frames)
                assert_same(counted(tr, prev, nxt, A, B), want, "after a refused label")
        tr.frame(A)
        tr.frame(B)
        for axis, extent in enumerate(SHAPE):
            for which in (0, 1):
                for step in (None, 64):
                    ends = [prev.copy(), nxt.copy()]
                    ends[which][250, axis] = extent
                    ends[which][200, axis] = extent
                    ends[1 - which][270, axis] = 65535
                    with pytest.raises(ValueError, match="row 200 "):
                        mr.transition_counts(*ends, A, B)
                    with pytest.raises(ValueError, match="row 200 holds a coordinate outside the frame"):
                        tr.count(*ends, rows_per_launch=step)
                    assert_same(tr.count(prev, nxt), want, "after a refused coordinate")
        wide = prev.astype(np.uint64)
        wide[299, 0] = 2 ** 63 + 1
        with pytest.raises(ValueError, match="row 299 "):
            tr.count(wide, nxt.astype(np.uint64))
        signed = prev.astype(np.int32)
        signed[5, 2] = -1
        with pytest.raises(ValueError, match="row 5 "):
            tr.count(signed, nxt.astype(np.int32))
        with pytest.raises(ValueError):
            tr.frame(np.zeros((3, 5, 8), np.int32))
        with pytest.raises(ValueError):
            tr.frame(np.full(SHAPE, 2 ** 63, np.uint64))
        assert_same(tr.count(prev, nxt), want, "at the end")
    with hipnative.Transitions(SHAPE) as tr:
        tr.frame(A)
        with pytest.raises(hipnative.NellieHipError):
            tr.count(prev, nxt)                                      # one frame only
    for shape in ((3,), (2, 3, 4, 5)):
        with pytest.raises(ValueError):
            hipnative.Transitions(shape)


def test_drops_and_empty(hip):
    from nellie_amd import hipnative
    from nellie_amd.tracking.match_transitions import transition_counts
    A, B = own_labels(), own_labels()
    A[0, 0, 0] = A[0, 0, 1] = 0                                      # voxels 0, 1
    B[0, 0, 1] = B[0, 0, 2] = 0                                      # voxels 1, 2
    pv = np.array([0, 0, 1, 1, 5, 5, 5, 6, 0, 1, 7])
    nv = np.array([5, 1, 1, 5, 2, 5, 5, 1, 2, 2, 7])
    prev, nxt = coords(pv), coords(nv)
    got = transition_counts(prev, nxt, A, B)
    assert_same(got, mr.transition_counts(prev, nxt, A, B), "drops")
    assert got[1] == 8 and got[0].tolist() == [[6, 6, 2], [8, 8, 1]]
    with hipnative.Transitions(SHAPE) as tr:
        none = counted(tr, prev[:0], nxt[:0], A, B)
        assert none[0].shape == (0, 3) and none[0].dtype == np.int64 and none[1] == 0 and tr.table_slots == 0        # nothing was launched
        gone = tr.count(prev[:5], nxt[:5])
        assert gone[0].shape == (0, 3) and gone[0].dtype == np.int64 and gone[1] == 5
        assert sum(tr.kernel_ms_parts().values()) > 0 and set(tr.kernel_ms_parts()) == {"clear", "count", "compact", "relabel"}
    with hipnative.Transitions(SHAPE) as tr:
        assert tr.count(prev[:0], nxt[:0])[0].shape == (0, 3)        # not even a frame is needed


def test_a_tie_goes_to_the_smaller_source(hip):
    from nellie_amd.tracking import match_transitions as mt
    A, B = own_labels(), np.full(SHAPE, 9, np.int32)
    pv = np.array([30, 30, 30, 4, 4, 4, 60, 60])                     # sources 31 and 5 tie at 3, 61 has 2: arrival order favours 31
    prev, nxt = coords(pv), coords(np.arange(8))
    table, dropped = mt.transition_counts(prev, nxt, A, B)
    assert table.tolist() == [[5, 9, 3], [31, 9, 3], [61, 9, 2]] and dropped == 0
    assert mt.best_src(table).tolist() == [[9, 5]] and mr.best_src(table) == {9: 5}
    assert mt.events(table)["fusion_dst"].tolist() == [9] and mt.events(table, min_count=4)["fusion_dst"].tolist() == []


@pytest.mark.parametrize("shape", (SHAPE, (6, 25, 28), (5, 21), (1, 1, 3), (64, 70)))
def test_relabel(hip, shape):
    """105 voxels: a scalar tail of one; 4200: none; 3 voxels: only the tail"""
    from nellie_amd import hipnative
    from nellie_amd.tracking import match_transitions as mt
    rng = np.random.default_rng(len(shape) * 1000 + shape[-1])
    size = int(np.prod(shape))
    for dtype in (np.int32, np.int64):
        A = rng.integers(0, 12, shape).astype(dtype)
        B = rng.integers(0, 40, shape).astype(dtype)
        B.flat[size - 1] = 77                                        # max(B), in the tail, with a source
        B.flat[0] = 60                                               # a label no match reaches
        nv = np.concatenate([np.nonzero((B.ravel()[:-1] > 0) & (B.ravel()[:-1] % 3 != 0))[0][::2], [size - 1]])        # labels divisible by 3 get no source
        pv = rng.integers(0, size, len(nv))
        A.flat[pv[-1]] = 11
        prev, nxt = coords(pv, shape), coords(nv, shape)
        want_table = mr.transition_counts(prev, nxt, A, B)
        with hipnative.Transitions(shape) as tr:
            got = counted(tr, prev, nxt, A, B)
            assert_same(got, want_table, (shape, dtype))
            assert tr.label_max() == 77
            best = mt.best_src(got[0])
            lut = np.zeros(78, np.int32)
            lut[best[:, 0]] = best[:, 1]
            out = tr.relabel(lut)
            want = mr.relabel(B, want_table[0])
            assert out.dtype == np.int32 and out.shape == want.shape and np.array_equal(out, want)
            assert out.flat[size - 1] == 11 and out.flat[0] == 0 and (out[B == 0] == 0).all()
            short = tr.relabel(lut[:40])                             # labels at or above the table's length become 0
            assert np.array_equal(short, np.where(B < 40, want, 0))
            keep = np.full(shape, -5, np.int32)
            assert tr.relabel(lut, out=keep) is keep and np.array_equal(keep, want)
            with pytest.raises(ValueError):
                tr.relabel(lut, out=np.zeros(shape, np.int64))
            with pytest.raises(ValueError):
                tr.relabel(np.array([0, 2 ** 31]))


def test_scale(hip):
    """300 000 rows, about half of them consecutive repeats, on a frame of 230 400 voxels with about 200 labels and a tenth
    background: runs of one, two and three rows, some 40 000 distinct keys"""
    from nellie_amd import hipnative
    shape = (24, 96, 100)
    rng = np.random.default_rng(26)
    A = (rng.integers(1, 201, shape) * (rng.random(shape) > 0.1)).astype(np.int32)
    B = (rng.integers(1, 201, shape) * (rng.random(shape) > 0.1)).astype(np.int32)
    rep = rng.choice([1, 2, 3], 160_000, p=[0.3, 0.4, 0.3])
    pv = np.repeat(rng.integers(0, A.size, len(rep)), rep)[:300_000]
    nv = np.repeat(rng.integers(0, A.size, len(rep)), rep)[:300_000]
    assert len(pv) == 300_000 and 0.4 < (pv[1:] == pv[:-1]).mean() < 0.6
    prev, nxt = coords(pv, shape), coords(nv, shape)
    want = mr.transition_counts(prev, nxt, A, B)
    a, b = mr.gather(prev, nxt, A, B)
    key = np.where((a != 0) & (b != 0), a * 2 ** 32 + b, -1)
    first = np.ones(len(key), bool)
    first[1:] = (key[1:] != key[:-1]) | (np.arange(1, len(key)) % 64 == 0)      # a run ends with its wave
    with hipnative.Transitions(shape) as tr:
        got = counted(tr, prev, nxt, A, B)
        assert_same(got, want, "scale")
        heads = tr.n_heads
        assert tr.regrown == 0 and tr.table_slots == 2 ** 20 and heads == int((first & (key >= 0)).sum()) and 0.3 * 300_000 < heads < 0.5 * 300_000
        assert_same(tr.count(prev, nxt, rows_per_launch=70_001, table_slots=2 ** 14), want, "scale, chunked, regrown")
        assert tr.regrown == 2                                       # 16 384 and 32 768 slots for some 40 000 keys
    assert want[1] > 40_000 and 32_768 < len(want[0]) <= 65_536
    print(f"scale: {len(want[0])} keys, {want[1]} dropped, {heads} heads for 300000 rows ({heads / 300000:.3f} atomic adds per row)")


# ---- the reference-made matches of the reassign goldens --------------------------------------------------------------------------
def golden_files(tmp_path, name):
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "reassign", name + ".npz"))
    stacks, matches = reassign_golden(name)
    im = im_files(tmp_path, z["branch"], z["obj"], z["flow"], z["spacing"], float(z["dt"]))
    np.save(im.pipeline_paths["voxel_matches"], np.array([[p, n] for p, n in matches], dtype=object))

    def create_output_path(key, ext=".ome.tif", for_nellie=True):
        im.pipeline_paths[key] = os.path.join(os.path.dirname(im.pipeline_paths["voxel_matches"]), key + ext)
        return im.pipeline_paths[key]
    im.create_output_path = create_output_path
    return im, stacks, matches, z


@pytest.mark.parametrize("name", REASSIGN)
def test_goldens(hip, tmp_path, name):
    from nellie_amd.tracking.match_transitions import MatchTransitions, transition_counts
    from nellie_amd.tracking import match_transitions as mt
    im, stacks, matches, z = golden_files(tmp_path, name)
    for level in ("organelle", "branch"):
        labels = stacks[level]
        want = [mr.transition_counts(p, n, labels[t], labels[t + 1]) for t, (p, n) in enumerate(matches)]
        for t, (p, n) in enumerate(matches):
            assert_same(transition_counts(p, n, labels[t], labels[t + 1]), want[t], (name, level, t))
        with MatchTransitions(im, level=level) as m:
            assert m.n_pairs == len(matches) == (1 if "empty" in name else labels.shape[0] - 1)
            for t in range(m.n_pairs):
                table = m.pair(t)
                assert_same((table, m.n_dropped[t]), want[t], (name, level, t, "class"))
                assert m.pair(t) is table and m.uploads == t + 2                # the shared frame went up once
                assert set(m.kernel_ms[t]) == {"clear", "count", "compact", "relabel"}
                ev, wev = m.events(t), mr.events(want[t][0])
                assert all(np.array_equal(ev[k], wev[k]) and ev[k].dtype == np.int64 for k in wev)
                n_src, n_dst = int(labels[t].max()), int(labels[t + 1].max())
                assert np.array_equal(m.dense(t, n_src, n_dst), mr.dense(want[t][0], n_src, n_dst))
                out = np.lib.format.open_memmap(str(tmp_path / f"{level}_{t}.npy"), mode="w+", dtype=np.int32, shape=labels.shape[1:])
                assert m.relabel(t, out=out) is out and np.array_equal(out, mr.relabel(labels[t + 1], want[t][0])) and m.uploads == t + 2
            if m.n_pairs > 1:
                m.pair(0)
                assert m.uploads == m.n_pairs + 3                                # going back takes both frames again
            with pytest.raises(ValueError, match="no stored pair"):
                m.pair(m.n_pairs)
        run = MatchTransitions(im, level=level, min_count=2)
        run.run()
        assert run.uploads == 0 and run.transitions_path == im.pipeline_paths["label_transitions"]
        with open(run.transitions_path, "rb") as f:
            saved = pickle.load(f)
        assert sorted(saved) == ["label_path", "level", "min_count", "n_dropped", "pairs"]
        assert (saved["level"], saved["min_count"], saved["label_path"]) == (level, 2, im.pipeline_paths[mt.LEVELS[level]])
        assert saved["n_dropped"] == [w[1] for w in want] and len(saved["pairs"]) == len(want)
        assert all(a.dtype == np.int64 and np.array_equal(a, w[0]) for a, w in zip(saved["pairs"], want))
    if name == "reassign_3d_converging":
        with MatchTransitions(im) as m:
            assert sum(len(m.events(t)["fusion_dst"]) for t in range(m.n_pairs)) >= 1
    # any label stack of the image's shape: the reassigned object labels the reference wrote
    path = str(tmp_path / "reassigned.npy")
    np.save(path, z["ref_obj"])
    with MatchTransitions(im, label_path=path, num_t=2) as m:
        assert m.n_pairs == 1
        assert_same((m.pair(0), m.n_dropped[0]), mr.transition_counts(*matches[0], z["ref_obj"][0], z["ref_obj"][1]), (name, "label_path"))
    os.remove(im.pipeline_paths["voxel_matches"])
    with pytest.raises(FileNotFoundError, match="voxel_matches"):
        MatchTransitions(im).pair(0)


def test_run_end_to_end(hip, tmp_path):
    from nellie_amd.im_info.verifier import ImInfo
    from nellie_amd.run import run
    from nellie_amd.synthetic import ISO_01, make_volume
    from nellie_amd.tracking.match_transitions import MatchTransitions
    vols = np.stack([make_volume((16, 48, 48), 60 + t) for t in range(3)])
    im_info = ImInfo(vols, dim_res=ISO_01, output_dir=str(tmp_path), name="transitions")
    assert run(im_info, network=True, skeletonize="hip", markers=True, tracking=True, reassign=True, transitions="branch") is im_info
    path = im_info.pipeline_paths["label_transitions"]
    assert os.path.exists(path) and path.endswith("label_transitions.pkl")
    with open(path, "rb") as f:
        saved = pickle.load(f)
    matches = np.load(im_info.pipeline_paths["voxel_matches"], allow_pickle=True)
    branch = np.asarray(im_info.get_memmap(im_info.pipeline_paths["im_skel_relabelled"]))
    with MatchTransitions(im_info, level="branch") as fresh:
        assert fresh.n_pairs == len(matches) == len(saved["pairs"]) == 2
        for t in range(fresh.n_pairs):
            table = fresh.pair(t)
            assert table.dtype == np.int64 and np.array_equal(saved["pairs"][t], table) and saved["n_dropped"][t] == fresh.n_dropped[t]
            want = mr.transition_counts(np.asarray(matches[t][0], np.uint16), np.asarray(matches[t][1], np.uint16), branch[t], branch[t + 1])
            assert_same((table, fresh.n_dropped[t]), want, ("end to end", t))
            assert len(table) > 0 and np.array_equal(fresh.relabel(t), mr.relabel(branch[t + 1], table))
    assert saved["level"] == "branch" and saved["label_path"] == im_info.pipeline_paths["im_skel_relabelled"]
