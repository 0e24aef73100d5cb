"""CPU tests of the label transitions: the numpy restatement (tests/match_transitions_restatement.py) against the
matrices the reference's `accumulate_pair_counts` made (tests/golden/transitions) and on the reference-made matches of the reassign
goldens, the host functions of nellie_amd.tracking.match_transitions against the restatement, run()'s keyword and the class where no
GPU is needed."""
import glob
import os
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import GOLDEN_DIR
import match_transitions_restatement as mr

GOLDENS = sorted(glob.glob(os.path.join(GOLDEN_DIR, "transitions", "transitions_*.npz")))
REASSIGN = ("reassign_3d_converging", "reassign_2d", "reassign_3d_empty_frame")
ids = lambda paths: [os.path.basename(p)[:-4] for p in paths]   # noqa: E731


def reassign_golden(name):
    """-> {level: label stack}, [(prev, next), ...]: the label stacks the golden recorded (the scene of its seed, as
    test_reassign_cpu.py reads them) and the matches the reference made on them"""
    z = np.load(os.path.join(GOLDEN_DIR, "reassign", name + ".npz"))
    return {"organelle": z["obj"], "branch": z["branch"]}, [(z[f"match_{t}_prev"], z[f"match_{t}_next"]) for t in range(int(z["n_matches"]))]


def test_goldens_cover_the_cases():
    zs = {os.path.basename(p)[:-4]: np.load(p) for p in GOLDENS}
    assert len(zs) >= 4 and any(len(z["src_ids"]) == 0 for z in zs.values())
    for name, z in zs.items():
        assert sorted(z.files) == ["dst_ids", "matrix", "n_dst", "n_src", "src_ids"], name
        assert z["matrix"].dtype == np.uint32 and z["matrix"].shape == (int(z["n_src"]), int(z["n_dst"])) and max(z["matrix"].shape) <= 200
        assert int(z["matrix"].sum()) == len(z["src_ids"])
    assert any((z["matrix"] > 1).any() for z in zs.values()) and all(os.path.getsize(p) < 200_000 for p in GOLDENS)


@pytest.mark.parametrize("path", GOLDENS, ids=ids(GOLDENS))
def test_restatement_reproduces_the_reference_matrix(path):
    from nellie_amd.tracking import match_transitions as mt
    z = np.load(path)
    n_src, n_dst = int(z["n_src"]), int(z["n_dst"])
    table, dropped = mr.table_of(z["src_ids"] + 1, z["dst_ids"] + 1)
    assert dropped == 0 and table.dtype == np.int64 and table.shape[1] == 3
    for fn in (mr.dense, mt.dense):
        M = fn(table, n_src, n_dst)
        assert M.dtype == np.uint32 and M.shape == z["matrix"].shape and np.array_equal(M, z["matrix"])
    # the demo's argmax line, the restated rule and the package's vectorised form agree where a destination has a source
    want = mr.best_src_by_argmax(table, n_src, n_dst)
    assert mr.best_src(table) == want
    got = mt.best_src(table)
    assert got.dtype == np.int64 and dict(zip(got[:, 0].tolist(), got[:, 1].tolist())) == want
    got = mt.best_dst(table)
    assert dict(zip(got[:, 0].tolist(), got[:, 1].tolist())) == mr.best_dst(table)
    if len(table):
        with pytest.raises(ValueError):
            mt.dense(table, int(table[:, 0].max()) - 1, n_dst)
        with pytest.raises(ValueError):
            mr.dense(table, n_src, int(table[:, 1].max()) - 1)


def test_table_is_np_unique_and_drops_zeros():
    rng = np.random.default_rng(3)
    A, B = rng.integers(0, 6, (4, 5, 6)).astype(np.int32), rng.integers(0, 6, (4, 5, 6)).astype(np.int64)
    prev = np.column_stack([rng.integers(0, n, 500) for n in A.shape]).astype(np.uint16)
    nxt = np.column_stack([rng.integers(0, n, 500) for n in A.shape]).astype(np.uint16)
    table, dropped = mr.transition_counts(prev, nxt, A, B)
    a, b = A[tuple(prev.T.astype(int))].astype(np.int64), B[tuple(nxt.T.astype(int))]
    keep = (a != 0) & (b != 0)
    pairs, counts = np.unique(np.stack([a, b], 1)[keep], axis=0, return_counts=True)
    assert dropped == int((~keep).sum()) > 0 and np.array_equal(table[:, :2], pairs) and np.array_equal(table[:, 2], counts)
    assert table[:, 2].sum() == keep.sum()
    empty, d = mr.transition_counts(prev[:0], nxt[:0], A, B)
    assert empty.shape == (0, 3) and empty.dtype == np.int64 and d == 0
    A0 = np.zeros_like(A)
    empty, d = mr.transition_counts(prev, nxt, A0, B)
    assert empty.shape == (0, 3) and d == 500


def test_restatement_refusals():
    A = np.ones((3, 5, 7), np.int64)
    rows = np.zeros((10, 3), np.uint16)
    for axis, extent in enumerate(A.shape):
        bad = rows.copy()
        bad[6, axis] = extent
        bad[8, axis] = extent
        with pytest.raises(ValueError, match="row 6 "):
            mr.transition_counts(rows, bad, A, A)
        with pytest.raises(ValueError, match="row 6 "):
            mr.transition_counts(bad, rows, A, A)
    for value in (2 ** 31, -1):
        B = A.copy()
        B[0, 0, 0] = value
        with pytest.raises(ValueError, match="label"):
            mr.transition_counts(rows, rows, A, B)
    B = A.copy()
    B[0, 0, 0] = 2 ** 31 - 1
    table, _ = mr.transition_counts(rows, rows, A, B)
    assert table.tolist() == [[1, 2 ** 31 - 1, 10]]


def test_ties_events_and_relabel_on_a_small_table():
    from nellie_amd.tracking import match_transitions as mt
    #        src dst count
    table = [[2, 5, 4], [3, 5, 4], [3, 6, 1], [4, 7, 9], [9, 5, 3]]
    assert mr.best_src(table) == {5: 2, 6: 3, 7: 4} and mt.best_src(table).tolist() == [[5, 2], [6, 3], [7, 4]]          # the tie: the smaller source
    assert mr.best_dst(table) == {2: 5, 3: 5, 4: 7, 9: 5} and mt.best_dst(table).tolist() == [[2, 5], [3, 5], [4, 7], [9, 5]]
    for min_count, fis, fus in ((1, [3], [5]), (2, [], [5]), (4, [], [5]), (5, [], [])):
        want, got = mr.events(table, min_count), mt.events(table, min_count)
        assert set(got) == set(want) == {"fission_src", "fission", "fusion_dst", "fusion"}
        for key in want:
            assert got[key].dtype == np.int64 and np.array_equal(got[key], want[key]), (min_count, key)
        assert got["fission_src"].tolist() == fis and got["fusion_dst"].tolist() == fus
    assert mt.events(table, 1)["fusion"].tolist() == [[2, 5, 4], [3, 5, 4], [9, 5, 3]] and mt.events(table, 1)["fission"].tolist() == [[3, 5, 4], [3, 6, 1]]
    B = np.array([[0, 5, 5, 6], [7, 8, 8, 0]], np.int32)
    out = mr.relabel(B, table)
    assert out.dtype == np.int32 and out.tolist() == [[0, 2, 2, 3], [4, 0, 0, 0]]          # label 8 has no counted pair: 0, where the demo paints 1


@pytest.mark.parametrize("name", REASSIGN)
@pytest.mark.parametrize("level", ("organelle", "branch"))
def test_restatement_on_the_reference_matches(name, level):
    from nellie_amd.tracking import match_transitions as mt
    stacks, matches = reassign_golden(name)
    labels = stacks[level]
    assert len(matches) == (1 if "empty" in name else labels.shape[0] - 1)
    fusions = 0
    for t, (prev, nxt) in enumerate(matches):
        table, dropped = mr.transition_counts(prev, nxt, labels[t], labels[t + 1])
        if level == "organelle":
            assert dropped == 0                          # every match lands on labelled voxels
        assert table[:, 2].sum() == len(prev) - dropped and len(table) > 0
        assert np.array_equal(table, table[np.lexsort((table[:, 1], table[:, 0]))]) and len(np.unique(table[:, :2], axis=0)) == len(table)
        ev = mt.events(table)
        fusions += len(ev["fusion_dst"])
        painted = mr.relabel(labels[t + 1], table)
        assert set(np.unique(painted).tolist()) <= set(np.unique(labels[t]).tolist()) | {0}
    if name == "reassign_3d_converging" and level == "organelle":
        assert fusions >= 1                              # two objects of frame 1 end in one of frame 2: the scene is built for it


# ---- run()'s keyword and the class without a GPU -----------------------------------------------------------------------------------
def _im_info(tmp_path, T=3):
    from nellie_amd.im_info.verifier import ImInfo
    data = np.zeros((T, 4, 8, 8) if T else (4, 8, 8), np.uint16)
    return ImInfo(data, dim_res={"X": .1, "Y": .1, "Z": .1, "T": 1.0}, output_dir=str(tmp_path), name="trans")


def _outputs(im_info):
    return sorted(k for k, p in im_info.pipeline_paths.items() if os.path.exists(p))


class _Stage:
    log = []

    def __init__(self, im_info, **kw):
        self.kw = kw

    def run(self):
        type(self).log.append((type(self).__name__, self.kw))


def _fake_stages(monkeypatch):
    from nellie_amd import run as run_mod
    from nellie_amd.feature_extraction import hierarchy
    from nellie_amd.segmentation import mocap_marking, networking
    from nellie_amd.tracking import hu_tracking, match_transitions, voxel_reassignment
    _Stage.log = []
    fake = lambda name: type(name, (_Stage,), {})   # noqa: E731
    monkeypatch.setattr(run_mod, "Filter", fake("Filter"))
    monkeypatch.setattr(run_mod, "Label", fake("Label"))
    for mod, name in ((networking, "Network"), (mocap_marking, "Markers"), (hu_tracking, "HuMomentTracking"), (voxel_reassignment, "VoxelReassigner"),
                      (match_transitions, "MatchTransitions"), (hierarchy, "Hierarchy")):
        monkeypatch.setattr(mod, name, fake(name))
    return run_mod


def test_run_transitions_needs_the_matches_before_any_stage(tmp_path, monkeypatch):
    from nellie_amd import run as run_mod
    im_info = _im_info(tmp_path)
    monkeypatch.setattr(run_mod, "Filter", None)             # run() must not get as far as building a stage
    for value in (True, "organelle", "branch"):
        with pytest.raises(FileNotFoundError) as exc:
            run_mod.run(im_info, transitions=value)
        assert "'voxel_matches'" in str(exc.value) and "run(transitions=True)" in str(exc.value) and "reassign=True" in str(exc.value)
    with pytest.raises(FileNotFoundError) as exc:            # reassign=True would write the matches, but needs files of its own
        run_mod.run(im_info, transitions=True, reassign=True)
    assert "run(reassign=True)" in str(exc.value)
    for value in ("node", "voxel", 1.5):
        with pytest.raises(ValueError, match="transitions must be"):
            run_mod.run(im_info, transitions=value)
    assert _outputs(im_info) == []


def test_run_orders_transitions_behind_the_reassigner_and_full_leaves_it_off(tmp_path, monkeypatch):
    import inspect
    run_mod = _fake_stages(monkeypatch)
    assert inspect.signature(run_mod.run).parameters["transitions"].default is False
    im_info = _im_info(tmp_path)
    thin = lambda mask: mask   # noqa: E731
    run_mod.run(im_info, full=True, skeletonize=thin)
    assert [n for n, _ in _Stage.log] == ["Filter", "Label", "Network", "Markers", "HuMomentTracking", "VoxelReassigner", "Hierarchy"]
    _Stage.log.clear()
    run_mod.run(im_info, network=True, skeletonize=thin, markers=True, tracking=True, reassign=True, transitions="branch", device="gpu")
    assert [n for n, _ in _Stage.log] == ["Filter", "Label", "Network", "Markers", "HuMomentTracking", "VoxelReassigner", "MatchTransitions"]
    assert _Stage.log[-1][1] == {"level": "branch", "device": "gpu"}
    _Stage.log.clear()
    run_mod.run(im_info, full=True, skeletonize=thin, transitions=True)
    assert [n for n, _ in _Stage.log][-3:] == ["VoxelReassigner", "MatchTransitions", "Hierarchy"] and _Stage.log[-2][1]["level"] == "organelle"
    _Stage.log.clear()
    os.makedirs(tmp_path / "still", exist_ok=True)
    still = _im_info(tmp_path / "still", T=0)                # no T: skipped, as tracking and the reassigner are, and nothing is asked for
    run_mod.run(still, transitions=True)
    assert [n for n, _ in _Stage.log] == ["Filter", "Label"]


def _fake_info(tmp_path, no_t=False):
    names = ("voxel_matches", "im_skel_relabelled", "im_instance_label")
    paths = {k: str(tmp_path / (k + ".npy")) for k in names}

    def boom(*a, **kw):
        raise AssertionError("must not touch files")
    return SimpleNamespace(no_t=no_t, no_z=False, shape=(3, 4, 8, 8), axes="TZYX", im_path="im", dim_res={"X": .1, "Y": .1, "Z": .3, "T": 1.0},
                           pipeline_paths=paths, get_memmap=boom, allocate_memory=boom, create_output_path=boom)


def test_class_keywords_and_device_errors(tmp_path):
    from nellie_amd.tracking.match_transitions import MatchTransitions, transition_counts
    from nellie_amd.tracking import match_transitions as mt
    assert MatchTransitions is mt.MatchTransitions and transition_counts is mt.transition_counts
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        MatchTransitions(_fake_info(tmp_path), device="cpu")
    with pytest.raises(ValueError, match="Unsupported device"):
        MatchTransitions(_fake_info(tmp_path), device="tpu")
    with pytest.raises(ValueError, match="level must be"):
        MatchTransitions(_fake_info(tmp_path), level="node")
    m = MatchTransitions(_fake_info(tmp_path), level="branch", min_count=3, num_t=2)
    assert (m.level, m.min_count, m.num_t, m.device_index, m.label_path, m.uploads) == ("branch", 3, 2, 0, None, 0)
    m.close()
    still = MatchTransitions(_fake_info(tmp_path, no_t=True), num_t=5)
    assert still.num_t == 1 and still.run() is None          # a stack without T: logs and returns
    assert not os.listdir(tmp_path)


def test_a_failed_upload_is_not_counted_as_resident():
    """the binding's `resident` follows the device: a failed frame() costs the "prev" slot, "next" stays, and count() asks for two"""
    from nellie_amd import hipnative
    tr = object.__new__(hipnative.Transitions)
    tr.ndim, tr.shape, tr.frames, tr.resident = 3, (2, 3, 4), 0, 0
    fail = []

    def call(name, *args):
        if fail:
            raise MemoryError("HIP out of memory: upload")
    tr._call = call
    frame = np.zeros(tr.shape, np.int32)
    tr.frame(frame)
    tr.frame(frame)
    tr.frame(frame)
    assert (tr.frames, tr.resident) == (3, 2)
    fail.append(1)
    with pytest.raises(MemoryError):
        tr.frame(frame)
    assert (tr.frames, tr.resident) == (3, 1)
    fail.clear()
    rows = np.zeros((1, 3), np.uint16)
    with pytest.raises(hipnative.NellieHipError, match="fewer than two"):
        tr.count(rows, rows)
    tr.frame(frame)
    assert (tr.frames, tr.resident) == (4, 2)
    tr._h = None                                             # nothing to destroy


def test_class_without_gpu_raises(tmp_path, monkeypatch):
    from nellie_amd.tracking.match_transitions import MatchTransitions, transition_counts
    from nellie_amd.utils import adaptive_run
    monkeypatch.setattr(adaptive_run, "gpu_available", lambda: False)
    with MatchTransitions(_fake_info(tmp_path)) as m:
        for call in (m.run, lambda: m.pair(0), lambda: m.relabel(0), lambda: m.events(0), lambda: m.dense(0, 3, 3)):
            with pytest.raises(RuntimeError, match="GPU backend requested but"):
                call()
    frame = np.zeros((2, 3, 4), np.int32)
    with pytest.raises(RuntimeError, match="GPU backend requested but"):
        transition_counts(np.zeros((1, 3), np.uint16), np.zeros((1, 3), np.uint16), frame, frame)
    assert not os.listdir(tmp_path)
