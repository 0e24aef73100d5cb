"""
GPU tests (-m gpu) of the paths of Label that ordinary frames never take: the voxel-level fallback (rows beyond 65535 voxels, a
run set beyond the scratch capacity n // 2, NELLIE_LABEL_VOXEL), the overflow machinery that leads to it in both counting modes,
and the row widths at which the run kernels change over.  Scenes: label_scenes.py; test_label_scenes_cpu.py proves on the CPU that
each scene reaches what it is named for, and that the oracle used here equals the scipy pipeline on it.

Every comparison is np.array_equal on the whole int32 volume plus the label count, and nl_ctx_info("last_label_path") must name
the path the capacity rule predicts -- a scene that quietly stopped overflowing would fail, not pass.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import label_scenes as ls
from conftest import FILTER_CASES, LABEL_ONLY_CASES, load_golden

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILLS = (True, False)


# ---------------------------------------------------------------------------------------------- scenes and references, built once
@functools.lru_cache(maxsize=None)
def _capacity():
    return {name: (mask, min_areas, path) for name, mask, min_areas, path, _ in ls.capacity_cases()}


@functools.lru_cache(maxsize=None)
def _topology():
    return {name: (mask, min_areas) for name, mask, min_areas in ls.topology_cases()}


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(mask, min_areas) of a scene by name"""
    if name in _capacity():
        return _capacity()[name][:2]
    if name in _topology():
        return _topology()[name]
    if name.startswith("ruler-"):
        return ls.ruler(int(name[6:])), (1, 3)
    if name.startswith("ordinary-"):
        return ls.ordinary(tuple(int(s) for s in name[9:].split("x"))), (2,)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _frame(name):
    fr = ls.frangi_of(_scene(name)[0])
    fr.setflags(write=False)
    return fr


@functools.lru_cache(maxsize=None)
def _ref(name, min_area, fill):
    ref = ls.oracle_labels(_frame(name), min_area, fill)
    ref.setflags(write=False)
    return ref


@functools.lru_cache(maxsize=None)
def _path(name, min_area, fill):
    return ls.expected_path(_scene(name)[0], min_area, fill)


def _ordinary_name(shape):
    return "ordinary-" + "x".join(str(int(s)) for s in shape)


@pytest.fixture(scope="module")
def pipes(hip):
    from nellie_amd.pipeline import FramePipeline
    cache = {}

    def get(shape):
        shape = tuple(int(s) for s in shape)
        if shape not in cache:
            cache[shape] = FramePipeline(shape)
        return cache[shape]
    yield get
    for p in cache.values():
        p.close()


def _label_and_check(pipe, name, min_area, fill, when=""):
    pipe.upload_frangi(_frame(name))
    n = pipe.label(ls.THR, min_area, fill)
    got = pipe.download_labels()
    ref = _ref(name, min_area, fill)
    what = (name, min_area, fill, when)
    assert int(pipe.ctx.info("last_label_path")) == _path(name, min_area, fill), what
    assert got.dtype == np.int32 and got.shape == ref.shape, what
    assert np.array_equal(got, ref), (what, int((got != ref).sum()))
    assert n == int(ref.max()), what


def _run_scene(pipes, name):
    """every (fill, min_area) of the scene; the first one twice in a row, and once more after an ordinary frame on the same
    pipeline: neither the overflow flag nor half-written scratch of one frame may reach the next, in either direction"""
    mask, min_areas = _scene(name)
    pipe = pipes(mask.shape)
    params = [(a, f) for f in FILLS for a in min_areas]
    _label_and_check(pipe, name, *params[0])
    for a, f in params:
        _label_and_check(pipe, name, a, f, "again" if (a, f) == params[0] else "")
    plain = _ordinary_name(mask.shape)
    _label_and_check(pipe, plain, 2, True, "after the scene")
    if mask.shape[2] <= 65535:
        assert _path(plain, 2, True) == ls.PATH_RUNS
    _label_and_check(pipe, name, *params[0], "after an ordinary frame")


# ---------------------------------------------------------------------------------------------- in process, default switches
@pytest.mark.parametrize("name", [c[0] for c in ls.capacity_cases()])
def test_capacity_scenes(name, pipes):
    """Groups a, b, c: the run set of the first labelling or of the hole fill exceeds n // 2 (path 2, the voxel kernels answer), or
    fills the scratch exactly / stays one run below the overflow (path 0)."""
    mask, min_areas, path = _capacity()[name]
    for fill in FILLS:
        for a in min_areas:
            want = path if path is not None else (ls.PATH_OVERFLOW if fill else ls.PATH_RUNS)     # overflow_bg: only the hole fill overflows
            assert _path(name, a, fill) == want
    _run_scene(pipes, name)


@pytest.mark.parametrize("nx", ls.RULER_WIDTHS)
def test_ruler_widths(nx, pipes):
    """Group d: one frame per change-over of the run kernels (P of the wave count, staged / unstaged emission, wave / per-thread
    count), the widest row a run's 16-bit fields hold (path 0) and the first two they do not (path 1)."""
    name = "ruler-%d" % nx
    for fill in FILLS:
        for a in _scene(name)[1]:
            assert _path(name, a, fill) == (ls.PATH_RUNS if nx <= 65535 else ls.PATH_WIDE)
    _run_scene(pipes, name)


@pytest.mark.parametrize("name", list(ls.TOPOLOGY) + ["specks"])
def test_topology_scenes(name, pipes):
    """Groups e, f on the run-level path: min_area at the largest component's area and one above (a union-find that loses one
    union drops or keeps the wrong object), specks with more roots per 4096 runs than rl_area_kernel's table holds."""
    _run_scene(pipes, name)


def test_frame_beyond_the_grid_limits_is_refused(hip):
    """The voxel kernels launch a (x, ny, nz) grid.  A frame with more rows per plane than a grid has in y is refused on the host,
    as an argument error with a message and before any launch: today by nl_ctx_create's own bound of 65535 rows and planes, and by
    label_run_voxels against the device's limits should that bound ever move.  The comb would overflow, so it would get there."""
    from nellie_amd.pipeline import FramePipeline
    shape = (2, 70000, 3)
    mask = ls.overflow_fg(shape)
    assert ls.runs(mask) > ls.cap(mask)
    pipe = None
    try:
        with pytest.raises(ValueError, match="65535|limits"):
            pipe = FramePipeline(shape)
            pipe.upload_frangi(ls.frangi_of(mask))
            pipe.label(ls.THR, 1, True)
    finally:
        if pipe is not None:
            pipe.close()


# ---------------------------------------------------------------------------------------------- child processes: the static switches
CHILD = r"""
import glob, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from nellie_amd.pipeline import FramePipeline
pipes = {}
for path in sorted(glob.glob(os.path.join(sys.argv[2], "case_*.npz"))):
    c = np.load(path)
    fr, ref = c["fr"], c["ref"]
    if fr.shape not in pipes:
        pipes[fr.shape] = FramePipeline(fr.shape)
    pipe = pipes[fr.shape]
    pipe.upload_frangi(fr)
    thr = None if np.isnan(c["thr"]) else np.float32(c["thr"])
    n = pipe.label(thr, int(c["min_area"]), bool(c["fill"]))
    got = pipe.download_labels()
    used = int(pipe.ctx.info("last_label_path"))
    ok = got.dtype == np.int32 and np.array_equal(got, ref) and n == int(ref.max()) and used == int(c["path"])
    print("VERDICT", "ok" if ok else "FAIL", str(c["name"]), "labels", n, "of", int(ref.max()), "path", used, "of", int(c["path"]),
          "voxels differing", int((got != ref).sum()), flush=True)
for p in pipes.values():
    p.close()
"""


def _write_case(tmp_path, k, name, fr, ref, thr, min_area, fill, path):
    np.savez(tmp_path / ("case_%04d.npz" % k), name=np.array(name), fr=fr, ref=ref, thr=np.float64(np.nan if thr is None else thr),
             min_area=np.int64(min_area), fill=np.bool_(fill), path=np.int64(path))


def _scene_cases(names, path_of):
    for name in names:
        for fill in FILLS:
            for a in _scene(name)[1]:
                yield ("%s min_area=%d fill=%d" % (name, a, fill), _frame(name), _ref(name, a, fill), ls.THR, a, fill,
                       path_of(name, a, fill))


def _run_child(tmp_path, cases, env_set):
    cases = list(cases)
    for k, case in enumerate(cases):
        _write_case(tmp_path, k, *case)
    env = dict(os.environ)
    for key in ("NELLIE_LABEL_VOXEL", "NELLIE_LABEL_HOST_COUNTS", "NELLIE_UF_PLANES"):
        env.pop(key, None)
    env.update(env_set)
    r = subprocess.run([sys.executable, "-c", CHILD, REPO, str(tmp_path)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    verdicts = [ln for ln in r.stdout.splitlines() if ln.startswith("VERDICT ")]
    assert len(verdicts) == len(cases), r.stdout[-2000:]
    failed = [ln for ln in verdicts if not ln.startswith("VERDICT ok ")]
    assert not failed, "\n".join(failed[:20])


def test_voxel_kernels_forced(hip, tmp_path):
    """NELLIE_LABEL_VOXEL=1 (read once per process): the voxel-level kernels on the topology scenes, the specks, the rulers up to
    4097, the random masks of test_ccl_random_masks_vs_oracle and the label goldens -- path 3, the same labels."""
    forced = lambda *_: ls.PATH_FORCED
    cases = list(_scene_cases(list(ls.TOPOLOGY) + ["specks"] + ["ruler-%d" % nx for nx in ls.RULER_WIDTHS_SMALL], forced))
    rng = np.random.default_rng(5)
    for shape, p in (((9, 14, 13), 0.3), ((20, 33, 70), 0.5), ((16, 64, 130), 0.62), ((7, 5, 200), 0.8)):
        fr = (rng.random(shape) < p).astype(np.float32) * rng.uniform(0.5, 1.0, shape).astype(np.float32)
        for a in (1, 5):
            cases.append(("random %s p=%g min_area=%d" % (shape, p, a), fr, ls.oracle_labels(fr, a, True), ls.THR, a, True, ls.PATH_FORCED))
    from nellie_amd import pipeline as pl
    n_golden = 0
    for name in list(FILTER_CASES) + list(LABEL_ONLY_CASES):
        g = load_golden(name)
        if "error_type" in g:
            continue
        thr = None if np.isnan(g["label_thr"]) else float(g["label_thr"])
        cases.append(("golden " + name, g["frangi"], g["labels"], thr, pl.min_area_pixels_of(g["dim_res_dict"]), True, ls.PATH_FORCED))
        n_golden += 1
    assert n_golden > 0
    _run_child(tmp_path, cases, {"NELLIE_LABEL_VOXEL": "1"})


def test_overflow_with_host_counts(hip, tmp_path):
    """NELLIE_LABEL_HOST_COUNTS=1: the host waits for every run count and sees the overflow itself (`nruns > cap`) instead of the
    sticky device flag -- the same paths and labels as in the default mode on the capacity scenes."""
    _run_child(tmp_path, _scene_cases([c[0] for c in ls.capacity_cases()], _path), {"NELLIE_LABEL_HOST_COUNTS": "1"})


def test_one_level_union_find(hip, tmp_path):
    """NELLIE_UF_PLANES=0: the one-level union-find (rl_union_kernel) on the topology scenes and the specks, path 0."""
    _run_child(tmp_path, _scene_cases(list(ls.TOPOLOGY) + ["specks"], _path), {"NELLIE_UF_PLANES": "0"})
