"""Label frames for the region sums by row runs (csrc/branchfeat.inc, bf_region_rows_kernel), shared by the CPU emulation of the
kernel's decomposition (tests/test_components_cpu.py) and the GPU differential (tests/test_hip_components.py); test infrastructure
only.  Every frame is the smallest that still shows its point: x extents that are no multiple of the 64-lane chunk, more rows than
one workgroup's band, runs on chunk boundaries, runs that touch both ends of a row.  `direct(name)` holds the restatement's sums by
direct summation, computed once and shared (do not modify)."""
import numpy as np

import component_features_restatement as cr

GENERIC = {"3d_3x70x130": (3, 70, 130), "3d_5x9x129": (5, 9, 129), "3d_2x3x63": (2, 3, 63), "3d_4x5x1": (4, 5, 1), "2d_65x129": (65, 129), "2d_7x64": (7, 64)}
LONGEST_RUN = (3, 32768)                                          # 98 304 voxels, one label: the longest run an extent of 2^15 allows
BOX = (20, 120, 130)                                              # 312 000 voxels, one label


def runs_frame(shape, seed, labels=9):
    """piecewise-constant rows: a new run starts at a fifth of the voxels; the values cycle through `labels` labels and background
    with a phase per row, so rows end and begin with equal and with different labels and regions sprawl over the frame"""
    rng = np.random.default_rng(seed)
    seg = np.cumsum(rng.random(shape) < 0.2, axis=-1)
    phase = rng.integers(0, labels + 2, shape[:-1] + (1,))
    return ((seg * 3 + phase) % (labels + 2)).clip(0, labels) % (labels + 1)


def _generic(name):
    return lambda: runs_frame(GENERIC[name], sum(GENERIC[name]))


def _one_label(shape, label):
    return lambda: np.full(shape, label, np.int64)


def _wrap():
    """every row ends and the next begins with label 4 (a run must not go on into the next row), label 2 in between in some"""
    lab = np.zeros((3, 6, 70), np.int64)
    lab[..., -3:] = 4
    lab[..., :2] = 4
    lab[:, ::2, 30:41] = 2
    return lab


def _adjacent():
    """label a directly followed by label b, and two labels alternating every voxel: 64 runs per chunk"""
    lab = np.zeros((2, 4, 130), np.int64)
    lab[0, :, :50], lab[0, :, 50:] = 3, 7
    lab[1] = 1 + np.arange(130) % 2
    lab[1, 3] = 1 + (np.arange(130) // 2) % 2
    return lab


def _straddle():
    """runs over x = 63 / 64 and x = 127 / 128, and runs that end at 63, begin at 64, end at 127 and begin at 128"""
    lab = np.zeros((2, 4, 200), np.int64)
    lab[:, 0, 60:70], lab[:, 0, 120:135] = 2, 3
    lab[:, 1, 50:64], lab[:, 1, 64:80] = 4, 5
    lab[:, 2, 100:128], lab[:, 2, 128:129] = 6, 7
    lab[:, 3, 0:200] = 8
    return lab


def _corners():
    """labels at x = 0 and x = nx - 1 on every corner (one label on the corners of a diagonal, another on the rest), nothing else"""
    lab = np.zeros((3, 5, 67), np.int64)
    for k, c in enumerate(np.ndindex(2, 2, 2)):
        lab[tuple(-1 if v else 0 for v in c)] = 1 + (sum(c) % 2)
    return lab


SCATTERED = 520                                                   # single-voxel labels of the scatter frame


def _scatter():
    """SCATTERED single-voxel labels, one every fourth voxel of the first 16 rows of plane 0 (one workgroup's band): every run is
    one voxel long and no two of a chunk share a region; a large region around them and in the next plane"""
    nx = 130
    lab = np.zeros((2, 20, nx), np.int64)
    flat = lab[0].reshape(-1)
    flat[np.arange(SCATTERED) * 4] = 10 + np.arange(SCATTERED)
    lab[1] = 5
    at = np.arange(lab[0].size).reshape(lab[0].shape)
    lab[0][(lab[0] == 0) & (at % 3 == 0)] = 5
    return lab


def _sparse():
    """label values sparse up to 2 000 000: the presence table has 31 250 words"""
    rng = np.random.default_rng(21)
    values = np.sort(rng.choice(np.arange(1_500_000, 2_000_001), 40, replace=False))
    values[-1] = 2_000_000
    lab = runs_frame((4, 20, 70), 5, labels=40)
    return np.where(lab > 0, values[lab - 1], 0)


FRAMES = dict({name: _generic(name) for name in GENERIC}, longest_run=_one_label(LONGEST_RUN, 5), box=_one_label(BOX, 3), wrap=_wrap, adjacent=_adjacent,
              straddle=_straddle, corners=_corners, scatter=_scatter, sparse=_sparse)
_CACHE = {}


def frame(name):
    if name not in _CACHE:
        lab = np.ascontiguousarray(FRAMES[name](), dtype=np.int64)
        lab.setflags(write=False)
        _CACHE[name] = (lab, cr.region_sums(lab))
    return _CACHE[name][0]


def direct(name):
    """(labels (R) int64, sums (F, R) int64) of frame(name) by direct summation"""
    frame(name)
    return _CACHE[name][1]


def box_sums(shape):
    """the sums of a box that fills a frame of `shape`, in closed form: n, 0 and extent - 1, S_a = n (e_a - 1) / 2,
    Q_aa = n (e_a - 1)(2 e_a - 1) / 6 and Q_ab = n (e_a - 1)(e_b - 1) / 4 in Python integers"""
    D, n = len(shape), int(np.prod(shape))
    e = [int(v) for v in shape]
    rows = [n] + [0] * D + [v - 1 for v in e] + [n * (v - 1) // 2 for v in e]
    rows += [n * (e[a] - 1) * (2 * e[a] - 1) // 6 if a == b else n * (e[a] - 1) * (e[b] - 1) // 4 for a in range(D) for b in range(a, D)]
    return np.array(rows, np.int64)[:, None]
