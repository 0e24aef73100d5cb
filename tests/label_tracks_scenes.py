"""Scenes of the LabelTracks tests (test_label_tracks_cpu.py checks their margins, test_hip_label_tracks.py runs them on the
device): label stacks, flow arrays, the im_info stand-in and the restatement's answer, computed once per scene and shared."""
import functools
import os
from types import SimpleNamespace

import numpy as np

import label_tracks_restatement as lrs

T = 4
MARGIN = 1e-9


def radius(maxd, dt=1.0):
    return max(maxd * dt, 0.5)


def im_double(tmp_path, flow, labels, spacing, dt=1.0, label_key="im_instance_label"):
    """what LabelTracks and FlowInterpolator ask of an ImInfo, over arrays"""
    labels = np.asarray(labels)
    D = labels.ndim - 1
    path = str(tmp_path / f"flow_{len(os.listdir(tmp_path))}.npy")
    np.save(path, flow)
    axes = "TYX" if D == 2 else "TZYX"
    dim_res = dict(zip(axes[1:], (float(s) for s in spacing)))
    dim_res["T"] = float(dt)
    stack = np.zeros(labels.shape, np.uint8)
    return SimpleNamespace(no_t=False, no_z=D == 2, shape=labels.shape, axes=axes, dim_res=dim_res, im_path="im",
                           pipeline_paths={"flow_vector_array": path, label_key: "labels"},
                           get_memmap=lambda p: labels if p == "labels" else stack)


def blob_labels(rng, shape, frames=T, blobs=5, radii=(2.0, 3.5)):
    """a few balls per frame (label = the ball's number) whose centres wander from frame to frame"""
    D = len(shape)
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1).astype(float)
    centres = np.column_stack([rng.uniform(0.15 * s, 0.85 * s, blobs) for s in shape])
    rad = rng.uniform(*radii, blobs)
    stack = np.zeros((frames,) + tuple(shape), np.int32)
    for t in range(frames):
        for b in range(blobs):
            stack[t][((grid - centres[b]) ** 2).sum(axis=-1) <= rad[b] ** 2] = b + 1
        centres = centres + rng.uniform(-1.5, 1.5, (blobs, D))
    return stack


def random_flow(rng, shape, rows_per_t, vmax, integer=True):
    """rows [t, pos, vec, cost] for t = 0 .. len(rows_per_t) - 1 (0 rows: a time point without any)"""
    D = len(shape)
    out = [np.zeros((0, 2 * D + 2))]
    for t, n in enumerate(rows_per_t):
        if integer:
            pos = np.column_stack([rng.integers(0, s, n) for s in shape]).astype(float).reshape(n, D)
            vec = rng.integers(-vmax, vmax + 1, (n, D)).astype(float)
        else:
            pos = np.column_stack([rng.uniform(0, s, n) for s in shape]).reshape(n, D)
            vec = rng.uniform(-vmax, vmax, (n, D))
        cost = rng.random(n).astype(np.float32).astype(float)
        out.append(np.column_stack([np.full(n, float(t)), pos, vec, cost]))
    return np.concatenate(out)


# ---- the fuzz slice ------------------------------------------------------------------------------------------------------------------
SPACING3, SPACING2 = [(0.29, 0.0973, 0.0973), (0.107,) * 3, (0.211, 0.083, 0.083)], [(0.107, 0.083), (0.0973, 0.0973)]
DENSE, SPARSE = 1.0, 0.12          # flow rows per time point, as a share of what covers the frame with balls of the radius


def _fuzz_specs():
    """24 cases: 2-D and 3-D, every start frame of T = 4, end_frame below, at and above T, skip_coords 1 / 3 / 100 / beyond the
    seed count, label_num absent / present / naming no voxel, vectors up to +-6 voxels (tracks leave the volume and the blobs),
    sparse flow (coordinates lost in mid-array), a time point without rows as the first and as a middle frame, rows at t = T - 1
    (frame T is produced and filtered out)"""
    specs = []
    for k in range(24):
        s = dict(k=k, D=2 if k % 2 else 3, start=k % 4, end=[None, None, 6, 2, 4, 1][k % 6], skip=[1, 3, 1, 100, 1, 10 ** 6][(k // 2) % 6],
                 label=[None, 99, 2, None, None][k % 5], vmax=[2, 6, 4][k % 3], density=SPARSE if k % 3 == 0 else DENSE,
                 empty_t=None, last_t=k % 4 == 1, min_track=[0, 7, 1000][k % 3], maxd=[0.5, 1.0][(k // 3) % 2], integer=k % 7 != 6)
        specs.append(s)
    specs[4]["empty_t"], specs[4]["start"] = 0, 0              # the first frame forward has no rows: the start rows are never emitted
    specs[9]["empty_t"], specs[9]["start"] = 1, 0              # a middle frame forward
    specs[14]["empty_t"], specs[14]["start"] = 2, 3            # the first frame backward (its rows are those of t - 1 = 2)
    specs[19]["empty_t"], specs[19]["start"] = 1, 3            # a middle frame backward
    for j in (4, 9, 14, 19):
        specs[j]["end"], specs[j]["skip"], specs[j]["label"] = None, 1, None
    return specs


@functools.lru_cache(maxsize=None)
def fuzz_case(k):
    """the k-th fuzz case: the first seed whose scene clears both margins (the restatement and the device then decide alike)"""
    s = _fuzz_specs()[k]
    D = s["D"]
    shape = (8, 26, 24) if D == 3 else (44, 40)
    spacing = (SPACING3 if D == 3 else SPACING2)[k % (3 if D == 3 else 2)]
    r = radius(s["maxd"])
    ball = np.prod([2 * r / sp for sp in spacing]) * (np.pi / 6 if D == 3 else np.pi / 4)      # voxels within the radius of a row
    rows = max(3, int(s["density"] * 3 * np.prod(shape) / ball))
    for seed in range(1000):
        rng = np.random.default_rng([seed, k])
        labels = blob_labels(rng, shape)
        per_t = [0 if t == s["empty_t"] else rows for t in range(T if s["last_t"] else T - 1)]
        flow = random_flow(rng, shape, per_t, s["vmax"], s["integer"])
        kw = dict(label_num=s["label"], start_frame=s["start"], end_frame=s["end"], min_track_num=s["min_track"], skip_coords=s["skip"])
        want = lrs.label_tracks(labels, flow, spacing, r, **kw)
        if want[2]["radius_margin"] > MARGIN and want[2]["half_margin"] > MARGIN:
            return dict(spec=s, seed=seed, labels=labels, flow=flow, spacing=spacing, maxd=s["maxd"], kw=kw, want=want,
                        vmax=float(s["vmax"]))
    raise AssertionError(f"fuzz case {k}: no seed clears the margins")


N_FUZZ = 24


# ---- exact cases ---------------------------------------------------------------------------------------------------------------------
EXACT_SPACING = 0.25               # r = 0.5 um is two voxels: a seed sees the one flow row that sits on it, weight exactly 1
# 2-D frame of 41 x 44 (odd and even extents); per case: seed (y, x), displacement (multiples of 0.5), the voxel of the other
# frame that is labelled, whether the row stays -- half to even against half up, and the faces
EXACT_2D = [
    ((3, 4), (0.0, 0.5), (3, 4), True),            # 4.5 -> 4 (half up: 5, unlabelled)
    ((9, 8), (0.0, 0.5), (9, 9), False),           # 8.5 -> 8, unlabelled (half up: 9, labelled)
    ((15, 5), (0.0, 0.5), (15, 6), True),          # 5.5 -> 6 (truncation: 5, unlabelled)
    ((21, 11), (0.0, 0.5), (21, 11), False),       # 11.5 -> 12, unlabelled (truncation: 11, labelled)
    ((27, 0), (0.0, -0.5), (27, 0), True),         # -0.5 -> -0.0: inside, voxel 0
    ((33, 0), (0.0, -1.5), (33, 0), False),        # -1.5 -> -2: outside (a clamp would keep it)
    ((3, 43), (0.0, 0.5), (3, 43), False),         # nx - 0.5 = 43.5 -> 44: outside (truncation: 43, labelled)
    ((40, 20), (0.5, 0.0), (40, 20), True),        # ny - 0.5 = 40.5 -> 40: inside
    ((40, 30), (1.5, 0.0), (40, 30), False),       # 41.5 -> 42: outside
    ((15, 20), (2.5, -3.5), (18, 16), True),       # (17.5, 16.5) -> (18, 16)
    ((27, 30), (-2.5, 3.5), (24, 34), True),       # (24.5, 33.5) -> (24, 34)
]
# 3-D frame of 7 x 41 x 44: the 2-D cases in plane 3, and the z faces
EXACT_3D = [((3,) + s, (0.0,) + d, (3,) + m, keep) for s, d, m, keep in EXACT_2D] + [
    ((0, 3, 30), (-0.5, 0.0, 0.0), (0, 3, 30), True),       # -0.5 -> voxel 0
    ((6, 9, 30), (0.5, 0.0, 0.0), (6, 9, 30), True),        # nz - 0.5 = 6.5 -> 6: inside
    ((6, 15, 30), (1.5, 0.0, 0.0), (6, 15, 30), False),     # 7.5 -> 8: outside
]


def exact_scene(D, forward):
    """two frames; forward: the seeds are frame 0's voxels and land in frame 1, backward the other way round.  Returns (labels,
    flow, spacing, start_frame, keep flags by seed in raster order)"""
    cases = EXACT_3D if D == 3 else EXACT_2D
    shape = (7, 41, 44)[3 - D:]
    labels = np.zeros((2,) + shape, np.int32)
    src, dst = (0, 1) if forward else (1, 0)
    order = sorted(range(len(cases)), key=lambda j: cases[j][0])
    rows = []
    for n, j in enumerate(order):
        seed, disp, mark, _ = cases[j]
        labels[src][seed] = n + 1
        labels[dst][mark] = n + 1
        seed, disp = np.asarray(seed, float), np.asarray(disp, float)
        # forward: the row sits on the seed with vector = displacement; backward: its check coordinate pos + vec is the seed and
        # the coordinate moves by - vec, so vec = - displacement and pos = seed + displacement
        pos, vec = (seed, disp) if forward else (seed + disp, -disp)
        rows.append(np.concatenate([[0.0], pos, vec, [0.25 + 0.03125 * n]]))
    return labels, np.array(rows), (EXACT_SPACING,) * D, src, [cases[j][3] for j in order]


# ---- kernel boundaries -----------------------------------------------------------------------------------------------------------------
BOUNDARY_SHAPE = (8, 192, 192)       # 294 912 voxels = 4 608 mask words: more than one scan workgroup (RA_SCAN_CHUNK = 4096 words)
BOUNDARY_SPACING = (0.29, 0.0973, 0.0973)
# seed counts around the ballot word (64 lanes), the block of every kernel (256 lanes) and one scan workgroup of kept-words
# (4096 words x 64 coordinates); 100 and 1000 leave a partial last word
BOUNDARY_COUNTS = [63, 64, 65, 100, 255, 256, 257, 1000, 4096 * 64 - 1, 4096 * 64, 4096 * 64 + 1]


@functools.lru_cache(maxsize=None)
def boundary_base():
    """three frames; the middle one is filled per case, the outer ones are half labelled; sparse flow with fractional vectors"""
    rng = np.random.default_rng(77)
    labels = np.zeros((3,) + BOUNDARY_SHAPE, np.int32)
    labels[0] = rng.integers(0, 3, BOUNDARY_SHAPE)
    labels[2] = rng.integers(0, 2, BOUNDARY_SHAPE) * 5
    flow = random_flow(rng, BOUNDARY_SHAPE, [900, 900], 5, integer=False)
    return labels, flow, rng.permutation(int(np.prod(BOUNDARY_SHAPE)))


@functools.lru_cache(maxsize=None)
def boundary_case(n):
    """n seeds: n voxels of the middle frame, spread over it by a fixed permutation, followed one step in each direction"""
    base, flow, spread = boundary_base()
    labels = base.copy()
    labels[1].reshape(-1)[spread[:n]] = 3
    want = lrs.label_tracks(labels, flow, BOUNDARY_SPACING, 0.5, start_frame=1)
    return labels, flow, want
