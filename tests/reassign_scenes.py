"""Synthetic scenes for the voxel-reassignment tests and goldens, test infrastructure only: blobs and tubes that drift by a
fractional number of voxels per frame, object ids permuted per frame, branch labels a strict subset of the object voxels, flow
rows [t, pos, vec, cost] at random labelled voxels (vector = the object's drift plus noise, random float32 costs)."""
import numpy as np


def _raster(shape, s, kind, p, size_um, axis_dir, half_len_um):
    grid = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), axis=-1)
    rel = (grid - p) * s
    if kind == "tube":
        along = np.clip(rel @ axis_dir, -half_len_um, half_len_um)
        rel = rel - along[..., None] * axis_dir
    return (rel ** 2).sum(axis=-1) <= size_um ** 2


def make_scene(rng, shape, T, spacing, n_obj=6, drift_um=0.16, rows_per_obj=12, noise=0.3, integer_flow=False, appear=False,
               vanish=False, converge=False, empty_t=None, no_flow_t=None, size_um=(0.3, 0.45), x_share=1.0, mismatch=0.5):
    """-> branch (T, ...) int32, obj (T, ...) int32, flow (n, 2 D + 2) float64.  x_share < 1 keeps the ordinary objects in the
    low part of the last axis (`appear` puts its object, which has no flow row, at the far end).  integer_flow: every vector is
    the object's drift rounded to whole voxels, and the drift itself is within `mismatch` voxels of that whole number."""
    s = np.asarray(spacing, np.float64)
    D = len(shape)
    objs = []
    for k in range(n_obj):
        size = rng.uniform(*size_um)
        pad = size / s + 1.0 + 1.5 * T * drift_um / s
        hi = np.asarray(shape, np.float64) - 1 - pad
        hi[-1] = (shape[-1] - 1) * x_share - pad[-1]
        lo = np.minimum(pad, hi)
        u = rng.normal(size=D)
        objs.append(dict(kind="tube" if k % 2 else "blob", p0=rng.uniform(lo, np.maximum(lo, hi)), size=size * (0.6 if k % 2 else 1.0),
                         dir=u / np.linalg.norm(u), half=rng.uniform(0.3, 0.7), drift=rng.uniform(-drift_um, drift_um, D) / s,
                         frames=range(T), flow=True, same_as=k))
    if integer_flow:
        for o in objs:
            o["drift"] = np.round(o["drift"]) + rng.uniform(-mismatch, mismatch, D)
    if vanish:
        objs[0]["frames"] = range(0, T // 2)
    if converge and n_obj >= 2:                          # object 1 runs into object 0 and carries its id from frame 2 on
        a, b = objs[0], objs[1]
        b.update(kind=a["kind"], size=a["size"], dir=a["dir"], half=a["half"])
        off = np.zeros(D)
        off[-2] = 2.0 * a["size"] / s[-2] + 2.0
        b["p0"] = a["p0"] + off
        a["drift"], b["drift"] = off / (2.0 * 2.2), -off / (2.0 * 2.2)
        b["merge_from"] = 2
    if appear:
        p = (np.asarray(shape, np.float64) - 1) / 2.0
        p[-1] = shape[-1] - 1 - 0.4 / s[-1] - 1.0
        objs.append(dict(kind="blob", p0=p, size=0.35, dir=None, half=0.0, drift=np.zeros(D), frames=range(1, T), flow=False,
                         same_as=n_obj))
    K = len(objs)
    branch, obj = np.zeros((T,) + tuple(shape), np.int32), np.zeros((T,) + tuple(shape), np.int32)
    rows = []
    for t in range(T):
        if t == empty_t:
            continue
        perm_o, perm_b = rng.permutation(K) + 1, rng.permutation(K) + 1 + K
        for k, o in enumerate(objs):
            if t not in o["frames"]:
                continue
            p = o["p0"] + t * o["drift"]
            ident = 0 if t >= o.get("merge_from", T + 1) else k
            body = _raster(shape, s, o["kind"], p, o["size"], o["dir"], o["half"])
            core = _raster(shape, s, o["kind"], p, o["size"] * 0.55, o["dir"], o["half"])
            obj[t][body] = perm_o[ident]
            branch[t][body] = 0
            branch[t][core] = perm_b[ident]
            vox = np.argwhere(body)
            if o["flow"] and t < T - 1 and t != no_flow_t and len(vox):
                pick = vox[rng.choice(len(vox), min(rows_per_obj, len(vox)), replace=False)].astype(np.float64)
                if integer_flow:
                    vec = np.tile(np.round(o["drift"]), (len(pick), 1))
                else:
                    vec = o["drift"] + rng.uniform(-noise, noise, pick.shape)
                cost = rng.random(len(pick)).astype(np.float32).astype(np.float64)
                rows.append(np.column_stack([np.full(len(pick), float(t)), pick, vec, cost]))
        branch[t][obj[t] == 0] = 0
    flow = np.concatenate(rows) if rows else np.zeros((0, 2 * D + 2))
    return branch, obj, flow


# ---- decisive scenes: tiny, deterministic, each built so that one of the discrete rules of DESIGN.md section 12 decides -------
LATTICE_VECTORS = [(0.0, 0.0, 0.0), (0.0, 0.5, 0.5), (0.5, 0.0, 0.5), (0.0, 1.0, 2.0), (0.0, 0.0, 5.0), (0.0, 4.0, 3.0)]
LATTICE_SPACINGS = [(0.25, 0.125, 0.125), (0.29, 0.0973, 0.0973), (0.107, 0.107, 0.107), (0.3, 0.1, 0.1)]
HALF_VOXEL_VECTORS = LATTICE_VECTORS[1:3]


def _index_sum(shape):
    return sum(np.meshgrid(*[np.arange(n) for n in shape], indexing="ij"))


def lattice_holes(D, vector):
    """-> branch, obj (2, ...) int32, flow.  Frame 0 is a solid block whose neighbouring voxels carry different labels, frame 1 the
    same block with a checkerboard of holes in (y, x), every flow row carries `vector` (its last D components): centroids fall on
    lattice or half-lattice points, so nearest voxels, best pairs and votes tie, and the long vectors put centroids at exactly r.
    The frame is 70 wide: the mask words straddle rows.  Flow rows sit on every other (y, x) of the block, dyadic costs."""
    shape = (5, 12, 70)[3 - D:]
    block = (slice(1, 4), slice(2, 10), slice(2, 68))[3 - D:]
    inside = np.zeros(shape, bool)
    inside[block] = True
    index = np.arange(int(np.prod(shape))).reshape(shape)
    obj = np.zeros((2,) + shape, np.int32)
    obj[0][inside] = 1 + index[inside] % 97
    obj[1][inside] = 5
    obj[1][..., ::2, ::2] = 0
    obj[1][..., 1::2, 1::2] = 0
    branch = np.where(_index_sum(shape) % 3 == 0, obj, 0).astype(np.int32)
    vec = np.asarray(vector, np.float64)[3 - D:]
    pos = np.argwhere(inside)
    pos = pos[(pos[:, -1] % 2 == 0) & (pos[:, -2] % 2 == 0)].astype(np.float64)
    cost = (np.arange(len(pos)) * 37 % 11) / 16.0
    flow = np.column_stack([np.zeros(len(pos)), pos, np.tile(vec, (len(pos), 1)), cost])
    return branch, obj, flow


CROWD_SPACING = (0.107, 0.107, 0.107)
CROWD_SHAPE = (15, 15, 15)
CROWD_TARGETS = ((8, 8, 8), (0, 0, 0))               # one in the interior, one at a corner of the frame
CROWD_LABELS = ((7, 9, 3), (11, 12, 4))              # per target: the mirrored labels A < B, and the label of the mirror plane


def crowd(r=0.5):
    """-> branch, obj (2, 15, 15, 15) int32, flow.  Frame 1 holds the two voxels of CROWD_TARGETS.  Frame 0 is a solid ball of
    radius r + one voxel around each, zero flow vectors: every voxel of a ball within r is a candidate of its target (more than
    300 for the interior one).  The object labels of a ball are mirrored -- about the plane x = x_target for the interior target
    (A beyond it, B before it), about the plane y = x for the corner target (A where y > x, B where x > y) -- so A and B collect
    the same weights in the same order and their sums are equal bit for bit; the mirror plane carries a third, smaller label with
    a smaller sum.  The voxel under the target itself (weight 1e6) carries a branch label only: it has no reassigned object label
    and goes last in the object vote, and it wins the branch vote.  Branch labels elsewhere: object label + 100 on every third voxel."""
    s = np.asarray(CROWD_SPACING)
    grid = np.stack(np.meshgrid(*[np.arange(n) for n in CROWD_SHAPE], indexing="ij"), axis=-1)
    branch, obj = np.zeros((2,) + CROWD_SHAPE, np.int32), np.zeros((2,) + CROWD_SHAPE, np.int32)
    third = _index_sum(CROWD_SHAPE) % 3 == 0
    rows = []
    for k, (target, (A, B, C)) in enumerate(zip(CROWD_TARGETS, CROWD_LABELS)):
        off = grid - np.asarray(target)
        ball = ((off * s) ** 2).sum(axis=-1) <= (r + s.max()) ** 2
        side = off[..., 2] if k == 0 else off[..., 1] - off[..., 2]
        lab = np.where(side > 0, A, np.where(side < 0, B, C)).astype(np.int32)
        obj[0][ball] = lab[ball]
        branch[0][ball & third] = lab[ball & third] + 100
        obj[0][target] = 0
        branch[0][target] = 50 + k
        obj[1][target] = 20 + k
        branch[1][target] = 30 + k
        for a in range(3):                               # rows at the target and three voxels along every axis: the whole ball is in reach
            for step in (-3, 3):
                p = np.asarray(target, np.float64)
                p[a] += step
                if 0 <= p[a] < CROWD_SHAPE[a]:
                    rows.append(p)
        rows.append(np.asarray(target, np.float64))
    pos = np.asarray(rows)
    flow = np.column_stack([np.zeros(len(pos)), pos, np.zeros((len(pos), 3)), (np.arange(len(pos)) % 5) / 8.0])
    return branch, obj, flow


FACES_SPACING = (0.25, 0.125, 0.125)                 # dyadic: r = 0.5 is 2 voxels in z and 4 in y and x, exactly
FACES_SHAPE = (8, 40, 70)
# name: (z, y, x slices of the region, the same in both frames; flow vector; cost).  The flow row sits on the region's first voxel.
# Regions are at least 2 r + 2 voxels apart (10 voxels in y or x, 6 in z), so a voxel sees the row of its own region only and
# gets its vector exactly.
FACES_REGIONS = {
    "corner_neg_half":    ((0, 0, 0), (-0.5, -0.5, -0.5), 0.25),          # rint(-0.5) = -0
    "corner_mixed_half":  ((7, 0, 0), (0.5, -1.5, 0.5), 0.5),             # rint(7.5) = 8, outside; rint(-1.5) = -2
    "corner_out_less":    ((0, 39, 0), (0.0, 2.0, 0.0), 0.125),           # 0.25 um outside: kept
    "corner_out_exact":   ((7, 39, 0), (0.0, 4.0, 0.0), 0.375),           # exactly r outside: d == r, dropped
    "corner_out_more":    ((0, 0, 69), (0.0, 0.0, 6.0), 0.75),            # 0.75 um outside
    "corner_out_exact_z": ((7, 0, 69), (2.0, 0.0, 0.0), 0.625),           # exactly r outside along z
    "corner_half_out":    ((0, 39, 69), (-0.5, 1.5, 1.5), 0.875),
    "corner_still":       ((7, 39, 69), (0.0, 0.0, 0.0), 0.0),
    "face_z0":            ((0, slice(13, 15), slice(14, 16)), (-1.5, 0.0, 0.5), 0.25),
    "face_z7":            ((7, slice(13, 15), slice(28, 30)), (0.5, -0.5, 0.0), 0.5),
    "face_y0":            ((slice(3, 5), 0, slice(28, 30)), (0.0, -2.5, 0.5), 0.125),    # rint(-2.5) = -2
    "face_y39":           ((slice(3, 5), 39, slice(42, 44)), (0.0, 0.5, -0.5), 0.375),
    "face_x0":            ((slice(3, 5), slice(26, 28), 0), (0.0, 0.0, -3.5), 0.625),    # rint(-3.5) = -4, every offset clipped
    "face_x69_3e9":       ((slice(3, 5), slice(26, 28), 69), (0.0, 0.0, 3e9), 0.75),     # beyond the 1e9 guard
    "face_x69_1e12":      ((slice(3, 5), slice(13, 15), 69), (0.0, 0.0, 1e12), 0.875),   # and far beyond: the flow grid's coarsest case
    "inner_nan":          ((3, slice(26, 28), slice(28, 30)), (0.0, 0.5, 1.0), np.nan),  # a NaN cost makes every component NaN
    # voxel (3, 27, 43) lands on (3.5, 27.5, 43.5), which rounds to (4, 28, 44): eight voxels tie, and the one with the lowest
    # index is the voxel itself, a whole diagonal from the rounded point -- the last offset the walk may not skip
    "inner_half":         ((slice(3, 5), slice(26, 29), slice(42, 45)), (0.5, 0.5, 0.5), 0.0),
}
FACES_DIAGONAL_TIE = (3, 27, 43)
FACES_STAY_ZERO = ("corner_out_exact", "corner_out_more", "corner_out_exact_z", "face_x69_3e9", "face_x69_1e12", "inner_nan")


def faces_region(name):
    """bool mask of a region of faces_and_outside"""
    m = np.zeros(FACES_SHAPE, bool)
    m[FACES_REGIONS[name][0]] = True
    return m


def faces_and_outside():
    """-> branch, obj (2, 8, 40, 70) int32, flow.  Small regions on every face and corner of both frames, each with one flow row
    and a vector of its own: out of the frame by less than r, by exactly r and by more, components ending in .5 on both sides
    of 0 (rint to even, offsets clipped at the frame), an eight-fold tie whose winner is the farthest offset from the rounded point, 3e9 and 1e12 voxels in one component, and a row whose NaN cost makes the
    interpolated vector NaN.  Every voxel of frame 0 has a label of its own; frame 1 has others."""
    branch, obj = np.zeros((2,) + FACES_SHAPE, np.int32), np.zeros((2,) + FACES_SHAPE, np.int32)
    rows = []
    third = _index_sum(FACES_SHAPE) % 3 == 0
    for k, (name, (_, vec, cost)) in enumerate(FACES_REGIONS.items()):
        vox = np.argwhere(faces_region(name))
        for j, p in enumerate(vox):
            obj[0][tuple(p)] = 1 + 32 * k + j
            obj[1][tuple(p)] = 1000 + 32 * k + j
        rows.append([0.0, *vox[0].astype(np.float64), *vec, cost])
    branch[0] = np.where(third, obj[0] + 2000, 0) * (obj[0] > 0)
    branch[1] = np.where(third, obj[1] + 2000, 0) * (obj[1] > 0)
    return branch, obj, np.asarray(rows, np.float64)


def decisive_cases():
    """every decisive case as a dict: id, D, spacing, dt, r, make() -> (branch, obj, flow), zero -- the margins (letters of
    a, b, c, d: nearest voxel, radius, vote, best pair) the case is built to bring to exactly 0 -- and half_voxel.  The lists of
    (b) and (c) were found by running the restatement with exact vectors; the reasons: (0, 0, 5) and (0, 4, 3) are 5 voxels long
    and put centroids 4 or 5 voxels from the nearest voxel, 0.5 um at 0.125 and 0.1 um per voxel (0.4865 and 0.535 at the other
    two spacings); a (0, .5, .5) centroid is equally far, float32(c - m) = +-0.5 on two axes of equal spacing, from sources with
    different labels, and (.5, 0, .5) in 3-D likewise at the dyadic spacing."""
    cases = []
    for D in (3, 2):
        for spacing in LATTICE_SPACINGS:
            for vector in LATTICE_VECTORS:
                long = vector in ((0.0, 0.0, 5.0), (0.0, 4.0, 3.0))
                zero = "ad"
                if long and spacing in ((0.25, 0.125, 0.125), (0.3, 0.1, 0.1)):
                    zero += "b"
                if vector == (0.0, 0.5, 0.5) or (vector == (0.5, 0.0, 0.5) and D == 3 and spacing == (0.25, 0.125, 0.125)):
                    zero += "c"
                dts = (1.0, 1.4) if (D == 3 and spacing == (0.29, 0.0973, 0.0973) and vector == (0.0, 4.0, 3.0)) else (1.0,)
                for dt in dts:
                    name = f"lattice_holes-{D}d-{'x'.join(f'{s:g}' for s in spacing[3 - D:])}-{'_'.join(f'{v:g}' for v in vector[3 - D:])}-dt{dt:g}"
                    cases.append(dict(id=name, scene="lattice_holes", D=D, spacing=spacing[3 - D:], dt=dt, r=max(0.5 * dt, 0.5), vector=vector,
                                      zero="ad" if dt != 1.0 else zero, half_voxel=vector in HALF_VOXEL_VECTORS,
                                      make=lambda D=D, vector=vector: lattice_holes(D, vector)))
    cases.append(dict(id="crowd", scene="crowd", D=3, spacing=CROWD_SPACING, dt=1.0, r=0.5, zero="c", half_voxel=False, make=crowd))
    cases.append(dict(id="faces_and_outside", scene="faces_and_outside", D=3, spacing=FACES_SPACING, dt=1.0, r=0.5, zero="b", half_voxel=False,
                      make=faces_and_outside))
    return cases
