"""Synthetic stacks for the voxel-feature tests at sizes where every scan and node kernel spans workgroups, test infrastructure
only -- never imported by the package.  The structure of tests/reassign_scenes.py (blobs and tubes that drift by a fractional
number of voxels per frame, branch label = a core subset and branch 0 on the rest of each object, object and branch ids permuted
per frame, flow rows [t, pos, vec, cost] at labelled voxels) with the additions the voxel goldens make (single-voxel branches,
intensity and structure lit at the labelled voxels and at 2 % of the background, node classes and radii), but every object is
drawn in a window around itself, so a stack of hundreds of objects takes about a second.

`stack()` returns the dict that tests/voxel_goldens.py's `hierarchy_double` reads.  `SCENES` names the stacks of
tests/test_hip_voxels_scale.py; `counts()` gives the figures their requirements are stated in."""
from types import SimpleNamespace

import numpy as np

import voxel_features_restatement as vr

SPACING_3D, SPACING_2D = (0.211, 0.083, 0.083), (0.107, 0.083)


def _window(shape, s, p, reach_um):
    """slices of the voxels within reach_um of p along every axis, and the window's origin"""
    lo = np.maximum(np.floor(p - reach_um / s).astype(int) - 1, 0)
    hi = np.minimum(np.ceil(p + reach_um / s).astype(int) + 2, np.asarray(shape))
    hi = np.maximum(hi, lo)
    return tuple(slice(a, b) for a, b in zip(lo, hi)), lo


def _raster(window, origin, s, kind, p, size_um, axis_dir, half_len_um):
    """the object's voxels inside its window"""
    sizes = [w.stop - w.start for w in window]
    grid = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in sizes], indexing="ij"), axis=-1) + origin
    rel = (grid - p) * s
    if kind == "tube":
        along = np.clip(rel @ axis_dir, -half_len_um, half_len_um)
        rel = rel - along[..., None] * axis_dir
    return (rel ** 2).sum(axis=-1) <= size_um ** 2


def draw(rng, shape, T, spacing, n_obj, size_um, big_um, big_core=0.8, drift_um=0.16, rows_per_obj=12, noise=0.3, integer_flow=False,
         no_flow_t=None):
    """-> branch (T, ...) int32, comp (T, ...) int32, flow (n, 2 D + 2) float64.  Object 0 is a blob of radius big_um whose core
    (the branch label) is big_core of the radius; every other object has a radius drawn from size_um and a core of 0.55 of it, odd
    ones are tubes; every seventh object has no flow row.  integer_flow: every row of an object carries the object's drift rounded
    to whole voxels, which is the zero vector for object 0 -- its voxels out of reach of other objects' rows share the norm 0."""
    s = np.asarray(spacing, np.float64)
    D = len(shape)
    objs = []
    for k in range(n_obj):
        size = big_um if k == 0 else rng.uniform(*size_um)
        tube = k % 2 == 1
        half = rng.uniform(0.3, 0.7) if tube else 0.0
        pad = (size + half) / s + 1.0 + 1.5 * T * drift_um / s
        hi = np.asarray(shape, np.float64) - 1 - pad
        lo = np.minimum(pad, hi)
        u = rng.normal(size=D)
        drift = rng.uniform(-drift_um, drift_um, D) / s
        if integer_flow:
            drift = (np.round(drift) if k else 0.0) + rng.uniform(-0.5, 0.5, D)
        objs.append(SimpleNamespace(kind="tube" if tube else "blob", p0=rng.uniform(lo, np.maximum(lo, hi)), size=size * (0.6 if tube else 1.0),
                                    core=big_core if k == 0 else 0.55, dir=u / np.linalg.norm(u), half=half, drift=drift))
    branch, comp = np.zeros((T,) + tuple(shape), np.int32), np.zeros((T,) + tuple(shape), np.int32)
    rows = []
    for t in range(T):
        perm_o, perm_b = rng.permutation(n_obj) + 1, rng.permutation(n_obj) + 1 + n_obj
        for k, o in enumerate(objs):
            p = o.p0 + t * o.drift
            window, origin = _window(shape, s, p, o.size + o.half)
            body = _raster(window, origin, s, o.kind, p, o.size, o.dir, o.half)
            core = _raster(window, origin, s, o.kind, p, o.size * o.core, o.dir, o.half)
            comp[t][window][body] = perm_o[k]
            branch[t][window][body] = 0
            branch[t][window][core] = perm_b[k]
            vox = np.argwhere(body) + origin
            if t < T - 1 and t != no_flow_t and len(vox) and k % 7 != 3:
                pick = vox[rng.choice(len(vox), min(max(rows_per_obj, len(vox) // 60), len(vox)), replace=False)].astype(np.float64)
                vec = np.tile(np.round(o.drift), (len(pick), 1)) if integer_flow else o.drift + rng.uniform(-noise, noise, pick.shape)
                cost = rng.random(len(pick)).astype(np.float32).astype(np.float64)
                rows.append(np.column_stack([np.full(len(pick), float(t)), pick, vec, cost]))
    flow = np.concatenate(rows) if rows else np.zeros((0, 2 * D + 2))
    return branch, comp, flow


def dress(rng, comp, branch, raw_dtype, struct_dtype, singles=3, node_share=0.22, far_nodes=2, zero_radius=0.1, radius=(0.0, 3.2),
          class_dtype=np.uint8, distance_dtype=np.float32, sparse_labels=0):
    """what a stack needs beside its labels; comp and branch are changed in place (single-voxel branches, sparse branch labels).
    -> raw, struct, pixel_class, distance.  Nodes: node_share of the labelled voxels of a frame get a class 1 .. 4 and a radius
    drawn uniformly from `radius`, zero_radius of them exactly 0, the first far_nodes one that passes every face.  A signed
    class_dtype also gets negative entries, on a tenth as many voxels, which are no nodes.  sparse_labels: the branch labels > 0 of
    every frame are replaced by distinct random values up to that number."""
    T, shape = len(comp), comp.shape[1:]
    D = len(shape)
    top_c, top_b = int(comp.max()), int(branch.max())
    for t in range(T):
        body = np.argwhere(comp[t] > 0)
        for _ in range(singles if len(body) else 0):
            p = body[rng.integers(len(body))] + rng.integers(-3, 4, D)
            if np.all(p >= 0) and np.all(p < shape) and comp[t][tuple(p)] == 0:
                top_c, top_b = top_c + 1, top_b + 1
                comp[t][tuple(p)], branch[t][tuple(p)] = top_c, top_b
    if sparse_labels:
        for t in range(T):
            table = np.zeros(top_b + 1, np.int32)
            table[1:] = rng.choice(sparse_labels, top_b, replace=False) + 1
            branch[t] = table[branch[t]]
    lit = (comp > 0) | (rng.random(comp.shape) < 0.02)
    raw = rng.gamma(2.0, 40.0, comp.shape) * lit
    raw = raw.astype(raw_dtype) if np.issubdtype(raw_dtype, np.floating) else np.clip(raw, 0, np.iinfo(raw_dtype).max).astype(raw_dtype)
    struct = (rng.random(comp.shape) * lit).astype(struct_dtype)
    pixel_class = np.zeros(comp.shape, class_dtype)
    distance = np.zeros(comp.shape, distance_dtype)
    for t in range(T):
        body = np.argwhere(comp[t] > 0)
        if len(body) == 0:
            continue
        pick = body[rng.choice(len(body), max(1, int(len(body) * node_share)), replace=False)]
        pixel_class[t][tuple(pick.T)] = rng.integers(1, 5, len(pick))
        rad = rng.uniform(*radius, len(pick)).astype(distance_dtype)
        rad[rng.random(len(pick)) < zero_radius] = 0.0
        rad[:far_nodes] = 1.5 * max(shape) + 0.25
        distance[t][tuple(pick.T)] = rad
        if np.issubdtype(class_dtype, np.signedinteger):
            free = np.argwhere(pixel_class[t] == 0)
            minus = free[rng.choice(len(free), max(1, len(pick) // 10), replace=False)]
            pixel_class[t][tuple(minus.T)] = -rng.integers(1, 5, len(minus))
            distance[t][tuple(minus.T)] = rng.uniform(*radius, len(minus))
    return raw, struct, pixel_class, distance


def as_stack(name, comp, branch, raw, struct, pixel_class, distance, flow, spacing, dt, skip_nodes=False, enable_motility=True):
    return dict(name=name, comp=comp, branch=branch, raw=raw, struct=struct, pixel_class=pixel_class, distance=distance, flow=flow,
                spacing=np.asarray(spacing, np.float64), dt=float(dt), skip_nodes=skip_nodes, enable_motility=enable_motility,
                T=len(comp), D=comp.ndim - 1, filename="scene_" + name)


# The stacks of tests/test_hip_voxels_scale.py.  S3: 312 000 voxels = 4876 mask words (two scan workgroups), X = 130 (words
# straddle rows and planes), a voxel count that is no multiple of 256.  S2: 420 000 pixels, X = 700.  The -ties variants carry
# whole-voxel flow: most norms of a label are bit-equal and the lowest index decides its pivot.
SCENES = {
    "S3": dict(shape=(20, 120, 130), spacing=SPACING_3D, dt=1.0, seed=31, raw=np.uint16, struct=np.float32,
               draw=dict(n_obj=110, size_um=(0.3, 0.45), big_um=1.4)),
    "S3-ties": dict(shape=(20, 120, 130), spacing=SPACING_3D, dt=0.5, seed=31, raw=np.uint16, struct=np.float32,
                    draw=dict(n_obj=110, size_um=(0.3, 0.45), big_um=1.4, integer_flow=True),
                    dress=dict(class_dtype=np.int16, distance_dtype=np.float64)),
    "S2": dict(shape=(600, 700), spacing=SPACING_2D, dt=1.7, seed=21, raw=np.float32, struct=np.float64,
               draw=dict(n_obj=100, size_um=(0.6, 1.0), big_um=4.0)),
    "S2-ties": dict(shape=(600, 700), spacing=SPACING_2D, dt=1.7, seed=21, raw=np.float32, struct=np.float64,
                    draw=dict(n_obj=100, size_um=(0.6, 1.0), big_um=4.0, integer_flow=True)),
}
_CACHE = {}


def stack(name, T=3):
    """the named stack of SCENES; built once and shared (do not modify)"""
    if name not in _CACHE:
        _CACHE[name] = build(name, T)
    return _CACHE[name]


def build(name, T=3):
    case = SCENES[name]
    rng = np.random.default_rng(case["seed"])
    branch, comp, flow = draw(rng, case["shape"], T, case["spacing"], **case["draw"])
    raw, struct, pixel_class, distance = dress(rng, comp, branch, case["raw"], case["struct"], sparse_labels=2_000_000, **case.get("dress", {}))
    return as_stack(name, comp, branch, raw, struct, pixel_class, distance, flow, case["spacing"], case["dt"])


def counts(g, t):
    """the figures of frame t that the scale tests' requirements are stated in"""
    comp, branch, pc, dist = g["comp"][t], g["branch"][t], g["pixel_class"][t], g["distance"][t]
    on = comp > 0
    labels, sizes = np.unique(branch[on], return_counts=True)
    nodes, lims = vr.node_boxes(pc, dist)
    radius = dist[tuple(nodes.T)]
    far = np.ones(len(nodes), bool)
    for ax, size in enumerate(comp.shape):
        far &= (lims[ax][:, 0] == 0) & (lims[ax][:, 1] == size) & (nodes[:, ax] - radius < 0) & (nodes[:, ax] + radius > size - 1)
    return dict(voxels=int(on.sum()), nodes=len(nodes), nodes_on_labelled=int((on & (pc > 0)).sum()), far_nodes=int(far.sum()),
                zero_radius=float(np.mean(radius == 0)) if len(radius) else 0.0, max_radius=float(np.max(radius[~far], initial=0.0)),
                label0=int(sizes[labels == 0].sum()), largest_branch=int(np.max(sizes[labels > 0], initial=0)),
                max_label=int(labels.max(initial=0)), negative_classes=int((pc.astype(np.int64) < 0).sum()))


RA_SCAN_CHUNK = 4096                  # counts per workgroup of the exclusive scan (csrc/rank_scan.inc)


def assert_scale(g, t):
    """the requirements of a large scene on frame t (asserted without a GPU by tests/test_voxel_scenes_cpu.py and again by the GPU tests before they compare)"""
    c = counts(g, t)
    n = int(np.prod(g["comp"].shape[1:]))
    assert (n + 63) // 64 > RA_SCAN_CHUNK and g["comp"].shape[-1] % 64 and n % 256, "two scan workgroups of mask words, straddling rows"
    assert 12_289 <= c["voxels"] <= 40_000 and c["voxels"] % RA_SCAN_CHUNK, c    # four chunks or more, no boundary at the end
    assert 4_097 <= c["nodes"] <= 8_000 and c["nodes"] == c["nodes_on_labelled"], c            # two chunks, 17 workgroups of nodes
    assert c["far_nodes"] >= 2 and c["max_radius"] <= 3.2 and 0.07 <= c["zero_radius"] <= 0.13, c
    assert c["largest_branch"] >= 3_000 and c["label0"] >= 3_000, c
    assert 1_500_000 < c["max_label"] <= 2_000_000, c
    return c


def longest_list(g, t):
    """the longest per-voxel node list of frame t"""
    _, lims = vr.node_boxes(g["pixel_class"][t], g["distance"][t])
    _, (vox_off, _) = vr.node_assignment(lims, np.argwhere(g["comp"][t] > 0))
    return int(np.max(np.diff(vox_off), initial=0))


# ---- the uneven stack ---------------------------------------------------------------------------------------------------------------
def _rows(rng, t, voxels, k, backward):
    """k flow rows of time t at (forward) or leading to (backward: pos + vec is a voxel) random voxels of `voxels`"""
    pick = voxels[rng.choice(len(voxels), min(k, len(voxels)), replace=False)].astype(np.float64)
    vec = rng.uniform(-1.2, 1.2, pick.shape)
    cost = rng.random(len(pick)).astype(np.float32).astype(np.float64)
    return np.column_stack([np.full(len(pick), float(t)), pick - vec if backward else pick, vec, cost])


def uneven(seed=5, shape=(12, 48, 70)):
    """T = 6 on one shape: a normal frame; an all-background frame; a frame with voxels but no node; a frame with nodes but no
    labelled voxel; a frame with about four times the voxels, nodes and label range of the first; the first frame again.  Flow
    rows exist at the time points 0, 1, 3 and 4, none at 2."""
    rng = np.random.default_rng(seed)
    small = dict(size_um=(0.3, 0.45), big_um=0.6, drift_um=0.08)
    b_a, c_a, _ = draw(rng, shape, 2, SPACING_3D, n_obj=5, **small)
    b_b, c_b, _ = draw(rng, shape, 1, SPACING_3D, n_obj=40, size_um=(0.3, 0.45), big_um=0.9, drift_um=0.08)
    parts_a = dress(rng, c_a, b_a, np.uint16, np.float32, singles=2, far_nodes=1)
    b_b[b_b > 0] += 500                                         # a larger pivot table
    parts_b = dress(rng, c_b, b_b, np.uint16, np.float32, singles=2, far_nodes=1)
    order = ((0, 0), None, (0, 1), (0, 0), (1, 0), (0, 0))      # (stack, frame) per time point
    src = ((c_a, b_a) + parts_a, (c_b, b_b) + parts_b)
    out = [np.zeros((6,) + shape, a.dtype) for a in src[0]]
    for t, pick in enumerate(order):
        if pick is not None:
            for dst, a in zip(out, src[pick[0]]):
                dst[t] = a[pick[1]]
    comp, branch, raw, struct, pixel_class, distance = out
    pixel_class[2] = 0                                          # voxels, no node
    comp[3] = 0                                                 # nodes, no labelled voxel
    vox = {t: np.argwhere(comp[t] > 0) for t in range(6)}
    flow = np.concatenate([_rows(rng, 0, vox[0], 60, False), _rows(rng, 1, vox[2], 60, True), _rows(rng, 3, vox[4], 200, True),
                           _rows(rng, 4, vox[4], 200, False), _rows(rng, 4, vox[5], 60, True)])
    return as_stack("uneven", comp, branch, raw, struct, pixel_class, distance, flow, SPACING_3D, 1.0)


# ---- every row geometry -----------------------------------------------------------------------------------------------------------
ROW_NX = (2, 63, 64, 65, 127, 128, 129)


def row_cases():
    """(shape, full mask?) of test_node_boxes_on_every_row_geometry"""
    cases = []
    for lead in ((3, 5), (7,)):
        for nx in ROW_NX:
            cases.append((lead + (nx,), False))
            if nx in (64, 65):
                cases.append((lead + (nx,), True))
    return cases


def rows_stack(shape, full, seed=0):
    """T = 1, every voxel a node, the radii cycling through 0, 0.5, 1.0, 1.5, 1.99, 2.0 and nx in raster order; a 50 % random
    label mask or a full one"""
    rng = np.random.default_rng([seed, len(shape), shape[-1], int(full)])
    n = int(np.prod(shape))
    comp = (np.ones(n, np.int32) if full else (rng.random(n) < 0.5).astype(np.int32)).reshape((1,) + shape)
    comp = comp * rng.integers(1, 9, comp.shape, dtype=np.int32)
    branch = (comp > 0) * rng.integers(0, 5, comp.shape, dtype=np.int32)
    cycle = np.array([0, 0.5, 1.0, 1.5, 1.99, 2.0, shape[-1]], np.float32)
    distance = cycle[np.arange(n) % len(cycle)].reshape((1,) + shape)
    pixel_class = rng.integers(1, 5, (1,) + shape).astype(np.uint8)
    raw = rng.integers(0, 256, (1,) + shape).astype(np.uint8)
    struct = rng.random((1,) + shape).astype(np.float32)
    spacing = SPACING_3D if len(shape) == 3 else SPACING_2D
    return as_stack(f"rows_{'x'.join(map(str, shape))}_{'full' if full else 'half'}", comp, branch, raw, struct, pixel_class, distance,
                    np.zeros((0, 2 * len(shape) + 2)), spacing, 1.0)


# ---- one frame whose per-voxel scan has more than 1024 workgroup sums ----------------------------------------------------------------
def all_labelled(seed=9, shape=(33, 360, 360), n_nodes=48):
    """-> comp, branch (int32, every voxel labelled, random labels), raw (uint8), struct (uint8), pixel_class (uint8, n_nodes nodes
    spread over the frame, one in the corner 0), distance (float32, radii <= 3)"""
    rng = np.random.default_rng(seed)
    comp = rng.integers(1, 1000, shape, dtype=np.int32)
    branch = rng.integers(0, 1000, shape, dtype=np.int32)
    raw = rng.integers(0, 256, shape, dtype=np.uint8)
    struct = rng.integers(0, 256, shape, dtype=np.uint8)
    pixel_class, distance = np.zeros(shape, np.uint8), np.zeros(shape, np.float32)
    n = int(np.prod(shape))
    at = np.unique(np.concatenate([[0, n - 1], np.linspace(0, n - 1, n_nodes - 2).astype(np.int64) + rng.integers(-5000, 5000, n_nodes - 2)]).clip(0, n - 1))
    while len(at) < n_nodes:
        at = np.unique(np.append(at, rng.integers(0, n)))
    pixel_class.reshape(-1)[at] = rng.integers(1, 5, len(at))
    distance.reshape(-1)[at] = rng.uniform(0.5, 3.0, len(at)).astype(np.float32)
    return comp, branch, raw, struct, pixel_class, distance
