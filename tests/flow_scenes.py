"""Seeded scenes for flow-vector interpolation at tracker-scale row counts and capped grids (tests/test_flow_scenes_cpu.py,
tests/test_hip_flow_scale.py), and a dense brute force of the rules of tests/flow_interpolation_restatement.py's docstring that uses
no grid at all.  Test infrastructure only.  Nothing here allocates a frame: row coordinates span up to 1024^3 voxels, no volume does.

scene(name) returns Scene(flow, spacing, r, queries, expect):
  flow     (n, 2 D + 2) float64 rows t | position | vector | cost, all at time point T_ROWS; rows on both extreme corners of the
           coordinate box are planted first, so the plan of the device's grid does not depend on the draw
  queries  a quarter on check coordinates (d == 0), a quarter within +-3 voxels of one (`near` says where not), the rest uniform over the box grown by
           2 voxels, some rows NaN; then the face block (face_block) -- expect["n_body"] rows come before it
  expect   what the device's plan (hipnative.FlowField.grid()) has to report for these rows -- literal numbers, worked out by hand
           from DESIGN.md section 11's rule (base cells floor(extent / h) + 1 with h = r (1 + 2^-20), the longest axis doubled
           until max_cells hold) -- and what the scene is there for.
"""
import math
from typing import NamedTuple

import numpy as np

T_ROWS = 1                      # the time point of every scene's rows: forward queries ask for t = 1, backward ones for t = 2
SLACK = 1.0 + 1.0 / 1048576.0   # the device's cells are r * SLACK wide before any doubling
ISO = (0.0973, 0.0973, 0.0973)
ANISO = (0.29, 0.0973, 0.0973)
BRUTE_SAMPLE = 2000


class Scene(NamedTuple):
    flow: np.ndarray
    spacing: tuple
    r: float
    queries: np.ndarray
    expect: dict


# extent: coordinates lie in 0 .. extent - 1 per axis.  mult / dims / max_cells: the plan.  fullest: (low, high) bounds of the
# fullest cell's row count.  chunk: queries per chunk of the restatement, so that its pair list stays below about 2 * 10^7.
SCENES = {
    # 1023 * 0.1013 um = 207.3 base cells -> 208 per axis; 208 -> 104 -> 52 on each axis in turn (52 * 52 * 104 is still above 2^18)
    "cube_1024": dict(extent=(1024, 1024, 1024), spacing=(0.1013, 0.1013, 0.1013), rows=200_000, queries=200_000,
                      mult=(4, 4, 4), dims=(52, 52, 52), max_cells=1 << 18, fullest=(4, 64), k_max=(1, 16)),
    # base cells (148, 200, 200): y, x -> 100, z -> 74, y, x -> 50
    "aniso_1024": dict(extent=(256, 1024, 1024), spacing=ANISO, rows=100_000, queries=200_000,
                       mult=(2, 4, 4), dims=(74, 50, 50), max_cells=1 << 18, fullest=(4, 64)),
    # base cells (37, 100, 100) = 370 000: one doubling of y (the first of the two longest)
    "cap_edge_32767": dict(extent=(64, 512, 512), spacing=ANISO, rows=32_767, queries=200_000,
                           mult=(1, 2, 1), dims=(37, 50, 100), max_cells=262_136, fullest=(2, 32)),
    "cap_edge_32768": dict(extent=(64, 512, 512), spacing=ANISO, rows=32_768, queries=200_000,
                           mult=(1, 2, 1), dims=(37, 50, 100), max_cells=262_144, fullest=(2, 32)),
    # base cells (12, 8, 8) = 768 below every budget; integer coordinates, so positions repeat
    "dense_small": dict(extent=(20, 40, 40), spacing=ANISO, rows=40_000, queries=20_000, integer=True,
                        mult=(1, 1, 1), dims=(12, 8, 8), max_cells=1 << 18, fullest=(70, 200), k_max=(200, 10 ** 6), chunk=2_000),
    # base cells (74, 200, 200): y, x -> 100, y, x -> 50
    "clustered": dict(extent=(128, 1024, 1024), spacing=ANISO, rows=150_000, queries=20_000, clusters=1500, sigma=3.0,
                      mult=(1, 4, 4), dims=(74, 50, 50), max_cells=1 << 18, fullest=(256, 4096), k_max=(200, 10 ** 6), chunk=2_000),
    # 2-D: base cells (877, 680): y -> 439, x -> 340
    "image_4096": dict(extent=(4096, 4096), spacing=(0.107, 0.083), rows=150_000, queries=200_000,
                       mult=(1, 2, 2), dims=(1, 439, 340), max_cells=1 << 18, fullest=(4, 64)),
    # integer coordinates at round spacings: base cells (153, 205, 205): y, x -> 103, z -> 77, y, x -> 52.  The near quarter lies in
    # plane within +-5 voxels: 9 dz^2 + dy^2 + dx^2 = 25 is the radius, and (0, 0, 5), (0, 3, 4) need the reach ((1, 0, 4) comes from
    # the uniform part)
    "round_spacing": dict(extent=(256, 1024, 1024), spacing=(0.3, 0.1, 0.1), rows=60_000, queries=200_000, integer=True, near=(0, 5, 5),
                          mult=(2, 4, 4), dims=(77, 52, 52), max_cells=1 << 18, fullest=(2, 64), exact_on_radius=1000),
    # every row at z = 17: base cells (1, 200, 200), no doubling
    "flat_axis": dict(extent=(1, 1024, 1024), spacing=ISO, rows=50_000, queries=200_000, z0=17.0, near=(6, 3, 3),
                      mult=(1, 1, 1), dims=(1, 200, 200), max_cells=1 << 18, fullest=(4, 64)),
    # 10^7 voxels are 1 945 999 base cells per axis: 16 doublings each leave 30^3 <= 8 * 5001 cells of 2^16 h, the body in one of them
    "outlier": dict(extent=(64, 300, 300), spacing=ISO, rows=5_001, queries=10_000, far=(1e7, 1e7, 1e7),
                    mult=(1 << 16,) * 3, dims=(30, 30, 30), max_cells=8 * 5001, fullest=(5000, 5000), brute_only=True),
    # 10^20 voxels on x: the base count is clamped to 10^15 and 2^30-fold cells still leave 931 323 > 4096: one cell, inv = 0
    "unresolved": dict(extent=(64, 300, 300), spacing=ISO, rows=301, queries=200_000, far=(63.0, 299.0, 1e20),
                       mult=(0, 0, 0), dims=(1, 1, 1), max_cells=4096, fullest=(301, 301), brute_only=True),
}
ORDER = list(SCENES)


def check_rows(flow, D, forward=True):
    """(check coordinates, vectors, costs) of the scene's rows in a direction: position forward, position + vector backward"""
    pos, vec = flow[:, 1:1 + D], flow[:, 1 + D:1 + 2 * D]
    return (pos if forward else pos + vec), vec, flow[:, -1]


def expected_edge(r, mult):
    """the cell edge per axis in um as the device reports it: 1 / inv with inv = 1 / (h * mult), 0 for the unresolved plan"""
    h = r * SLACK
    return tuple(1.0 / (1.0 / (h * float(m))) if m else 0.0 for m in mult)


def _rows(rng, cfg):
    ext = np.asarray(cfg["extent"], np.float64)
    D = len(ext)
    hi = ext - 1.0
    planted = [np.zeros(D), hi.copy()]                               # both extreme corners of the box
    if "far" in cfg:
        planted.append(np.asarray(cfg["far"], np.float64))
    n = cfg["rows"] - len(planted)                                   # `rows` counts the planted ones
    if "clusters" in cfg:
        n_uni = n // 10
        size = rng.lognormal(0.0, 1.5, cfg["clusters"])
        size = np.maximum(1, np.floor(size / size.sum() * (n - n_uni))).astype(np.int64)
        size[np.argmax(size)] += (n - n_uni) - size.sum()
        centre = rng.uniform(0, hi, (cfg["clusters"], D))
        pos = np.repeat(centre, size, axis=0) + rng.normal(0.0, cfg["sigma"], (n - n_uni, D))
        pos = np.concatenate([np.clip(pos, 0, hi), rng.uniform(0, hi, (n_uni, D))])
        pos = pos[rng.permutation(n)]                                # a cell's rows are no run of row indices
    elif cfg.get("integer"):
        pos = np.column_stack([rng.integers(0, int(e), n) for e in ext]).astype(np.float64)
    else:
        pos = rng.uniform(0, hi, (n, D))
    pos = np.concatenate([np.asarray(planted), pos])
    if "z0" in cfg:
        pos[:, 0] = cfg["z0"]
    vec = rng.uniform(-5.0, 5.0, pos.shape)
    cost = rng.random(len(pos)).astype(np.float32).astype(np.float64)
    cost[2:4] = (0.0, 1.0)
    return np.column_stack([np.full(len(pos), float(T_ROWS)), pos, vec, cost])


def face_block(cc, spacing, r, cell_edge, lo_row=0, hi_row=1):
    """For each of the 2 D faces of the rows' box and for its two planted corners, queries displaced outward from the planted row on
    it by r (1 - 1e-6), r (1 + 1e-6), one cell edge, one cell edge (1 + 1e-6) and two cell edges (um, converted to voxels).  A face
    displaces along its normal; a corner along the diagonal for the two radii and by each axis's own cell edge for the rest, so
    that its cell index is -1 (or dims) on every axis at once.  cell_edge: the last D entries of what grid() reports.
    Returns (queries (10 (D + 1), D), the row each belongs to (10 (D + 1)))."""
    s = np.asarray(spacing, np.float64)
    D = len(s)
    edge = np.asarray(cell_edge, np.float64)[-D:]
    q, row = [], []
    for sign, at in ((-1.0, lo_row), (1.0, hi_row)):
        for axis in list(range(D)) + [None]:
            for kind, f in (("r", 1.0 - 1e-6), ("r", 1.0 + 1e-6), ("e", 1.0), ("e", 1.0 + 1e-6), ("e", 2.0)):
                d = np.zeros(D)
                if axis is None:
                    d[:] = r * f / math.sqrt(D) if kind == "r" else edge * f
                else:
                    d[axis] = r * f if kind == "r" else edge[axis] * f
                q.append(cc[at] + sign * d / s)
                row.append(at)
    return np.asarray(q), np.asarray(row)


def _body_queries(rng, cfg, cc):
    ext = np.asarray(cfg["extent"], np.float64)
    D, n = len(ext), cfg["queries"]
    integer = bool(cfg.get("integer"))
    near = np.asarray(cfg.get("near", (3,) * D), np.float64)
    lo, hi = np.full(D, -2.0), ext + 1.0                             # the box grown by 2 voxels (the body's, where a row lies far out)
    if "z0" in cfg:
        lo[0], hi[0] = cfg["z0"] - 6.0, cfg["z0"] + 6.0
    if integer or "z0" in cfg:
        q = np.column_stack([rng.integers(int(a), int(b) + 1, n) for a, b in zip(lo, hi)]).astype(np.float64)
    else:
        q = rng.uniform(lo, hi, (n, D))
    n4 = n // 4
    q[:n4] = cc[rng.integers(0, len(cc), n4)]
    at = cc[rng.integers(0, len(cc), n4)]
    if integer:
        off = np.column_stack([rng.integers(-int(w), int(w) + 1, n4) for w in near]).astype(np.float64)
    else:
        off = rng.uniform(-near, near, (n4, D))
    if "z0" in cfg:                                                  # whole voxels off the rows' plane: +-1 .. +-6
        off[:, 0] = rng.integers(1, 7, n4) * rng.choice([-1.0, 1.0], n4)
    q[n4:2 * n4] = at + off
    q[rng.choice(n, max(1, n // 50), replace=False)] = np.nan        # the fuzz slice's nan_rows
    q[n // 2, D - 1] = np.nan
    return q


_CACHE = {}


def scene(name, forward=True, cell_edge=None):
    """the scene `name` (a key of SCENES); cell_edge: the edge per axis that grid() reported, for the face block (default: the
    expected plan's).  Scenes are cached: treat the arrays as read-only."""
    cfg = SCENES[name]
    if cell_edge is not None and tuple(cell_edge) == expected_edge(0.5, cfg["mult"]):
        cell_edge = None
    key = (name, forward, None if cell_edge is None else tuple(cell_edge))
    if key in _CACHE:
        return _CACHE[key]
    D = len(cfg["extent"])
    rng = np.random.default_rng([ORDER.index(name), 20261021])
    flow = _rows(rng, cfg)
    cc, _, _ = check_rows(flow, D, forward)
    body = _body_queries(rng, cfg, cc)
    edge = expected_edge(0.5, cfg["mult"]) if cell_edge is None else cell_edge
    # a displacement of r is lost beside 10^20 (below the spacing of doubles there): that scene's block stays on the body's corners
    hi_row = 2 if "far" in cfg and max(cfg["far"]) < 1e15 else 1
    fq, frow = face_block(cc, cfg["spacing"], 0.5, edge, 0, hi_row)
    expect = dict(cfg, n_body=len(body), face_rows=frow, cell_edge=expected_edge(0.5, cfg["mult"]), ndim=D)
    for a in (flow, body, fq):
        a.setflags(write=False)
    q = np.concatenate([body, fq])
    q.setflags(write=False)
    _CACHE[key] = Scene(flow, tuple(cfg["spacing"]), 0.5, q, expect)
    return _CACHE[key]


def reference(name, forward=True, cell_edge=None):
    """(values, k, vmax, margin) for all queries of scene(name, forward, cell_edge), computed once: the restatement, or the brute
    force where the restatement's grid cannot hold the extent"""
    sc = scene(name, forward, cell_edge)
    if id(sc) not in _REFERENCE:
        import flow_interpolation_restatement as rs
        cc, v, c = check_rows(sc.flow, sc.expect["ndim"], forward)
        if sc.expect.get("brute_only"):
            _REFERENCE[id(sc)] = brute(cc, v, c, sc.spacing, sc.r, sc.queries)
        else:
            _REFERENCE[id(sc)] = rs.interpolate(cc, v, c, sc.spacing, sc.r, sc.queries, chunk=sc.expect.get("chunk", 200_000))
    return _REFERENCE[id(sc)]


def brute_reference(name, forward=True, cell_edge=None):
    """(indices, (values, k, vmax, margin)) of the brute force on sample() of that scene, computed once"""
    sc = scene(name, forward, cell_edge)
    if id(sc) not in _BRUTE:
        cc, v, c = check_rows(sc.flow, sc.expect["ndim"], forward)
        pick = sample(sc)
        _BRUTE[id(sc)] = pick, brute(cc, v, c, sc.spacing, sc.r, sc.queries[pick])
    return _BRUTE[id(sc)]


_REFERENCE, _BRUTE = {}, {}


def sample(sc, n=BRUTE_SAMPLE):
    """indices of n seeded queries of the scene, the face block always among them"""
    nb = sc.expect["n_body"]
    rng = np.random.default_rng(7)
    pick = np.sort(rng.choice(nb, min(nb, n - (len(sc.queries) - nb)), replace=False))
    return np.concatenate([pick, np.arange(nb, len(sc.queries))])


def brute(check_coords, vectors, costs, spacing, r, queries, block=100):
    """The rules of flow_interpolation_restatement's docstring with no grid: d2 against every row, axis by axis with the products
    formed first; neighbours d2 <= r * r in (d2, row) order; blocks of `block` queries, so memory stays flat.  Returns (values
    (n, D) with NaN rows, k, largest |vector component| among each row's neighbours, smallest |d2 - r * r| / (r * r) over all pairs)."""
    s = np.asarray(spacing, np.float64)
    D = len(s)
    q = np.asarray(queries, np.float64).reshape(-1, D)
    out = np.full((len(q), D), np.nan)
    k = np.zeros(len(q), np.int64)
    vmax = np.zeros(len(q))
    margin = np.inf
    if len(q) == 0 or len(check_coords) == 0:
        return out, k, vmax, margin
    cs = np.asarray(check_coords, np.float64) * s
    v, cost = np.asarray(vectors, np.float64), np.asarray(costs, np.float64)
    vabs = np.abs(v).max(axis=1)
    r2 = r * r
    for at in range(0, len(q), block):
        qs = q[at:at + block] * s
        with np.errstate(invalid="ignore"):
            d2 = (qs[:, None, 0] - cs[None, :, 0]) ** 2
            for ax in range(1, D):
                d2 = d2 + (qs[:, None, ax] - cs[None, :, ax]) ** 2
        good = ~np.isnan(d2)
        if good.any():
            margin = min(margin, float(np.min(np.abs(d2[good] - r2))) / r2)
        with np.errstate(invalid="ignore"):
            qi, ri = np.nonzero(d2 <= r2)                            # row-major: by query, then by row
        for j in np.unique(qi):
            rows = ri[qi == j]
            dd = d2[j, rows]
            o = np.lexsort((rows, dd))
            rows, dd = rows[o], dd[o]
            d = np.sqrt(dd)
            with np.errstate(divide="ignore"):
                dw = (d == 0) * 1.0 if (d == 0).any() else 1 / d
            w = -cost[rows] * dw
            w = w - (w.min() - 1)
            w = w / np.add.reduceat(w, [0])[0]
            out[at + j] = np.add.reduceat(v[rows] * w[:, None], [0], axis=0)[0]
            k[at + j] = len(rows)
            vmax[at + j] = vabs[rows].max()
    return out, k, vmax, margin
