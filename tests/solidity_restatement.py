"""Restatements of skimage's `regionprops(...).solidity` = area / area_convex for the solidity tests.

`area_convex / pixel volume` is the number of set voxels of `convex_hull_image(region.image)` with its defaults
(offset_coordinates=True, tolerance=1e-10, include_borders=True): every voxel centre is moved by +-1/2 along every axis, the hull of
the moved points is taken and a lattice point of the bounding box counts when it lies in the closed hull; a 3-D region whose raw
centres qhull cannot hull (affine rank < 3) has an all-zero convex image: count 0, solidity inf.  Two independent forms:

(a) `count_float`: the float rule through scipy.spatial.ConvexHull (imported lazily), `equations . p + offset < 1e-10`;
(b) `count_exact`: numpy int64 and Python integers on doubled box-relative coordinates.  Degeneracy from the exact rank
    (det(n Q - S S^T) == 0), candidates reduced to the ends of every row (z, y), facets by brute force over point triples (pairs in
    2-D) while the point set is small and by gift wrapping (pivot a supporting plane about every edge of every face) beyond that --
    brute force is O(m^4) -- and row intervals by integer floor division.  Both facet searches first take the hull of the centres
    and move only its vertices: hull(centres + diamond) = hull(centres) + diamond.

`solidity_of(n, count, spacing)` is the column: float64 (n * P) / (count * P), inf where count is 0.
"""
from __future__ import annotations

import math
from itertools import combinations

import numpy as np

BRUTE_MAX = 40                        # points up to which count_exact searches facets by brute force


def regions_of(labels):
    """[(label, coords (n, D) int64 relative to the region's box, extents (D,))] for every label > 0, ascending"""
    lab = np.asarray(labels)
    out = []
    idx = np.argwhere(lab > 0)
    vals = lab[lab > 0].astype(np.int64)
    order = np.argsort(vals, kind="stable")
    idx, vals = idx[order], vals[order]
    starts = np.flatnonzero(np.concatenate([[True], vals[1:] != vals[:-1]])) if len(vals) else np.zeros(0, np.int64)
    for a, b in zip(starts, np.append(starts[1:], len(vals))):
        c = idx[a:b].astype(np.int64)
        lo = c.min(axis=0)
        out.append((int(vals[a]), c - lo, c.max(axis=0) - lo + 1))
    return out


# ---- (a) the float rule ------------------------------------------------------------------------------------------------------------
def count_float(coords, ext):
    from scipy.spatial import ConvexHull, QhullError
    c = np.asarray(coords, dtype=np.float64)
    D = c.shape[1]
    if D == 3:
        try:
            h0 = ConvexHull(c)
        except QhullError:
            return 0
        c = h0.points[h0.vertices]
    offs = np.concatenate([0.5 * np.eye(D), -0.5 * np.eye(D)])
    pts = np.unique((c[:, None, :] + offs[None]).reshape(-1, D), axis=0)
    hull = ConvexHull(pts)
    grid = np.stack(np.meshgrid(*[np.arange(e) for e in ext], indexing="ij"), axis=-1).reshape(-1, D).astype(np.float64)
    inside = np.ones(len(grid), bool)
    for eq in hull.equations:
        inside &= grid @ eq[:D] + eq[D] < 1e-10
    return int(inside.sum())


# ---- (b) exact ---------------------------------------------------------------------------------------------------------------------
def is_flat(coords):
    """a 3-D point set has affine rank < 3: det(n Q - S S^T) == 0 in Python integers"""
    c = [[int(v) for v in row] for row in np.asarray(coords)]
    n = len(c)
    S = [sum(r[a] for r in c) for a in range(3)]
    M = [[n * sum(r[a] * r[b] for r in c) - S[a] * S[b] for b in range(3)] for a in range(3)]
    det = (M[0][0] * (M[1][1] * M[2][2] - M[1][2] * M[2][1]) - M[0][1] * (M[1][0] * M[2][2] - M[1][2] * M[2][0])
           + M[0][2] * (M[1][0] * M[2][1] - M[1][1] * M[2][0]))
    return det == 0


def row_ends(coords):
    """the first and last voxel of every row (all but the last axis equal): a superset of the hull's vertices"""
    c = np.asarray(coords, dtype=np.int64)
    order = np.lexsort(c.T[::-1])
    c = c[order]
    new = np.concatenate([[True], (c[1:, :-1] != c[:-1, :-1]).any(axis=1)])
    last = np.concatenate([new[1:], [True]])
    return np.unique(c[new | last], axis=0)


def _reduce(N, d):
    g = 0
    for v in N:
        g = math.gcd(g, abs(int(v)))
    return tuple(int(v) // g for v in N) + (int(d) // g,)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def facets_brute(P):
    """every plane through three (two in 2-D) of the points P (m, D) int64 that has all points on one side, as reduced (N..., d) with
    N . p <= d inside"""
    P = np.asarray(P, dtype=np.int64)
    m, D = P.shape
    out = set()
    if D == 2:
        i, j = np.triu_indices(m, 1)
        e = P[j] - P[i]
        N = np.stack([e[:, 1], -e[:, 0]], axis=1)
    else:
        tri = np.array(list(combinations(range(m), 3)), dtype=np.int64).reshape(-1, 3)
        i = tri[:, 0]
        N = _cross(P[tri[:, 1]] - P[i], P[tri[:, 2]] - P[i])
    ok = (N != 0).any(axis=1)
    N, i = N[ok], i[ok]
    for a in range(0, len(N), 20000):
        Nc = N[a:a + 20000]
        s = Nc @ P.T - np.einsum("ij,ij->i", Nc, P[i[a:a + 20000]])[:, None]
        for k in np.flatnonzero((s <= 0).all(axis=1)):
            out.add(_reduce(Nc[k], Nc[k] @ P[i[a + k]]))
        for k in np.flatnonzero((s >= 0).all(axis=1)):
            out.add(_reduce(-Nc[k], -(Nc[k] @ P[i[a + k]])))
    return sorted(out)


def _pivot(P, a, direction):
    """the supporting plane of P (all N . (p - a) <= 0) that holds the line a + t * direction, which touches the hull, and at least
    one point off that line; N = direction x (p_k - a) for the point k it ends on"""
    rel = P - a
    off = np.flatnonzero((_cross(direction[None], rel) != 0).any(axis=1))
    k = off[0]
    while True:
        N = _cross(direction, rel[k])
        s = rel @ N
        if s.max() <= 0:
            return N
        k = int(np.argmax(s))


def _polygon(P, idx, N):
    """the vertices (indices into P) of the convex polygon of the coplanar points P[idx], counter-clockwise seen against N; two for
    collinear points"""
    drop = int(np.argmax(np.abs(N)))
    keep = [a for a in range(3) if a != drop]
    pts = sorted((int(P[k, keep[0]]), int(P[k, keep[1]]), int(k)) for k in idx)

    def half(seq):
        st = []
        for p in seq:
            while len(st) >= 2 and (st[-1][0] - st[-2][0]) * (p[1] - st[-2][1]) - (st[-1][1] - st[-2][1]) * (p[0] - st[-2][0]) <= 0:
                st.pop()
            st.append(p)
        return st

    lower, upper = half(pts), half(pts[::-1])
    ring = [p[2] for p in lower[:-1] + upper[:-1]]
    if len(ring) >= 3:
        turn = _cross(P[ring[1]] - P[ring[0]], P[ring[2]] - P[ring[0]]) @ N
        if turn < 0:
            ring = ring[::-1]
    return ring


def facets_wrap(P):
    """the facet planes of the hull of P (m, 3) int64 (full rank) by gift wrapping: from a first face, pivot about every edge of
    every face found; coplanar points are one face, a convex polygon"""
    P = np.unique(np.asarray(P, dtype=np.int64), axis=0)                # sorted: P[0] is the lexicographic minimum, a vertex
    N = _pivot(P, P[0], np.array([0, 0, 1], np.int64))                  # the hull lies on one side of the line P[0] + t x
    planes, todo = {}, [N]
    first = True
    while todo:
        N = todo.pop()
        d = int(N @ P[np.argmax(P @ N)])
        idx = np.flatnonzero(P @ N == d)
        ring = _polygon(P, idx, N)
        if len(ring) < 3:                                              # the first plane may touch the hull in an edge only
            assert first and len(ring) == 2
            todo.append(_pivot(P, P[ring[0]], P[ring[1]] - P[ring[0]]))
            first = False
            continue
        first = False
        key = _reduce(N, d)
        if key in planes:
            continue
        planes[key] = True
        for a, b in zip(ring, ring[1:] + ring[:1]):
            M = _pivot(P, P[b], P[a] - P[b])                           # the face beyond the edge a -> b
            if _reduce(M, M @ P[b]) not in planes:
                todo.append(M)
    return sorted(planes)


def _facets3(P):
    return facets_brute(P) if len(P) <= BRUTE_MAX else facets_wrap(P)


def _vertices(P, facets):
    """the points of P that lie on at least D of the facet planes: every vertex of the hull does, so this is a superset of them"""
    P = np.asarray(P, dtype=np.int64)
    F = np.array(facets, dtype=np.int64)
    on = (P @ F[:, :-1].T == F[:, -1][None]).sum(axis=1)
    return P[on >= P.shape[1]]


def exact_facets(coords, search=None):
    """the reduced facets (N..., d), N . p <= d inside in doubled box-relative coordinates, of the hull of the voxels' diamonds; [] for
    a flat 3-D region.  `search`: the facet search for 3-D point sets (default: brute force up to BRUTE_MAX points, else wrapping)"""
    c = np.asarray(coords, dtype=np.int64)
    D = c.shape[1]
    if D == 3 and is_flat(c):
        return []
    search = search or _facets3
    ends = 2 * row_ends(c)
    if D == 2:
        verts = _vertices(ends, facets_brute(ends)) if len(ends) > 2 and not _collinear(ends) else ends
    else:
        verts = _vertices(ends, search(ends))
    offs = np.concatenate([np.eye(D, dtype=np.int64), -np.eye(D, dtype=np.int64)])
    moved = np.unique((verts[:, None, :] + offs[None]).reshape(-1, D), axis=0)
    return facets_brute(moved) if D == 2 else search(moved)


def _collinear(P):
    e = P[1:] - P[0]
    return not (e[:, 0] * e[0, 1] - e[:, 1] * e[0, 0]).any()


def count_facets(facets, ext):
    """the lattice points x of the box (extents ext) with N . 2 x <= d for every facet, row by row with integer division"""
    D = len(ext)
    if not facets:
        return 0
    lead = np.stack(np.meshgrid(*[2 * np.arange(e, dtype=np.int64) for e in ext[:-1]], indexing="ij"), axis=-1).reshape(-1, D - 1)
    lo, hi = np.zeros(len(lead), np.int64), np.full(len(lead), int(ext[-1]) - 1, np.int64)
    for f in facets:
        N, d = np.array(f[:-1], np.int64), int(f[-1])
        rhs = d - lead @ N[:-1]
        if N[-1] == 0:
            hi[rhs < 0] = -1
        elif N[-1] > 0:
            hi = np.minimum(hi, np.floor_divide(rhs, 2 * N[-1]))
        else:
            lo = np.maximum(lo, -np.floor_divide(rhs, -2 * N[-1]))
    return int(np.clip(hi - lo + 1, 0, None).sum())


def count_exact(coords, ext, search=None):
    return count_facets(exact_facets(coords, search), [int(e) for e in ext])


def solidity_of(n, count, spacing):
    """the column: area / area_convex with area = n * P in float64; inf where the convex count is 0"""
    P = float(np.prod(spacing))
    with np.errstate(divide="ignore"):
        return (np.asarray(n, np.int64) * P) / (np.asarray(count, np.int64) * P)


def frame_exact(labels, spacing=None):
    """(region labels, n, convex count, solidity) of a label frame by (b)"""
    regs = regions_of(labels)
    lab = np.array([r[0] for r in regs], np.int64)
    n = np.array([len(r[1]) for r in regs], np.int64)
    count = np.array([count_exact(r[1], r[2]) for r in regs], np.int64)
    sp = np.ones(np.ndim(labels)) if spacing is None else np.asarray(spacing, np.float64)
    return lab, n, count, solidity_of(n, count, sp)
