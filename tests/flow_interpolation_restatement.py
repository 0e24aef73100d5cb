"""numpy restatement of flow-vector interpolation (the rules of DESIGN.md section 11), test infrastructure only -- never imported
by the package.

For the check rows of a time point (coordinates c_i, vectors v_i, costs), spacing s and radius r, a query q has the neighbours
with d2_i = sum over axes, in axis order, of (q*s - c_i*s)^2 <= r*r (float64; the products are formed first).  With
d_i = sqrt(d2_i): dw_i = (d_i == 0) * 1.0 if any d_i == 0 else 1 / d_i; w_i = -cost_i * dw_i; w -= min(w) - 1; w /= sum(w);
vector = sum_i v_i * w_i.  No neighbour (a NaN query included) gives a NaN row; one neighbour gives its vector.  Neighbours are
taken in (d2, row index) order.  If no query of a call has a neighbour the result has shape (0, D).
"""
import itertools

import numpy as np


def select_rows(flow, t, forward, ndim):
    """(check_rows, check_coords) of time point t: column 0 == t forward, t - 1 backward (position + vector)"""
    rows = flow[flow[:, 0] == (t if forward else t - 1)]
    pos, vec = rows[:, 1:1 + ndim], rows[:, 1 + ndim:1 + 2 * ndim]
    return rows, (pos if forward else pos + vec)


def neighbour_pairs(cs, qs, reach):
    """all (query, row, d2) with every |axis difference| below about `reach` (a superset of d2 <= reach^2): rows binned into
    cells of edge 1.001 * reach, every query looks into the 3^D cells around its own"""
    n, D = qs.shape
    h = reach * 1.001
    mn = cs.min(axis=0)
    rc = np.floor((cs - mn) / h).astype(np.int64) + 1                        # 1 .. dims - 2
    dims = rc.max(axis=0) + 2
    lin = np.ravel_multi_index(tuple(rc.T), tuple(dims))
    order = np.argsort(lin, kind="stable")
    lin_sorted = lin[order]
    good = np.all(np.isfinite(qs), axis=1)
    qidx = np.nonzero(good)[0]
    qc = np.clip(np.floor((qs[qidx] - mn) / h), -1, dims - 2).astype(np.int64) + 1      # 0 .. dims - 1
    out_q, out_r, out_d2 = [], [], []
    for off in itertools.product((-1, 0, 1), repeat=D):
        c = qc + np.asarray(off)
        ok = np.all((c >= 0) & (c < dims), axis=1)
        if not ok.any():
            continue
        l = np.ravel_multi_index(tuple(c[ok].T), tuple(dims))
        a, b = np.searchsorted(lin_sorted, l, "left"), np.searchsorted(lin_sorted, l, "right")
        cnt = b - a
        tot = int(cnt.sum())
        if tot == 0:
            continue
        qi = np.repeat(qidx[ok], cnt)
        ramp = np.arange(tot) - np.repeat(np.cumsum(cnt) - cnt, cnt)
        ri = order[np.repeat(a, cnt) + ramp]
        d2 = np.zeros(tot)
        for ax in range(D):
            d2 = d2 + (qs[qi, ax] - cs[ri, ax]) ** 2
        out_q.append(qi); out_r.append(ri); out_d2.append(d2)
    if not out_q:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0)
    return np.concatenate(out_q), np.concatenate(out_r), np.concatenate(out_d2)


def interpolate(check_coords, vectors, costs, spacing, r, queries, chunk=200_000):
    """(vectors (n, D) with NaN rows, neighbour count per row, largest |vector component| among each row's neighbours, smallest
    |d2 - r*r| / (r*r) over all candidate pairs)"""
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
    r2 = r * r
    for at in range(0, len(q), chunk):
        qs = q[at:at + chunk] * s
        qi, ri, d2 = neighbour_pairs(cs, qs, r)
        if len(d2):
            margin = min(margin, float(np.min(np.abs(d2 - r2))) / r2)
        keep = d2 <= r2
        qi, ri, d2 = qi[keep], ri[keep], d2[keep]
        if len(qi) == 0:
            continue
        o = np.lexsort((ri, d2, qi))
        qi, ri, d2 = qi[o], ri[o], d2[o]
        first = np.nonzero(np.concatenate([[True], qi[1:] != qi[:-1]]))[0]
        cnt = np.diff(np.concatenate([first, [len(qi)]]))
        seg = np.repeat(np.arange(len(first)), cnt)
        d = np.sqrt(d2)
        any_zero = (np.minimum.reduceat(d, first) == 0)[seg]
        with np.errstate(divide="ignore"):
            dw = np.where(any_zero, (d == 0) * 1.0, 1 / d)
        w = -cost[ri] * dw
        w = w - (np.minimum.reduceat(w, first) - 1)[seg]
        w = w / np.add.reduceat(w, first)[seg]
        res = np.add.reduceat(v[ri] * w[:, None], first, axis=0)
        rows = at + qi[first]
        out[rows] = res
        k[rows] = cnt
        vmax[rows] = np.maximum.reduceat(np.abs(v[ri]).max(axis=1), first)
    return out, k, vmax, margin


def interpolate_coord(flow, spacing, r, queries, t, forward):
    """the public call: (result, neighbour counts, per-row max |v|, margin); the result has shape (0, D) when no query found a
    neighbour"""
    D = len(spacing)
    rows, cc = select_rows(np.asarray(flow), t, forward, D)
    out, k, vmax, margin = interpolate(cc, rows[:, 1 + D:1 + 2 * D], rows[:, -1], spacing, r, queries)
    if not k.any():
        return np.zeros((0, D)), k, vmax, margin
    return out, k, vmax, margin


def interpolate_all(flow, spacing, r, coords, start_t, end_t, forward, min_track_num=0):
    """interpolate_all_forward / _backward with the rules above: (tracks, frame_num, smallest margin); coords is updated in
    place"""
    D = len(spacing)
    tracks, frame_num, margin = [], [], np.inf
    frames = list(range(start_t, end_t)) if forward else list(range(end_t, start_t + 1))[::-1]
    for t in frames:
        vec, _, _, m = interpolate_coord(flow, spacing, r, coords, t, forward)
        margin = min(margin, m)
        if len(vec) == 0:
            continue
        nxt = t + 1 if forward else t - 1
        for n in range(len(coords)):
            if np.all(np.isnan(vec[n])):
                coords[n] = np.nan
                continue
            if t == frames[0]:
                tracks.append([n + min_track_num, frames[0], *coords[n].tolist()])
                frame_num.append(frames[0])
            coords[n] = coords[n] + vec[n] if forward else coords[n] - vec[n]
            tracks.append([n + min_track_num, nxt, *coords[n].tolist()])
            frame_num.append(nxt)
    return tracks, frame_num, margin


def tolerance(k, vmax):
    """the issue's bound per row: 16 * k * 2^-52 * max(1, max_i |v_i|) -- reordering either sum moves the result by at most about
    k * 2^-53 * max|v| (all weights >= 1 after the shift, summing to 1 after normalisation); every other operation is the same
    IEEE operation on the same bits; 16 is the margin"""
    return 16.0 * np.asarray(k, np.float64) * 2.0 ** -52 * np.maximum(1.0, np.asarray(vmax, np.float64))


def assert_close(got, want, k, vmax, what=""):
    """identical NaN rows (no row is left out), values within tolerance(k, vmax) per row"""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaN rows differ", int(np.sum(np.isnan(got) != np.isnan(want))))
    assert np.array_equal(np.isnan(want).any(axis=1), np.asarray(k) == 0), (what, "NaN rows and neighbour counts disagree")
    err = np.nan_to_num(np.abs(got - want), nan=0.0).max(axis=1, initial=0.0)
    tol = tolerance(k, vmax)
    worst = float((err / np.maximum(tol, 1e-300)).max(initial=0.0))
    print(f"{what}: {len(got)} rows, {int(np.sum(np.asarray(k) > 0))} with neighbours, max k {int(np.max(k, initial=0))}, "
          f"max err {float(err.max(initial=0.0)):.3g}, worst err / bound {worst:.3g}")
    assert np.all(err <= tol), (what, float(err.max()), worst)
