"""
numpy restatement of Nellie's Hu-moment tracking arithmetic (nellie/tracking/hu_tracking.py, dense ROI path), written from the
arithmetic DESIGN.md's tracking section states.  The GPU tests compare the HIP stage with it on random cases; the CPU tests check
it against the captured goldens.

    frame_features(intensity, frangi, distance, marker, scaling)  -> coords (N, d) int64, phys (N, d) float64,
                                                                     stats (N, 4) float32, log_hu (N, 6 or 18) float64
    dense_costs(...)                                              -> (N_post, N_pre) float16 cost matrix
    match_dense(...) / match_sparse(...)                          -> row indices, column indices, costs
    track(frames, scaling, ...)                                   -> flow_vector_array
"""
from __future__ import annotations

import numpy as np


# ---------------------------------------------------------------------------------------------------------- features
def normalise_frangi(frangi):
    fr = np.asarray(frangi, dtype=np.float32).copy()
    pos = fr > 0
    if pos.any():
        fr[pos] = np.log10(fr[pos])
    neg = fr < 0
    if neg.any():
        fr[neg] -= fr[neg].min()
    return fr


def _max3(distance):
    """size-3 maximum filter, faces clamped (= scipy's 'reflect' for size 3)"""
    d = np.asarray(distance, dtype=np.float32)
    out = d.copy()
    for ax in range(d.ndim):
        p = np.pad(out, [(1, 1) if a == ax else (0, 0) for a in range(d.ndim)], mode="edge")
        sl = lambda k: tuple(slice(k, k + d.shape[ax]) if a == ax else slice(None) for a in range(d.ndim))  # noqa: E731
        out = np.maximum(np.maximum(p[sl(0)], p[sl(1)]), p[sl(2)])
    return out


def _stats(roi, R):
    """[mean, variance] of the non-zero voxels with the reference's dtypes (integer squares wrap in the input dtype; float32
    sums are numpy's pairwise sums over the ROI zero-padded to R^d and flattened)"""
    m = roi != 0
    cnt = int(m.sum())
    if cnt == 0:
        return 0.0, 0.0
    v = roi * m
    if roi.dtype.kind in "ui":
        s = np.sum(v, dtype=np.uint64)
        sq = np.sum(v ** 2, dtype=np.uint64)               # v ** 2 wraps in the input dtype
        s2 = np.uint64(s) * np.uint64(s)                   # wraps in uint64 like sum_nonzero ** 2
        mean = float(s) / cnt
        var = (float(sq) - float(s2) / cnt) / cnt
    else:
        pad = np.zeros((R,) * roi.ndim, np.float32)
        pad[tuple(slice(0, k) for k in roi.shape)] = v
        s = np.sum(pad.ravel())
        sq = np.sum((pad * pad).ravel())
        mean = float(s) / cnt
        var = (float(sq) - float(np.float32(s * s)) / cnt) / cnt
    return mean, var


def _moments(img):
    """log-Hu of one 2-D image (rows = y, columns = x)"""
    h, w = img.shape
    y, x = np.mgrid[0:h, 0:w]
    if img.dtype.kind in "ui":
        v = img.astype(np.int64)
        M = np.array([[np.sum(v * x ** p * y ** q) for q in range(4)] for p in range(4)], dtype=np.int64)
        M = M.astype(np.float64)
    else:
        v = img.astype(np.float64)
        M = np.array([[np.sum((v * x ** p) * y ** q) for q in range(4)] for p in range(4)])
    xb = M[1, 0] / (M[0, 0] + 1e-12)
    yb = M[0, 1] / (M[0, 0] + 1e-12)
    dx, dy = x - xb, y - yb
    pw = lambda a, k: np.ones_like(a) if k == 0 else (a if k == 1 else (a * a if k == 2 else a * a * a))  # noqa: E731
    mu = np.array([[np.sum((img.astype(np.float64) * pw(dx, p)) * pw(dy, q)) for q in range(4)] for p in range(4)])
    eta = np.empty((4, 4))
    for p in range(4):
        for q in range(4):
            eta[p, q] = mu[p, q] / (M[0, 0] ** ((p + q + 2) / 2.0) + 1e-12)
    e20, e02, e11, e30, e12, e21, e03 = eta[2, 0], eta[0, 2], eta[1, 1], eta[3, 0], eta[1, 2], eta[2, 1], eta[0, 3]
    a, b = e30 + e12, e21 + e03
    hu = np.array([
        e20 + e02,
        (e20 - e02) ** 2 + 4 * e11 ** 2,
        (e30 - 3 * e12) ** 2 + (3 * e21 - e03) ** 2,
        a ** 2 + b ** 2,
        (e30 - 3 * e12) * a * (a ** 2 - 3 * b ** 2) + (3 * e21 - e03) * b * (3 * a ** 2 - b ** 2),
        (e20 - e02) * (a ** 2 - b ** 2) + 4 * e11 * a * b,
    ])
    with np.errstate(all="ignore"):
        lh = -np.sign(hu) * np.log10(np.maximum(np.abs(hu), np.finfo(np.float64).tiny))
    return np.where(np.isfinite(lh), lh, 0.0)


def frame_features(intensity, frangi, distance, marker, scaling):
    """One frame: (coords int64, phys float64, stats float32 (N, 4), log_hu float64 (N, 6 | 18))."""
    intensity = np.asarray(intensity)
    two_d = intensity.ndim == 2
    d = intensity.ndim
    coords = np.argwhere(np.asarray(marker) > 0).astype(np.int64)
    n = len(coords)
    nh = 6 if two_d else 18
    if n == 0:
        return coords.reshape(0, d), np.zeros((0, d)), np.zeros((0, 4), np.float32), np.zeros((0, nh))
    phys = coords * np.asarray(scaling, dtype=float)
    fr = normalise_frangi(frangi)
    dmax = _max3(distance) * np.float32(2)
    radii = np.ceil(dmax[tuple(coords.T)])
    R = int(np.ceil(radii.max())) * 2 + 1
    stats = np.zeros((n, 4), np.float32)
    hu = np.zeros((n, nh))
    for k, c in enumerate(coords):
        r = radii[k]
        lo = [int(np.clip(c[a] - r, 0, intensity.shape[a])) for a in range(d)]
        hi = [int(np.clip(c[a] + (r + 1), 0, intensity.shape[a])) for a in range(d)]
        sl = tuple(slice(lo[a], hi[a]) for a in range(d))
        roi, froi = intensity[sl], fr[sl]
        stats[k] = (*_stats(roi, R), *_stats(froi, R))
        pad = np.zeros((R,) * d, dtype=intensity.dtype)
        pad[tuple(slice(0, hi[a] - lo[a]) for a in range(d))] = roi
        if two_d:
            hu[k] = _moments(pad)
        else:
            hu[k] = np.concatenate([_moments(pad.max(axis=0)), _moments(pad.max(axis=1)), _moments(pad.max(axis=2))])
    return coords, phys, stats, hu


# ---------------------------------------------------------------------------------------------------------- matching
def half_round(x):
    """float64 -> float16, rounded once (numpy's astype does this)"""
    return np.asarray(x, dtype=np.float64).astype(np.float16)


def half_nansum(z16):
    """np.nansum(z16, axis=-1) for float16: NaN -> 0, float32 pairwise sum (8 accumulators), rounded to half"""
    a = np.nan_to_num(np.asarray(z16, np.float16).astype(np.float32), nan=0.0, posinf=np.inf, neginf=-np.inf)
    k = a.shape[-1]
    if k < 8:
        res = np.zeros(a.shape[:-1], np.float32)
        for i in range(k):
            res = res + a[..., i]
    else:
        r = [a[..., j].copy() for j in range(8)]
        for i in range(8, k - k % 8, 8):
            for j in range(8):
                r[j] = r[j] + a[..., i + j]
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for i in range(k - k % 8, k):
            res = res + a[..., i]
    return res.astype(np.float16)


def _z(m, mask):
    cnt = mask.sum()
    mean = (m * mask[..., None]).sum(axis=(0, 1)) / cnt
    var = (((m - mean) ** 2) * mask[..., None]).sum(axis=(0, 1)) / cnt
    z = (m - mean) / (np.sqrt(var) + 1e-8)
    return np.where(mask[..., None], z, np.inf)


def dense_costs(phys_post, phys_pre, st_post, st_pre, hu_post, hu_pre, maxd):
    """(N_post, N_pre) float16 costs of _get_cost_matrix (None when no pair lies within reach)"""
    d = np.sqrt(((phys_post[:, None, :] - phys_pre[None, :, :]) ** 2).sum(axis=2))
    mask = d < maxd
    if not mask.any():
        return None
    zd = half_round(_z((d / maxd)[..., None], mask))
    sd = np.abs(st_post[:, None, :].astype(np.float64) - st_pre[None, :, :].astype(np.float64))
    zs = half_round(_z(sd, mask) / sd.shape[2])
    hd = np.abs(hu_post[:, None, :].astype(np.float64) - hu_pre[None, :, :].astype(np.float64))
    zh = half_round(_z(hd, mask) / hd.shape[2])
    with np.errstate(invalid="ignore"):
        return half_nansum(np.concatenate((zd, zs, zh), axis=2))


def best_of(cost16):
    """(row argmin, row min, column argmin, column min) of a float16 cost matrix as float32, numpy's first-index rule"""
    c = cost16.astype(np.float32)
    return np.argmin(c, axis=1), np.min(c, axis=1), np.argmin(c, axis=0), np.min(c, axis=0)


def match_dense(phys_post, phys_pre, st_post, st_pre, hu_post, hu_pre, maxd):
    if len(phys_post) == 0 or len(phys_pre) == 0:
        return [], [], []
    c = dense_costs(phys_post, phys_pre, st_post, st_pre, hu_post, hu_pre, maxd)
    if c is None:
        return [], [], []
    ri, rv, ci, cv = best_of(c)
    rows, cols, costs = [], [], []
    for i in range(len(ri)):
        if not rv[i] > 1.0:
            rows.append(i); cols.append(int(ri[i])); costs.append(float(rv[i]))
    for j in range(len(ci)):
        if not cv[j] > 1.0:
            rows.append(int(ci[j])); cols.append(j); costs.append(float(cv[j]))
    return rows, cols, costs


def _pw_mean(a):
    """np.mean(a, axis=1) of a float64 (k, F) block"""
    return np.mean(a, axis=1)


def match_sparse(phys_post, phys_pre, st_post, st_pre, hu_post, hu_pre, maxd):
    n_post, n_pre = len(phys_post), len(phys_pre)
    if n_post == 0 or n_pre == 0:
        return [], [], []
    st_post, st_pre = np.asarray(st_post, np.float32), np.asarray(st_pre, np.float32)
    hu_post, hu_pre = np.asarray(hu_post, np.float32), np.asarray(hu_pre, np.float32)
    cand = []                                                                # cKDTree.query_ball_point, sorted
    for b0 in range(0, n_post, 256):                                         # row blocks: no N x N matrix at 57 k markers
        p = phys_post[b0:b0 + 256]
        d2 = ((p[:, None, 0] - phys_pre[None, :, 0]) ** 2 + (p[:, None, 1] - phys_pre[None, :, 1]) ** 2)
        if phys_post.shape[1] == 3:
            d2 = d2 + (p[:, None, 2] - phys_pre[None, :, 2]) ** 2
        cand += [np.nonzero(row <= maxd * maxd)[0] for row in d2]
    n = 0
    s = np.zeros(2); ss = np.zeros((2, st_post.shape[1])); sh = np.zeros((2, hu_post.shape[1]))
    blocks = []
    for i, idx in enumerate(cand):
        if idx.size == 0:
            blocks.append(None)
            continue
        dg = np.linalg.norm(phys_post[i] - phys_pre[idx], axis=1) / maxd
        sd = np.abs(st_post[i][None, :] - st_pre[idx])
        hd = np.abs(hu_post[i][None, :] - hu_pre[idx])
        blocks.append((dg, sd, hd))
        s += (float(np.sum(dg)), float(np.sum(dg * dg)))
        ss += (np.sum(sd, axis=0, dtype=np.float64), np.sum(sd * sd, axis=0, dtype=np.float64))
        sh += (np.sum(hd, axis=0, dtype=np.float64), np.sum(hd * hd, axis=0, dtype=np.float64))
        n += dg.size
    if n == 0:
        return [], [], []
    md = s[0] / n
    sdv = np.sqrt(max(0.0, s[1] / n - md ** 2)) + 1e-8
    ms = ss[0] / n
    sds = np.sqrt(np.maximum(ss[1] / n - ms ** 2, 0.0)) + 1e-8
    mh = sh[0] / n
    sdh = np.sqrt(np.maximum(sh[1] / n - mh ** 2, 0.0)) + 1e-8
    row_v = np.full(n_post, np.inf, np.float32); row_i = np.full(n_post, -1, np.int64)
    col_v = np.full(n_pre, np.inf, np.float32); col_i = np.full(n_pre, -1, np.int64)
    for i, b in enumerate(blocks):
        if b is None:
            continue
        dg, sd, hd = b
        cost = (dg - md) / sdv + _pw_mean((sd - ms) / sds) + _pw_mean((hd - mh) / sdh)
        ok = cost <= 1.0
        if not ok.any():
            continue
        cv, iv = cost[ok], cand[i][ok]
        k = int(np.argmin(cv))
        if float(cv[k]) < row_v[i]:
            row_v[i] = cv[k]; row_i[i] = iv[k]
        for j, c in zip(iv, cv):
            if float(c) < col_v[j]:
                col_v[j] = c; col_i[j] = i
    rows, cols, costs = [], [], []
    for i in range(n_post):
        if row_i[i] >= 0 and row_v[i] <= 1.0:
            rows.append(i); cols.append(int(row_i[i])); costs.append(float(row_v[i]))
    for j in range(n_pre):
        if col_i[j] >= 0 and col_v[j] <= 1.0:
            rows.append(int(col_i[j])); cols.append(j); costs.append(float(col_v[j]))
    return rows, cols, costs


def vectors(t, coords_post, coords_pre, rows, cols, costs):
    """the frame pair's rows of flow_vector_array (hu_tracking.py:1186-1222)"""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    pre, post = coords_pre[cols], coords_post[rows]
    v = post - pre
    return np.column_stack([np.full(len(rows), t - 1, np.int64), *pre.T.astype(np.int64), *v.T.astype(np.int64),
                            np.asarray(costs, np.float32)])


def track(frames, scaling, dt=1.0, max_distance_um=1.0, mode="auto", max_dense_pairs=int(1e7), features=None):
    """frames: list of (intensity, frangi, distance, marker) per t.  features: precomputed frame_features per t (optional)."""
    maxd = max(max_distance_um * (dt if dt is not None else 1.0), 0.5)
    ndim = np.asarray(frames[0][0]).ndim
    out, prev = [], None
    for t, fr in enumerate(frames):
        cur = features[t] if features is not None else frame_features(*fr, scaling)
        if prev is not None and len(cur[0]) and len(prev[0]):
            dense = mode == "dense" or (mode == "auto" and len(cur[0]) * len(prev[0]) <= max_dense_pairs)
            fn = match_dense if dense else match_sparse
            r, c, k = fn(cur[1], prev[1], cur[2], prev[2], cur[3], prev[3], maxd)
            if len(r):
                out.append(vectors(t, cur[0], prev[0], r, c, k))
        prev = cur
    if out:
        return np.concatenate(out, axis=0)
    return np.empty((0, 6 if ndim == 2 else 8), np.float32)
