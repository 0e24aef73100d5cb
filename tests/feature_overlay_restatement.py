"""The analysis overlay restated in numpy (reference nellie_napari/nellie_analysis.py:964-1192); test infrastructure only.

`overlay_literal` is the definition: dense matrices in the reference's own order of operations and memory layouts -- a boolean
(voxels x groups) matrix per frame, its transposed copy (which keeps the Fortran order of the transpose), zero padding below it up
to the largest table label (np.vstack), the product with the column, NaN off the edges, and
np.nanmean down the groups.  np.nanmean sums with np.sum from +0.0: row by row down a C-ordered matrix, and as pairwise trees over
pieces of 8192 entries down a contiguous column (a Fortran-ordered matrix, or a matrix one voxel wide).  np.vstack of the
Fortran-ordered matrix and ONE row of padding (a single row is contiguous either way) is Fortran-ordered again; two rows or more
make it C-ordered.  Which of the two sums a frame gets therefore depends on how far the table's largest label reaches past the
largest group index: by at most one, pairwise; by more, row by row.

`overlay_sparse` gives the same values from the edge list alone: distinct groups per voxel, the column gathered, the sum in the order
that `column_sum` / ascending order prescribes.  `same` is the equality of the tests: equal values, NaN in the same places, zeros of
the same sign; NaN payloads are not compared.
"""
import warnings

import numpy as np

LEVELS = ("voxel", "node", "branch", "organelle")
EDGE_KEYS = {"node": "v_n", "branch": "v_b", "organelle": "v_o"}
LEAF, BLOCK = 128, 8192                    # numpy's PW_BLOCKSIZE and its ufunc buffer in elements


def same(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype.kind != "f":
        return bool(np.array_equal(got, want))
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan], want[~nan]) and np.array_equal(np.signbit(got[~nan]), np.signbit(want[~nan])))


def frame_list(edge_frames, t):
    return None if edge_frames is None or t >= len(edge_frames) else edge_frames[t]


# ---- the literal form ------------------------------------------------------------------------------------------------------------------
def literal_values(n_rows, level, labels, vals, edges):
    """(n_rows,) float64 for one frame, or None when the rule leaves the frame NaN.  `labels`, `vals`: the frame's table rows."""
    vals = np.asarray(vals).astype(float)
    if len(vals) == 0:
        return None
    if level == "voxel":
        return vals if len(vals) == n_rows else None
    if n_rows == 0 or edges is None or np.size(edges) == 0:
        return None
    edges = np.asarray(edges)
    groups = int(np.max(edges[:, 1])) + 1
    by_voxel = np.zeros((n_rows, groups), dtype=bool)
    by_voxel[edges[:, 0], edges[:, 1]] = True
    by_group = np.array(by_voxel.T)                                # a copy in the transpose's own (Fortran) order
    labels = np.asarray(labels).astype(int)
    max_idx = max(by_group.shape[0], int(np.max(labels)) + 1)
    if by_group.shape[0] < max_idx:
        by_group = np.vstack([by_group, np.zeros((max_idx - by_group.shape[0], by_group.shape[1]), dtype=bool)])
    attr_vec = np.full(max_idx, np.nan)
    attr_vec[labels] = vals
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        spread = by_group * attr_vec.reshape(-1, 1)
        spread[~by_group] = np.nan
        return np.nanmean(spread, axis=0)


def overlay_literal(label_stack, level, t_col, label_col, val_col, edge_frames):
    """the (T, ...) float64 stack: NaN, and at the voxels with label > 0 of every frame the rule's value"""
    label_stack = np.asarray(label_stack)
    out = np.full(label_stack.shape, np.nan)
    t_col = np.asarray(t_col)
    for t in range(label_stack.shape[0]):
        coords = np.argwhere(label_stack[t] > 0)
        rows = t_col == t
        vals = literal_values(len(coords), level, np.asarray(label_col)[rows], np.asarray(val_col)[rows], frame_list(edge_frames, t))
        if vals is not None:
            out[t][tuple(coords.T)] = vals
    return out


def contrast_limits(column):
    """nellie_analysis.py:1172-1187 on a plain array"""
    v = np.asarray(column, dtype=float)
    v = np.where(np.isinf(v), np.nan, v)
    v = v[~np.isnan(v)]
    if len(v) == 0:
        return [0.0, 1.0]
    perc98 = float(np.nanpercentile(v, 98))
    lowest = float(np.nanmin(v))
    lowest = lowest - (abs(lowest) * 0.01)
    if np.isnan(lowest):
        lowest = float(np.nanmin(v))
    if lowest == perc98:
        perc98 = lowest + (abs(lowest) * 0.01)
    if np.isnan(perc98):
        perc98 = float(np.nanmax(v))
    return [lowest, perc98]


def as_labels(frames):
    """the uint64 label volume of float frames: the truncated value, 0 where it is NaN, negative or infinite (or 2^64 and above)"""
    f = np.asarray(frames, dtype=np.float64)
    ok = np.isfinite(f) & (f >= 1.0) & (f < 2.0 ** 64)
    out = np.zeros(f.shape, np.uint64)
    out[ok] = f[ok].astype(np.uint64)
    return out


# ---- the sparse form -------------------------------------------------------------------------------------------------------------------
def _tree(pos, vals, lo, n):
    """numpy's pairwise sum of the n column entries from lo on, of which those at `pos` (ascending) hold `vals` and the others +0.0"""
    if len(pos) == 0:
        return 0.0
    if n <= LEAF:
        res = 0.0
        if n >= 8:
            m8 = lo + n - n % 8
            r = [0.0] * 8
            for p, v in zip(pos, vals):
                if p < m8:
                    r[(p - lo) % 8] = r[(p - lo) % 8] + v
            res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
            keep = pos >= m8
            pos, vals = pos[keep], vals[keep]
        for v in vals:
            res = res + v
        return res
    n2 = n // 2
    n2 -= n2 % 8
    k = int(np.searchsorted(pos, lo + n2))
    return _tree(pos[:k], vals[:k], lo, n2) + _tree(pos[k:], vals[k:], lo + n2, n - n2)


def column_sum(pos, vals, n, pairwise):
    """np.sum of a float64 column of n entries, +0.0 but for `vals` at the ascending positions `pos`: from +0.0, one add per entry
    (pairwise false), or the pairwise tree of every piece of BLOCK entries (pairwise true)"""
    pos, vals = np.asarray(pos, np.int64), [float(v) for v in vals]
    total = 0.0
    with np.errstate(all="ignore"):
        if not pairwise:
            for v in vals:
                total = total + v
            return total
        vals = np.asarray(vals, np.float64)
        for base in np.unique(pos // BLOCK) * BLOCK:
            k = (pos >= base) & (pos < base + BLOCK)
            total = total + _tree(pos[k], vals[k], int(base), int(min(BLOCK, n - base)))
    return float(total)


def attr_vector(labels, vals, groups, shift=0):
    idx = np.asarray(labels).astype(int) - shift
    if (idx < 0).any():
        raise ValueError("a label below the first index")
    vec = np.full(max(groups, int(idx.max()) + 1), np.nan)
    for i, v in zip(idx, np.asarray(vals, float)):                # a repeated label keeps its last row
        vec[i] = v
    return vec


def sparse_values(n_rows, level, labels, vals, edges, align_branches=False):
    """literal_values without a matrix; align_branches: the branch column is indexed by label - 1"""
    vals = np.asarray(vals, dtype=np.float64)
    if len(vals) == 0:
        return None
    if level == "voxel":
        return vals if len(vals) == n_rows else None
    if n_rows == 0 or edges is None or np.size(edges) == 0:
        return None
    e = np.unique(np.asarray(edges, np.int64).reshape(-1, 2), axis=0)       # distinct (voxel, group), ascending in both
    groups = int(e[:, 1].max()) + 1
    vec = attr_vector(labels, vals, groups, shift=1 if level == "branch" and align_branches else 0)
    return edge_values(n_rows, e, vec, groups)


def edge_values(n_rows, e, vec, groups=None):
    """the rows' means for distinct ascending edges e and the column by group index vec"""
    groups = int(e[:, 1].max()) + 1 if groups is None else groups
    pairwise = len(vec) <= groups + 1 or n_rows == 1             # no padding, one row of it (np.vstack keeps the Fortran order), or one voxel
    v = vec[e[:, 1]]
    ok = ~np.isnan(v)
    rows, pos, v = e[ok, 0], e[ok, 1], v[ok]
    cnt = np.bincount(rows, minlength=n_rows)
    with np.errstate(all="ignore"):
        total = np.bincount(rows, weights=v, minlength=n_rows)     # exact for one or two terms in any order
        start = np.concatenate([[0], np.cumsum(cnt)])
        for r in np.flatnonzero(cnt >= 3):
            a, b = start[r], start[r + 1]
            total[r] = column_sum(pos[a:b], v[a:b], len(vec), pairwise)
        out = np.full(n_rows, np.nan)
        has = cnt > 0
        out[has] = (total[has] + 0.0) / cnt[has]
    return out


def overlay_sparse(label_stack, level, t_col, label_col, val_col, edge_frames, align_branches=False):
    label_stack = np.asarray(label_stack)
    out = np.full(label_stack.shape, np.nan)
    t_col = np.asarray(t_col)
    for t in range(label_stack.shape[0]):
        on = label_stack[t] > 0
        rows = t_col == t
        vals = sparse_values(int(on.sum()), level, np.asarray(label_col)[rows], np.asarray(val_col)[rows], frame_list(edge_frames, t), align_branches)
        if vals is not None:
            out[t][on] = vals
    return out
