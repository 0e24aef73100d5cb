"""numpy restatement of voxel reassignment (the rules of DESIGN.md section 12), test infrastructure only -- never imported by the
package.  No scipy: the nearest voxel is a chunked brute force in float64.

For a frame pair (t, t + 1) with voxel sets vox_prev / vox_next (argwhere of branch > 0 | obj > 0, raster order), spacing s and
radius r:

  forward   v = flow vectors at vox_prev for t (NaN rows dropped), c = vox_prev + v, m = nearest voxel of vox_next to c,
            candidate (prev voxel, m, d);
  backward  v = backward flow vectors at vox_next for t + 1, c = vox_next - v, m = nearest voxel of vox_prev, candidate (m, next voxel, d).

Nearest: d2 = sum over axes, in axis order, of (float64(float32(c)) * s - m * s)^2 (products first); a tie goes to the lowest
raveled index.  d = float32(sqrt(sum over axes in order of (float64(float32(c - m)) * s)^2)), kept when float64(d) < r.  Candidates are
the forward ones in vox_prev order, then the backward ones in vox_next order.  Best pair per target: smallest d, then the
earlier candidate.  Vote per label type: candidates whose source has reassigned[t] > 0 and whose target has label[t + 1] > 0,
weight 1 / (d + 1e-6); per target the weights are summed per source label in (label, -weight, candidate) order, one after the
other; the largest sum wins, a tie goes to the smaller label.

Every discrete decision comes with its margin (see `reassign`).  Each of the four rules can be turned into its opposite (`RULES`),
for tests that show a scene observes the rule; the default is the project's rule."""
import numpy as np

import flow_interpolation_restatement as fr


TIE = 1e-9          # squared distances within this (relative) of the nearest count as tied: margin (a)'s bound
# the opposite of each rule: a nearest-voxel tie goes to the highest index; d <= r is kept; the best pair is the later candidate
# on equal d; a vote tie goes to the larger label
RULES = ("nearest_highest", "radius_inclusive", "best_later", "vote_larger")


def select_match_coord_dtype(spatial_shape):
    if spatial_shape is None or len(spatial_shape) == 0:
        return np.uint16
    m = int(max(spatial_shape))
    if m <= 65536:
        return np.uint16
    if m <= 2 ** 32:
        return np.uint32
    return np.uint64


def error_distance(c, m, s):
    """float32(|float32(c - m) * s|): the squares are summed in axis order (what np.linalg.norm does over an axis of 2 or 3)"""
    diff = (c - m).astype(np.float32).astype(np.float64) * s
    d2 = diff[:, 0] * diff[:, 0]
    for a in range(1, diff.shape[1]):
        d2 = d2 + diff[:, a] * diff[:, a]
    return np.sqrt(d2).astype(np.float32)


def nearest(vox_real, c, s, r, pairs=4_000_000, highest=False):
    """per row of c: (index of the nearest voxel, lowest index on a tie; margin (a): (second d2 - nearest d2) / nearest d2 where the
    nearest lies within 1.01 r, inf elsewhere; the tie sets (e): {row: indices of the voxels tied for nearest -- d2 within TIE,
    relative, of the nearest: another summation order may decide those differently}, same rows)"""
    qs = c.astype(np.float32).astype(np.float64) * s
    ms = vox_real.astype(np.float64) * s
    n = len(qs)
    idx = np.zeros(n, np.int64)
    gap = np.full(n, np.inf)
    ties = {}
    step = max(1, pairs // max(1, len(ms)))
    lim = (1.01 * r) ** 2
    for at in range(0, n, step):
        q = qs[at:at + step]
        d2 = np.zeros((len(q), len(ms)))
        for a in range(qs.shape[1]):
            diff = q[:, a, None] - ms[None, :, a]
            d2 = d2 + diff * diff
        i = len(ms) - 1 - np.argmin(d2[:, ::-1], axis=1) if highest else np.argmin(d2, axis=1)
        best = d2[np.arange(len(q)), i]
        idx[at:at + step] = i
        near = np.nonzero(best <= lim)[0]
        if len(ms) > 1 and len(near):
            sub = d2[near]
            sub[np.arange(len(near)), i[near]] = np.inf
            second = sub.min(axis=1)
            with np.errstate(divide="ignore", invalid="ignore"):
                g = np.where(second == best[near], 0.0, (second - best[near]) / np.maximum(best[near], 1e-300))
            gap[at + near] = g
            for k in near[g <= TIE]:
                ties[at + int(k)] = np.nonzero(d2[k] <= best[k] * (1.0 + TIE))[0]
    return idx, gap, ties


def _direction(vox_q, vox_real, vec, sign, s, r, nearest_highest=False, radius_inclusive=False):
    """candidates of one direction: (query rows kept, matched rows of vox_real, d as float64), margins a and b, tie sets"""
    none = (np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0), np.inf, np.inf, {})
    if len(vec) == 0:
        return none
    qi = np.nonzero(~np.isnan(vec).any(axis=1))[0]
    if len(qi) == 0:
        return none
    c = vox_q[qi] + vec[qi] if sign > 0 else vox_q[qi] - vec[qi]
    m, gap, ties = nearest(vox_real, c, s, r, highest=nearest_highest)
    d = error_distance(c, vox_real[m], s)
    margin_b = float(np.min(np.abs(d.astype(np.float64) - r))) / r
    keep = d.astype(np.float64) < r                      # the reference compares the float32 d with a float64 radius
    if radius_inclusive:
        keep = d.astype(np.float64) <= r
    ties = {int(qi[k]): v for k, v in ties.items()}
    return qi[keep], m[keep], d[keep].astype(np.float64), float(gap.min()), margin_b, ties


def best_pairs(src, tgt, d, later=False):
    """per target the candidate with the smallest d, the earlier one on a tie, in target order; margin (d)"""
    order = np.lexsort((-np.arange(len(d)) if later else np.arange(len(d)), d, tgt))
    ts, ds = tgt[order], d[order]
    first = np.concatenate([[True], ts[1:] != ts[:-1]])
    same = ~first[1:] & first[:-1]                       # second entry of a target with several
    margin = np.inf
    if same.any():
        a, b = ds[:-1][same], ds[1:][same]
        margin = float(np.min((b - a) / np.maximum(b, 1e-300)))
    return order[first], margin


def vote(tgt, labels, d, larger=False):
    """(targets, winning labels, margin (c)): weights summed per (target, label) in (label, -weight, candidate) order"""
    w = 1.0 / (d + 1e-6)
    order = np.lexsort((np.arange(len(w)), -w, labels, tgt))
    ts, ls, ws = tgt[order], labels[order], w[order]
    start = np.concatenate([[True], (ts[1:] != ts[:-1]) | (ls[1:] != ls[:-1])])
    first = np.nonzero(start)[0]
    seg = np.cumsum(start) - 1
    pos = np.arange(len(ws)) - first[seg]
    sums = np.zeros(len(first))
    for k in range(int(pos.max(initial=-1)) + 1):        # one after the other: sum = ((w0 + w1) + w2) + ...
        at = pos == k
        sums[seg[at]] = sums[seg[at]] + ws[at] if k else ws[at]
    pt, plab = ts[first], ls[first]
    order2 = np.lexsort((-plab if larger else plab, -sums, pt))
    pt2, pl2, ps2 = pt[order2], plab[order2], sums[order2]
    head = np.concatenate([[True], pt2[1:] != pt2[:-1]])
    second = ~head[1:] & head[:-1]
    margin = np.inf
    if second.any():
        margin = float(np.min((ps2[:-1][second] - ps2[1:][second]) / ps2[:-1][second]))
    return pt2[head], pl2[head], margin


def reassign(branch, obj, flow, spacing, r, store_running_matches=True, max_refine_iterations=3, interp=None, nearest_highest=False,
             radius_inclusive=False, best_later=False, vote_larger=False):
    """branch / obj: (T, ...) label stacks.  interp(coords, t, forward) -> flow vectors (n, D), NaN rows, or shape (0, D); by
    default the flow restatement on `flow`.  Returns a dict:
      reassigned_branch, reassigned_obj  int32 stacks
      running_matches                    list of [prev coords, next coords] per frame pair (None when not stored)
      margin_a .. margin_d               the smallest margin of each kind over the run (inf when no decision of the kind arose)
      tainted                            per frame pair a bool mask over the frame: the targets whose candidates rest on a tie of
                                         the nearest-voxel step (the voxels of a forward query's tie set, a tied backward query itself)
      min_max_k                          the smallest, over the interpolation calls that found a neighbour, of the largest neighbour
                                         count of a call (0 when none did)
      pairs                              the number of frame pairs that ran to the end
      tie_sets                           the number of queries whose nearest-voxel step was tied
      max_candidates                     the longest candidate list of a target
      zero_ties                          per frame pair a bool mask over the frame: the targets with two or more candidates at d = 0
    The four keywords after `interp` turn a rule into its opposite (RULES)."""
    branch, obj = np.asarray(branch), np.asarray(obj)
    T, shape = branch.shape[0], branch.shape[1:]
    D = len(shape)
    s = np.asarray(spacing, np.float64)
    flow = None if flow is None else np.asarray(flow, np.float64)
    ks = []
    if interp is None:
        def interp(coords, t, forward):
            out, k, _, _ = fr.interpolate_coord(flow, s, r, coords, t, forward)
            ks.append(int(k.max(initial=0)))
            return out
    re_b, re_o = np.zeros(branch.shape, np.int32), np.zeros(obj.shape, np.int32)
    re_b[0][branch[0] > 0] = branch[0][branch[0] > 0]
    re_o[0][obj[0] > 0] = obj[0][obj[0] > 0]
    dtype = select_match_coord_dtype(shape)
    res = dict(margin_a=np.inf, margin_b=np.inf, margin_c=np.inf, margin_d=np.inf, tainted=[], pairs=0, tie_sets=0, max_candidates=0, zero_ties=[])
    how = dict(nearest_highest=nearest_highest, radius_inclusive=radius_inclusive)
    matches = []
    for t in range(T - 1):
        vox_prev = np.argwhere((branch[t] > 0) | (obj[t] > 0))
        vox_next = np.argwhere((branch[t + 1] > 0) | (obj[t + 1] > 0))
        if len(vox_prev) == 0 or len(vox_next) == 0:
            break
        fq, fm, fd, fa, fb, fties = _direction(vox_prev, vox_next, np.asarray(interp(vox_prev, t, True), np.float64).reshape(-1, D), 1, s, r, **how)
        bq, bm, bd, ba, bb, bties = _direction(vox_next, vox_prev, np.asarray(interp(vox_next, t + 1, False), np.float64).reshape(-1, D), -1, s, r, **how)
        res["margin_a"] = min(res["margin_a"], fa, ba)
        res["margin_b"] = min(res["margin_b"], fb, bb)
        taint = np.zeros(shape, bool)
        for v in fties.values():
            taint[tuple(vox_next[v].T)] = True
        if bties:
            taint[tuple(vox_next[np.fromiter(bties, np.int64)].T)] = True
        res["tainted"].append(taint)
        res["tie_sets"] += len(fties) + len(bties)
        src = np.concatenate([fq, bm])                   # rows of vox_prev
        tgt = np.concatenate([fm, bq])                   # rows of vox_next
        d = np.concatenate([fd, bd])
        if len(src) == 0:
            break
        res["max_candidates"] = max(res["max_candidates"], int(np.bincount(tgt).max()))
        zero = np.zeros(shape, bool)
        zero[tuple(vox_next[np.nonzero(np.bincount(tgt[d == 0], minlength=len(vox_next)) > 1)[0]].T)] = True
        res["zero_ties"].append(zero)
        if store_running_matches:
            best, md = best_pairs(src, tgt, d, later=best_later)
            res["margin_d"] = min(res["margin_d"], md)
            matches.append([vox_prev[src[best]].astype(dtype), vox_next[tgt[best]].astype(dtype)])
        for lab, re in ((branch, re_b), (obj, re_o)):
            prev_labels = re[t][tuple(vox_prev[src].T)]
            ok = (prev_labels > 0) & (lab[t + 1][tuple(vox_next[tgt].T)] > 0)
            c_tgt, c_lab, c_d = tgt[ok], prev_labels[ok], d[ok]
            for _ in range(max(1, int(max_refine_iterations))):
                un = re[t + 1][tuple(vox_next[c_tgt].T)] == 0
                if not un.any():
                    break
                wt, wl, mc = vote(c_tgt[un], c_lab[un], c_d[un], larger=vote_larger)
                res["margin_c"] = min(res["margin_c"], mc)
                re[t + 1][tuple(vox_next[wt].T)] = wl
        res["pairs"] += 1
    res.update(reassigned_branch=re_b, reassigned_obj=re_o, running_matches=matches if store_running_matches else None,
               min_max_k=min((k for k in ks if k > 0), default=0))
    return res


def save_matches(path, matches):
    """the reference's call, shape quirks included (voxel_reassignment.py:1062)"""
    np.save(path, np.array(matches, dtype=object))
