"""numpy restatement of LabelTracks (the rules of DESIGN.md section 23), test infrastructure only -- never imported by the package.

Seeds: the voxels of labels[start_frame] that are > 0 (== label_num when given), raster order, every skip-th; ids = index in that
list + min_track_num.  Each direction follows flow_interpolation_restatement.interpolate_all's rules (the frames of `follow`
are its frames, the vectors its interpolate_coord; `follow` only builds the rows array-wise, and test_label_tracks_cpu.py holds
it to interpolate_all row for row).  The backward rows are reversed and ordered by id with kind="stable" -- id ascending, within
an id frame ascending -- and precede the forward rows.  A row stays if (frame, (z,) y, x), rounded half to even, lies inside the
label stack on a label > 0; a NaN or infinite coordinate goes.
"""
import numpy as np

import flow_interpolation_restatement as rs


def half_margin(coords):
    """the smallest distance of any finite coordinate from a half-integer (where rounding decides)"""
    c = np.asarray(coords, np.float64)
    c = c[np.isfinite(c)]
    if c.size == 0:
        return np.inf
    return float(np.min(np.abs(c - np.floor(c) - 0.5)))


def follow(flow, spacing, r, coords, start_t, end_t, forward, min_track_num=0):
    """interpolate_all as arrays: (rows (n, 2 + D), radius margin, largest neighbour count); coords is updated in place"""
    D = len(spacing)
    out, margin, kmax = [], np.inf, 0
    frames = list(range(start_t, end_t)) if forward else list(range(end_t, start_t + 1))[::-1]
    for t in frames:
        vec, k, _, m = rs.interpolate_coord(flow, spacing, r, coords, t, forward)
        margin = min(margin, m)
        kmax = max(kmax, int(np.max(k, initial=0)))
        if len(vec) == 0:
            continue
        lost = np.all(np.isnan(vec), axis=1)
        keep = np.nonzero(~lost)[0]
        ids = (keep + min_track_num).astype(np.float64)
        before = coords[keep].copy()
        coords[lost] = np.nan
        coords[keep] = before + vec[keep] if forward else before - vec[keep]
        nxt = t + 1 if forward else t - 1
        after = np.column_stack([ids, np.full(len(keep), float(nxt)), coords[keep]])
        if t == frames[0]:
            both = np.empty((2 * len(keep), 2 + D))
            both[0::2] = np.column_stack([ids, np.full(len(keep), float(t)), before])
            both[1::2] = after
            after = both
        out.append(after)
    return (np.concatenate(out) if out else np.zeros((0, 2 + D))), margin, kmax


def seeds(labels, start_frame, label_num=None, skip_coords=1):
    frame = np.asarray(labels[start_frame])
    coords = np.argwhere(frame > 0 if label_num is None else frame == label_num).astype(np.float64)
    return coords[::skip_coords].copy()


def keep_rows(labels, rows):
    """the final filter: which rows stay"""
    labels = np.asarray(labels)
    pos = rows[:, 1:]
    ok = np.all(np.isfinite(pos), axis=1)
    idx = np.zeros(pos.shape, np.int64)
    idx[ok] = np.rint(pos[ok]).astype(np.int64)
    ok &= np.all((idx >= 0) & (idx < np.asarray(labels.shape)), axis=1)
    ok[ok] = labels[tuple(idx[ok].T)] > 0
    return ok


def label_tracks(labels, flow, spacing, r, num_t=None, label_num=None, start_frame=0, end_frame=None, min_track_num=0, skip_coords=1):
    """(rows (n, 2 + D) float64, frame_num (n,) int64, info): info holds `ran` (False where LabelTracks.run returns ([], {})),
    `raw` (the unfiltered rows in the defined order, the first `n_back` of them backward rows), `radius_margin`, `half_margin`,
    `kmax` and `steps` (the longest chain of steps behind a coordinate)"""
    labels = np.asarray(labels)
    D = labels.ndim - 1
    flow = np.asarray(flow, np.float64)
    info = dict(ran=False, raw=np.zeros((0, 2 + D)), n_back=0, radius_margin=np.inf, half_margin=np.inf, kmax=0, steps=0)
    empty = np.zeros((0, 2 + D)), np.zeros(0, np.int64), info
    if end_frame is None:
        end_frame = labels.shape[0] if num_t is None else num_t
    if start_frame > labels.shape[0] - 1:
        return empty
    coords = seeds(labels, start_frame, label_num, skip_coords)
    if len(coords) == 0:
        return empty
    backup = coords.copy()
    parts = []
    if start_frame < end_frame:
        fw, m, k = follow(flow, spacing, r, coords, start_frame, end_frame, True, min_track_num)
        info.update(ran=True, radius_margin=min(info["radius_margin"], m), kmax=max(info["kmax"], k), steps=max(info["steps"], end_frame - start_frame))
        parts.append(fw)
    if start_frame > 0:
        bw, m, k = follow(flow, spacing, r, backup, start_frame, 0, False, min_track_num)
        info.update(ran=True, radius_margin=min(info["radius_margin"], m), kmax=max(info["kmax"], k), steps=max(info["steps"], start_frame + 1))
        bw = bw[::-1]
        info["n_back"] = len(bw)
        parts.insert(0, bw[np.argsort(bw[:, 0], kind="stable")])
    if not info["ran"]:
        return empty
    raw = np.concatenate(parts)
    info["raw"] = raw
    info["half_margin"] = half_margin(raw[:, 2:])
    rows = raw[keep_rows(labels, raw)]
    return rows, rows[:, 1].astype(np.int64), info


def sort_rows(rows):
    """rows in a stable lexicographic order by (id, frame): what two sides are compared in where the order within an id is not
    defined"""
    rows = np.asarray(rows, np.float64)
    if len(rows) == 0:
        return rows
    return rows[np.lexsort((rows[:, 1], rows[:, 0]))]
