"""numpy restatement of the label transitions (the rule of DESIGN.md section 26), test infrastructure only -- never imported by the
package.  It restates what the reference's scripts/voxel_reassignment_demo.py does with `voxel_matches`: both ends of every match
are mapped to a label, the label pairs are counted (`accumulate_pair_counts`, lines 15-48), and frame t + 1 is painted with the
argmax over the sources of every destination (lines 96-110).

One frame pair t -> t + 1: `prev`, `next` (n, D) unsigned coordinates, label frames A (frame t) and B (frame t + 1).

  gather   a_k = A[prev_k], b_k = B[next_k].  A coordinate outside the frame is a ValueError naming the lowest such row; a gathered
           label below 0 or above 2^31 - 1 is a ValueError, before anything is counted; rows with a_k == 0 or b_k == 0 are dropped
           and counted in n_dropped.
  table    the distinct (a, b) of the kept rows in lexicographic order with their multiplicities: (E, 3) int64 (src, dst, count).
  dense    M[a - 1, b - 1] = count, uint32 (n_src, n_dst): the demo's matrix.
  best_src per destination in the table the source with the largest count, the smallest source on a tie (np.argmax's first
           occurrence over ascending sources); best_dst the same the other way round.
  events   edges with count >= min_count; fission: sources with two or more of them, fusion: destinations with two or more.
  relabel  frame t + 1 with every label b > 0 replaced by best_src[b], int32; a label without a counted pair becomes 0 (the demo's
           argmax of an all-zero column is 0, so it paints label 1: the deliberate difference)."""
import numpy as np

MAX_LABEL = 2 ** 31 - 1


def gather(prev, next, A, B):
    """-> (a, b) int64 labels of every row; raises as the rule says"""
    prev, next = np.asarray(prev), np.asarray(next)
    A, B = np.asarray(A), np.asarray(B)
    D = A.ndim
    if prev.ndim != 2 or prev.shape != next.shape or prev.shape[1] != D or A.shape != B.shape:
        raise ValueError(f"coordinates {prev.shape} / {next.shape} for frames {A.shape} / {B.shape}")
    bad = np.zeros(len(prev), bool)
    for c in (prev, next):
        c = c.astype(np.int64)                           # a uint64 of 2^63 or more wraps below 0: outside either way
        bad |= ((c < 0) | (c >= np.asarray(A.shape, np.int64))).any(axis=1)
    if bad.any():
        raise ValueError(f"row {int(np.nonzero(bad)[0][0])} holds a coordinate outside the frame {A.shape}")
    a = A[tuple(prev.astype(np.int64).T)].astype(np.int64) if len(prev) else np.zeros(0, np.int64)
    b = B[tuple(next.astype(np.int64).T)].astype(np.int64) if len(prev) else np.zeros(0, np.int64)
    wrong = (a < 0) | (a > MAX_LABEL) | (b < 0) | (b > MAX_LABEL)
    if wrong.any():
        k = int(np.nonzero(wrong)[0][0])
        raise ValueError(f"row {k} gathers a label outside [0, 2^31 - 1]: {int(a[k])}, {int(b[k])}")
    return a, b


def table_of(a, b):
    """-> ((E, 3) int64, n_dropped): np.unique over the kept rows"""
    keep = (a != 0) & (b != 0)
    n_dropped = int((~keep).sum())
    if not keep.any():
        return np.zeros((0, 3), np.int64), n_dropped
    pairs, counts = np.unique(np.stack([a, b], 1)[keep], axis=0, return_counts=True)
    return np.column_stack([pairs, counts]).astype(np.int64), n_dropped


def transition_counts(prev, next, A, B):
    return table_of(*gather(prev, next, A, B))


def dense(table, n_src, n_dst):
    """the demo's matrix, built as it builds it: np.add.at on zeros, from rows repeated by their counts"""
    table = np.asarray(table, np.int64).reshape(-1, 3)
    if len(table) and (table[:, 0].max() > n_src or table[:, 1].max() > n_dst):
        raise ValueError(f"a label above n_src = {n_src} or n_dst = {n_dst}")
    M = np.zeros((n_src, n_dst), np.uint32)
    np.add.at(M, (np.repeat(table[:, 0] - 1, table[:, 2]), np.repeat(table[:, 1] - 1, table[:, 2])), 1)
    return M


def _best(table, key, other):
    """{label of column `key`: the label of column `other` with the largest count, the smallest on a tie}"""
    out = {}
    for row in np.asarray(table, np.int64).reshape(-1, 3):
        k, o, c = int(row[key]), int(row[other]), int(row[2])
        if k not in out or c > out[k][1] or (c == out[k][1] and o < out[k][0]):
            out[k] = (o, c)
    return {k: v[0] for k, v in out.items()}


def best_src(table):
    return _best(table, 1, 0)


def best_dst(table):
    return _best(table, 0, 1)


def best_src_by_argmax(table, n_src, n_dst):
    """the demo's own line, `np.argmax(M, axis=0) + 1`, for the destinations that have a counted pair"""
    M = dense(table, n_src, n_dst)
    return {b + 1: int(np.argmax(M[:, b])) + 1 for b in range(n_dst) if M[:, b].any()}


def events(table, min_count=1):
    """{"fission_src": the sources with two or more edges that count, "fission": their edges (src, dst, count) by (src, dst);
    "fusion_dst": the destinations with two or more, "fusion": their edges by (dst, src)}, int64 -- one edge at a time"""
    table = np.asarray(table, np.int64).reshape(-1, 3)
    edges = [tuple(int(v) for v in row) for row in table if row[2] >= min_count]
    fis = sorted({s for s, _, _ in edges if sum(1 for e in edges if e[0] == s) >= 2})
    fus = sorted({d for _, d, _ in edges if sum(1 for e in edges if e[1] == d) >= 2})
    as_rows = lambda rows: np.asarray(rows, np.int64).reshape(-1, 3)   # noqa: E731
    return {"fission_src": np.asarray(fis, np.int64), "fission": as_rows(sorted(e for e in edges if e[0] in fis)),
            "fusion_dst": np.asarray(fus, np.int64), "fusion": as_rows(sorted((e for e in edges if e[1] in fus), key=lambda e: (e[1], e[0])))}


def relabel(B, table):
    """frame t + 1 painted with best_src, int32"""
    B = np.asarray(B)
    best = best_src(table)
    out = np.zeros(B.shape, np.int32)
    for b, a in best.items():
        out[B == b] = a
    return out
