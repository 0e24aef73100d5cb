"""The hierarchy's adjacency maps restated in numpy, in this project's own words; test infrastructure only.  Three primitives and
the six edge lists made of them.  Every list is an (m, 2) int64 array of (row, column) pairs, ascending in the row, C-contiguous;
(0, 2) without edges.

    pairs(labels, bias)       (i, labels[i] - bias) for the rows with a label above 0
    expand(offsets, values)   the CSR of one value list per row as (row, value), values in their order
    lookup(children, parents) (i, j) with j the LAST position of children[i] among the parents, for the children that occur there;
                              a child above the parents' largest label raises IndexError (what numpy raises for the reference's
                              table), no parents give no rows

`adjacency_lists(hierarchy)` is the dict the reference pickles: v_b, v_n, v_o, n_b, n_o, b_o, one array per frame; the frame counts
are len(voxels.time), len(nodes.time) and len(branches.time); v_n, n_b and n_o are [] under skip_nodes.

tests/golden/make_golden_adjacency.py checks this file against the reference's output for every fixture."""
import numpy as np

KEYS = ("v_b", "v_n", "v_o", "n_b", "n_o", "b_o")


def _rows(rows, cols):
    out = np.empty((len(rows), 2), np.int64)
    out[:, 0] = rows
    out[:, 1] = cols
    return out


def pairs(labels, bias=0):
    lab = np.asarray(labels).astype(np.int64).reshape(-1)
    rows = np.flatnonzero(lab > 0)
    return _rows(rows, lab[rows] - bias)


def expand(offsets, values):
    off, val = np.asarray(offsets, np.int64), np.asarray(values, np.int64)
    assert off[0] == 0 and off[-1] == len(val) and (np.diff(off) >= 0).all()
    return _rows(np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off)), val)


def lookup(children, parents):
    child, parent = np.asarray(children).astype(np.int64).reshape(-1), np.asarray(parents).astype(np.int64).reshape(-1)
    if len(parent) == 0:
        return np.zeros((0, 2), np.int64)
    if len(child) and child.max() > parent.max():
        raise IndexError(f"label {child.max()} above the parents' largest label {parent.max()}")
    order = np.argsort(parent, kind="stable")                    # equal labels keep their order: the last of a run is the last position
    ranked = parent[order]
    last = np.append(ranked[1:] != ranked[:-1], True)
    known, where = ranked[last], order[last]
    k = np.minimum(np.searchsorted(known, child), len(known) - 1)
    rows = np.flatnonzero(known[k] == child)
    return _rows(rows, where[k[rows]])


def node_lists_csr(lists):
    """a frame's list of node-index arrays per voxel (None or empty: no node) as (offsets, values)"""
    arrays = [np.zeros(0, np.int64) if a is None else np.asarray(a).astype(np.int64).reshape(-1) for a in lists]
    off = np.zeros(len(arrays) + 1, np.int64)
    np.cumsum([len(a) for a in arrays], out=off[1:])
    return off, (np.concatenate(arrays) if off[-1] else np.zeros(0, np.int64))


def adjacency_lists(h):
    v, n, b, c = h.voxels, h.nodes, h.branches, h.components
    out = {key: [] for key in KEYS}
    for t in range(len(v.time)):
        if not h.skip_nodes:
            out["v_n"].append(expand(*node_lists_csr(v.node_labels[t])))
        out["v_b"].append(pairs(v.branch_labels[t], 1))
        out["v_o"].append(pairs(v.component_labels[t], 0))
    if not h.skip_nodes:
        for t in range(len(n.time)):
            out["n_b"].append(lookup(n.branch_label[t], b.branch_label[t]))
            out["n_o"].append(lookup(n.component_label[t], c.component_label[t]))
    for t in range(len(b.time)):
        out["b_o"].append(lookup(b.component_label[t], c.component_label[t]))
    return out


def same_lists(got, want):
    """two dicts of edge lists: the same keys in the same order, and per frame the same values, dtype int64, shape (m, 2), C order"""
    assert list(got) == list(want) == list(KEYS), (list(got), list(want))
    for key in KEYS:
        assert isinstance(got[key], list) and len(got[key]) == len(want[key]), (key, len(got[key]), len(want[key]))
        for t, (a, b) in enumerate(zip(got[key], want[key])):
            assert isinstance(a, np.ndarray) and a.dtype == np.int64 and a.ndim == 2 and a.shape[1] == 2 and a.flags.c_contiguous, (key, t, a.dtype, a.shape)
            assert a.shape == np.shape(b) and np.array_equal(a, b), (key, t, a.shape, np.shape(b))
    return True
