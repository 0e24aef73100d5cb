"""numpy restatement of the reference's Nodes and aggregate_stats_for_class (nellie/feature_extraction/hierarchical.py:1165-1441),
test infrastructure only -- never imported by the package.  It is checked bit for bit against the reference by the capture of the
goldens (tests/golden/make_golden_nodes.py) and against the goldens without a GPU (tests/test_nodes_cpu.py); the GPU tests compare
the HIP engine with it where no golden exists.

Every sum is written out as numpy's reduction, with element-wise additions only and no call to a numpy reduction of floats
(`PaddedSum`): for the rows of a matrix padded to L columns it takes the row in numpy's buffer blocks of 8192 columns and walks
each block's whole pairwise tree, padding included, so it shares nothing with the device routine, which skips the padding.  The
thickness is the minimum over every border voxel, no search structure."""
import numpy as np

LEAF = 128                            # numpy's PW_BLOCKSIZE
BUFFER = 8192                         # numpy's ufunc buffer in elements (np.getbufsize()): a reduction's inner loop runs in such pieces
KEYS = ("mean", "std_dev", "min", "max", "sum")
NODE_STATS = ("z", "y", "x", "divergence", "convergence", "vergere")


def as_csr(list_of_idxs):
    """list of index arrays (an empty one may be numpy's empty float64 array), or an (offsets, values) pair -> (offsets, values) int64"""
    if isinstance(list_of_idxs, tuple) and len(list_of_idxs) == 2:
        return np.asarray(list_of_idxs[0], np.int64), np.asarray(list_of_idxs[1], np.int64)
    lens = [len(a) for a in list_of_idxs]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    val = np.concatenate([np.asarray(a).astype(np.int64) for a in list_of_idxs]) if off[-1] else np.zeros(0, np.int64)
    return off, val


def leaves(L):
    """the leaves (lo, n) of numpy's pairwise tree over L elements, in order"""
    out = []

    def walk(lo, n):
        if n <= LEAF:
            out.append((lo, n))
            return
        n2 = n // 2
        n2 -= n2 % 8
        walk(lo, n2)
        walk(lo + n2, n - n2)
    walk(0, L)
    return out


def leaf_sum(M):
    """numpy's sum of n <= 128 contiguous elements for every row of M (rows, n)"""
    n = M.shape[1]
    if n < 8:
        res = np.zeros(len(M))
        for i in range(n):
            res = res + M[:, i]
        return res
    r = M[:, 0:8].copy()
    m8 = n - n % 8
    for i in range(8, m8, 8):
        r = r + M[:, i:i + 8]
    res = ((r[:, 0] + r[:, 1]) + (r[:, 2] + r[:, 3])) + ((r[:, 4] + r[:, 5]) + (r[:, 6] + r[:, 7]))
    for i in range(m8, n):
        res = res + M[:, i]
    return res


class PaddedSum:
    """np.sum(axis=1) of the matrix whose row j holds group j's values followed by +0.0 up to column L (default: the longest
    group).  numpy runs the inner loop of a reduction in pieces of its ufunc buffer, BUFFER elements, which restart at every row:
    the sum is the identity 0.0, then for each block b of BUFFER columns `+ the pairwise tree of that block`, the block's length
    being min(BUFFER, L - BUFFER * b).  For L <= BUFFER that is 0.0 + one tree over L.  A block that is padding in some row adds
    +0.0 to a sum that began as 0.0 + ..., which is never -0.0, and so changes nothing there: only the blocks that start below k
    matter to a row of k values.  Built once per set of groups, called per value array with one value per (group, position)
    pair in CSR order."""

    def __init__(self, offsets, L=None):
        self.off = np.asarray(offsets, np.int64)
        self.k = np.diff(self.off)
        self.G = len(self.k)
        self.L = int(self.k.max(initial=0)) if L is None else int(L)
        assert self.L >= int(self.k.max(initial=0))
        self.gid = np.repeat(np.arange(self.G), self.k)
        self.pos = np.arange(int(self.off[-1])) - np.repeat(self.off[:-1], self.k)
        self.blocks = [(base, min(BUFFER, self.L - base)) for base in range(0, self.L, BUFFER)]
        self.leaves = [(base + lo, n) for base, length in self.blocks for lo, n in leaves(length)]
        los = np.array([lo for lo, _ in self.leaves], np.int64)
        leaf_of = np.searchsorted(los, self.pos, side="right") - 1
        self.order = np.argsort(leaf_of, kind="stable")
        self.bounds = np.searchsorted(leaf_of[self.order], np.arange(len(self.leaves) + 1))

    def __call__(self, per_pair):
        per_pair = np.asarray(per_pair, np.float64)
        sums = {}
        for i, (lo, n) in enumerate(self.leaves):
            pairs = self.order[self.bounds[i]:self.bounds[i + 1]]
            if len(pairs) == 0:
                continue                                          # a leaf of padding in every row: +0.0, as `tree` has it
            rows, inverse = np.unique(self.gid[pairs], return_inverse=True)
            M = np.zeros((len(rows), n))
            M[inverse, self.pos[pairs] - lo] = per_pair[pairs]
            full = np.zeros(self.G)
            full[rows] = leaf_sum(M)
            sums[lo] = full

        def tree(lo, n):
            if n <= LEAF:
                return sums[lo] if lo in sums else np.zeros(self.G)
            n2 = n // 2
            n2 -= n2 % 8
            return tree(lo, n2) + tree(lo + n2, n - n2)
        total = np.zeros(self.G)
        for base, length in self.blocks:
            total = total + tree(base, length)
        return total


def aggregate_values(values, offsets, idx, plan=None):
    """{key: (G,) float64} of one 1-D statistic over the groups, as nanmean / nanstd / nanmin / nanmax / nansum of the padded matrix"""
    values = np.asarray(values).astype(np.float64)
    off, idx = np.asarray(offsets, np.int64), np.asarray(idx, np.int64)
    plan = plan or PaddedSum(off)
    G, gid = plan.G, plan.gid
    x = values[idx] if len(idx) else np.zeros(0)
    nan = np.isnan(x)
    count = np.bincount(gid[~nan], minlength=G).astype(np.int64)
    with np.errstate(all="ignore"):
        total = plan(np.where(nan, 0.0, x))
        mean = total / count
        dev = x - mean[gid]
        dev[nan] = 0.0
        std = np.sqrt(plan(dev * dev) / count)
    out = {"mean": mean, "std_dev": std, "sum": total}
    at = np.arange(len(x))
    for key, fill, ufunc in (("min", np.inf, np.minimum), ("max", -np.inf, np.maximum)):
        best = np.full(G, fill)
        ufunc.at(best, gid, np.where(nan, fill, x))
        hit = ~nan & (x == best[gid])                             # +0.0 == -0.0: the latest of the equals is numpy's answer
        last = np.full(G, -1, np.int64)
        np.maximum.at(last, gid[hit], at[hit])
        res = np.full(G, np.nan)
        res[last >= 0] = x[last[last >= 0]]
        out[key] = res
    return out


def aggregate_stats_for_class(child, t, list_of_idxs):
    """the reference's function: {stat: {key: (1, G) float64}}; a statistic with more than one dimension keeps numpy's empty array"""
    off, idx = as_csr(list_of_idxs)
    plan = PaddedSum(off)
    out = {}
    for name in child.stats_to_aggregate:
        if name == "reassigned_label":
            continue
        values = np.array(getattr(child, name)[t])
        if values.ndim > 1:
            out[name] = {key: np.array([]) for key in KEYS}
            continue
        res = aggregate_values(values, off, idx, plan)
        out[name] = {key: res[key][None, :] for key in KEYS}
    return out


def thickness(border, nodes, spacing, chunk=256):
    """2 * the distance in um from every node to the nearest voxel with border != 0: per axis node * s - border * s, the squares
    added in axis order, the minimum over all border voxels, sqrt"""
    s = np.asarray(spacing, np.float64)
    b = np.argwhere(border) * s
    if b.size == 0:
        return np.full(len(nodes), np.nan)
    p = np.asarray(nodes) * s
    out = np.empty(len(nodes))
    for a in range(0, len(nodes), chunk):
        d2 = 0.0
        for ax in range(len(s)):
            d = p[a:a + chunk, ax, None] - b[None, :, ax]
            d2 = d * d if ax == 0 else d2 + d * d
        out[a:a + chunk] = np.sqrt(d2.min(axis=1)) * 2
    return out


def node_stats(nodes, offsets, idx, coords, vec01, vec12, spacing):
    """{name: (m,) float64} for NODE_STATS (hierarchical.py:1323-1393); vec01 / vec12 with no rows count as all NaN"""
    nodes, coords = np.asarray(nodes, np.int64), np.asarray(coords, np.int64)
    off, idx = np.asarray(offsets, np.int64), np.asarray(idx, np.int64)
    m, D = len(nodes), nodes.shape[1]
    k = np.diff(off)
    gid = np.repeat(np.arange(m), k)
    out = {name: np.full(m, np.nan) for name in NODE_STATS}
    if m == 0:
        return out
    xyz = coords[idx] if len(idx) else np.zeros((0, D), np.int64)
    with np.errstate(all="ignore"):
        for ax in range(D):
            tot = np.zeros(m, np.int64)
            np.add.at(tot, gid, xyz[:, ax])
            out[NODE_STATS[3 - D + ax]] = np.where(k > 0, tot.astype(np.float64) / k * float(spacing[ax]), np.nan)
        d = (xyz - nodes[gid]).astype(np.float64)
        sq = np.zeros(len(d))
        for ax in range(D):
            sq = sq + d[:, ax] * d[:, ax]
        norm = np.sqrt(sq)
        direction = np.where(norm[:, None] != 0, d / norm[:, None], np.nan)
        means = []
        for vec, sign in ((vec01, -1.0), (vec12, 1.0)):
            vec = np.asarray(vec)
            v = vec[idx].astype(np.float64) if len(vec) else np.full((len(idx), D), np.nan)
            dot = np.zeros(len(d))
            for ax in range(D):
                dot = dot + (sign * v[:, ax]) * direction[:, ax]
            nan = np.isnan(dot)
            count = np.bincount(gid[~nan], minlength=m)
            total = np.zeros(m)
            for kk in np.unique(k[k > 0]):                        # nanmean of a vector of kk elements: the tree over L = kk
                sel = np.flatnonzero(k == kk)
                pairs = (off[sel][:, None] + np.arange(kk)[None, :]).reshape(-1)
                total[sel] = PaddedSum(np.arange(len(sel) + 1) * kk, kk)(np.where(nan[pairs], 0.0, dot[pairs]))
            means.append(np.where(k > 0, total / count, np.nan))
        out["convergence"] = -means[0]
        out["divergence"] = means[1]
        out["vergere"] = out["convergence"] + out["divergence"]
    return out


class Nodes:
    """the reference's Nodes on a hierarchy double: same attributes, per frame"""

    def __init__(self, hierarchy):
        self.hierarchy = hierarchy
        self.time, self.nodes, self.aggregate_voxel_metrics = [], [], []
        self.z, self.x, self.y, self.node_thickness, self.divergence, self.convergence, self.vergere = [], [], [], [], [], [], []
        self.stats_to_aggregate = ["divergence", "convergence", "vergere", "node_thickness"]
        self.features_to_save = self.stats_to_aggregate + ["x", "y", "z"]
        self.voxel_idxs = hierarchy.voxels.node_voxel_idxs
        self.branch_label, self.component_label, self.image_name = [], [], []
        self.node_z_lims, self.node_y_lims, self.node_x_lims = (hierarchy.voxels.node_dim0_lims, hierarchy.voxels.node_dim1_lims,
                                                                hierarchy.voxels.node_dim2_lims)
        self.longest = []                                         # L per frame

    def run(self):
        h = self.hierarchy
        if h.skip_nodes:
            return
        v = h.voxels
        for t in range(h.num_t):
            nodes = np.argwhere(np.asarray(h.im_pixel_class[t]) > 0)
            self.nodes.append(nodes)
            self.time.append(np.ones(len(nodes), dtype=int) * t)
            self.component_label.append(np.asarray(h.label_components[t])[tuple(nodes.T)])
            self.branch_label.append(np.asarray(h.label_branches[t])[tuple(nodes.T)])
            self.image_name.append(np.ones(len(nodes), dtype=object) * h.im_info.file_info.filename_no_ext)
            off, idx = as_csr(v.node_voxel_idxs[t])
            self.longest.append(int(np.diff(off).max(initial=0)))
            self.aggregate_voxel_metrics.append(aggregate_stats_for_class(v, t, (off, idx)))
            self.node_thickness.append(thickness(np.asarray(h.im_border_mask[t]), nodes, h.spacing))
            stats = node_stats(nodes, off, idx, v.coords[t], v.vec01[t], v.vec12[t], h.spacing)
            for name in NODE_STATS:
                getattr(self, name).append(stats[name])


def feature_table(nodes):
    """header and text of features_nodes by the reference's saving rule (hierarchical.py:279-337, 362-379, 611-625): per frame one
    float64 array through pandas' to_csv, header once; columns t, label (the row number), <stat>_<key> of the voxel aggregates in
    stats_to_aggregate order, then <feature>_raw of features_to_save"""
    import io
    import pandas as pd
    buf = io.StringIO()
    header = None
    for t in range(len(nodes.aggregate_voxel_metrics)):
        cols, names = [], []
        for stat, keys in nodes.aggregate_voxel_metrics[t].items():
            for key, vals in keys.items():
                cols.append(np.array(vals)[0])
                names.append(f"{stat}_{key}")
        for feature in nodes.features_to_save:
            cols.append(np.array([np.array(getattr(nodes, feature)[t])])[0])
            names.append(f"{feature}_raw")
        n = len(cols[0])
        cols = [np.full(n, t, dtype=np.int64), np.arange(n, dtype=np.int64)] + cols
        if header is None:
            header = ["t", "label"] + names
        pd.DataFrame(np.array(cols).T, columns=header).to_csv(buf, index=False, mode="a", header=t == 0)
    return header, buf.getvalue()
