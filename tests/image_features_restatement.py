"""numpy restatement of the reference's Image (nellie/feature_extraction/hierarchical.py:2046-2116) and of the block decomposition
the device uses for wide groups (csrc/nodefeat.inc, nf_wide_block_kernel / nf_wide_chain_kernel), test infrastructure only -- never
imported by the package.  It is checked bit for bit against the reference by the capture of the goldens
(tests/golden/make_golden_image.py) and against the goldens without a GPU (tests/test_image_cpu.py); the GPU tests compare the HIP
engine with it where no golden exists.

`Image` is literal: per frame and child level one group, arange(rows), through tests/node_features_restatement.py's
aggregate_stats_for_class.  `block_items` and `aggregate_by_blocks` restate what the device does with a wide group: the (group,
block) items, every block's own tree with its own base, k and n_block, the chain over the blocks in ascending order, and the merge
of the blocks' extremes by latest position."""
import numpy as np

import node_features_restatement as nr

BLOCK = nr.BUFFER
LEVELS = (("voxel", "voxels"), ("node", "nodes"), ("branch", "branches"), ("component", "components"))


def rows_of(h, t):
    """the number of rows of every child level at frame t, by the reference's rule (hierarchical.py:2063-2103)"""
    rows = {"voxel": len(h.voxels.coords[t]), "branch": len(h.branches.branch_length[t]), "component": len(h.components.organelle_area[t])}
    if not h.skip_nodes:
        rows["node"] = len(h.nodes.nodes[t])
    return rows


class Image:
    """the reference's Image on a hierarchy double: same attributes, per frame"""

    def __init__(self, hierarchy):
        self.hierarchy = hierarchy
        self.time, self.image_name = [], []
        self.aggregate_voxel_metrics, self.aggregate_node_metrics = [], []
        self.aggregate_branch_metrics, self.aggregate_component_metrics = [], []
        self.stats_to_aggregate, self.features_to_save = [], []

    def run(self):
        h = self.hierarchy
        for t in range(h.num_t):
            self.time.append(t)
            self.image_name.append(h.im_info.file_info.filename_no_ext)
            rows = rows_of(h, t)
            for key, attr in LEVELS:
                if key in rows:
                    agg = nr.aggregate_stats_for_class(getattr(h, attr), t, [np.arange(rows[key], dtype=int)])
                    getattr(self, f"aggregate_{key}_metrics").append(agg)


def feature_table(image):
    """header and text of features_image by the reference's saving rule (hierarchical.py:279-337, 417-431, 611-625): per frame one
    float64 array through pandas' to_csv, header once; columns t, label (the row number: 0), <stat>_<key> of the node aggregates (if
    any), of the voxel, of the branch and of the component aggregates, merged as the reference's dict.update does.  One row per
    frame, a frame without voxels included."""
    import io
    import pandas as pd
    buf = io.StringIO()
    header = None
    for t in range(len(image.time)):
        merged = {}
        for frames in (image.aggregate_node_metrics, image.aggregate_voxel_metrics, image.aggregate_branch_metrics, image.aggregate_component_metrics):
            if frames:
                merged.update(frames[t])
        cols, names = [], []
        for stat, keys in merged.items():
            for key, vals in keys.items():
                cols.append(np.array(vals)[0])
                names.append(f"{stat}_{key}")
        labels = np.arange(len(cols[0]), dtype=np.int64)
        cols = [np.full(labels.shape[0], t, dtype=np.int64), labels] + cols
        first = header is None
        if first:
            header = ["t", "label"] + names
        pd.DataFrame(np.array(cols).T, columns=header).to_csv(buf, index=False, mode="a", header=first)
    return header, buf.getvalue()


# ---- the block decomposition of a wide group -------------------------------------------------------------------------------------
def block_items(offsets, wide_from):
    """(wide, items): wide = [(group, first item)] for every group of k >= max(wide_from, 1) values (none for wide_from = 0), items
    = [(row of wide, block)] for every buffer block of such a group that starts below k, blocks ascending"""
    wide, items = [], []
    for j, k in enumerate(np.diff(np.asarray(offsets, np.int64)).tolist()):
        if wide_from <= 0 or k == 0 or k < wide_from:
            continue
        wide.append((j, len(items)))
        items += [(len(wide) - 1, b) for b in range((k + BLOCK - 1) // BLOCK)]
    return wide, items


def block_geometry(k, L, b):
    """(base, kb, n_block) of block b of a group of k values in a row of L columns: the tree is over n_block elements, the first
    kb of which are values"""
    base = BLOCK * b
    n_block = min(BLOCK, L - base)
    return base, min(k - base, n_block), n_block


def tree(x, n):
    """numpy's pairwise sum of n elements, the first len(x) of them x and the rest +0.0: the whole tree, padding included"""
    x = np.concatenate([np.asarray(x, np.float64), np.zeros(n - len(x))])

    def walk(lo, m):
        if m <= nr.LEAF:
            return nr.leaf_sum(x[None, lo:lo + m])[0]
        m2 = m // 2
        m2 -= m2 % 8
        return walk(lo, m2) + walk(lo + m2, m - m2)
    return walk(0, n)


def _block_extremes(x, base):
    """(count, lo, lo_at, hi, hi_at) of a block's values, positions in the group; among equals the latest"""
    at = np.flatnonzero(~np.isnan(x))
    if len(at) == 0:
        return 0, np.nan, -1, np.nan, -1
    lo_at, hi_at = at[x[at] == x[at].min()][-1], at[x[at] == x[at].max()][-1]      # +0.0 == -0.0
    return len(at), x[lo_at], base + int(lo_at), x[hi_at], base + int(hi_at)


def aggregate_by_blocks(values, offsets, idx, wide_from, L=None, descending=False):
    """{key: (G,) float64} with NaN for the groups that stay on the narrow path: the wide groups of the call as the device's block
    kernels take them.  descending: the chain over the blocks in the wrong order (what the tests must be able to tell)."""
    values = np.asarray(values).astype(np.float64)
    off, idx = np.asarray(offsets, np.int64), np.asarray(idx, np.int64)
    ks = np.diff(off)
    L = int(ks.max(initial=0)) if L is None else L
    out = {key: np.full(len(ks), np.nan) for key in nr.KEYS}
    wide, items = block_items(off, wide_from)
    partial = [None] * len(items)
    geometry = {}
    for n, (w, b) in enumerate(items):                            # pass A: every item on its own
        grp = wide[w][0]
        base, kb, n_block = block_geometry(int(ks[grp]), L, b)
        geometry[n] = (base, kb, n_block)
        x = values[idx[off[grp] + base:off[grp] + base + kb]]
        partial[n] = (tree(np.where(np.isnan(x), 0.0, x), n_block),) + _block_extremes(x, base)
    mean = {}
    with np.errstate(all="ignore"):
        for w, (grp, first) in enumerate(wide):                   # combine A
            nb = (int(ks[grp]) + BLOCK - 1) // BLOCK
            order = range(nb - 1, -1, -1) if descending else range(nb)
            total, count, lo, lo_at, hi, hi_at = np.float64(0.0), 0, np.nan, -1, np.nan, -1
            for b in order:
                s, c, bl, bl_at, bh, bh_at = partial[first + b]
                total = total + s
                count += c
                if bl_at >= 0 and (lo_at < 0 or bl < lo or (bl == lo and bl_at > lo_at)):
                    lo, lo_at = bl, bl_at
                if bh_at >= 0 and (hi_at < 0 or bh > hi or (bh == hi and bh_at > hi_at)):
                    hi, hi_at = bh, bh_at
            mean[w] = (total / np.float64(count), count)
            out["sum"][grp], out["mean"][grp], out["min"][grp], out["max"][grp] = total, mean[w][0], lo, hi
        dev = [None] * len(items)
        for n, (w, b) in enumerate(items):                        # pass B
            grp = wide[w][0]
            base, kb, n_block = geometry[n]
            x = values[idx[off[grp] + base:off[grp] + base + kb]]
            d = x - mean[w][0]
            dev[n] = tree(np.where(np.isnan(x), 0.0, d * d), n_block)
        for w, (grp, first) in enumerate(wide):                   # combine B
            nb = (int(ks[grp]) + BLOCK - 1) // BLOCK
            total = np.float64(0.0)
            for b in (range(nb - 1, -1, -1) if descending else range(nb)):
                total = total + dev[first + b]
            out["std_dev"][grp] = np.sqrt(total / np.float64(mean[w][1]))
    return out
