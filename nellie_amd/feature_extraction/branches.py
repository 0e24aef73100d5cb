"""
`Branches`: drop-in for nellie.feature_extraction.hierarchical.Branches (reference hierarchical.py:1444-1877), the third level of the
reference's Hierarchy, on the MI355X HIP engine.  Per frame it lists the skeleton voxels (`im_skel` > 0) with their labels, counts
every voxel's same-label neighbours and every label's same-label pairs per offset, measures every skeleton voxel's distance to the
border, takes the median thickness per label, sums the voxel coordinates of every region of `label_branches` exactly, finds the
most frequent reassigned label of every region, and aggregates the voxel and node statistics per branch label.  Same constructor
argument, same `.run()`, same attributes (lists with one entry per frame).

Everything that touches voxels runs on the device (csrc/branchfeat.inc); what is left is O(branches) numpy in the reference's
operation order: length (one rounding to float32 per addition), thickness and the swap, aspect ratio, tortuosity, and the region
columns from the integer sums.

`BranchFeatures(im_info).run()` opens the files the reference's Hierarchy opens, runs `Voxels`, `Nodes` and `Branches` and writes
`features_voxels`, `features_nodes` and `features_branches` as the reference's Hierarchy does.

`hierarchy.voxels` and `hierarchy.nodes` may be this package's objects, the reference's or any object with the same lists.
Differences: `branch_solidity` is NaN unless `hierarchy.solidity` is true, when it is the exact restatement of
skimage's area / area_convex; the region columns follow skimage's documented formulas and a negative
square-root argument gives 0 where the reference's `except ValueError` gives NaN; the region columns and `reassigned_label` are
float64 arrays where the reference keeps lists; a frame without branches writes no rows to the table; `hierarchy.low_memory` is
accepted and ignored.  There is no CPU engine behind these classes (`device="cpu"` raises).
"""
from __future__ import annotations

import numpy as np

from nellie_amd.feature_extraction.hierarchy import Level
from nellie_amd.feature_extraction.nodes import NodeFeatures, aggregate_groups
from nellie_amd.feature_extraction.voxels import _image_name

SKELETON_STATS = ("branch_length", "branch_thickness", "branch_aspect_ratio", "branch_tortuosity")
REGION_STATS = ("branch_area", "branch_axis_length_maj", "branch_axis_length_min", "branch_extent", "branch_solidity", "reassigned_label", "z", "y", "x")


def _positive_offsets(D):
    """the reference's offsets: dz, dy, dx each over -1, 0, 1, kept when the first non-zero component is +1 (the device's order)"""
    out = []
    for d in np.ndindex(*(3,) * D):
        d = tuple(v - 1 for v in d)
        if any(d) and next(v for v in d if v) > 0:
            out.append(d)
    return out


def _edge_lengths(spacing, D):
    """float32 sqrt(sum (d_a * s_a)^2) per offset, the squares added in axis order"""
    out = []
    for d in _positive_offsets(D):
        sq = 0.0
        for a in range(D):
            sq = sq + (d[a] * float(spacing[a])) * (d[a] * float(spacing[a]))
        out.append(np.float32(np.sqrt(sq)))
    return out


def _label_groups(labels):
    """CSR (offsets, indices) of the positions of every distinct non-zero label, labels ascending and positions ascending within a
    label: one stable sort"""
    lab = np.asarray(labels).reshape(-1)
    order = np.argsort(lab, kind="stable")
    sorted_lab = lab[order]
    keep = sorted_lab != 0
    order, sorted_lab = order[keep].astype(np.int64, copy=False), sorted_lab[keep]
    starts = np.flatnonzero(np.concatenate([[True], sorted_lab[1:] != sorted_lab[:-1]])) if len(sorted_lab) else np.zeros(0, np.int64)
    return np.append(starts, len(sorted_lab)).astype(np.int64), order


def _by_rank(rank, n_labels):
    """(order, offsets): the positions of `rank` sorted stably by it, and where every label's run starts"""
    order = np.argsort(rank, kind="stable")
    off = np.zeros(n_labels + 1, np.int64)
    np.cumsum(np.bincount(rank, minlength=n_labels), out=off[1:])
    return order, off


def _add_in_order(length, order, off, addend):
    """length[b] = f32(f64(length[b]) + addend[k]) for every k of label b's run, in the run's order: round j takes the j-th of
    every run that has one"""
    count = np.diff(off)
    for j in range(int(count.max(initial=0))):
        alive = np.flatnonzero(count > j)
        length[alive] = (length[alive].astype(np.float64) + addend[order[off[alive] + j]]).astype(np.float32)


def skeleton_columns(f, spacing, D):
    """the four float32 statistics per label from what the device fetched (hipnative.BranchFeatures.fetch), in the reference's
    operation order (hierarchical.py:1692-1750)"""
    B = len(f["branch_label"])
    length = np.zeros(B, np.float32)
    for j, edge in enumerate(_edge_lengths(spacing, D)):
        length = (length.astype(np.float64) + f["edges"][:, j].astype(np.int64) * np.float64(edge)).astype(np.float32)
    rank = {k: np.searchsorted(f["branch_label"], f["labels"][f[k]]) for k in ("lone", "tips")}
    order, off = _by_rank(rank["lone"], B)
    _add_in_order(length, order, off, 2.0 * f["radius"][f["lone"]])
    order, off = _by_rank(rank["tips"], B)
    _add_in_order(length, order, off, f["radius"][f["tips"]])
    with np.errstate(all="ignore"):
        thick = f["median"].astype(np.float32)
        swap = ~np.isnan(thick) & (thick > length)
        length[swap], thick[swap] = thick[swap], length[swap]
        aspect = np.divide(length, thick, out=np.full_like(length, np.nan), where=thick != 0)
        tort = np.ones(B, np.float32)
        two = np.flatnonzero(np.diff(off) >= 2)
        if len(two):
            tips = f["tips"][order]
            p0, p1 = f["coords"][tips[off[two]]], f["coords"][tips[off[two] + 1]]
            sq = 0.0
            for a in range(D):
                d = (p0[:, a] - p1[:, a]) * float(spacing[a])
                sq = sq + d * d
            dist = np.sqrt(sq)
            ok = dist > 0
            tort[two[ok]] = (length[two[ok]].astype(np.float64) / dist[ok]).astype(np.float32)
    return dict(branch_length=length, branch_thickness=thick, branch_aspect_ratio=aspect, branch_tortuosity=tort)


def region_stats(prefix):
    """the names of the region columns of a level: REGION_STATS with `prefix` in place of `branch`"""
    return tuple(prefix + k[len("branch"):] if k.startswith("branch_") else k for k in REGION_STATS)


def region_columns(sums, mode, spacing, D, prefix="branch", convex=None):
    """{name: (regions,) float64} of REGION_STATS (of region_stats(prefix)) from the exact sums of every region
    (hipnative.BranchFeatures.fetch_regions): skimage's area, extent, centroid and major / minor axis length with `spacing`,
    restated on n, S_a = sum c_a and Q_ab = sum c_a c_b; mode < 0: no reassigned labels.  `convex`: the int64 convex count of
    every region (hipnative.BranchFeatures.fetch_convex), from which <prefix>_solidity = area / (convex * P), inf where it is 0;
    None: NaN"""
    R = sums.shape[1]
    s = [float(v) for v in spacing]
    P = float(np.prod(spacing))
    out = {k: np.full(R, np.nan) for k in region_stats(prefix)}
    if R == 0:
        return out
    n, lo, hi, S = sums[0], sums[1:1 + D], sums[1 + D:1 + 2 * D], sums[1 + 2 * D:1 + 3 * D]
    Q = np.zeros((D, D, R), np.int64)
    f = 1 + 3 * D
    for a in range(D):
        for b in range(a, D):
            Q[a, b] = Q[b, a] = sums[f]
            f += 1
    area = n * P
    out[prefix + "_area"] = area
    if convex is not None:
        with np.errstate(divide="ignore"):
            out[prefix + "_solidity"] = area / (np.asarray(convex, dtype=np.int64) * P)
    out[prefix + "_extent"] = area / (np.prod(hi - lo + 1, axis=0).astype(np.float64) * P)
    for a in range(D):
        out["zyx"[3 - D + a]] = (S[a] / n) * s[a]
    n_big, S_big = n.astype(object), S.astype(object)             # Python integers: n * Q - S * S is formed exactly
    nn = (n_big * n_big).astype(np.float64)
    C = np.zeros((R, D, D))
    for a in range(D):
        for b in range(D):
            C[:, a, b] = (n_big * Q[a, b].astype(object) - S_big[a] * S_big[b]).astype(np.float64) / nn * (s[a] * s[b])
    lam = np.clip(np.linalg.eigvalsh(C), 0.0, None)
    if D == 3:
        out[prefix + "_axis_length_maj"], out[prefix + "_axis_length_min"] = np.sqrt(20.0 * lam.max(axis=1)), np.sqrt(20.0 * lam.min(axis=1))
    else:
        out[prefix + "_axis_length_maj"], out[prefix + "_axis_length_min"] = 4.0 * np.sqrt(lam.max(axis=1)), 4.0 * np.sqrt(lam.min(axis=1))
    out["reassigned_label"] = np.where(mode >= 0, mode.astype(np.float64), np.nan)
    return out


def convex_of(engine, hierarchy):
    """(the convex counts of the engine's loaded regions, {"convex": device ms, "convex_hull_host": host ms}) when
    `hierarchy.solidity` is true, else (None, {})"""
    if not getattr(hierarchy, "solidity", False):
        return None, {}
    engine.convex()
    ms = engine.convex_ms_parts()
    return engine.fetch_convex(), dict(convex=ms["extremes"] + ms["planes"] + ms["count"], convex_hull_host=ms["hull"])


def convex_counts(labels, spacing=None, device=0):
    """(region_labels, n, convex_count, solidity) of a 2-D or 3-D label array (an integer dtype), without files: the distinct labels
    > 0 ascending (int64), their voxel counts (int64), the lattice points in the closed convex hull of their voxels' diamonds (int64,
    0 for a 3-D region that lies in one plane) and float64 area / area_convex with `spacing` (default 1 per axis), inf where the
    convex count is 0"""
    from nellie_amd import hipnative
    from nellie_amd.stage import require_gpu
    require_gpu()
    lab = np.asarray(labels)
    sp = np.ones(lab.ndim) if spacing is None else np.asarray(spacing, dtype=np.float64)
    with hipnative.BranchFeatures(lab.shape, sp, device=device) as eng:
        eng.regions(lab, rows=True)
        region_labels, sums, mode = eng.fetch_regions()
        eng.convex()
        count = eng.fetch_convex()
    return region_labels, sums[0].copy(), count, region_columns(sums, mode, sp, lab.ndim, convex=count)["branch_solidity"]


class Branches(Level):
    word, name, table_key, label_list = "branch", "branches", "features_branches", "branch_label"
    handles = ("_engine", "_aggregator")
    reads_reassigned = True

    def __init__(self, hierarchy):
        self.hierarchy = hierarchy
        self.time = []
        self.branch_label = []
        self.aggregate_voxel_metrics = []
        self.aggregate_node_metrics = []
        self.z = []
        self.y = []
        self.x = []
        self.branch_length = []
        self.branch_thickness = []
        self.branch_aspect_ratio = []
        self.branch_tortuosity = []
        self.branch_area = []
        self.branch_axis_length_maj = []
        self.branch_axis_length_min = []
        self.branch_extent = []
        self.branch_solidity = []
        self.reassigned_label = []
        self.branch_idxs = []
        self.component_label = []
        self.image_name = []
        self.stats_to_aggregate = ["branch_length", "branch_thickness", "branch_aspect_ratio", "branch_tortuosity", "branch_area",
                                   "branch_axis_length_maj", "branch_axis_length_min", "branch_extent", "branch_solidity", "reassigned_label"]
        self.features_to_save = self.stats_to_aggregate + ["x", "y", "z"]
        self.region_label = []                                    # the labels of label_branches per frame, the rows of the region columns
        self.kernel_ms = []                                       # device time per frame and part of the last run
        self._engine = None
        self._aggregator = None

    def _aggregate(self, child, labels, t):
        """the reference's dict of dicts of `child`'s statistics over the groups of equal non-zero `labels`, and the device time"""
        return aggregate_groups(self._aggregator, child, t, *_label_groups(labels), np.size(labels), "branch labels")

    def _run_frame(self, t):
        h, eng = self.hierarchy, self._engine
        D = eng.ndim
        n, B, _, _ = eng.frame(h.im_skel[t], h.label_components[t], h.im_border_mask[t])
        f = eng.fetch()
        self.branch_idxs.append(f["coords"])
        if n == 0:
            self.time.append(np.array([], dtype=int))
            self.component_label.append(np.array([], dtype=int))
            self.branch_label.append(np.array([], dtype=int))
            self.image_name.append(np.array([], dtype=object))
            self.aggregate_voxel_metrics.append({})
            if not h.skip_nodes:
                self.aggregate_node_metrics.append({})
            for k in SKELETON_STATS + REGION_STATS:
                getattr(self, k).append([])
            self.region_label.append(np.zeros(0, np.int64))
            self.kernel_ms.append(dict(eng.kernel_ms_parts(), regions=0.0, aggregation=0.0))
            return
        self.time.append(np.ones(B, dtype=int) * t)
        self.component_label.append(f["comp"])
        self.branch_label.append(f["branch_label"].astype(int))
        self.image_name.append(np.ones(B, dtype=object) * _image_name(h.im_info))
        agg, ms = self._aggregate(h.voxels, h.voxels.branch_labels[t], t)
        self.aggregate_voxel_metrics.append(agg)
        if not h.skip_nodes:
            agg, more = self._aggregate(h.nodes, h.nodes.branch_label[t], t)
            self.aggregate_node_metrics.append(agg)
            ms += more
        for k, v in skeleton_columns(f, h.spacing, D).items():
            getattr(self, k).append(v)
        reassigned = getattr(h, "im_branch_reassigned", None)
        eng.regions(h.label_branches[t], None if reassigned is None or h.im_info.no_t else reassigned[t])
        labels, sums, mode = eng.fetch_regions()
        convex, convex_ms = convex_of(eng, h)
        for k, v in region_columns(sums, mode, h.spacing, D, convex=convex).items():
            getattr(self, k).append(v)
        self.region_label.append(labels)
        self.kernel_ms.append(dict(eng.kernel_ms_parts(), aggregation=ms, **convex_ms))

    def _open(self, device):
        from nellie_amd import hipnative
        h = self.hierarchy
        self._engine = hipnative.BranchFeatures(tuple(np.shape(h.im_skel[0])), h.spacing, device=device)
        self._aggregator = hipnative.NodeFeatures(device=device)          # one for the run: groups and aggregation need no frame


class BranchFeatures(NodeFeatures):
    """The voxel, node and branch level of the hierarchy from an ImInfo's files to their tables: opens also, by the reference's
    rule (hierarchical.py:217-233), the reassigned label stacks; runs `Voxels`, `Nodes` and `Branches`; writes `features_voxels`,
    `features_nodes` (unless `skip_nodes`) and `features_branches`; the objects stay in `.voxels`, `.nodes` and `.branches`."""

    levels = NodeFeatures.levels + (Branches,)
