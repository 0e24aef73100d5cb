"""numpy restatement of the reference's Branches (nellie/feature_extraction/hierarchical.py:1444-1877), test infrastructure only --
never imported by the package.  Literal loops in the reference's order: one pass per label, per offset and per tip, no search
structure, no sort.  It is checked bit for bit against the reference by the capture of the goldens
(tests/golden/make_golden_branches.py) and against the goldens without a GPU (tests/test_branches_cpu.py); the GPU tests compare
the HIP engine with it where no golden exists.

The region columns (area, extent, centroid, axis lengths) are computed straight from the voxel coordinates of every region by
skimage's documented formulas with `spacing`; they are NOT reference output (skimage is not installed where the goldens are made),
and `branch_solidity` is NaN.  The aggregates are tests/node_features_restatement.py's."""
import numpy as np

import node_features_restatement as nr

SKELETON_STATS = ("branch_length", "branch_thickness", "branch_aspect_ratio", "branch_tortuosity")
REGION_STATS = ("branch_area", "branch_axis_length_maj", "branch_axis_length_min", "branch_extent", "branch_solidity", "reassigned_label", "z", "y", "x")
STATS_TO_AGGREGATE = ["branch_length", "branch_thickness", "branch_aspect_ratio", "branch_tortuosity", "branch_area", "branch_axis_length_maj",
                      "branch_axis_length_min", "branch_extent", "branch_solidity", "reassigned_label"]


def positive_offsets(D):
    """the reference's offsets: dz, dy, dx each over -1, 0, 1, kept when the first non-zero component is +1"""
    out = []
    for d in np.ndindex(*(3,) * D):
        d = tuple(v - 1 for v in d)
        if any(d) and next(v for v in d if v) > 0:
            out.append(d)
    return out


def pair_counts(skel, labels):
    """(len(labels), offsets) int64: same-label pairs per label and positive offset; and the degree image (uint8)"""
    skel = np.asarray(skel)
    D = skel.ndim
    degree = np.zeros(skel.shape, np.uint8)
    offsets = positive_offsets(D)
    counts = np.zeros((len(labels), len(offsets)), np.int64)
    for j, d in enumerate(offsets):
        base = skel[tuple(slice(max(0, v), skel.shape[a] + min(0, v)) for a, v in enumerate(d))]
        neigh = skel[tuple(slice(max(0, -v), skel.shape[a] - max(0, v)) for a, v in enumerate(d))]
        same = (base > 0) & (base == neigh)
        degree[tuple(slice(max(0, v), skel.shape[a] + min(0, v)) for a, v in enumerate(d))] += same.astype(np.uint8)
        degree[tuple(slice(max(0, -v), skel.shape[a] - max(0, v)) for a, v in enumerate(d))] += same.astype(np.uint8)
        got, n = np.unique(base[same], return_counts=True)
        counts[np.searchsorted(labels, got), j] = n
    return counts, degree


def radii(border, idxs, spacing):
    """the distance in um from every voxel of idxs to the nearest voxel with border != 0: the minimum over all of them"""
    return nr.thickness(border, idxs, spacing) / 2.0              # sqrt(d2) * 2 / 2: exact


def skeleton_stats(skel, border, spacing):
    """dict: branch_idxs, labels per voxel, branch_label, the four float32 statistics, and degree, radius, tips, lone per voxel"""
    skel = np.asarray(skel)
    D = skel.ndim
    s = [float(v) for v in spacing]
    idxs = np.argwhere(skel > 0)
    lab = skel[tuple(idxs.T)]
    uniq = np.unique(lab)
    out = dict(branch_idxs=idxs, labels=lab, branch_label=uniq.astype(int))
    if len(idxs) == 0:
        return out
    counts, degree = pair_counts(skel, uniq)
    deg = degree[tuple(idxs.T)]
    rad = radii(border, idxs, spacing)
    tips, lone = np.where(deg == 1)[0], np.where(deg == 0)[0]
    length = np.zeros(len(uniq), np.float32)
    for j, d in enumerate(positive_offsets(D)):
        sq = 0.0
        for a in range(D):
            sq = sq + (d[a] * s[a]) * (d[a] * s[a])
        edge = np.float32(np.sqrt(sq))
        for i in range(len(uniq)):
            length[i] = np.float32(np.float64(length[i]) + counts[i, j] * np.float64(edge))
    at = {int(l): i for i, l in enumerate(uniq)}
    for k in lone:
        i = at[int(lab[k])]
        length[i] = np.float32(np.float64(length[i]) + 2.0 * rad[k])
    for k in tips:
        i = at[int(lab[k])]
        length[i] = np.float32(np.float64(length[i]) + rad[k])
    thick = np.zeros(len(uniq), np.float32)
    with np.errstate(all="ignore"):
        for i, l in enumerate(uniq):
            thick[i] = np.median((rad * 2.0)[lab == l])
        for i in range(len(uniq)):
            if not np.isnan(thick[i]) and thick[i] > length[i]:
                thick[i], length[i] = length[i], thick[i]
        aspect = np.full(len(uniq), np.nan, np.float32)
        for i in range(len(uniq)):
            if thick[i] != 0:
                aspect[i] = length[i] / thick[i]
        tort = np.ones(len(uniq), np.float32)
        for i, l in enumerate(uniq):
            mine = idxs[tips[lab[tips] == l]]
            if len(mine) >= 2:
                sq = 0.0
                for a in range(D):
                    d = (mine[0][a] - mine[1][a]) * s[a]
                    sq = sq + d * d
                dist = np.sqrt(sq)
                if dist > 0:
                    tort[i] = np.float32(np.float64(length[i]) / dist)
    out.update(branch_length=length, branch_thickness=thick, branch_aspect_ratio=aspect, branch_tortuosity=tort, degree=deg, radius=rad, tips=tips,
               lone=lone, pair_counts=counts)
    return out


def reassigned_mode(values):
    """argmax(bincount(values)) by counting: the most frequent value, zeros counted, the smallest among equals"""
    seen = {}
    for v in np.asarray(values).tolist():
        seen[v] = seen.get(v, 0) + 1
    top = max(seen.values())
    return min(v for v, c in seen.items() if c == top)


def region_columns(label_branches, spacing, reassigned=None):
    """{name: (regions,) float64} for REGION_STATS plus `label` (int64): every label > 0 of the volume, ascending"""
    lab = np.asarray(label_branches)
    D = lab.ndim
    s = [float(v) for v in spacing]
    P = float(np.prod(spacing))
    where = np.argwhere(lab > 0)
    of = lab[tuple(where.T)]
    order = np.argsort(of, kind="stable")
    where, of = where[order], of[order]
    labels, start = np.unique(of, return_index=True)
    stop = np.append(start[1:], len(of))
    out = {k: np.full(len(labels), np.nan) for k in REGION_STATS}
    out["label"] = labels.astype(np.int64)
    for r, (a, b) in enumerate(zip(start, stop)):
        c = where[a:b]
        n = int(b - a)
        S = [int(c[:, ax].sum()) for ax in range(D)]
        Q = [[int((c[:, ax] * c[:, bx]).sum()) for bx in range(D)] for ax in range(D)]
        extents = [int(c[:, ax].max() - c[:, ax].min() + 1) for ax in range(D)]
        area = n * P
        out["branch_area"][r] = area
        out["branch_extent"][r] = area / (float(np.prod(extents)) * P)
        for ax in range(D):
            out["zyx"[3 - D + ax]][r] = (S[ax] / n) * s[ax]
        C = np.array([[float(n * Q[ax][bx] - S[ax] * S[bx]) / float(n * n) * (s[ax] * s[bx]) for bx in range(D)] for ax in range(D)])
        lam = np.clip(np.linalg.eigvalsh(C), 0.0, None)
        if D == 3:
            out["branch_axis_length_maj"][r], out["branch_axis_length_min"][r] = np.sqrt(20.0 * lam.max()), np.sqrt(20.0 * lam.min())
        else:
            out["branch_axis_length_maj"][r], out["branch_axis_length_min"][r] = 4.0 * np.sqrt(lam.max()), 4.0 * np.sqrt(lam.min())
        if reassigned is not None:
            out["reassigned_label"][r] = reassigned_mode(np.asarray(reassigned)[tuple(c.T)])
    return out


def label_groups(labels):
    """CSR (offsets, indices) of the positions of every distinct non-zero label, labels ascending, positions ascending"""
    labels = np.asarray(labels)
    groups = [np.argwhere(labels == l).flatten() for l in np.unique(labels) if l != 0]
    return nr.as_csr(groups)


class Branches:
    """the reference's Branches on a hierarchy double: same attributes, per frame"""

    def __init__(self, hierarchy):
        self.hierarchy = hierarchy
        self.time, self.branch_label, self.aggregate_voxel_metrics, self.aggregate_node_metrics = [], [], [], []
        for k in SKELETON_STATS + REGION_STATS:
            setattr(self, k, [])
        self.branch_idxs, self.component_label, self.image_name = [], [], []
        self.stats_to_aggregate = list(STATS_TO_AGGREGATE)
        self.features_to_save = self.stats_to_aggregate + ["x", "y", "z"]
        self.region_label = []                                    # the labels of label_branches per frame: not in the reference

    def run(self, regions=True):
        h = self.hierarchy
        for t in range(h.num_t):
            sk = skeleton_stats(h.im_skel[t], h.im_border_mask[t], h.spacing)
            self.branch_idxs.append(sk["branch_idxs"])
            if len(sk["branch_idxs"]) == 0:
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
                continue
            B = len(sk["branch_label"])
            self.time.append(np.ones(B, dtype=int) * t)
            first = np.array([sk["branch_idxs"][np.flatnonzero(sk["labels"] == l)[0]] for l in sk["branch_label"]])
            self.component_label.append(np.asarray(h.label_components[t])[tuple(first.T)])
            self.branch_label.append(sk["branch_label"])
            self.image_name.append(np.ones(B, dtype=object) * h.im_info.file_info.filename_no_ext)
            self.aggregate_voxel_metrics.append(nr.aggregate_stats_for_class(h.voxels, t, label_groups(h.voxels.branch_labels[t])))
            if not h.skip_nodes:
                self.aggregate_node_metrics.append(nr.aggregate_stats_for_class(h.nodes, t, label_groups(h.nodes.branch_label[t])))
            for k in SKELETON_STATS:
                getattr(self, k).append(sk[k])
            if not regions:                                        # the reference with regionprops returning []
                for k in REGION_STATS:
                    getattr(self, k).append([])
                self.region_label.append(np.zeros(0, np.int64))
                continue
            re = getattr(h, "im_branch_reassigned", None)
            cols = region_columns(h.label_branches[t], h.spacing, None if re is None or h.im_info.no_t else re[t])
            for k in REGION_STATS:
                getattr(self, k).append(cols[k])
            self.region_label.append(cols["label"])


def feature_table(branches):
    """header and text of features_branches by the reference's saving rule (hierarchical.py:279-337, 381-397, 611-625): per frame
    one float64 array through pandas' to_csv, header once; columns t, label (branch_label[t]), <stat>_<key> of the node aggregates
    (if any), of the voxel aggregates, then <feature>_raw of features_to_save.  A frame without branches writes no rows."""
    import io
    import pandas as pd
    buf = io.StringIO()
    header = None
    for t in range(len(branches.branch_label)):
        if len(branches.branch_label[t]) == 0:
            continue
        cols, names = [], []
        for frames in (branches.aggregate_node_metrics, branches.aggregate_voxel_metrics):
            if not frames:
                continue
            for stat, keys in frames[t].items():
                for key, vals in keys.items():
                    cols.append(np.array(vals)[0])
                    names.append(f"{stat}_{key}")
        for feature in branches.features_to_save:
            cols.append(np.array([np.array(getattr(branches, feature)[t])])[0])
            names.append(f"{feature}_raw")
        labels = np.asarray(branches.branch_label[t])
        cols = [np.full(len(labels), t, dtype=np.int64), labels] + cols
        first = header is None
        if first:
            header = ["t", "label"] + names
        pd.DataFrame(np.array(cols).T, columns=header).to_csv(buf, index=False, mode="a", header=first)
    return header, buf.getvalue()
