"""numpy restatement of the reference's Components (nellie/feature_extraction/hierarchical.py:1880-2043), test infrastructure only --
never imported by the package.  Literal loops in the reference's order: one pass per label, no search structure, no sort.  It is
checked bit for bit against the reference by the capture of the goldens (tests/golden/make_golden_components.py) and against the
goldens without a GPU (tests/test_components_cpu.py); the GPU tests compare the HIP engine with it where no golden exists.

The region sums are direct sums over the voxel coordinates of every label.  The region columns (area, extent, centroid, axis
lengths) come from tests/branch_features_restatement.py's region_columns, which takes them straight from the coordinates by
skimage's documented formulas with `spacing`; they are NOT reference output (skimage is not installed where the goldens are made),
and `organelle_solidity` is NaN.  The aggregates are tests/node_features_restatement.py's."""
import numpy as np

import branch_features_restatement as br
import node_features_restatement as nr

REGION_STATS = ("organelle_area", "organelle_axis_length_maj", "organelle_axis_length_min", "organelle_extent", "organelle_solidity", "reassigned_label",
                "z", "y", "x")
STATS_TO_AGGREGATE = ["organelle_area", "organelle_axis_length_maj", "organelle_axis_length_min", "organelle_extent", "organelle_solidity",
                      "reassigned_label"]


def region_sums(labels):
    """(labels (R) int64 ascending, sums (F, R) int64) of a label frame by direct summation, in the layout of the device's fetch: n,
    the smallest and the largest coordinate per axis, S_a, Q_ab for a <= b in row order"""
    lab = np.asarray(labels)
    D = lab.ndim
    found = np.unique(lab[lab > 0]).astype(np.int64)
    sums = np.zeros((1 + 3 * D + D * (D + 1) // 2, len(found)), np.int64)
    for r, l in enumerate(found):
        c = np.argwhere(lab == l).astype(np.int64)
        rows = [len(c)] + [c[:, a].min() for a in range(D)] + [c[:, a].max() for a in range(D)] + [c[:, a].sum() for a in range(D)]
        rows += [(c[:, a] * c[:, b]).sum() for a in range(D) for b in range(a, D)]
        sums[:, r] = rows
    return found, sums


def mode_of(labels, reassigned):
    """(R) int64: argmax(bincount) of the reassigned labels over every region, labels ascending"""
    lab, re = np.asarray(labels), np.asarray(reassigned)
    return np.array([br.reassigned_mode(re[lab == l]) for l in np.unique(lab[lab > 0])], np.int64)


def region_columns(label_components, spacing, reassigned=None):
    """{name: (regions,) float64} for REGION_STATS plus `label` (int64): every label > 0 of the frame, ascending"""
    cols = br.region_columns(label_components, spacing, reassigned)
    return {("organelle" + k[len("branch"):] if k.startswith("branch_") else k): v for k, v in cols.items()}


def label_groups(label_list, labels):
    """the reference's lists: for every label of the list the positions where `labels` equals it"""
    labels = np.asarray(labels)
    return [np.argwhere(labels == l).flatten() for l in label_list]


class Components:
    """the reference's Components on a hierarchy double: same attributes, per frame"""

    def __init__(self, hierarchy):
        self.hierarchy = hierarchy
        self.time, self.component_label, self.image_name = [], [], []
        self.aggregate_voxel_metrics, self.aggregate_node_metrics, self.aggregate_branch_metrics = [], [], []
        for k in REGION_STATS:
            setattr(self, k, [])
        self.stats_to_aggregate = list(STATS_TO_AGGREGATE)
        self.features_to_save = self.stats_to_aggregate + ["x", "y", "z"]

    def run(self, regions=True):
        h = self.hierarchy
        for t in range(h.num_t):
            frame = np.asarray(h.label_components[t])
            mask = frame > 0
            if not np.any(mask):
                self.component_label.append(np.array([], dtype=int))
                self.time.append(np.array([], dtype=int))
                self.image_name.append(np.array([], dtype=object))
                self.aggregate_voxel_metrics.append({})
                if not h.skip_nodes:
                    self.aggregate_node_metrics.append({})
                self.aggregate_branch_metrics.append({})
                for k in REGION_STATS:
                    getattr(self, k).append([])
                continue
            found = np.unique(frame[mask])
            self.component_label.append(found)
            self.time.append(np.ones(len(found), dtype=int) * t)
            self.image_name.append(np.ones(len(found), dtype=object) * h.im_info.file_info.filename_no_ext)
            voxel_labels = h.voxels.component_labels[t]
            label_list = [l for l in np.unique(voxel_labels) if l != 0]
            self.aggregate_voxel_metrics.append(nr.aggregate_stats_for_class(h.voxels, t, label_groups(label_list, voxel_labels)))
            if not h.skip_nodes:
                self.aggregate_node_metrics.append(nr.aggregate_stats_for_class(h.nodes, t, label_groups(label_list, h.nodes.component_label[t])))
            self.aggregate_branch_metrics.append(nr.aggregate_stats_for_class(h.branches, t, label_groups(label_list, h.branches.component_label[t])))
            if not regions:                                        # the reference with regionprops returning []
                for k in REGION_STATS:
                    getattr(self, k).append([])
                continue
            re = getattr(h, "im_obj_reassigned", None)
            cols = region_columns(frame, h.spacing, None if re is None or h.im_info.no_t else re[t])
            for k in REGION_STATS:
                getattr(self, k).append(cols[k])


def feature_table(components):
    """header and text of features_organelles by the reference's saving rule (hierarchical.py:279-337, 399-415): per frame one float64
    array through pandas' to_csv, header once; columns t, label (component_label[t]), <stat>_<key> of the node aggregates (if any),
    of the voxel aggregates and of the branch aggregates, merged as the reference's dict.update does, then <feature>_raw of
    features_to_save.  A frame without components writes no rows."""
    import io
    import pandas as pd
    buf = io.StringIO()
    header = None
    for t in range(len(components.component_label)):
        if len(components.component_label[t]) == 0:
            continue
        merged = {}
        for frames in (components.aggregate_node_metrics, components.aggregate_voxel_metrics, components.aggregate_branch_metrics):
            if frames:
                merged.update(frames[t])
        cols, names = [], []
        for stat, keys in merged.items():
            for key, vals in keys.items():
                cols.append(np.array(vals)[0])
                names.append(f"{stat}_{key}")
        for feature in components.features_to_save:
            cols.append(np.array([np.array(getattr(components, feature)[t])])[0])
            names.append(f"{feature}_raw")
        labels = np.asarray(components.component_label[t])
        cols = [np.full(len(labels), t, dtype=np.int64), labels] + cols
        first = header is None
        if first:
            header = ["t", "label"] + names
        pd.DataFrame(np.array(cols).T, columns=header).to_csv(buf, index=False, mode="a", header=first)
    return header, buf.getvalue()
