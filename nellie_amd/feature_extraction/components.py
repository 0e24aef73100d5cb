"""
`Components`: drop-in for nellie.feature_extraction.hierarchical.Components (reference hierarchical.py:1880-2043), the fourth level
of the reference's Hierarchy (the organelles), on the MI355X HIP engine.  Per frame it sums the voxel coordinates of every region
of `label_components` exactly, finds the most frequent reassigned label of every region, and aggregates the voxel, node and branch
statistics per component label.  Same constructor argument, same `.run()`, same attributes (lists with one entry per frame).

The region sums are taken on the device per run of equal labels along X (csrc/branchfeat.inc, bf_region_rows_kernel): an organelle
network holds 10^5 - 10^6 voxels, which one set of atomics per voxel would all send to the same sixteen addresses (DESIGN.md
section 18 has the measurement).  What is left is O(components) numpy: the region columns from the integer sums
(branches.region_columns).

The groups follow the reference exactly (hierarchical.py:1917-1950): the label list is np.unique(voxels.component_labels[t])
without 0, and the voxels, the nodes and the branches are all grouped by that list, positions ascending; a label without a node or
a branch is an empty group, whose row is NaN with sum 0.

`ComponentFeatures(im_info).run()` opens the files the reference's Hierarchy opens, runs `Voxels`, `Nodes`, `Branches` and
`Components` and writes `features_voxels`, `features_nodes`, `features_branches` and `features_organelles` as the reference's
Hierarchy does.

`hierarchy.voxels`, `hierarchy.nodes` and `hierarchy.branches` may be this package's objects, the reference's or any object with
the same lists.  Differences: `organelle_solidity` is NaN unless `hierarchy.solidity` is true, when it is the exact restatement of
skimage's area / area_convex; the region columns follow skimage's documented
formulas and a negative square-root argument gives 0 where the reference's `except ValueError` gives NaN; the region columns and
`reassigned_label` are float64 arrays where the reference keeps lists; a frame without components writes no rows to the table;
`hierarchy.low_memory` is accepted and ignored.  There is no CPU engine behind these classes (`device="cpu"` raises).
"""
from __future__ import annotations

import numpy as np

from nellie_amd.feature_extraction.branches import BranchFeatures, convex_of, region_columns, region_stats
from nellie_amd.feature_extraction.hierarchy import Level
from nellie_amd.feature_extraction.nodes import aggregate_groups
from nellie_amd.feature_extraction.voxels import _image_name

REGION_STATS = region_stats("organelle")


def _groups_of(label_list, labels):
    """CSR (offsets, indices): for every label of `label_list` (ascending, distinct) the positions where `labels` equals it,
    ascending -- the reference's [argwhere(labels == l).flatten() for l in label_list] with one stable sort; a label that does not
    occur is an empty group"""
    lab = np.asarray(labels).reshape(-1)
    order = np.argsort(lab, kind="stable")
    sorted_lab = lab[order]
    lo, hi = np.searchsorted(sorted_lab, label_list, side="left"), np.searchsorted(sorted_lab, label_list, side="right")
    off = np.zeros(len(label_list) + 1, np.int64)
    np.cumsum(hi - lo, out=off[1:])
    return off, order[np.isin(sorted_lab, label_list)].astype(np.int64, copy=False)      # sorted: the groups follow one another


class Components(Level):
    word, name, table_key, label_list = "organelle", "components", "features_organelles", "component_label"
    handles = ("_engine", "_aggregator")
    reads_reassigned = True

    def __init__(self, hierarchy):
        self.hierarchy = hierarchy
        self.time = []
        self.component_label = []
        self.aggregate_voxel_metrics = []
        self.aggregate_node_metrics = []
        self.aggregate_branch_metrics = []
        self.z = []
        self.y = []
        self.x = []
        self.organelle_area = []
        self.organelle_axis_length_maj = []
        self.organelle_axis_length_min = []
        self.organelle_extent = []
        self.organelle_solidity = []
        self.reassigned_label = []
        self.image_name = []
        self.stats_to_aggregate = ["organelle_area", "organelle_axis_length_maj", "organelle_axis_length_min", "organelle_extent", "organelle_solidity",
                                   "reassigned_label"]
        self.features_to_save = self.stats_to_aggregate + ["x", "y", "z"]
        self.kernel_ms = []                                       # device time per frame and part of the last run
        self._engine = None
        self._aggregator = None

    def _aggregate(self, child, label_list, labels, t):
        """the reference's dict of dicts of `child`'s statistics over the groups of `label_list` in `labels`, and the device time"""
        return aggregate_groups(self._aggregator, child, t, *_groups_of(label_list, labels), np.size(labels), "component labels")

    def _run_frame(self, t):
        h, eng = self.hierarchy, self._engine
        frame = h.label_components[t]
        reassigned = getattr(h, "im_obj_reassigned", None)
        R = eng.regions(frame, None if reassigned is None or h.im_info.no_t else reassigned[t], rows=True)
        if R == 0:
            self.component_label.append(np.array([], dtype=int))
            self.time.append(np.array([], dtype=int))
            self.image_name.append(np.array([], dtype=object))
            self.aggregate_voxel_metrics.append({})
            if not h.skip_nodes:
                self.aggregate_node_metrics.append({})
            self.aggregate_branch_metrics.append({})
            for k in REGION_STATS:
                getattr(self, k).append([])
            self.kernel_ms.append(dict(regions=eng.kernel_ms_parts()["regions"], aggregation=0.0))
            return
        labels, sums, mode = eng.fetch_regions()
        convex, convex_ms = convex_of(eng, h)
        self.component_label.append(labels.astype(np.asarray(frame).dtype))
        self.time.append(np.ones(R, dtype=int) * t)
        self.image_name.append(np.ones(R, dtype=object) * _image_name(h.im_info))
        label_list = np.unique(h.voxels.component_labels[t])
        label_list = label_list[label_list != 0]
        agg, ms = self._aggregate(h.voxels, label_list, h.voxels.component_labels[t], t)
        self.aggregate_voxel_metrics.append(agg)
        if not h.skip_nodes:
            agg, more = self._aggregate(h.nodes, label_list, h.nodes.component_label[t], t)
            self.aggregate_node_metrics.append(agg)
            ms += more
        agg, more = self._aggregate(h.branches, label_list, h.branches.component_label[t], t)
        self.aggregate_branch_metrics.append(agg)
        for k, v in region_columns(sums, mode, h.spacing, eng.ndim, prefix="organelle", convex=convex).items():
            getattr(self, k).append(v)
        self.kernel_ms.append(dict(regions=eng.kernel_ms_parts()["regions"], aggregation=ms + more, **convex_ms))

    def _open(self, device):
        from nellie_amd import hipnative
        h = self.hierarchy
        self._engine = hipnative.BranchFeatures(tuple(np.shape(h.label_components[0])), h.spacing, device=device)
        self._aggregator = hipnative.NodeFeatures(device=device)          # one for the run: groups and aggregation need no frame


class ComponentFeatures(BranchFeatures):
    """The voxel, node, branch and organelle level of the hierarchy from an ImInfo's files to their tables: runs `Voxels`, `Nodes`,
    `Branches` and `Components`, writes `features_voxels`, `features_nodes` (unless `skip_nodes`), `features_branches` and
    `features_organelles` (t, label = component_label[t], the node, voxel and branch aggregates in that order, then
    <feature>_raw); the objects stay in `.voxels`, `.nodes`, `.branches` and `.components`."""

    levels = BranchFeatures.levels + (Components,)
