"""
`Image`: drop-in for nellie.feature_extraction.hierarchical.Image (reference hierarchical.py:2046-2116), the fifth and last level of
the reference's Hierarchy, on the MI355X HIP engine.  Per frame it aggregates every 1-D statistic of the voxels, the nodes, the
branches and the organelles over one group that holds every row of the frame.  Same constructor argument, same `.run()`, same
attributes (lists with one entry per frame).

One group of 10^5 - 10^6 values is what the aggregator's block path is for (csrc/nodefeat.inc, nf_wide_block_kernel; DESIGN.md
section 19): numpy sums a row in blocks of 8192 elements added in order, so one wave takes one block and a last wave adds the
blocks' sums in numpy's order.  The values are those of the reference's default path, bit for bit.

The groups follow the reference exactly (hierarchical.py:2063-2103): arange(len(voxels.coords[t])), arange(len(nodes.nodes[t])),
arange(len(branches.branch_length[t])) and arange(len(components.organelle_area[t])).  A level without rows in a frame is one group
of no values: NaN, with sum 0.

`ImageFeatures(im_info).run()` opens the files the reference's Hierarchy opens, runs `Voxels`, `Nodes`, `Branches`, `Components` and
`Image` and writes `features_voxels`, `features_nodes`, `features_branches`, `features_organelles` and `features_image` as the
reference's Hierarchy does.

`hierarchy.voxels`, `.nodes`, `.branches` and `.components` may be this package's objects, the reference's or any object with the
same lists.  Differences: a 1-D statistic whose length differs from the row count of its level raises
ValueError where the reference would index out of range; `hierarchy.low_memory` is accepted and ignored.  There is no CPU engine
behind these classes (`device="cpu"` raises).
"""
from __future__ import annotations

import numpy as np

from nellie_amd.feature_extraction.components import ComponentFeatures
from nellie_amd.feature_extraction.hierarchy import Level
from nellie_amd.feature_extraction.nodes import aggregate_groups
from nellie_amd.feature_extraction.voxels import _image_name


class Image(Level):
    word, name, table_key = "image", "image", "features_image"
    handles = ("_aggregator",)

    def __init__(self, hierarchy):
        self.hierarchy = hierarchy
        self.time = []
        self.image_name = []
        self.aggregate_voxel_metrics = []
        self.aggregate_node_metrics = []
        self.aggregate_branch_metrics = []
        self.aggregate_component_metrics = []
        self.stats_to_aggregate = []
        self.features_to_save = []
        self.kernel_ms = []                                       # device time per frame of the last run
        self._aggregator = None

    def table_labels(self):
        """one row per frame, a frame without voxels included: its label is 0"""
        return [np.zeros(1, np.int64)] * len(self.time)

    def _aggregate(self, child, rows, t, what):
        """the reference's dict of dicts of `child`'s statistics over the one group of all `rows` rows, and the device time"""
        return aggregate_groups(self._aggregator, child, t, np.array([0, rows], np.int64), np.arange(rows, dtype=np.int64), rows, what)

    def _run_frame(self, t):
        h = self.hierarchy
        self.time.append(t)
        self.image_name.append(_image_name(h.im_info))
        agg, ms = self._aggregate(h.voxels, len(h.voxels.coords[t]), t, "voxels")
        self.aggregate_voxel_metrics.append(agg)
        if not h.skip_nodes:
            agg, more = self._aggregate(h.nodes, len(h.nodes.nodes[t]), t, "nodes")
            self.aggregate_node_metrics.append(agg)
            ms += more
        agg, more = self._aggregate(h.branches, len(h.branches.branch_length[t]), t, "branches")
        self.aggregate_branch_metrics.append(agg)
        ms += more
        agg, more = self._aggregate(h.components, len(h.components.organelle_area[t]), t, "components")
        self.aggregate_component_metrics.append(agg)
        self.kernel_ms.append(dict(aggregation=ms + more))

    def _open(self, device):
        from nellie_amd import hipnative
        self._aggregator = hipnative.NodeFeatures(device=device)          # groups and aggregation need no frame


class ImageFeatures(ComponentFeatures):
    """Every level of the hierarchy from an ImInfo's files to their tables: runs `Voxels`, `Nodes`, `Branches`, `Components` and
    `Image`, writes `features_voxels`, `features_nodes` (unless `skip_nodes`), `features_branches`, `features_organelles` and
    `features_image` (t, label = 0, the node, voxel, branch and component aggregates in that order); the objects stay in `.voxels`,
    `.nodes`, `.branches`, `.components` and `.image`."""

    levels = ComponentFeatures.levels + (Image,)
