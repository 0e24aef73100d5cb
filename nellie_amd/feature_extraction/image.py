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

from nellie_amd.feature_extraction.branches import feature_frames
from nellie_amd.feature_extraction.components import ComponentFeatures, _disjoint_statistics
from nellie_amd.feature_extraction.nodes import _aggregate
from nellie_amd.feature_extraction.voxels import _image_name
from nellie_amd.stage import require_gpu
from nellie_amd.utils.base_logger import logger


class Image:
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

    def close(self):
        if self._aggregator is not None:
            self._aggregator.close()
            self._aggregator = None

    def _aggregate(self, child, rows, t, what):
        """the reference's dict of dicts of `child`'s statistics over the one group of all `rows` rows, and the device time"""
        for name in child.stats_to_aggregate:
            values = np.asarray(getattr(child, name)[t]) if name != "reassigned_label" else None
            if values is not None and values.ndim == 1 and len(values) != rows:
                raise ValueError(f"frame {t}: {name} has {len(values)} values for {rows} {what}")
        self._aggregator.groups(np.array([0, rows], np.int64), np.arange(rows, dtype=np.int64))
        out = _aggregate(self._aggregator, child, t)
        return out, self._aggregator.kernel_ms_parts()["aggregation"]

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

    def run(self):
        from nellie_amd import hipnative
        h = self.hierarchy
        require_gpu()
        self.kernel_ms = []
        try:
            self._aggregator = hipnative.NodeFeatures(device=int(getattr(h, "device_index", 0)))      # groups and aggregation need no frame
            for t in range(h.num_t):
                if h.viewer is not None:
                    h.viewer.status = f"Extracting image features. Frame: {t + 1} of {h.num_t}."
                self._run_frame(t)
        finally:
            self.close()


class ImageFeatures(ComponentFeatures):
    """Every level of the hierarchy from an ImInfo's files to their tables: opens what `ComponentFeatures` opens, runs `Voxels`,
    `Nodes`, `Branches`, `Components` and `Image`, writes `features_voxels`, `features_nodes` (unless `skip_nodes`),
    `features_branches`, `features_organelles` and `features_image`; the objects stay in `.voxels`, `.nodes`, `.branches`,
    `.components` and `.image`."""

    def __init__(self, im_info, skip_nodes: bool = False, enable_motility: bool = True, device: str = "auto", device_index: int = 0, viewer=None):
        super().__init__(im_info, skip_nodes=skip_nodes, enable_motility=enable_motility, device=device, device_index=device_index, viewer=viewer)
        self.image = None

    def _save_image(self):
        """the image table by the reference's rule (hierarchical.py:280-337, 417-431): t, label = 0, the node, voxel, branch and
        component aggregates in that order; one row per frame, a frame without voxels included"""
        import pandas as pd
        im = self.image
        path = self.im_info.pipeline_paths["features_image"]
        header = None
        for t in range(len(im.time)):
            _disjoint_statistics(im, t)
        for t, frame, names in feature_frames(im, [np.zeros(1, np.int64)] * len(im.time)):
            first = header is None
            header = header or names
            pd.DataFrame(frame, columns=header).to_csv(path, index=False, mode="w" if first else "a", header=first)

    def run(self):
        super().run()
        logger.info("Running image feature extraction (HIP).")
        self.image = Image(self)
        self.image.run()
        self._save_image()
        return self.image
