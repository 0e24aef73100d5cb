"""
`Nodes`: drop-in for nellie.feature_extraction.hierarchical.Nodes (reference hierarchical.py:1275-1441), the second level of the
reference's Hierarchy, on the MI355X HIP engine.  Per frame it lists the skeleton nodes (pixel class > 0) with their component
and branch labels, measures their thickness (twice the distance to the nearest border voxel), derives the position, divergence,
convergence and vergere of every node from the voxels assigned to it, and aggregates the eleven voxel statistics over those
voxels.  Same constructor argument, same `.run()`, same attributes (lists with one entry per frame).

`aggregate_stats_for_class` is the reference's function of that name (hierarchical.py:1165-1272) on the device: mean, std_dev,
min, max and sum of every 1-D statistic of a class over groups of indices.  Its sums are numpy's sums over rows padded to the
longest group of the call (pairwise within numpy's buffer blocks of 8192 elements, the blocks added in order), which is what the
reference's default path computes; the padded matrix itself is never built.

`NodeFeatures(im_info).run()` opens the files the reference's Hierarchy opens, runs `Voxels` then `Nodes` and writes the voxel
and the node table (`features_voxels`, `features_nodes`) as the reference's Hierarchy does.

`hierarchy.voxels` may be this package's Voxels, the reference's or any object with the same lists: its attributes are read as
host arrays.  Differences: `hierarchy.low_memory` is accepted and ignored, the values are always those of
the reference's default path; a frame whose vec01 / vec12 has no rows counts as all NaN where the reference raises; the six
per-node sequences the reference keeps as lists of floats are float64 arrays.  There is no CPU engine behind these classes
(`device="cpu"` raises).
"""
from __future__ import annotations

import numpy as np

from nellie_amd.feature_extraction.hierarchy import Level
from nellie_amd.feature_extraction.voxels import VoxelFeatures, _image_name
from nellie_amd.stage import require_gpu

KEYS = ("mean", "std_dev", "min", "max", "sum")


def _as_csr(list_of_idxs):
    """a list of index arrays (an empty one may be numpy's empty float64 array) or an (offsets, values) pair -> int64 (offsets, values)"""
    if isinstance(list_of_idxs, tuple) and len(list_of_idxs) == 2:
        return np.asarray(list_of_idxs[0], np.int64), np.asarray(list_of_idxs[1], np.int64)
    groups = [np.asarray(a).reshape(-1) for a in list_of_idxs]
    off = np.zeros(len(groups) + 1, np.int64)
    np.cumsum([len(a) for a in groups], out=off[1:])
    val = np.concatenate([a.astype(np.int64) for a in groups]) if off[-1] else np.zeros(0, np.int64)
    return off, val


def _aggregate(engine, child_class, t):
    """the reference's dict of dicts over the groups loaded in `engine`"""
    out = {}
    for name in child_class.stats_to_aggregate:
        if name == "reassigned_label":
            continue
        values = np.array(getattr(child_class, name)[t])
        if values.ndim > 1:                                       # skipped, as in the reference: its lists stay empty
            out[name] = {key: np.array([]) for key in KEYS}
            continue
        res = engine.aggregate(values)
        out[name] = {key: res[key][None, :] for key in KEYS}
    return out


def aggregate_groups(engine, child_class, t, offsets, idx, rows, what):
    """(the reference's dict of dicts of `child_class`'s statistics over the CSR groups, the device time): every 1-D statistic must
    have one value per row of the child level, `rows` of them (`what` names them in the error)"""
    for name in child_class.stats_to_aggregate:
        values = np.asarray(getattr(child_class, name)[t]) if name != "reassigned_label" else None
        if values is not None and values.ndim == 1 and len(values) != rows:
            raise ValueError(f"frame {t}: {name} has {len(values)} values for {rows} {what}")
    engine.groups(offsets, idx)
    return _aggregate(engine, child_class, t), engine.kernel_ms_parts()["aggregation"]


def aggregate_stats_for_class(child_class, t, list_of_idxs, low_memory: bool = False, device_index: int = 0):
    """{statistic: {mean | std_dev | min | max | sum: (1, groups) float64}} of every 1-D statistic in
    child_class.stats_to_aggregate at frame t over the groups `list_of_idxs`: a list of index arrays, or a CSR pair (offsets,
    values).  Groups are taken in the order given; they need be neither sorted nor disjoint.  `low_memory` is ignored."""
    from nellie_amd import hipnative
    require_gpu()
    off, idx = _as_csr(list_of_idxs)
    with hipnative.NodeFeatures(device=device_index) as engine:
        engine.groups(off, idx)
        return _aggregate(engine, child_class, t)


class Nodes(Level):
    word, name = "node", "nodes"
    handles = ("_engine",)

    @property
    def table_key(self):
        return None if self.hierarchy.skip_nodes else "features_nodes"

    def __init__(self, hierarchy):
        self.hierarchy = hierarchy
        self.time = []
        self.nodes = []
        self.aggregate_voxel_metrics = []
        self.z = []
        self.x = []
        self.y = []
        self.node_thickness = []
        self.divergence = []
        self.convergence = []
        self.vergere = []
        self.stats_to_aggregate = ["divergence", "convergence", "vergere", "node_thickness"]
        self.features_to_save = self.stats_to_aggregate + ["x", "y", "z"]
        self.voxel_idxs = self.hierarchy.voxels.node_voxel_idxs
        self.branch_label = []
        self.component_label = []
        self.image_name = []
        self.node_z_lims = self.hierarchy.voxels.node_dim0_lims
        self.node_y_lims = self.hierarchy.voxels.node_dim1_lims
        self.node_x_lims = self.hierarchy.voxels.node_dim2_lims
        self.longest = []                                         # L, the longest voxel list, per frame of the last run
        self.kernel_ms = []                                       # device time per frame and part of the last run
        self._engine = None

    def _voxel_lists(self, t):
        """the frame's node -> voxel lists as CSR: this package's Voxels has them in that form already"""
        v = self.hierarchy.voxels
        csr = getattr(v, "node_voxel_idxs_csr", None)
        if csr is not None and len(csr) > t and getattr(v, "node_voxel_idxs", None) is self.voxel_idxs:
            return np.asarray(csr[t][0], np.int64), np.asarray(csr[t][1], np.int64)
        return _as_csr(self.voxel_idxs[t])

    def _run_frame(self, t):
        h, v, eng = self.hierarchy, self.hierarchy.voxels, self._engine
        m = eng.frame(h.im_pixel_class[t], h.label_components[t], h.label_branches[t], h.im_border_mask[t])
        coords, comp, branch, thickness = eng.fetch()
        self.nodes.append(coords)
        self.time.append(np.ones(m, dtype=int) * t)
        self.component_label.append(comp)
        self.branch_label.append(branch)
        self.image_name.append(np.ones(m, dtype=object) * _image_name(h.im_info))
        off, idx = self._voxel_lists(t)
        if len(off) - 1 != m:
            raise ValueError(f"frame {t}: {len(off) - 1} voxel lists for {m} nodes")
        self.longest.append(eng.groups(off, idx))
        self.aggregate_voxel_metrics.append(_aggregate(eng, v, t))
        self.node_thickness.append(thickness)
        vecs = [np.asarray(a[t]) for a in (v.vec01, v.vec12)]
        stats = eng.node_stats(np.asarray(v.coords[t]), *[a if len(a) else None for a in vecs])
        for name in eng.STATS:
            getattr(self, name).append(stats[name])
        self.kernel_ms.append(eng.kernel_ms_parts())

    def _open(self, device):
        from nellie_amd import hipnative
        h = self.hierarchy
        self.longest = []
        self._engine = hipnative.NodeFeatures(tuple(np.shape(h.im_pixel_class[0])), h.spacing, device=device)

    def run(self):
        if not self.hierarchy.skip_nodes:
            super().run()


class NodeFeatures(VoxelFeatures):
    """The voxel and the node level of the hierarchy from an ImInfo's files to their tables: runs `Voxels` then `Nodes`, writes
    `features_voxels` and, unless `skip_nodes`, `features_nodes`; the objects stay in `.voxels` and `.nodes`."""

    low_memory = False
    levels = VoxelFeatures.levels + (Nodes,)
