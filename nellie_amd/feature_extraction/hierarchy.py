"""
What the five feature levels share: `Level`, the life-cycle of one level (its device handles, `close()`, the per-frame loop of
`run()`); `LevelDriver`, which opens the files the reference's Hierarchy opens (hierarchical.py:190-233) and runs a list of levels
in order, one loop as the reference's (hierarchical.py:538-566); and `write_table`, the one writer of the five feature tables by
the reference's saving rule (`feature_frames`; hierarchical.py:279-337, 611-625).

`Hierarchy` is the drop-in for the reference's class of that name (hierarchical.py:44-608): a `LevelDriver` over all five levels
that then writes the adjacency maps.  `adjacency_maps` builds those six edge lists (hierarchical.py:433-536) on the device
(csrc/adjacency.inc).

The level modules import this one; it imports none of them: `Hierarchy` looks its levels up when it is first asked for them.
"""
from __future__ import annotations

import os
import pickle

import numpy as np

from nellie_amd.stage import frame_count, require_gpu, resolve_device, spacing_of
from nellie_amd.utils.base_logger import logger

AGGREGATES = ("aggregate_node_metrics", "aggregate_voxel_metrics", "aggregate_branch_metrics", "aggregate_component_metrics")


class Level:
    """One level of the hierarchy.  A level class names itself (`word` in the messages, `name` of the driver's attribute that holds
    it), its table (`table_key` in pipeline_paths, `label_list`: the attribute with the labels per frame, None for the row number),
    what it reads of the driver (`reads_flow`, `reads_reassigned`) and its device handles; it opens them in `_open(device)` and
    does a frame in `_run_frame(t)`."""

    word = name = table_key = label_list = None
    handles = ()
    reads_flow = reads_reassigned = False

    def table_labels(self):
        return None if self.label_list is None else getattr(self, self.label_list)

    def close(self):
        for name in self.handles:
            if getattr(self, name) is not None:
                getattr(self, name).close()
                setattr(self, name, None)

    def run(self):
        h = self.hierarchy
        require_gpu()
        self.kernel_ms = []
        try:
            self._open(int(getattr(h, "device_index", 0)))
            for t in range(h.num_t):
                if h.viewer is not None:
                    h.viewer.status = f"Extracting {self.word} features. Frame: {t + 1} of {h.num_t}."
                self._run_frame(t)
        finally:
            self.close()


def _names(level, t=None):
    """the column names after t and label: <statistic>_<key> of frame t's aggregates (none for t = None), then <feature>_raw"""
    names = []
    for frames in (getattr(level, attr, None) for attr in AGGREGATES):
        if frames and t is not None:
            names += [f"{stat}_{key}" for stat, keys in frames[t].items() for key in keys]
    return names + [f"{name}_raw" for name in level.features_to_save]


def feature_frames(level, labels):
    """per frame with rows: (t, float64 array (rows, columns), header) by the reference's saving rule (hierarchical.py:279-337): the
    columns t, label, <statistic>_<key> of the node aggregates (if any), of the voxel aggregates, of the branch aggregates and of the
    component aggregates (a level that has them), then <feature>_raw for every feature of features_to_save.  Columns of different lengths raise ValueError."""
    for t in range(len(labels)):
        lab = np.asarray(labels[t])
        if len(lab) == 0:
            continue
        names, columns = _names(level, t), []
        for frames in (getattr(level, attr, None) for attr in AGGREGATES):
            if frames:
                columns += [np.array(vals)[0] for keys in frames[t].values() for vals in keys.values()]
        columns += [np.asarray(getattr(level, name)[t]) for name in level.features_to_save]
        for name, col in zip(names, columns):
            if col.shape != lab.shape:
                raise ValueError(f"frame {t}: column {name} has {len(col)} rows for {len(lab)} labels: the region columns (one row per label "
                                 f"of label_branches), the aggregates (one per label of the voxels or nodes) and the skeleton columns "
                                 f"(one per label of im_skel) differ in length")
        columns = [np.full(len(lab), t, dtype=np.int64), lab] + columns
        yield t, np.array(columns).T, ["t", "label"] + names


def _disjoint_statistics(level, t):
    """the reference merges the aggregate dicts of a frame (three for the organelles, four for the image) with dict.update:
    concatenating them is the same table only while no statistic has the same name in two of them"""
    seen = set()
    for frames in (getattr(level, attr, None) for attr in AGGREGATES):
        if not frames:
            continue
        names = set(frames[t])
        assert not (seen & names), f"frame {t}: statistics {sorted(seen & names)} are aggregated from two levels"
        seen |= names


def write_table(level, path, labels=None):
    """a level's table as the reference's Hierarchy writes it: per frame one float64 array (feature_frames) through pandas' to_csv,
    the header once.  `labels`: the label column per frame; None: the row number within the frame, as many rows as the level's first
    feature has.  The column names are those of the first frame with rows; when no frame has rows the header alone is written, with
    the names of frame 0 as it stands (without frames: t, label and the <feature>_raw names)."""
    import pandas as pd
    if labels is None:
        labels = [np.arange(len(col), dtype=np.int64) for col in getattr(level, level.features_to_save[0])]
    for t in range(len(labels)):
        _disjoint_statistics(level, t)
    header = None
    for t, frame, names in feature_frames(level, labels):
        first = header is None
        header = header or names
        pd.DataFrame(frame, columns=header).to_csv(path, index=False, mode="w" if first else "a", header=first)
    if header is None:
        header = ["t", "label"] + _names(level, 0 if len(labels) else None)
        pd.DataFrame(np.zeros((0, len(header))), columns=header).to_csv(path, index=False)


class LevelDriver:
    """Runs the levels listed in `levels` from an ImInfo's files to their tables: opens what the reference's Hierarchy opens
    (hierarchical.py:190-233), then per level builds it (it stays in the attribute the level names), runs it and writes its table,
    so a failure in a late level leaves the earlier tables on disk.  `solidity=True` makes `Branches` and `Components` fill their
    solidity column; it is NaN otherwise."""

    levels = ()

    def __init__(self, im_info, skip_nodes: bool = False, enable_motility: bool = True, device: str = "auto", device_index: int = 0, viewer=None,
                 solidity: bool = False):
        self.im_info = im_info
        self.solidity = bool(solidity)                           # Branches and Components: exact convex counts instead of NaN
        resolve_device(device)
        self.device = device or "auto"
        self.device_index = int(device_index)
        self.skip_nodes = skip_nodes
        self.enable_motility = enable_motility
        self.viewer = viewer
        self.num_t = frame_count(im_info)
        self.spacing = spacing_of(im_info)
        self.im_raw = self.im_struct = self.im_distance = self.im_skel = self.im_pixel_class = self.im_border_mask = None
        self.label_components = self.label_branches = None
        self.im_obj_reassigned = self.im_branch_reassigned = None
        self.flow_interpolator_fw = self.flow_interpolator_bw = None
        self.voxels = self.nodes = self.branches = self.components = self.image = None

    def _allocate_memory(self):
        paths, get = self.im_info.pipeline_paths, self.im_info.get_memmap
        self.im_raw = get(self.im_info.im_path)
        self.im_struct = get(paths["im_preprocessed"])
        self.im_distance = get(paths["im_distance"])
        self.im_skel = get(paths["im_skel"])
        self.label_components = get(paths["im_instance_label"])
        self.label_branches = get(paths["im_skel_relabelled"])
        self.im_border_mask = get(paths["im_border"])
        self.im_pixel_class = get(paths["im_pixel_class"])
        if self.im_info.no_t:                                    # the files of a single frame have no T axis: one frame per stack
            for name in ("im_raw", "im_struct", "im_distance", "im_skel", "label_components", "label_branches", "im_border_mask", "im_pixel_class"):
                setattr(self, name, getattr(self, name)[None])
            return
        if not any(cls.reads_reassigned for cls in self.levels):
            return
        obj, branch = paths.get("im_obj_label_reassigned"), paths.get("im_branch_label_reassigned")   # the reference's rule (hierarchical.py:217-233)
        if obj and branch and os.path.exists(obj) and os.path.exists(branch):
            self.im_obj_reassigned = get(obj)
            self.im_branch_reassigned = get(branch)

    def _run_with_flow(self, level):
        """the flow interpolators live as long as the level that reads them"""
        from nellie_amd.tracking.flow_interpolation import FlowInterpolator
        try:
            if self.enable_motility and not self.im_info.no_t and self.num_t > 1:
                self.flow_interpolator_fw = FlowInterpolator(self.im_info, device_index=self.device_index)
                self.flow_interpolator_bw = FlowInterpolator(self.im_info, forward=False, device_index=self.device_index)
            level.run()
        finally:
            for obj in (self.flow_interpolator_fw, self.flow_interpolator_bw):
                if obj is not None:
                    obj.close()

    def run(self):
        require_gpu()
        level = None
        for cls in self.levels:
            logger.info(f"Running {cls.word} feature extraction (HIP).")
            if level is None:
                self._allocate_memory()
            level = cls(self)
            setattr(self, cls.name, level)
            if cls.reads_flow:
                self._run_with_flow(level)
            else:
                level.run()
            if level.table_key is None:
                continue
            if self.viewer is not None and cls is self.levels[0]:
                self.viewer.status = "Saving features to csv files."
            write_table(level, self.im_info.pipeline_paths[level.table_key], level.table_labels())
        return level


ADJACENCY_KEYS = ("v_b", "v_n", "v_o", "n_b", "n_o", "b_o")         # the pickle's keys, in the reference's order


def adjacency_maps(hierarchy, device_index: int = 0, kernel_ms=None):
    """The reference's adjacency maps (hierarchical.py:433-536) of any object with its attributes (`voxels`, `nodes`, `branches`,
    `components`, `skip_nodes`): {key: one (m, 2) int64 array per frame} for v_b (voxel, branch label - 1), v_n (voxel, every node of
    its list), v_o (voxel, component label), n_b, n_o and b_o (row, position of its label among the parent level's labels); v_n, n_b
    and n_o are empty lists under skip_nodes.  The frame counts are the reference's: len(voxels.time) for the voxel lists,
    len(nodes.time) for the node lists, len(branches.time) for b_o.  v_n comes from `voxels.node_labels_csr[t]` where that exists,
    else from `voxels.node_labels[t]` (a None entry is an empty list).  One device handle serves all frames.
    Differences: a child label above its parents' largest raises ValueError (IndexError in the reference), a negative label raises
    ValueError (numpy would wrap it around).  `kernel_ms`: a dict that receives the device time per operation, summed."""
    from nellie_amd import hipnative
    from nellie_amd.feature_extraction.nodes import _as_csr
    require_gpu()
    v, n, b, c = hierarchy.voxels, hierarchy.nodes, hierarchy.branches, hierarchy.components
    skip_nodes = bool(hierarchy.skip_nodes)
    maps = {key: [] for key in ADJACENCY_KEYS}
    ms = dict.fromkeys(hipnative.Adjacency.PARTS, 0.0)
    adj = hipnative.Adjacency(device=device_index)

    def timed(op, *args):
        out = getattr(adj, op)(*args)
        ms[op] += adj.kernel_ms_parts()[op]
        return out

    try:
        csr = getattr(v, "node_labels_csr", None)
        for t in range(len(v.time)):
            if not skip_nodes:
                if csr is not None and len(csr) > t:
                    off, val = _as_csr(tuple(csr[t]))
                else:
                    off, val = _as_csr([() if a is None else a for a in v.node_labels[t]])
                maps["v_n"].append(timed("expand", off, val))
            maps["v_b"].append(timed("pairs", np.asarray(v.branch_labels[t]), 1))
            maps["v_o"].append(timed("pairs", np.asarray(v.component_labels[t]), 0))
        if not skip_nodes:
            for t in range(len(n.time)):
                maps["n_b"].append(timed("lookup", np.asarray(n.branch_label[t]), np.asarray(b.branch_label[t])))
                maps["n_o"].append(timed("lookup", np.asarray(n.component_label[t]), np.asarray(c.component_label[t])))
        for t in range(len(b.time)):
            maps["b_o"].append(timed("lookup", np.asarray(b.component_label[t]), np.asarray(c.component_label[t])))
    finally:
        adj.close()
    if kernel_ms is not None:
        kernel_ms.update(ms)
    return maps


class _WithOptions(type):
    """`Hierarchy.__init__` keeps the reference's parameters and `device_index`, nothing else, so that it stays a drop-in by position
    and by introspection; what this package adds beyond them is a keyword taken off here: Hierarchy(im_info, ..., solidity=True)."""

    def __call__(cls, *args, solidity: bool = False, **kwargs):
        obj = super().__call__(*args, **kwargs)
        obj.solidity = bool(solidity)
        return obj


class Hierarchy(LevelDriver, metaclass=_WithOptions):
    """Drop-in for nellie.feature_extraction.hierarchical.Hierarchy: same constructor arguments and defaults (and `device_index`),
    same `.run()`, same files -- the five feature tables, written level by level as `ImageFeatures` writes them, and the
    `adjacency_maps` pickle unless `enable_adjacency` is false.  The keyword `solidity=True` (default False: the two solidity columns
    stay NaN) fills them from exact convex counts.  `low_memory`, `node_chunk_size` and `max_node_mask_elems` are
    accepted and ignored; there is no CPU engine (`device="cpu"` raises).  The level objects stay in `.voxels`, `.nodes`,
    `.branches`, `.components` and `.image`; `adjacency_kernel_ms` holds the device time of the last run's edge lists."""

    def __init__(self, im_info, skip_nodes: bool = True, viewer=None, use_gpu: bool = True, low_memory: bool = False,
                 enable_motility: bool = True, enable_adjacency: bool = True, device: str = None, node_chunk_size: int = None,
                 max_node_mask_elems: int = int(5e7), device_index: int = 0):
        super().__init__(im_info, skip_nodes=skip_nodes, enable_motility=enable_motility, device=device, device_index=device_index, viewer=viewer)
        self.use_gpu = True
        self.low_memory = low_memory
        self.enable_adjacency = enable_adjacency
        self.node_chunk_size = node_chunk_size
        self.max_node_mask_elems = int(max_node_mask_elems)
        self.adjacency_kernel_ms = {}

    @property
    def levels(self):
        from nellie_amd.feature_extraction.image import ImageFeatures
        return ImageFeatures.levels

    def _save_adjacency_maps(self):
        edges = adjacency_maps(self, device_index=self.device_index, kernel_ms=self.adjacency_kernel_ms)
        with open(self.im_info.pipeline_paths["adjacency_maps"], "wb") as f:
            pickle.dump(edges, f)

    def run(self):
        super().run()
        if self.viewer is not None:
            self.viewer.status = "Finalizing run."
        if self.enable_adjacency:
            self._save_adjacency_maps()
        if self.viewer is not None:
            self.viewer.status = "Done!"
