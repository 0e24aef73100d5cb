"""
`Voxels`: drop-in for nellie.feature_extraction.hierarchical.Voxels (reference hierarchical.py:683-1162), the first level of the
reference's Hierarchy, on the MI355X HIP engine.  Per frame it lists the voxels with a component label, gathers their labels,
intensity and structure value, interpolates the flow at every one of them backward and forward, derives the motility features
(linear and angular velocity and acceleration, the same relative to the branch's pivot voxel, directionality) and, unless
`skip_nodes`, assigns every voxel to the skeleton nodes whose radius box holds it.  Same constructor argument, same `.run()`, same
attributes (lists with one entry per frame, the reference's shapes and dtypes), so the reference's Nodes, Branches and Components
can index them.

`VoxelFeatures(im_info).run()` opens the files the reference's Hierarchy opens, runs `Voxels` and writes the voxel table
(`features_voxels`) as the reference's Hierarchy does.

A frame is uploaded once; flow queries, pivots and features never leave the device, and only per-voxel results, the two node
lists (CSR) and the node limits come back.  Differences: a direction in which no voxel has a flow neighbour
gives (n, D) NaN vectors where the reference appends an empty array, and the two differences of the flow interpolation
(section 11) carry over.  There is no CPU engine behind these classes (`device="cpu"` raises).
"""
from __future__ import annotations

import os

import numpy as np

from nellie_amd.feature_extraction.hierarchy import Level, LevelDriver


def _split(offsets, values):
    """CSR -> the reference's list of index arrays: np.array(list), so an empty list is numpy's empty float64 array"""
    return [np.array([]) if a == b else values[a:b] for a, b in zip(offsets[:-1].tolist(), offsets[1:].tolist())]


def _image_name(im_info):
    """the reference's im_info.file_info.filename_no_ext; an ImInfo of this package, which has no file_info, gives the name of its
    canonical input file"""
    name = getattr(getattr(im_info, "file_info", None), "filename_no_ext", None)
    if name is None:
        name = os.path.basename(str(getattr(im_info, "im_path", "image")))
        for ext in (".ome.tif", ".ome.tiff", ".tif", ".tiff", ".npy"):
            if name.lower().endswith(ext):
                name = name[:-len(ext)]
                break
    return name


class Voxels(Level):
    word, name, table_key = "voxel", "voxels", "features_voxels"
    handles = ("_engine",)
    reads_flow = True

    def __init__(self, hierarchy):
        self.hierarchy = hierarchy
        self.time = []
        self.coords = []
        self.x = []
        self.y = []
        self.z = []
        self.intensity = []
        self.structure = []
        self.vec01 = []
        self.vec12 = []
        self.angular_acc = []
        self.angular_vel = []
        self.angular_vel_vector = []
        self.linear_acc = []
        self.linear_vel = []
        self.linear_vel_vector = []
        self.rel_angular_acc = []
        self.rel_angular_vel = []
        self.rel_linear_acc = []
        self.rel_linear_vel = []
        self.rel_directionality = []
        self.node_labels = []
        self.branch_labels = []
        self.component_labels = []
        self.image_name = []
        self.node_dim0_lims = []
        self.node_dim1_lims = []
        self.node_dim2_lims = []
        self.node_voxel_idxs = []
        # the two node lists as CSR (offsets, values) per frame, as they come from the device
        self.node_labels_csr = []
        self.node_voxel_idxs_csr = []
        self.kernel_ms = []                                      # device time per frame and part of the last run
        self.stats_to_aggregate = ["linear_vel", "angular_vel", "linear_acc", "angular_acc", "rel_linear_vel", "rel_angular_vel",
                                   "rel_linear_acc", "rel_angular_acc", "rel_directionality", "structure", "intensity"]
        self.features_to_save = self.stats_to_aggregate + ["x", "y", "z"]
        self._engine = None
        self._own_interpolators = []
        self._flow = (None, None)                                # the (forward, backward) interpolators of the run

    def _interpolators(self):
        """(forward, backward) interpolators with a device_field method, (None, None) when the stack has no motility.  The
        hierarchy's own are used when they are this package's; otherwise this package's are built from im_info."""
        h = self.hierarchy
        fw, bw = getattr(h, "flow_interpolator_fw", None), getattr(h, "flow_interpolator_bw", None)
        if not getattr(h, "enable_motility", True) or fw is None or bw is None or h.num_t is None or h.num_t < 2:
            return None, None
        if hasattr(fw, "device_field") and hasattr(bw, "device_field"):
            return fw, bw
        from nellie_amd.tracking.flow_interpolation import FlowInterpolator
        index = int(getattr(h, "device_index", 0))
        fw = FlowInterpolator(h.im_info, forward=True, device_index=index)
        self._own_interpolators.append(fw)
        bw = FlowInterpolator(h.im_info, forward=False, device_index=index)
        self._own_interpolators.append(bw)
        return fw, bw

    def close(self):
        for obj in self._own_interpolators:
            obj.close()
        self._own_interpolators = []
        self._flow = (None, None)
        super().close()

    def _run_frame(self, t):
        h = self.hierarchy
        eng = self._engine
        fw, bw = self._flow
        comp = h.label_components[t]
        n = eng.frame(comp, h.label_branches[t], h.im_raw[t], h.im_struct[t])
        vox, comp_l, branch_l, intensity, structure = eng.fetch_voxels()
        coords = np.column_stack(np.unravel_index(vox, eng.shape)).astype(np.int64, copy=False).reshape(n, eng.ndim)
        self.coords.append(coords)
        self.component_labels.append(comp_l.astype(comp.dtype, copy=False))
        self.branch_labels.append(branch_l.astype(h.label_branches[t].dtype, copy=False))
        self.intensity.append(intensity)
        self.structure.append(structure)
        self.z.append(coords[:, 0] if eng.ndim == 3 else np.full(n, np.nan))
        self.y.append(coords[:, eng.ndim - 2])
        self.x.append(coords[:, eng.ndim - 1])
        self.time.append(np.ones(n, dtype=int) * t)
        self.image_name.append(np.ones(n, dtype=object) * _image_name(h.im_info))
        if not h.skip_nodes:
            eng.nodes(h.im_pixel_class[t], h.im_distance[t])
            lims, node_csr, vox_csr = eng.fetch_nodes()
            self.node_dim0_lims.append(lims[0])
            self.node_dim1_lims.append(lims[1])
            self.node_dim2_lims.append(lims[2] if eng.ndim == 3 else None)
            self.node_voxel_idxs_csr.append(node_csr)
            self.node_labels_csr.append(vox_csr)
            self.node_voxel_idxs.append(_split(*node_csr))
            self.node_labels.append(_split(*vox_csr))
        field_bw = bw.device_field(t) if bw is not None and t > 0 else None
        field_fw = fw.device_field(t) if fw is not None and t < h.num_t - 1 else None
        eng.motility(field_bw, field_fw)
        for name, values in eng.fetch_motility().items():
            getattr(self, name).append(values)
        self.kernel_ms.append(eng.kernel_ms_parts())

    def _open(self, device):
        from nellie_amd import hipnative
        h = self.hierarchy
        self._flow = self._interpolators()
        dt = h.im_info.dim_res.get("T") or 1.0
        device = int(getattr(self._flow[0], "device_index", device))
        self._engine = hipnative.VoxelFeatures(tuple(h.label_components[0].shape), h.spacing, float(dt), device=device)

    def run(self):
        if self.hierarchy.num_t is None:
            self.hierarchy.num_t = 1
        super().run()


class VoxelFeatures(LevelDriver):
    """The voxel level of the hierarchy from an ImInfo's files to the voxel table: opens what the reference's Hierarchy opens
    (hierarchical.py:190-233), runs `Voxels` and writes `features_voxels`; the `Voxels` object stays in `.voxels`."""

    levels = (Voxels,)
