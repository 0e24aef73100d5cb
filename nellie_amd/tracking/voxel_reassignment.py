"""
`VoxelReassigner`: drop-in for nellie.tracking.voxel_reassignment.VoxelReassigner (reference voxel_reassignment.py:26-1112) on the
MI355X HIP engine.  For every frame pair the labelled voxels (branch > 0 | obj > 0) of both frames follow the interpolated flow
forward and backward, each predicted centroid takes the nearest labelled voxel of the other frame within `max_distance_um`, and
every voxel of the later frame takes, per label type, the label with the largest sum of 1 / (d + 1e-6) over its candidates.
Writes `im_branch_label_reassigned`, `im_obj_label_reassigned` and, with `store_running_matches`, `voxel_matches`.

Same constructor keywords, same `.run()`, same files.  A label frame is uploaded once and stays on the device as "prev" of the
next pair; the predicted centroids never leave it; the reassigned labels of the labelled voxels (and the best pairs) come back.
Differences: a tie of the nearest-voxel step goes to the voxel with the lowest raveled index (cKDTree's
choice is an accident of its tree); `max_refine_iterations` is accepted and one pass runs (a second never finds an unassigned
target); `low_memory`, `max_query_points` and `max_bruteforce_pairs` are accepted and ignored; there is no CPU engine behind this
class (`device="cpu"` raises).
"""
from __future__ import annotations

import numpy as np

from nellie_amd.stage import FrameCounted, flush, frame_count, require_gpu, resolve_device
from nellie_amd.utils.base_logger import logger


def select_match_coord_dtype(spatial_shape):
    """the narrowest of uint16 / uint32 / uint64 that holds every coordinate of a frame of this shape (what the reference stores
    running_matches in)"""
    longest = max((int(n) for n in spatial_shape), default=0) if spatial_shape is not None else 0
    for dtype, bits in ((np.uint16, 16), (np.uint32, 32)):
        if longest <= 2 ** bits:
            return dtype
    return np.uint64


class VoxelReassigner(FrameCounted):
    def __init__(self, im_info, num_t=None, viewer=None, store_running_matches: bool = True, max_refine_iterations: int = 3,
                 device: str = "auto", low_memory: bool = False, max_query_points: int = int(1e6),
                 max_bruteforce_pairs: int = int(1e7), device_index: int = 0):
        self.im_info = im_info
        self.device_type = resolve_device(device)
        self.device = device or "auto"
        self.device_index = int(device_index)
        self.low_memory = bool(low_memory)                       # accepted, ignored (module docstring)
        self.max_query_points = max(1, int(max_query_points))
        self.max_bruteforce_pairs = max(1, int(max_bruteforce_pairs))
        self.viewer = viewer
        self.store_running_matches = store_running_matches
        self.max_refine_iterations = max_refine_iterations
        self.flow_interpolator_fw = None
        self.flow_interpolator_bw = None
        self.running_matches = []
        self.voxel_matches_path = None
        self.branch_label_memmap = None
        self.obj_label_memmap = None
        self.reassigned_branch_memmap = None
        self.reassigned_obj_memmap = None
        self.debug = None
        self.shape = None
        self.spatial_shape = None
        self.match_coord_dtype = None
        self.kernel_ms = []                                      # device time per frame pair of the last run
        self._reassigner = None
        self.num_t = 1 if self.im_info.no_t else frame_count(im_info, num_t)

    def _select_match_coord_dtype(self):
        return select_match_coord_dtype(self.spatial_shape)

    def _allocate_memory(self):
        """voxel_reassignment.py:859-887"""
        logger.debug("Allocating memory for voxel reassignment.")
        paths = self.im_info.pipeline_paths
        self.voxel_matches_path = paths["voxel_matches"]
        self.branch_label_memmap = self.im_info.get_memmap(paths["im_skel_relabelled"])
        self.obj_label_memmap = self.im_info.get_memmap(paths["im_instance_label"])
        self.shape = self.branch_label_memmap.shape
        self.spatial_shape = self.shape[1:]
        self.match_coord_dtype = self._select_match_coord_dtype()
        self.reassigned_branch_memmap = self.im_info.allocate_memory(
            paths["im_branch_label_reassigned"], dtype="int32", description="branch label reassigned", return_memmap=True)
        self.reassigned_obj_memmap = self.im_info.allocate_memory(
            paths["im_obj_label_reassigned"], dtype="int32", description="object label reassigned", return_memmap=True)

    def close(self):
        for name in ("flow_interpolator_fw", "flow_interpolator_bw", "_reassigner"):
            obj = getattr(self, name, None)
            if obj is not None and hasattr(obj, "close"):
                obj.close()
        self._reassigner = None

    def _write_frame(self, t, vox, re_branch, re_obj):
        """the reassigned labels of frame t's labelled voxels into the two files (the rest of a frame stays 0)"""
        for memmap, lab in ((self.reassigned_branch_memmap, re_branch), (self.reassigned_obj_memmap, re_obj)):
            on = lab > 0
            if on.any():
                memmap[t][np.unravel_index(vox[on], self.spatial_shape)] = lab[on]

    def _run_reassignment(self):
        from nellie_amd import hipnative
        from nellie_amd.tracking.flow_interpolation import FlowInterpolator
        self._get_t()
        self._allocate_memory()
        self.close()
        self.flow_interpolator_fw = FlowInterpolator(self.im_info, device_index=self.device_index)
        self.flow_interpolator_bw = FlowInterpolator(self.im_info, forward=False, device_index=self.device_index)
        fw, bw = self.flow_interpolator_fw, self.flow_interpolator_bw
        self.running_matches = []
        self.kernel_ms = []
        match_dtype = self.match_coord_dtype or np.uint16
        self._reassigner = hipnative.Reassigner(self.spatial_shape, fw.scaling, float(fw.max_distance_um), device=self.device_index)
        ra = self._reassigner
        n_prev = ra.frame(self.branch_label_memmap[0], self.obj_label_memmap[0], seed=True)
        vox_prev, re_b, re_o, _ = ra.fetch(0)
        self._write_frame(0, vox_prev, re_b, re_o)
        for t in range(self.num_t - 1):
            if self.viewer is not None:
                self.viewer.status = f"Reassigning voxels. Frame: {t + 1} of {self.num_t}."
            logger.info(f"Reassigning pixels between frames {t} and {t + 1}")
            n_next = ra.frame(self.branch_label_memmap[t + 1], self.obj_label_memmap[t + 1])
            if n_prev == 0 or n_next == 0:
                logger.info(f"No voxels to match between frames {t} and {t + 1}; stopping.")
                break
            n_cand = ra.pair(fw.device_field(t), bw.device_field(t + 1))
            self.kernel_ms.append(ra.kernel_ms())
            if n_cand == 0:
                logger.info(f"No valid matches between frames {t} and {t + 1}; stopping.")
                break
            vox_next, re_b, re_o, best = ra.fetch(0, best=bool(self.store_running_matches))
            if self.store_running_matches:
                hit = np.nonzero(best >= 0)[0]
                best_prev = np.column_stack(np.unravel_index(vox_prev[best[hit]], self.spatial_shape))
                best_next = np.column_stack(np.unravel_index(vox_next[hit], self.spatial_shape))
                self.running_matches.append([best_prev.astype(match_dtype, copy=False), best_next.astype(match_dtype, copy=False)])
            self._write_frame(t + 1, vox_next, re_b, re_o)
            vox_prev, n_prev = vox_next, n_next
        flush(self.reassigned_branch_memmap, self.reassigned_obj_memmap)
        if self.store_running_matches and self.voxel_matches_path is not None:
            np.save(self.voxel_matches_path, np.array(self.running_matches, dtype=object))

    def run(self):
        if self.im_info.no_t:
            logger.info("Skipping voxel reassignment for non-temporal dataset.")
            return
        require_gpu()
        logger.info("Running voxel reassignment (HIP).")
        try:
            self._run_reassignment()
        finally:
            if self._reassigner is not None:
                self._reassigner.close()
                self._reassigner = None
