"""
`HuMomentTracking`: drop-in for nellie.tracking.hu_tracking.HuMomentTracking (reference hu_tracking.py:35-1282) on the MI355X
HIP engine -- marker features (coordinates, intensity / Frangi stats, log-Hu moments of the ROI projections) per frame and the
match of every frame against the one before, written as `flow_vector_array` rows [t-1, (z0,) y0, x0, (vz,) vy, vx, cost].

Same constructor keywords, same `.run()`, same file.  Matching runs dense (the cost matrix of _get_cost_matrix, float16 costs)
or sparse (candidates within max_distance_um, float64 costs), chosen as the reference does (`mode`, `max_dense_pairs`).
Differences (documented in DESIGN.md): `max_dense_roi_voxels_cpu` / `max_dense_roi_voxels_gpu` / `low_memory` are accepted and
ignored -- the features are always those of the reference's dense ROI path; there is no CPU engine behind this class
(`device="cpu"` raises).
"""
from __future__ import annotations

import numpy as np

from nellie_amd.stage import frame_count, require_gpu, resolve_device, scaled_max_distance, spacing_of
from nellie_amd.utils.base_logger import logger


def frame_vectors(t, coords_post, coords_pre, rows, cols, costs):
    """the frame pair's rows of flow_vector_array (hu_tracking.py:1186-1222)"""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    pre, post = coords_pre[cols], coords_post[rows]
    vec = post - pre
    return np.column_stack([np.full(len(rows), t - 1, np.int64), *pre.T.astype(np.int64), *vec.T.astype(np.int64),
                            np.asarray(costs, np.float32)])


def candidates(row_idx, row_cost, col_idx, col_cost, dense):
    """row-based candidates first, column-based after them (hu_tracking.py:919-941 dense, 1081-1093 sparse)"""
    if dense:
        rk = np.nonzero(~(row_cost > 1.0))[0]
        ck = np.nonzero(~(col_cost > 1.0))[0]
    else:
        rk = np.nonzero((row_idx >= 0) & (row_cost <= 1.0))[0]
        ck = np.nonzero((col_idx >= 0) & (col_cost <= 1.0))[0]
    rows = np.concatenate([rk, col_idx[ck].astype(np.int64)])
    cols = np.concatenate([row_idx[rk].astype(np.int64), ck])
    costs = np.concatenate([row_cost[rk], col_cost[ck]]).astype(np.float32)
    return rows, cols, costs


class HuMomentTracking:
    def __init__(self, im_info, num_t=None, max_distance_um=1.0, viewer=None, device="auto", mode="auto",
                 max_dense_pairs=int(1e7), max_dense_roi_voxels_cpu=int(5e7), max_dense_roi_voxels_gpu=int(2e7),
                 low_memory=False, device_index: int = 0):
        self.im_info = im_info
        self.device_type = resolve_device(device)
        if mode not in ("auto", "dense", "sparse"):
            raise ValueError(f"Unsupported mode '{mode}'. Use 'auto', 'dense' or 'sparse'.")
        self.device = device or "auto"
        self.device_index = int(device_index)
        self.viewer = viewer
        self.mode = mode
        self.max_dense_pairs = int(max_dense_pairs)
        self.max_dense_roi_voxels_cpu = int(max_dense_roi_voxels_cpu)     # accepted, ignored (module docstring)
        self.max_dense_roi_voxels_gpu = int(max_dense_roi_voxels_gpu)
        self.low_memory = bool(low_memory)
        self.num_t = num_t
        self.flow_vector_array_path = None
        if self.im_info.no_t:
            return
        self.num_t = frame_count(im_info, num_t)
        self.scaling = spacing_of(im_info)
        self.max_distance_um = scaled_max_distance(im_info, max_distance_um)
        require_gpu()

    def _allocate_memory(self):
        paths = self.im_info.pipeline_paths
        self.im_memmap = self.im_info.get_memmap(self.im_info.im_path)
        self.im_frangi_memmap = self.im_info.get_memmap(paths["im_preprocessed"])
        self.im_marker_memmap = self.im_info.get_memmap(paths["im_marker"])
        self.im_distance_memmap = self.im_info.get_memmap(paths["im_distance"])
        self.flow_vector_array_path = paths["flow_vector_array"]

    def _use_dense(self, n_post, n_pre):
        return self.mode == "dense" or (self.mode == "auto" and n_post * n_pre <= self.max_dense_pairs)

    def _run_hu_tracking(self):
        from nellie_amd import hipnative
        frame_shape = tuple(self.im_marker_memmap.shape[1:])
        out = []
        with hipnative.Tracker(frame_shape, self.scaling, device=self.device_index) as trk:
            coords_prev = None
            for t in range(self.num_t):
                if self.viewer is not None:
                    self.viewer.status = f"Tracking markers. Frame: {t + 1} of {self.num_t}."
                im = np.asarray(self.im_memmap[t])
                if im.dtype not in (np.uint8, np.uint16, np.float32):
                    raise ValueError(f"tracking intensities must be uint8, uint16 or float32, not {im.dtype}")
                trk.frame(im, self.im_frangi_memmap[t], self.im_distance_memmap[t], self.im_marker_memmap[t])
                coords = trk.features(0)[0]
                n_post, n_pre = trk.n
                if t > 0 and n_post and n_pre:
                    dense = self._use_dense(n_post, n_pre)
                    ri, rc, ci, cc = trk.match("dense" if dense else "sparse", self.max_distance_um)
                    rows, cols, costs = candidates(ri, rc, ci, cc, dense)
                    if len(rows):
                        out.append(frame_vectors(t, coords, coords_prev, rows, cols, costs))
                coords_prev = coords
        if out:
            return np.concatenate(out, axis=0)
        return np.empty((0, 6 if self.im_info.no_z else 8), np.float32)

    def run(self):
        if self.im_info.no_t:
            logger.info("Skipping Hu moment tracking for non-temporal dataset.")
            return
        logger.info("Running Hu-moment tracking (HIP).")
        self._allocate_memory()
        flow = self._run_hu_tracking()
        np.save(self.flow_vector_array_path, flow)
        logger.debug(f"Saved flow vector array to {self.flow_vector_array_path}")
