"""
`FlowInterpolator`: drop-in for nellie.tracking.flow_interpolation.FlowInterpolator (reference flow_interpolation.py:14-314) on
the MI355X HIP engine, and the track helpers `interpolate_all_forward` / `interpolate_all_backward` (:317-426).

For a time point t the rows of `flow_vector_array` with column 0 == t (forward) or t - 1 (backward) are the check rows; a query
coordinate takes the cost- and distance-weighted mean of the vectors of the check rows within `max_distance_um` (at least
0.5 um) of it, NaN when there is none.  The rows of a t stay on the device while t does not change.

Deliberate differences: a NaN query row gives a NaN row and disturbs no other row, and a call in which no
query has more than one neighbour fills every row (the reference loses rows in both situations).  There is no CPU engine
behind this class: without a GPU the constructor raises.
"""
from __future__ import annotations

import numpy as np

from nellie_amd.stage import FrameCounted, frame_count, require_gpu, scaled_max_distance, spacing_of
from nellie_amd.utils.base_logger import logger


class FlowInterpolator(FrameCounted):
    def __init__(self, im_info, num_t=None, max_distance_um=0.5, forward=True, device_index: int = 0):
        self.im_info = im_info
        if self.im_info.no_t:
            return
        self.num_t = frame_count(im_info, num_t)
        self.scaling = spacing_of(im_info)
        self.max_distance_um = np.float64(scaled_max_distance(im_info, max_distance_um))     # (the reference's is numpy's)
        self.forward = forward
        self.device_index = int(device_index)
        self.shape = ()
        self.im_memmap = None
        self.flow_vector_array = None
        # the rows of the time point that is on the device
        self.current_t = None
        self.check_rows = None
        self.check_coords = None
        self.debug = None
        self._field = None
        require_gpu()
        self._initialize()

    def _allocate_memory(self):
        logger.debug("Allocating memory for flow interpolation.")
        self.im_memmap = self.im_info.get_memmap(self.im_info.im_path)
        self.shape = self.im_memmap.shape
        self.flow_vector_array = np.load(self.im_info.pipeline_paths["flow_vector_array"])

    def _initialize(self):
        if self.im_info.no_t:
            return
        self._get_t()
        self._allocate_memory()

    def close(self):
        if getattr(self, "_field", None) is not None:
            self._field.close()
            self._field = None

    def _load_t(self, t):
        """selects the check rows of t (flow_interpolation.py:277-292) and puts them on the device"""
        from nellie_amd import hipnative
        nd = len(self.scaling)
        flow = self.flow_vector_array
        self.check_rows = flow[np.where(flow[:, 0] == (t if self.forward else t - 1))[0], :]
        if self.forward:
            self.check_coords = self.check_rows[:, 1:1 + nd]
        else:
            self.check_coords = self.check_rows[:, 1:1 + nd] + self.check_rows[:, 1 + nd:1 + 2 * nd]
        if self._field is None:
            self._field = hipnative.FlowField(nd, self.scaling, float(self.max_distance_um), device=self.device_index)
        self._field.load(self.check_coords, self.check_rows[:, 1 + nd:1 + 2 * nd], self.check_rows[:, -1])
        self.current_t = t

    def device_field(self, t):
        """the device field (hipnative.FlowField) with the rows of time point t loaded, None when t has no rows: for stages that
        interpolate at coordinates which are already on the device (VoxelReassigner)"""
        if self.current_t != t:
            self._load_t(t)
        return self._field if len(self.check_rows) else None

    def interpolate_coord(self, coords, t):
        """flow vectors (n, D) at coords (n, D) for time point t; NaN rows where no flow row is in reach; shape (0, D) when no
        row of the call found one (flow_interpolation.py:165-170)"""
        nd = len(self.scaling)
        if self.current_t != t:
            self._load_t(t)
        q = np.asarray(coords, dtype=np.float64).reshape(-1, nd)
        if len(q) == 0 or len(self.check_rows) == 0:
            return np.zeros((0, nd))
        out, found = self._field.interpolate(q)
        if found == 0:
            return np.zeros((0, nd))
        return out


def _tracks(ids, frame, coords):
    return [[i, frame, *c] for i, c in zip(ids, coords.tolist())]


def interpolate_all_forward(coords, start_t, end_t, im_info, min_track_num=0, max_distance_um=0.5):
    """flow_interpolation.py:317-370: follows coords from start_t to end_t; coords is updated in place (NaN once a track is
    lost).  Returns (tracks, {'frame_num': [...]}) in the reference's order: per frame the coordinates in order, at the first
    frame each one's start entry before its next one."""
    flow_interpx = FlowInterpolator(im_info, forward=True, max_distance_um=max_distance_um)
    tracks, frame_num = [], []
    frame_range = np.arange(start_t, end_t)
    try:
        for t in frame_range:
            final_vector = flow_interpx.interpolate_coord(coords, t)
            if final_vector is None or len(final_vector) == 0:
                continue
            lost = np.all(np.isnan(final_vector), axis=1)
            keep = np.nonzero(~lost)[0]
            ids = (keep + min_track_num).tolist()
            before = coords[keep].copy()
            coords[lost] = np.nan
            coords[keep] = before + final_vector[keep]
            after = _tracks(ids, t + 1, coords[keep])
            if t == frame_range[0]:
                first = _tracks(ids, frame_range[0], before)
                tracks.extend(row for pair in zip(first, after) for row in pair)
                frame_num.extend([frame_range[0], t + 1] * len(keep))
            else:
                tracks.extend(after)
                frame_num.extend([t + 1] * len(keep))
    finally:
        flow_interpx.close()
    return tracks, {"frame_num": frame_num}


def interpolate_all_backward(coords, start_t, end_t, im_info, min_track_num=0, max_distance_um=0.5):
    """flow_interpolation.py:373-426: follows coords from start_t back to end_t; see interpolate_all_forward."""
    flow_interpx = FlowInterpolator(im_info, forward=False, max_distance_um=max_distance_um)
    tracks, frame_num = [], []
    frame_range = list(np.arange(end_t, start_t + 1))[::-1]
    try:
        for t in frame_range:
            final_vector = flow_interpx.interpolate_coord(coords, t)
            if final_vector is None or len(final_vector) == 0:
                continue
            lost = np.all(np.isnan(final_vector), axis=1)
            keep = np.nonzero(~lost)[0]
            ids = (keep + min_track_num).tolist()
            before = coords[keep].copy()
            coords[lost] = np.nan
            coords[keep] = before - final_vector[keep]
            after = _tracks(ids, t - 1, coords[keep])
            if t == frame_range[0]:
                first = _tracks(ids, frame_range[0], before)
                tracks.extend(row for pair in zip(first, after) for row in pair)
                frame_num.extend([frame_range[0], t - 1] * len(keep))
            else:
                tracks.extend(after)
                frame_num.extend([t - 1] * len(keep))
    finally:
        flow_interpx.close()
    return tracks, {"frame_num": frame_num}
