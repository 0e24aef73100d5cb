"""
`LabelTracks`: drop-in for nellie.tracking.all_tracks_for_label.LabelTracks (reference all_tracks_for_label.py:13-156 over
flow_interpolation.py:317-426) on the MI355X HIP engine.  Every labelled voxel of a frame, or every `skip_coords`-th one, follows
the interpolated flow forward to the last frame and backward to frame 0; a track point that does not land on a labelled voxel of
its frame is dropped; what is left are napari's track rows [id, frame, (z,) y, x].

Same constructor and `run()` keywords, same return values, and `run_arrays()` for the same rows as one float64 array.  The seeds
are made on the device, the coordinates never leave it, and the surviving rows come down once.  The 1-bit
masks of the frames stay on the device across `run()` calls of one object, at most `max_masks` of them, least recently used out
first.  Differences: the backward rows are in the stable order (id, then frame ascending) where the reference's `np.argsort`
leaves ties to chance, and a row with a NaN or infinite coordinate is dropped where the reference raises; the two differences of
flow interpolation (section 11) are inherited.  There is no CPU engine behind this class: without a GPU `initialize()` raises.
"""
from __future__ import annotations

from collections import OrderedDict

import numpy as np

from nellie_amd.stage import Held, require_gpu, shape_key
from nellie_amd.utils import adaptive_run
from nellie_amd.utils.base_logger import logger

MASK_HBM_SHARE = 0.25        # of the free HBM: what the resident frame masks may take by default


class LabelTracks:
    def __init__(self, im_info, num_t=None, label_im_path=None, device_index: int = 0, max_masks=None):
        self.im_info = im_info
        if "T" not in im_info.axes:
            raise ValueError(f"LabelTracks follows voxels through time: the stack has axes '{im_info.axes}', without T")
        self.num_t = num_t
        if label_im_path is None:
            label_im_path = self.im_info.pipeline_paths["im_instance_label"]
        self.label_im_path = label_im_path
        if num_t is None:
            self.num_t = im_info.shape[im_info.axes.index("T")]
        self.device_index = int(device_index)
        self.max_masks = max_masks                               # None: as many as fit MASK_HBM_SHARE of the free HBM, all T at most
        self.im_memmap = None
        self.label_memmap = None
        self.kernel_ms = {}                                      # device time per part of the last run
        self._tracks = Held()                                    # hipnative.LabelTrackSet for (frame shape, mask slots)
        self._masks = OrderedDict()                              # frame -> slot, least recently used first
        self._free_slots, self._n_slots = [], 0                  # slots of the track set that hold no frame; how many it has
        self._interpolators = {}                                 # (forward, max_distance_um) -> (FlowInterpolator, its time points)

    def initialize(self):
        require_gpu()
        self.label_memmap = self.im_info.get_memmap(self.label_im_path)
        self.im_memmap = self.im_info.get_memmap(self.im_info.im_path)
        self._drop_masks()

    def close(self):
        for fi, _ in self._interpolators.values():
            fi.close()
        self._interpolators = {}
        self._n_slots = 0
        self._drop_masks()
        self._tracks.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- device state --------------------------------------------------------------------------------------------------------------
    def _drop_masks(self):
        self._masks.clear()
        self._free_slots = list(range(self._n_slots))[::-1]

    def _mask_slots(self):
        """how many frame masks stay resident"""
        frames = max(1, int(self.label_memmap.shape[0]))
        if self.max_masks is not None:
            return max(1, min(int(self.max_masks), frames))
        free = adaptive_run.get_gpu_free_bytes(self.device_index)
        if free is None:
            return frames
        mask_bytes = (int(np.prod(self.label_memmap.shape[1:], dtype=np.int64)) + 255) // 256 * 32
        return max(1, min(frames, int(free * MASK_HBM_SHARE) // mask_bytes))

    def _track_set(self):
        from nellie_amd import hipnative
        shape, slots = shape_key(self.label_memmap.shape[1:]), self._mask_slots()

        def make():
            self._n_slots = 0
            self._drop_masks()
            made = hipnative.LabelTrackSet(shape, mask_slots=slots, device=self.device_index)
            self._n_slots = slots
            self._drop_masks()
            return made
        return self._tracks.get((shape, slots), make)

    def _take_slot(self):
        if self._free_slots:
            return self._free_slots.pop()
        return self._masks.popitem(last=False)[1]

    def _mask_slot(self, ts, t):
        """the slot with frame t's mask, built when it is not resident"""
        if t in self._masks:
            self._masks.move_to_end(t)
            return self._masks[t]
        slot = self._take_slot()
        try:
            ts.mask(slot, self.label_memmap[t])
        except Exception:
            self._free_slots.append(slot)
            raise
        self._masks[t] = slot
        return slot

    def _seed(self, ts, t, label, skip):
        if label is None and t in self._masks:
            self._masks.move_to_end(t)
            return ts.seed(self._masks[t], skip=skip)
        slot = self._masks.pop(t) if t in self._masks else self._take_slot()
        try:
            n = ts.seed(slot, labels=self.label_memmap[t], label=label, skip=skip)       # also the frame's mask
        except Exception:
            self._free_slots.append(slot)
            raise
        self._masks[t] = slot
        return n

    def _interpolator(self, forward, max_distance_um):
        """one FlowInterpolator per direction and reach, kept until close(), and the time points its flow file has rows for"""
        key = (bool(forward), float(max_distance_um))
        if key not in self._interpolators:
            from nellie_amd.tracking.flow_interpolation import FlowInterpolator
            fi = FlowInterpolator(self.im_info, forward=forward, max_distance_um=max_distance_um, device_index=self.device_index)
            times = np.unique(fi.flow_vector_array[:, 0])
            self._interpolators[key] = (fi, {int(v) for v in times[np.isfinite(times)].tolist() if v == int(v)})
        return self._interpolators[key]

    # ---- the run -------------------------------------------------------------------------------------------------------------------
    def _run(self, label_num, start_frame, end_frame, min_track_num, skip_coords, max_distance_um):
        """(rows, frame_num, whether a direction ran)"""
        if self.label_memmap is None:
            raise RuntimeError("LabelTracks.run needs initialize() first")
        D = self.label_memmap.ndim - 1
        empty = np.zeros((0, 2 + D)), np.zeros(0, np.int64)
        start_frame, skip = int(start_frame), int(skip_coords)
        if start_frame < 0 or skip < 1:
            raise ValueError("start_frame must not be negative and skip_coords must be at least 1")
        if end_frame is None:
            end_frame = self.num_t
        end_frame = int(end_frame)
        n_frames = int(self.label_memmap.shape[0])
        if start_frame > n_frames - 1:
            return (*empty, False)
        label = None
        if label_num is not None:
            if label_num != int(label_num) or not -2 ** 31 <= int(label_num) < 2 ** 31:
                return (*empty, False)                            # no voxel of an int32 frame equals it
            label = int(label_num)
        ts = self._track_set()
        n = self._seed(ts, start_frame, label, min(skip, 2 ** 31 - 1))
        if n == 0:
            return (*empty, False)
        run_fw, run_bw = start_frame < end_frame, start_frame > 0
        if not (run_fw or run_bw):
            return (*empty, False)
        # the frames of each direction whose flow rows exist: only they can move a coordinate or emit a row
        plan = []
        for forward, frames in ((False, range(start_frame, -1, -1) if run_bw else ()), (True, range(start_frame, end_frame) if run_fw else ())):
            if not frames or self.im_info.no_t:
                plan.append((forward, None, []))
                continue
            fi, times = self._interpolator(forward, max_distance_um)
            if forward:
                have = [t for t in times if start_frame <= t < end_frame]
            else:
                have = [t + 1 for t in times if 0 <= t + 1 <= start_frame]
            plan.append((forward, fi, sorted((int(t) for t in have), reverse=not forward)))
        steps_bw, steps_fw = len(plan[0][2]), len(plan[1][2])
        self._check_rows_fit(n, D, steps_fw, steps_bw)
        try:
            ts.begin(steps_fw, steps_bw, int(min_track_num))
        except MemoryError as e:
            raise MemoryError(f"{e}; track fewer voxels: raise skip_coords (now {skip})") from e
        frames_with_rows = set()
        for forward, fi, have in plan:
            if fi is None:
                continue
            if not have or have[0] != start_frame:
                ts.step(None, not forward, True, start_frame, start_frame + (1 if forward else -1))      # the direction starts from the seeds
            for t in have:
                to = t + 1 if forward else t - 1
                if ts.step(fi.device_field(t), not forward, t == start_frame, t, to):
                    frames_with_rows.add(to)
                    if t == start_frame:
                        frames_with_rows.add(t)
        for f in sorted(frames_with_rows):
            ts.filter(f, self._mask_slot(ts, f) if 0 <= f < n_frames else None)
        kept = ts.finish()
        rows = ts.fetch() if kept else empty[0]
        self.kernel_ms = ts.kernel_ms_parts()
        logger.debug(f"LabelTracks: {n} seeds from frame {start_frame}, {kept} track rows.")
        return rows, rows[:, 1].astype(np.int64), True

    def _check_rows_fit(self, n, D, steps_fw, steps_bw):
        """MemoryError before any work when the row buffers of n seeds cannot fit the free HBM"""
        rows = n * ((steps_fw + 1 if steps_fw else 0) + (steps_bw + 1 if steps_bw else 0))
        need = rows * (2 * (2 + D) * 8 + 12) + n * (3 * D * 8 + 10)
        free = adaptive_run.get_gpu_free_bytes(self.device_index)
        if rows >= 2 ** 31 or (free is not None and need > free):
            raise MemoryError(f"out of memory: {n} seeds over {steps_fw} + {steps_bw} frames are {rows} track rows ({need / 2 ** 30:.1f} GiB on "
                              f"the device" + (f", {free / 2 ** 30:.1f} GiB free" if free is not None else "") + "); track fewer voxels: raise skip_coords")

    def run_arrays(self, label_num=None, start_frame=0, end_frame=None, min_track_num=0, skip_coords=1, max_distance_um=0.5):
        """run() as arrays: (rows (n, 2 + D) float64 [id, frame, (z,) y, x], frame_num (n,) int64); napari's add_tracks takes
        `rows` as it is"""
        rows, frame_num, _ = self._run(label_num, start_frame, end_frame, min_track_num, skip_coords, max_distance_um)
        return rows, frame_num

    def run(self, label_num=None, start_frame=0, end_frame=None, min_track_num=0, skip_coords=1, max_distance_um=0.5):
        """(tracks, track_properties): rows [id, frame, (z,) y, x] and {'frame_num': [...]}; ([], {}) where the reference returns
        that: a start frame beyond the stack, no seed voxel, no direction to follow"""
        rows, frame_num, ran = self._run(label_num, start_frame, end_frame, min_track_num, skip_coords, max_distance_um)
        if not ran:
            return [], {}
        table = rows.astype(object)                               # Python floats; the two leading columns as Python ints
        table[:, 0] = rows[:, 0].astype(np.int64)
        table[:, 1] = frame_num
        return table.tolist(), {"frame_num": frame_num.tolist()}
