"""
`MatchTransitions`: the reader of `voxel_matches`, the per-frame-pair coordinates of every best voxel pair that `VoxelReassigner`
writes.  It is the reference's scripts/voxel_reassignment_demo.py as a product, on the MI355X HIP engine: both ends of every match
are mapped to a label of their frame, the label pairs are counted, and the counts say which label of frame t each label of frame
t + 1 comes from -- a source that feeds two destinations has split (fission), a destination fed by two sources has merged (fusion).

The counts of a pair are an (E, 3) int64 table of (src, dst, count) rows in lexicographic order, the sparse form of the demo's
(n_src, n_dst) matrix; `dense`, `best_src`, `best_dst` and `events` are made from it on the host (it is small).  The gather, the
counting and the relabelled frame run on the device (csrc/transitions.inc; DESIGN.md section 26, which also lists what is out of
scope).  Deliberate difference: a label of frame t + 1 without any counted pair is relabelled 0; the demo's argmax over an all-zero
column paints it with label 1.  There is no CPU engine behind this module (`device="cpu"` raises).
"""
from __future__ import annotations

import os
import pickle

import numpy as np

from nellie_amd.stage import FrameCounted, frame_count, require_gpu, resolve_device
from nellie_amd.tracking.voxel_reassignment import select_match_coord_dtype
from nellie_amd.utils.base_logger import logger

LEVELS = {"organelle": "im_instance_label", "branch": "im_skel_relabelled"}


def _rows(table):
    return np.asarray(table, dtype=np.int64).reshape(-1, 3)


def dense(table, n_src, n_dst):
    """the demo's matrix: uint32 (n_src, n_dst) with M[src - 1, dst - 1] = count"""
    table = _rows(table)
    n_src, n_dst = int(n_src), int(n_dst)
    if len(table) and (table[:, 0].max() > n_src or table[:, 1].max() > n_dst):
        raise ValueError(f"the table holds labels up to ({int(table[:, 0].max())}, {int(table[:, 1].max())}), above n_src = {n_src} or n_dst = {n_dst}")
    M = np.zeros((n_src, n_dst), np.uint32)
    M[table[:, 0] - 1, table[:, 1] - 1] = table[:, 2]
    return M


def _best(table, key, other):
    table = _rows(table)
    order = np.lexsort((table[:, other], -table[:, 2], table[:, key]))       # per key: largest count first, then the smallest label
    t = table[order]
    first = np.ones(len(t), bool)
    first[1:] = t[1:, key] != t[:-1, key]
    return np.ascontiguousarray(t[first][:, [key, other]])


def best_src(table):
    """(K, 2) int64 rows (dst, src), ascending in dst: per destination label of the table the source with the largest count, the
    smallest source on a tie (np.argmax's first occurrence over ascending sources, as in the demo)"""
    return _best(table, 1, 0)


def best_dst(table):
    """(K, 2) int64 rows (src, dst), ascending in src: the same rule the other way round"""
    return _best(table, 0, 1)


def events(table, min_count=1):
    """An edge counts when count >= min_count.  -> {"fission_src": the sources with two or more such edges, "fission": their edges
    (src, dst, count), ascending in (src, dst); "fusion_dst": the destinations with two or more, "fusion": their edges, ascending
    in (dst, src)}, all int64."""
    table = _rows(table)
    edges = table[table[:, 2] >= int(min_count)]
    src, n_out = np.unique(edges[:, 0], return_counts=True)
    dst, n_in = np.unique(edges[:, 1], return_counts=True)
    fis, fus = src[n_out >= 2], dst[n_in >= 2]
    fusion = edges[np.isin(edges[:, 1], fus)]
    return {"fission_src": fis, "fission": edges[np.isin(edges[:, 0], fis)], "fusion_dst": fus,
            "fusion": fusion[np.lexsort((fusion[:, 0], fusion[:, 1]))]}


def transition_counts(prev, next, labels_prev, labels_next, device_index=0):
    """One frame pair without files: `prev` / `next` (n, D) coordinates of the matches in frame t / t + 1, the two label frames
    (int32 or int64, the same 2-D or 3-D shape) -> ((E, 3) int64 table, n_dropped: the rows with a label of 0 at either end)."""
    from nellie_amd import hipnative
    a, b = np.asarray(labels_prev), np.asarray(labels_next)
    if a.shape != b.shape:
        raise ValueError(f"label frames of shapes {a.shape} and {b.shape}")
    require_gpu()
    with hipnative.Transitions(a.shape, device=device_index) as tr:
        tr.frame(a)
        tr.frame(b)
        return tr.count(prev, next)


class MatchTransitions(FrameCounted):
    def __init__(self, im_info, level="organelle", num_t=None, device="auto", device_index=0, min_count=1, label_path=None):
        if level not in LEVELS:
            raise ValueError(f"level must be one of {sorted(LEVELS)}, got {level!r}")
        self.im_info = im_info
        self.level = level
        self.device_type = resolve_device(device)
        self.device = device or "auto"
        self.device_index = int(device_index)
        self.min_count = int(min_count)
        self.label_path = label_path
        self.num_t = 1 if im_info.no_t else frame_count(im_info, num_t)
        self.label_memmap = None
        self.matches = None
        self.spatial_shape = None
        self.n_dropped = {}                                    # t -> dropped rows of the pair t -> t + 1
        self.kernel_ms = {}                                    # t -> device time per part of the pair's last count / relabel
        self.transitions_path = None
        self._tr = None
        self._resident = None                                  # (frame in "prev", frame in "next")
        self._last = None                                      # (t, table) of the last pair

    # ---- files and device ----------------------------------------------------------------------------------------------------------
    @property
    def uploads(self):
        """label frames uploaded so far"""
        return 0 if self._tr is None else self._tr.frames

    def _open(self):
        if self._tr is not None:
            return
        if self.im_info.no_t:
            raise ValueError("label transitions need a T axis")
        require_gpu()
        from nellie_amd import hipnative
        paths = self.im_info.pipeline_paths
        matches_path = paths["voxel_matches"]
        if not os.path.exists(matches_path):
            raise FileNotFoundError(f"MatchTransitions needs {matches_path}: run VoxelReassigner (store_running_matches=True) first")
        self.label_path = self.label_path or paths[LEVELS[self.level]]
        self.label_memmap = self.im_info.get_memmap(self.label_path)
        want = tuple(self.im_info.shape)
        if tuple(self.label_memmap.shape) != want:
            raise ValueError(f"label stack {self.label_path} has shape {tuple(self.label_memmap.shape)}, the image {want}")
        self.spatial_shape = tuple(self.label_memmap.shape[1:])
        self.matches = np.load(matches_path, allow_pickle=True)
        self._tr = hipnative.Transitions(self.spatial_shape, device=self.device_index)

    @property
    def n_pairs(self):
        """the stored pairs within num_t frames: the reassigner stops at an empty frame, so there may be fewer than T - 1"""
        self._open()
        return max(0, min(len(self.matches), self.num_t - 1))

    def _ends(self, t):
        dtype = select_match_coord_dtype(self.spatial_shape)
        D = len(self.spatial_shape)
        ends = []
        for a in (self.matches[t][0], self.matches[t][1]):
            a = np.asarray(a)
            if a.dtype == object:                              # equally long pairs are saved as one object array of numbers
                a = a.astype(dtype)
            ends.append(a.reshape(-1, D))
        return ends

    def close(self):
        tr, self._tr = self._tr, None
        if tr is not None:
            tr.close()
        self._resident = self._last = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- one pair ------------------------------------------------------------------------------------------------------------------
    def _frames(self, t):
        """frames t and t + 1 on the device; the later frame of the pair before stays there as this pair's earlier one"""
        if self._resident == (t, t + 1):
            return
        shared = self._resident is not None and self._resident[1] == t
        self._resident = None                                  # an upload that fails leaves nothing to build on: both go up next time
        if not shared:
            self._tr.frame(np.asarray(self.label_memmap[t]))
        self._tr.frame(np.asarray(self.label_memmap[t + 1]))
        self._resident = (t, t + 1)

    def pair(self, t):
        """the (E, 3) int64 table (src, dst, count) of t -> t + 1; its dropped rows in n_dropped[t]"""
        self._open()
        t = int(t)
        if not 0 <= t < self.n_pairs:
            raise ValueError(f"no stored pair {t} -> {t + 1}: voxel_matches holds {self.n_pairs} pairs within {self.num_t} frames")
        if self._last is not None and self._last[0] == t:
            return self._last[1]
        prev, next = self._ends(t)
        self._frames(t)
        table, dropped = self._tr.count(prev, next)
        self.n_dropped[t] = dropped
        self.kernel_ms[t] = self._tr.kernel_ms_parts()
        self._last = (t, table)
        return table

    def relabel(self, t, out=None):
        """frame t + 1 with every voxel of label b > 0 replaced by best_src[b] (0 where b has no counted pair), int32; `out` may be
        a memmap of the frame's shape"""
        table = self.pair(t)
        self._frames(t)
        top = self._tr.label_max()
        if top > 2 ** 31 - 1:
            raise ValueError(f"frame {t + 1} holds label {top}, above 2^31 - 1")
        lut = np.zeros(max(top + 1, 0), np.int32)
        best = best_src(table)
        lut[best[:, 0]] = best[:, 1]
        out = self._tr.relabel(lut, out=out)
        self.kernel_ms[t] = self._tr.kernel_ms_parts()
        return out

    def events(self, t):
        return events(self.pair(t), self.min_count)

    def dense(self, t, n_src, n_dst):
        return dense(self.pair(t), n_src, n_dst)

    # ---- every stored pair -----------------------------------------------------------------------------------------------------------
    def run(self):
        if self.im_info.no_t:
            logger.info("Skipping label transitions for non-temporal dataset.")
            return
        require_gpu()
        logger.info("Counting label transitions (HIP).")
        try:
            self._open()
            pairs = [self.pair(t) for t in range(self.n_pairs)]
            self.transitions_path = self.im_info.create_output_path("label_transitions", ext=".pkl")
            with open(self.transitions_path, "wb") as f:
                pickle.dump({"level": self.level, "label_path": self.label_path, "min_count": self.min_count, "pairs": pairs,
                             "n_dropped": [self.n_dropped[t] for t in range(len(pairs))]}, f)
        finally:
            self.close()
