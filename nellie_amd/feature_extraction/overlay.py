"""
`FeatureOverlay`: the analysis panel's overlay (reference nellie_napari/nellie_analysis.py:955-1218) on the MI355X HIP engine.  A
column of one of the feature tables is painted onto the labelled voxels of every frame: a voxel column lands on its own voxel, a
node, branch or organelle column goes through the `adjacency_maps` pickle, and a voxel with several nodes shows their mean.

Per frame the device makes the 1-bit mask `label > 0`, ranks it (the voxel rows, in raster order), looks every row's group or
groups up in the column and streams the dense frame out once (csrc/overlay.inc).  The reference builds a
dense (groups x voxels) matrix per frame for this.  `overlay_values` and `overlay_frame` are the file-free core.

Differences from the reference, all deliberate (section 24.3): a stack without T is one frame and gives the frame's shape; a label
volume is defined where the value is NaN, negative or infinite (0); a negative group index, a negative label and a voxel row beyond
the frame raise ValueError; `align_branches=True` indexes the branch column by `label - 1`, which the reference's pickle means but
its panel does not do.  There is no CPU engine behind this class.
"""
from __future__ import annotations

import os
import pickle

import numpy as np

from nellie_amd.stage import Held, frame_count, require_gpu, shape_key

LEVELS = ("voxel", "node", "branch", "organelle")
TABLE_KEYS = {"voxel": "features_voxels", "node": "features_nodes", "branch": "features_branches", "organelle": "features_organelles"}
EDGE_KEYS = {"node": "v_n", "branch": "v_b", "organelle": "v_o"}
MAX_INDEX = 2 ** 31 - 2          # group indices and labels are ints on the device


# ---- host rules --------------------------------------------------------------------------------------------------------------------
def contrast_limits(values):
    """[min - 0.01 |min|, 98th percentile] of the finite values of a column, with the reference's fallbacks
    (nellie_analysis.py:1172-1187): no finite value gives [0, 1]; a minimum equal to the percentile moves the percentile up by
    0.01 |min|; a limit that came out NaN is replaced by the plain minimum / maximum."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    v = v[np.isfinite(v)]
    if len(v) == 0:
        return [0.0, 1.0]
    hi = float(np.nanpercentile(v, 98))
    lo = float(np.nanmin(v))
    lo = lo - abs(lo) * 0.01
    if np.isnan(lo):
        lo = float(np.nanmin(v))
    if lo == hi:
        hi = lo + abs(lo) * 0.01
    if np.isnan(hi):
        hi = float(np.nanmax(v))
    return [lo, hi]


def check_edges(edges, n_rows):
    """An edge list (E, 2) of (voxel row, group index) as int64, stably sorted by voxel row when it is not already non-decreasing
    there.  ValueError naming the first edge with a negative group index, a negative voxel row or a voxel row >= n_rows."""
    e = np.asarray(edges)
    if e.size == 0:
        return np.zeros((0, 2), np.int64)
    if e.ndim != 2 or e.shape[1] != 2:
        raise ValueError(f"an edge list is (E, 2), got shape {e.shape}")
    if e.dtype != np.int64:
        from nellie_amd.hipnative import _refuse_lossy_cast
        _refuse_lossy_cast(e, np.dtype(np.int64), "edges")
        e = e.astype(np.int64)
    for bad, what in ((e[:, 1] < 0, "a negative group index"), (e[:, 1] > MAX_INDEX, f"a group index above {MAX_INDEX}"),
                      (e[:, 0] < 0, "a negative voxel row"), (e[:, 0] >= n_rows, f"a voxel row beyond the frame's {n_rows}")):
        if bad.any():
            k = int(np.flatnonzero(bad)[0])
            raise ValueError(f"edge {k} ({int(e[k, 0])}, {int(e[k, 1])}) holds {what}")
    if (np.diff(e[:, 0]) < 0).any():
        e = e[np.argsort(e[:, 0], kind="stable")]
    return e


def edges_to_csr(edges, n_rows):
    """(offsets (n_rows + 1) int64, group indices int32) of a checked edge list"""
    off = np.zeros(n_rows + 1, np.int64)
    np.cumsum(np.bincount(edges[:, 0], minlength=n_rows), out=off[1:])
    return off, np.ascontiguousarray(edges[:, 1], dtype=np.int32)


def check_csr(offsets, idx, n_rows):
    off, val = np.asarray(offsets), np.asarray(idx)
    if off.shape != (n_rows + 1,) or val.ndim != 1 or (n_rows >= 0 and (int(off[0]) != 0 or int(off[-1]) != val.size)) or (np.diff(off) < 0).any():
        raise ValueError(f"a CSR over {n_rows} voxel rows has {n_rows + 1} offsets from 0, not decreasing, ending at the number of group indices")
    bad = (val < 0) | (val > MAX_INDEX)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        raise ValueError(f"entry {k} of the CSR holds group index {int(val[k])}, negative or above {MAX_INDEX}")
    return off.astype(np.int64, copy=False), val.astype(np.int32, copy=False)


def attr_vector(labels, values, n_groups, shift=0):
    """The column by group index (nellie_analysis.py:1138-1158): max(n_groups, max(labels - shift) + 1) entries, NaN where no table
    row has the index, and a repeated label keeps its last row.  ValueError naming the first row whose index is negative."""
    lab = np.asarray(labels)
    vals = np.asarray(values, dtype=np.float64)
    if lab.shape != vals.shape or lab.ndim != 1:
        raise ValueError(f"{lab.shape} labels for {vals.shape} values")
    if lab.dtype.kind == "f":
        lab = lab.astype(int)                                     # the reference's astype(int) of the table's float column
    idx = lab.astype(np.int64) - int(shift)
    bad = (idx < 0) | (idx > MAX_INDEX)
    if bad.any():
        k = int(np.flatnonzero(bad)[0])
        why = "a negative label" if lab[k] < 0 else f"below {shift}" if idx[k] < 0 else f"above {MAX_INDEX + int(shift)}"
        raise ValueError(f"table row {k} holds label {int(lab[k])}: {why}")
    vec = np.full(max(int(n_groups), int(idx.max()) + 1 if len(idx) else 0), np.nan)
    if len(idx):
        _, first_from_end = np.unique(idx[::-1], return_index=True)
        keep = len(idx) - 1 - first_from_end
        vec[idx[keep]] = vals[keep]
    return vec


# ---- the core ----------------------------------------------------------------------------------------------------------------------
class _Frame:
    """A label frame on the device (hipnative.Overlay) with the groups it was last given"""

    def __init__(self, handle, label_frame):
        self.handle = handle
        self.n_rows = handle.load(label_frame)
        self.n_groups = None                                       # None: no groups (the frame stays NaN at this level)

    def set_groups(self, edges_or_csr):
        V = self.n_rows
        self.n_groups = None
        if edges_or_csr is None or V == 0:
            return
        if isinstance(edges_or_csr, tuple):
            off, idx = check_csr(*edges_or_csr, V)
        else:
            e = check_edges(edges_or_csr, V)
            off, idx = edges_to_csr(e, V)
        if idx.size == 0:
            return
        counts = np.diff(off)
        if counts.max() <= 1:                                      # one group per row: no run to walk
            group = np.full(V, -1, np.int32)
            group[counts == 1] = idx
            self.handle.groups(group)
        else:
            self.handle.groups_csr(off, idx)
        self.n_groups = int(idx.max()) + 1

    def set_values(self, attr_vec, direct=False):
        V = self.n_rows
        a = np.asarray(attr_vec, dtype=np.float64).reshape(-1)
        if direct:
            self.handle.values_direct(a if len(a) == V else np.full(V, np.nan))
        elif self.n_groups is None or len(a) == 0:
            self.handle.values_direct(np.full(V, np.nan))
        else:
            if len(a) < self.n_groups:
                raise ValueError(f"a column of {len(a)} entries for group indices up to {self.n_groups - 1}")
            # np.sum's order over the reference's dense column: pairwise down a contiguous column -- the matrix is Fortran-ordered
            # when it got no padding or one row of it, or is one voxel wide -- and row by row otherwise
            self.handle.values(a, pairwise=len(a) <= self.n_groups + 1 or V == 1)


def _open(label_frame, device_index):
    from nellie_amd import hipnative
    require_gpu()
    return hipnative.Overlay(shape_key(np.shape(label_frame)), device=device_index)


def overlay_values(label_frame, level_edges_or_csr, attr_vec, device_index: int = 0):
    """The per-voxel result (V,) float64 for the voxels with label > 0 of a 2-D or 3-D label frame, in raster order.
    `level_edges_or_csr`: an (E, 2) edge list of (voxel row, group index), a CSR pair (offsets, group indices), or None: the voxel
    level, where `attr_vec` holds the V values themselves (another length leaves the frame NaN).  Otherwise `attr_vec` is the column
    by group index (`attr_vector`), and a row's value is the mean over its distinct groups with a value that is not NaN."""
    with _open(label_frame, device_index) as handle:
        f = _Frame(handle, label_frame)
        f.set_groups(level_edges_or_csr)
        f.set_values(attr_vec, direct=level_edges_or_csr is None)
        return handle.fetch_values()


def overlay_frame(label_frame, level_edges_or_csr, attr_vec, dtype=np.float64, out=None, device_index: int = 0):
    """The dense frame of `overlay_values`: float64 or float32 (rounded once) with NaN off the labelled voxels, or uint64 labels (the
    truncated value; 0 where it is NaN, negative or infinite, and off the labelled voxels)."""
    with _open(label_frame, device_index) as handle:
        f = _Frame(handle, label_frame)
        f.set_groups(level_edges_or_csr)
        f.set_values(attr_vec, direct=level_edges_or_csr is None)
        handle.paint(dtype)
        return _fetch(handle, out)


def _fetch(handle, out):
    if out is None or (isinstance(out, np.ndarray) and type(out) is np.ndarray and out.flags.c_contiguous and out.flags.writeable and out.dtype == handle.painted):
        return handle.fetch_frame(out)
    if out.shape != handle.shape or out.dtype != handle.painted:
        raise ValueError(f"out must be a {handle.painted} array of shape {handle.shape}")
    out[...] = handle.fetch_frame()                                # a memmap or a strided view is filled from a landing array
    return out


# ---- from an ImInfo's files ----------------------------------------------------------------------------------------------------------
class FeatureOverlay:
    def __init__(self, im_info, device_index: int = 0, align_branches: bool = False, hierarchy=None):
        self.im_info = im_info
        self.device_index = int(device_index)
        self.align_branches = bool(align_branches)
        self.hierarchy = hierarchy                                  # its voxels.node_labels_csr serves the node level without the pickle
        self.num_t = frame_count(im_info)
        self.kernel_ms = {}                                         # device time per part of the last frame
        self._tables, self._maps, self._label_stack = {}, None, None
        self._held = Held()                                         # hipnative.Overlay for the frame shape
        self._state = None                                          # (t, level, _Frame): what is resident

    def close(self):
        self._state = None
        self._held.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # ---- files, each read once and when first needed ---------------------------------------------------------------------------------
    def _path(self, key):
        path = self.im_info.pipeline_paths[key]
        if not os.path.exists(path):
            raise FileNotFoundError(f"{key} not found: {path}")
        return path

    def _table(self, level):
        if level not in LEVELS:
            raise ValueError(f"no level '{level}': the overlay paints {', '.join(LEVELS)}")
        if level not in self._tables:
            import pandas as pd
            # round_trip: the values the table states; pandas' default parser is up to an ulp off a third of them
            self._tables[level] = pd.read_csv(self._path(TABLE_KEYS[level]), float_precision="round_trip")
        return self._tables[level]

    def _edges(self, level, t):
        """the frame's edge list or CSR, None when the level has none there"""
        if level == "node":
            csr = getattr(getattr(self.hierarchy, "voxels", None), "node_labels_csr", None)
            if csr is not None and len(csr) > t:
                return tuple(np.asarray(a) for a in csr[t])
        if self._maps is None:
            with open(self._path("adjacency_maps"), "rb") as f:
                self._maps = pickle.load(f)
        frames = self._maps.get(EDGE_KEYS[level])
        if frames is None or t >= len(frames) or frames[t] is None or np.size(frames[t]) == 0:
            return None
        return frames[t]

    def _labels(self):
        if self._label_stack is None:
            stack = self.im_info.get_memmap(self._path("im_instance_label"))
            self._label_stack = stack[None] if self.im_info.no_t else stack
        return self._label_stack

    @property
    def levels(self):
        return LEVELS

    def columns(self, level):
        """the columns of the level's table that can be painted"""
        return [c for c in self._table(level).columns if c not in ("t", "label")]

    def _column(self, level, column):
        df = self._table(level)
        if column not in df.columns:
            raise KeyError(f"the {level} table has no column '{column}'")
        return df

    def contrast_limits(self, level, column):
        return contrast_limits(self._column(level, column)[column].to_numpy(dtype=np.float64))

    # ---- a frame -----------------------------------------------------------------------------------------------------------------------
    def _valued(self, level, column, t):
        """the resident frame t with the level's groups and the column's values on the device"""
        df = self._column(level, column)
        t = int(t)
        if not 0 <= t < self.num_t:
            raise IndexError(f"frame {t} of {self.num_t}")
        rows = df["t"].to_numpy() == t
        vals = df[column].to_numpy(dtype=np.float64)[rows]
        resident = self._state is not None and self._state[0] == t
        edges = None if level == "voxel" or (resident and self._state[1] == level) else self._edges(level, t)
        stack = self._labels()
        if self._state is None or self._state[0] != t:
            handle = self._held.get(shape_key(stack.shape[1:]), lambda: _open(stack[t], self.device_index))
            self._state = None
            self._state = (t, None, _Frame(handle, stack[t]))
        _, had, frame = self._state
        if level != "voxel" and had != level:
            self._state = (t, None, frame)
            frame.set_groups(edges)
            self._state = (t, level, frame)
        if level == "voxel":
            frame.set_values(vals, direct=True)
        elif len(vals) == 0 or frame.n_groups is None:
            frame.set_values(np.zeros(0))
        else:
            labels = df["label"].to_numpy()[rows]
            frame.set_values(attr_vector(labels, vals, frame.n_groups, shift=1 if level == "branch" and self.align_branches else 0))
        return frame.handle

    def _done(self, handle):
        self.kernel_ms = handle.kernel_ms_parts()

    def values(self, level, column, t):
        """(V,) float64: the value of every voxel with label > 0 of frame t, in raster order"""
        handle = self._valued(level, column, t)
        out = handle.fetch_values()
        self._done(handle)
        return out

    def frame(self, level, column, t, out=None, dtype=np.float64):
        """the dense frame ((Z,) Y, X), NaN off the labelled voxels; float32: the float64 result rounded once"""
        if np.dtype(dtype) not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise TypeError("an overlay frame is float64 or float32; labels() gives the uint64 volume")
        return self._frame(level, column, t, out, dtype)

    def _frame(self, level, column, t, out, dtype):
        handle = self._valued(level, column, t)
        handle.paint(dtype)
        got = _fetch(handle, out)
        self._done(handle)
        return got

    def _stack(self, level, column, out, dtype):
        self._column(level, column)
        shape = tuple(self._labels().shape[1:])
        if self.im_info.no_t:
            return self._frame(level, column, 0, out, dtype)
        if out is None:
            out = np.empty((self.num_t,) + shape, dtype)
        if out.shape != (self.num_t,) + shape or out.dtype != np.dtype(dtype):
            raise ValueError(f"out must be a {np.dtype(dtype)} array of shape {(self.num_t,) + shape}")
        for t in range(self.num_t):
            self._frame(level, column, t, out[t], dtype)
        return out

    def run(self, level, column, out=None, dtype=np.float64):
        """the (T, ...) stack, filled frame by frame (`out` may be a memmap); a stack without T gives its one frame"""
        if np.dtype(dtype) not in (np.dtype(np.float64), np.dtype(np.float32)):
            raise TypeError("an overlay stack is float64 or float32; labels() gives the uint64 volume")
        return self._stack(level, column, out, dtype)

    def labels(self, level, column, t=None, out=None):
        """the column as a uint64 label volume (the reference's `reassigned_label` case, nellie_analysis.py:1189-1192): the truncated
        value, 0 where it is NaN, negative or infinite and off the labelled voxels; frame t, or the whole stack"""
        if t is None:
            return self._stack(level, column, out, np.uint64)
        return self._frame(level, column, t, out, np.uint64)
