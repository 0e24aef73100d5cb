"""
Per-frame orchestration of the HIP engine: the host half of Nellie's Filter -> Label hot path.

The device does every full-volume pass (libnellie_hip.so, include/nellie_amd.h); the host
decides the data-dependent thresholds between passes exactly where the reference does
(nellie/segmentation/filtering.py:806-853, 952-967; labelling.py:385-455), from 256-bin
histograms / <= 1e6 samples the device hands back.  No array math on full volumes happens
here, and there is no CPU fallback: without the HIP library this module cannot run.

`FramePipeline` keeps one frame resident in HBM from upload to label download; the
`Filter` / `Label` stage classes (nellie_amd/segmentation) wrap it behind the reference's
stage API and on-disk layout.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import NamedTuple, Optional

import os

import numpy as np

from nellie_amd import hipnative
from nellie_amd.hipnative import FIELD_FRANGI, FIELD_FROB, FIELD_GAUSS, FIELD_VESSELNESS
from nellie_amd.utils.gpu_functions import (histogram_edges, min_triangle_otsu, otsu_threshold,
                                            triangle_threshold)

_EPS32 = float(np.finfo(np.float32).eps)
_TRUNCATE = 3.0


# ----------------------------------------------------------------------------- parameters
def z_ratio_of(dim_res) -> float:
    """filtering.py:75-78."""
    z_res = dim_res.get("Z") or dim_res.get("X") or 1.0
    x_res = dim_res.get("X") or 1.0
    return float(z_res) / float(x_res)


def spacing_of(dim_res):
    """filtering.py:265-275."""
    z = dim_res.get("Z") or dim_res.get("X") or 1.0
    y = dim_res.get("Y") or 1.0
    x = dim_res.get("X") or 1.0
    return (float(z), float(y), float(x))


def default_sigmas(dim_res, min_radius_um=0.25, max_radius_um=1.0):
    """filtering.py:88-89, 288-316."""
    min_radius_px = min_radius_um / dim_res["X"]
    max_radius_px = max_radius_um / dim_res["X"]
    min_sigma_step_size = 0.2
    num_sigma = 5
    sigma_1 = min_radius_px / 2.0
    sigma_2 = max_radius_px / 3.0
    sigma_min = min(sigma_1, sigma_2)
    sigma_max = max(sigma_1, sigma_2)
    if sigma_max <= sigma_min:
        sigma_max = sigma_min + min_sigma_step_size
    sigma_step_size_calculated = (sigma_max - sigma_min) / float(num_sigma)
    sigma_step_size = max(min_sigma_step_size, sigma_step_size_calculated)
    sigmas = list(np.arange(sigma_min, sigma_max, sigma_step_size, dtype=float))
    sigmas.sort()
    return sigmas


def sample_strides(shape, max_samples):
    """filtering.py:328-340."""
    if max_samples is None or max_samples <= 0:
        return (1,) * len(shape)
    total = int(np.prod(shape))
    if total <= max_samples:
        return (1,) * len(shape)
    ndim = len(shape)
    stride = int(np.ceil((total / max_samples) ** (1.0 / ndim)))
    strides = [max(1, stride) for _ in range(ndim)]
    while int(np.prod([int(np.ceil(s / st)) for s, st in zip(shape, strides)])) > max_samples:
        idx = int(np.argmax([s / st for s, st in zip(shape, strides)]))
        strides[idx] += 1
    return tuple(strides)


_WEIGHTS_CACHE = {}


def gaussian_weights(sigma: float):
    """
    scipy.ndimage `gaussian_filter1d` + `_gaussian_kernel1d` (order 0, truncate 3.0):
    lw = int(truncate*sd + 0.5); w = exp(-0.5/sd^2 * x^2) / sum.  None when the axis is
    skipped (scipy `gaussian_filter` skips sigma <= 1e-15).  Computed with numpy exactly as
    scipy does, so the float64 weights carry scipy's bits.  The (read-only) array of a sigma is kept: a stack's frames
    ask for the same fifteen kernels again and again, 70 us of numpy per frame with the GPU waiting for the first of them.
    """
    sd = float(sigma)
    if not sd > 1e-15:
        return None
    got = _WEIGHTS_CACHE.get(sd)
    if got is not None:
        return got
    lw = int(_TRUNCATE * sd + 0.5)
    sigma2 = sd * sd
    x = np.arange(-lw, lw + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    phi_x = phi_x / phi_x.sum()
    w = np.ascontiguousarray(phi_x[::-1])
    w.setflags(write=False)
    if len(_WEIGHTS_CACHE) < 4096:
        _WEIGHTS_CACHE[sd] = w
    return w


def gaussian_derivative_weights(sigma: float, order: int, truncate: float = 4.0):
    """scipy.ndimage `_gaussian_kernel1d(sigma, order, radius)` reversed as `gaussian_filter1d` does, radius =
    int(truncate*sd + 0.5) -- `gaussian_laplace` runs with scipy's default truncate = 4.0 (filtering.py:781)."""
    sd = float(sigma)
    radius = int(truncate * sd + 0.5)
    exponent_range = np.arange(order + 1)
    sigma2 = sd * sd
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    phi_x = phi_x / phi_x.sum()
    if order == 0:
        return np.ascontiguousarray(phi_x[::-1])
    q = np.zeros(order + 1)
    q[0] = 1
    D = np.diag(exponent_range[1:], 1)
    P = np.diag(np.ones(order) / -sigma2, -1)
    Q_deriv = D + P
    for _ in range(order):
        q = Q_deriv.dot(q)
    q = (x[:, None] ** exponent_range).dot(q)
    return np.ascontiguousarray((q * phi_x)[::-1])


def marker_sigmas(dim_res, min_radius_um=0.20, max_radius_um=1, num_sigma=5):
    """mocap_marking.py:121-134, 329-362: (sigmas, max_radius_px)."""
    x_res = dim_res.get("X") or 1.0
    min_r = max(min_radius_um, float(x_res)) / float(x_res)
    max_r = max_radius_um / float(x_res)
    sigma_min, sigma_max = min_r / 2.0, max_r / 3.0
    rng = sigma_max - sigma_min
    if rng <= 0:
        return [sigma_min], max_r
    step = max(0.2, rng / max(num_sigma, 1))
    sig = list(np.arange(sigma_min, sigma_max, step))
    return (sig if len(sig) else [sigma_min]), max_r


_DELTAS_CACHE = {}


def cascade_deltas(sigmas, z_ratio):
    """filtering.py:814-825 (kept per (sigmas, z_ratio): the same for every frame of a stack)."""
    key = (tuple(float(s) for s in sigmas), float(z_ratio))
    got = _DELTAS_CACHE.get(key)
    if got is None:
        got = _cascade_deltas(sigmas, z_ratio)
        if len(_DELTAS_CACHE) < 256:
            _DELTAS_CACHE[key] = got
    return list(got)


def _cascade_deltas(sigmas, z_ratio):
    out = []
    prev = 0.0
    for sigma in sigmas:
        vp = (float(prev) / z_ratio, float(prev), float(prev))
        vc = (float(sigma) / z_ratio, float(sigma), float(sigma))
        delta = []
        for sp, sc in zip(vp, vc):
            diff = max(0.0, float(sc) ** 2 - float(sp) ** 2)
            delta.append(np.sqrt(diff))
        out.append(tuple(delta))
        prev = sigma
    return out


def min_area_pixels_of(dim_res, min_radius_um=0.25, no_z=False):
    """labelling.py:95-97, 209-219."""
    x_res = dim_res.get("X") or 1.0
    y_res = dim_res.get("Y") or x_res
    r = max(float(min_radius_um), float(x_res))
    if no_z:
        area_px = (np.pi * (r ** 2)) / (float(x_res) * float(y_res))
        return max(1, int(np.ceil(area_px)))
    z_res = dim_res.get("Z") or x_res
    volume_um3 = (4.0 / 3.0) * np.pi * (r ** 3)
    volume_px = volume_um3 / (float(x_res) * float(y_res) * float(z_res))
    return max(1, int(np.ceil(volume_px)))


@dataclass
class FilterParams:
    dim_res: dict
    min_radius_um: float = 0.25
    max_radius_um: float = 1.0
    alpha_sq: float = 0.5
    beta_sq: float = 0.5
    frob_thresh: Optional[float] = None
    frob_thresh_division: object = 2
    max_threshold_samples: int = int(1e6)
    sigmas: Optional[list] = None

    def resolved_sigmas(self):
        if self.sigmas is not None:
            return list(self.sigmas)
        return default_sigmas(self.dim_res, self.min_radius_um, self.max_radius_um)


@dataclass
class ScaleTrace:
    sigma: float
    gamma: float
    max_abs: float
    frob_thr: Optional[float]
    mask_count: int
    skipped: bool
    one_pass: bool = False          # the scale needed a single walk over the Hessian (nl_vesselness_spec hit)


@dataclass
class FrameTrace:
    scales: list = field(default_factory=list)
    n_positive: int = 0
    percentile_thr: Optional[float] = None
    label_thr: Optional[float] = None
    n_labels: int = 0


# ----------------------------------------------------------------------------- the pipeline
def run_scale_schedule(n, order, step, walk, choose):
    """A frame of n scales inside three Gaussian volumes: step(k) runs cascade step k and its first sampling round (sigma order), walk(k)
    walks a sampled scale.  A volume is busy while its scale waits for the walk, and the newest one while a step still needs it as its
    source; steps run ahead while a volume is free.  The LAST step also wants its third volume dead (it pre-zeroes the label volume
    there), so it waits until only its own source is pending -- unless an explicit order asks for the last scale earlier.
    order: a permutation of range(n), or None: choose(pending, steps_left) picks.  False: the order does not fit (nothing run twice)."""
    pending, done, newest, pos = [], 0, None, 0
    while pos < n:
        busy = set(pending) | ({newest} if newest is not None else set())
        can_step = done < n and len(busy) <= 2
        want = order[pos] if order is not None else None
        if can_step and done == n - 1 and not set(pending) <= {newest}:
            can_step = want is not None and want not in pending
        if can_step:
            step(done)
            pending.append(done)
            newest = done
            done += 1
            continue
        if want is None:
            want = choose(list(pending), n - done)
        if want not in pending:
            return False
        walk(want)
        pending.remove(want)
        pos += 1
    return True


def scale_order_fits(order) -> bool:
    """Can the scales be walked in this order (a permutation of range(n)) inside three Gaussian volumes?"""
    return run_scale_schedule(len(order), list(order), lambda k: None, lambda k: None, None)


class FramePlan(NamedTuple):
    """What the scale loops of one frame share, worked out once per compute_vesselness call."""
    sigmas: tuple
    spacing: tuple
    strides: tuple           # of the threshold sample lattice (max_samples points at most)
    deltas: tuple            # cascade_deltas; an image's have no Z part: sigma_vec = (s, s) (filtering.py:281-282)
    alpha_sq: float
    beta_sq: float
    frob_thresh: Optional[float]
    division: object         # frob_thresh_division as given (0 / None: mask = frob > 0)
    max_samples: int


class ChainTail(NamedTuple):
    """What the scale loops left behind for filter()'s epilogue: nothing, the host samples of the tail field (gathered under the device
    chain's wait), or an epilogue that nl_tail_enqueue started and _finish_device_tail still has to finish or cancel."""
    samples: Optional[np.ndarray] = None
    pending: bool = False


class _DeferredMaskCount:
    """The h_mask count of a scale the one-pass walk completed: its resolve kernel overlaps the next scale's Gaussian, so the count is
    read (vesselness_count waits for the kernel) only when the next walk is about to start, or at the end of the frame."""

    def __init__(self, pipe):
        self.pipe, self.entry = pipe, None

    def defer(self, entry: ScaleTrace):
        self.entry = entry

    def settle(self):
        if self.entry is not None:
            self.entry.mask_count = self.pipe._reduce_mask_count(self.pipe.ctx.vesselness_count())
            self.entry = None


# entry points a context may lack (the reduced contexts of the CPU tests, older libraries): asked once per pipeline
_OPTIONAL_ENTRY_POINTS = ("one_pass_available", "sample_range_hist", "sample_range_hist2", "sample_gather_positive",
                          "flat_sample_gather_positive", "chain_begin", "chain_available", "chain_begin_unordered",
                          "sample_gather_positive_begin", "mask_volume_dev", "tail_enqueue", "gauss_commit", "mask_volume_fused")


class FramePipeline:
    """One (Z, Y, X) frame on one GPU, resident in HBM across Filter and Label."""

    def __init__(self, shape, device: int = 0, ctx=None):
        self.shape = tuple(int(s) for s in shape)      # the GLOBAL frame shape (thresholds sample its lattice)
        self.two_d = len(self.shape) == 2              # (Y, X) image, im_info.no_z: held as one plane
        if self.two_d:
            self.shape = (1,) + self.shape
        if len(self.shape) != 3:
            raise ValueError("FramePipeline takes a (Z, Y, X) or a (Y, X) shape")
        self.ctx = ctx if ctx is not None else hipnative.Context(self.shape, device=device)
        self._ctx_has = frozenset(name for name in _OPTIONAL_ENTRY_POINTS if hasattr(self.ctx, name))
        if self.two_d:
            self.ctx.set_ndim(2)
        self.trace = FrameTrace()
        # One walk over the Hessian per scale instead of two (statistics, then masks): the mask threshold is
        # predicted from the sample lattice and bracketed by a relative margin; a scale whose exact threshold
        # falls outside the bracket is redone the two-pass way, so results never depend on it.
        self.one_pass = "one_pass_available" in self._ctx_has and bool(self.ctx.one_pass_available()) and not self.two_d
        self.one_pass_margin = 1e-3
        # range + histogram of a threshold in one device round trip (a Z-slab pipeline reduces the range across ranks
        # between the two passes and keeps them apart)
        self._chain_hist = "sample_range_hist" in self._ctx_has and os.environ.get("NELLIE_CHAIN_HIST", "1") != "0"
        self._pair_hist = "sample_range_hist2" in self._ctx_has and os.environ.get("NELLIE_PAIR_HIST", "1") != "0"
        self.check_device_edges = os.environ.get("NELLIE_CHECK_EDGES", "0") == "1"
        self._one_pass_test_scale = 1.0      # tests: shifts the prediction to force a miss
        try:
            self._yx_max_r = int(self.ctx.info("gauss_yx_max_r"))
        except (KeyError, AttributeError):
            self._yx_max_r = 0

    def _step_fits_ahead(self, ws) -> bool:
        """nl_gauss_step_ahead takes steps that write at most two of the three ping-pong volumes (a Z pass and a fused Y+X pass):
        the third pass of a one-kernel-per-axis step lands in the volume the current scale still reads."""
        wz, wy, wx = ws
        n = 0 if wz is None else 1
        if wy is not None and wx is not None and len(wy) == len(wx) and 1 <= (len(wy) - 1) // 2 <= min(self._yx_max_r, self.shape[1]):
            n += 1
        else:
            n += (wy is not None) + (wx is not None)
        return n <= 2

    def close(self):
        self.ctx.close()

    def _strides(self, max_samples):
        """filtering.py:328-340 on the frame's own dimensionality (a 2-D image samples a 2-D lattice)."""
        if self.two_d:
            return (1,) + tuple(sample_strides(self.shape[1:], max_samples))
        return sample_strides(self.shape, max_samples)

    def _positive_lattice_samples(self, fld, strides):
        """arr[::sz, ::sy, ::sx][... > 0] of a device field (filtering.py:348-363), compacted on the device."""
        if "sample_gather_positive" in self._ctx_has:
            return self._gather(self.ctx.sample_gather_positive(fld, strides))
        sample = self._gather(self.ctx.sample_gather(fld, strides))
        return sample[sample > 0]

    def _positive_flat_samples(self, fld, offset, step):
        """flat[offset::step][... > 0] (labelling.py:418-433), compacted on the device."""
        if "flat_sample_gather_positive" in self._ctx_has:
            return self._gather(self.ctx.flat_sample_gather_positive(fld, offset, step))
        sample = self._gather(self.ctx.flat_sample_gather(fld, offset, step))
        return sample[sample > 0]

    def _as_frame(self, a):
        a = np.asarray(a)
        return a[None] if (self.two_d and a.ndim == 2) else a

    # ---- hooks a Z-slab pipeline overrides (nellie_amd/sharded.py); identity on a single GPU -------------
    def _after_load(self, p):
        pass

    def _gauss_range(self, rz):
        return 0, self.shape[0]

    def _after_cascade_step(self, k):
        pass

    def _vess_range(self):
        return -1, -1

    def _reduce_minmax(self, mn, mx, npos):
        return mn, mx, npos

    def _reduce_counts(self, counts):
        return counts

    def _reduce_stats(self, max_abs, max_fsq, any_inf, overflow=0, fused_call=False):
        return max_abs, max_fsq, any_inf, overflow

    def _reduce_sum(self, n):
        return n

    def _reduce_mask_count(self, n):
        """h_mask count of a scale the one-pass walk completed: reporting only (ScaleTrace), nothing downstream waits for it."""
        return self._reduce_sum(n)

    def _settle_mask_counts(self):
        """Called once the scale loop is over: Z slabs turn the per-rank counts kept so far into global ones here."""

    def _gather(self, samples):
        return samples

    def _reduce_fused_count(self, n):
        return self._reduce_sum(n)      # (a Z-slab pipeline with a fused communicator gets the global count from the call itself)

    # ------------------------------------------------------------------ Filter
    def load_input(self, frame):
        """Keep the raw frame resident in HBM; `filter(None, ...)` then starts from device memory."""
        self.ctx.input_load(self._as_frame(frame))

    def _load(self, frame):
        self.ctx.filter_load(self._as_frame(frame))

    def _restart_frame(self, frame, p: FilterParams):
        """A frame starts (again: the chain's fallback) from the frame handed over, or from the one load_input() keeps resident."""
        self.trace = FrameTrace()
        if frame is None:
            self.ctx.filter_begin()
        else:
            self._load(frame)
        self._after_load(p)

    def _frame_plan(self, p: FilterParams, max_samples: int) -> FramePlan:
        sigmas = p.resolved_sigmas()
        deltas = cascade_deltas(sigmas, z_ratio_of(p.dim_res))
        if self.two_d:
            deltas = [(0.0, d[1], d[2]) for d in deltas]          # sigma_vec = (s, s): no Z axis (filtering.py:281-282)
        return FramePlan(tuple(sigmas), spacing_of(p.dim_res), self._strides(max_samples), tuple(deltas), float(p.alpha_sq), float(p.beta_sq),
                         p.frob_thresh, p.frob_thresh_division, max_samples)

    # ---- the Gaussian cascade --------------------------------------------------------------------------------------------------------
    def _cascade_step(self, plan: FramePlan, k: int, ahead: bool) -> bool:
        """Cascade step k (filtering.py:814-835) -- ahead: on the side stream, where it becomes current at gauss_commit().  False: not
        run -- the step blurs nothing (all-zero delta), or it was asked to run ahead and writes all three volumes (_step_fits_ahead:
        it then runs in order at the top of the next scale)."""
        delta = plan.deltas[k]
        if not any(s > 0 for s in delta):
            return False
        ws = [gaussian_weights(d) for d in delta]
        if ahead and not self._step_fits_ahead(ws):
            return False
        z0, z1 = self._gauss_range(0 if ws[0] is None else (len(ws[0]) - 1) // 2)
        self.ctx.gauss_step(*ws, z0=z0, z1=z1, **({"ahead": True} if ahead else {}))
        return True

    def _next_gaussian(self, plan: FramePlan, k: int, ahead: bool, run_ahead: bool) -> bool:
        """Sigma order: the Gaussian of scale k becomes current (ahead: its step was enqueued during the previous scale), and with
        run_ahead step k+1 is enqueued at once -- it only reads the Gaussian of THIS scale, so on the side stream it runs beside this
        scale's sampling and Hessian walk (filtering.py:814-835 has no such dependency either).  -> is step k+1 ahead now?"""
        if ahead:
            self.ctx.gauss_commit()
        else:
            self._cascade_step(plan, k, False)
        self._after_cascade_step(k)      # Z slabs: the ghost planes the NEXT step needs start travelling now
        return bool(run_ahead and k + 1 < len(plan.sigmas) and self._cascade_step(plan, k + 1, True))

    # ---- thresholds from lattice samples ---------------------------------------------------------------------------------------------
    def _range_hist(self, fld, strides, pre=None, finite_only=False):
        """Range and 256-bin histogram of the positive lattice samples of a device field -> (mn, mx, npos, counts, edges); counts and
        edges are None without a positive sample.  One device round trip where nothing sits between the two passes (a single GPU, a
        fused communicator; pre: its result when it was fetched together with another field's): the device builds numpy's float32 edges
        itself and they serve the threshold arithmetic too (the GPU tests run with NELLIE_CHECK_EDGES=1: every such chain compares them
        with numpy's, bit for bit); a degenerate range goes through numpy on the host, which raises numpy's errors.  Otherwise two
        calls with the cross-rank reductions between them; finite_only: the caller drops a range that is not finite, so its histogram
        is not asked for."""
        if self._chain_hist:
            mn, mx, npos, counts, dev_edges, valid = pre if pre is not None else self.ctx.sample_range_hist(fld, strides, 256)
            if npos and valid == 1 and self.check_device_edges:
                assert np.array_equal(dev_edges, histogram_edges(mn, mx, 256)), "device-built histogram edges differ from numpy's"
            edges = dev_edges if (npos and valid == 1) else (histogram_edges(mn, mx, 256) if npos else None)
            return mn, mx, npos, counts, edges
        mn, mx, npos = self._reduce_minmax(*self.ctx.sample_minmax(fld, strides))
        if npos == 0 or (finite_only and not np.isfinite(mx)):
            return mn, mx, npos, None, None
        return (mn, mx, npos) + self._hist_in_range(fld, strides, mn, mx)

    def _hist_in_range(self, fld, strides, mn, mx):
        """-> (counts, edges) of the positive lattice samples over numpy's 256 bins of [mn, mx]."""
        edges = histogram_edges(mn, mx, 256)
        return self._reduce_counts(self.ctx.sample_hist(fld, strides, edges)), edges

    def _threshold_from_field(self, fld, strides, known_range=None, pre=None):
        """min(triangle, otsu) over the positive lattice samples of a device field, or None if none.
        known_range: their (min, max) where the caller has it already; pre: see _range_hist."""
        if known_range is not None:
            counts, edges = self._hist_in_range(fld, strides, known_range[0], known_range[1])
        else:
            _, _, npos, counts, edges = self._range_hist(fld, strides, pre)
            if npos == 0:
                return None
        return float(min_triangle_otsu(counts, edges))

    def _fsq_bracket(self, strides, division, pre=None):
        """Predicted [lo, hi] for the un-normalised frob_sq threshold of the current scale and the (min, max) of the raw samples it
        was predicted from -> (lo, hi, raw_range), or None.
        Normalising by 1 instead of the (unknown) global max |H| rescales samples and threshold alike
        (filtering.py:421-444), so the histogram threshold of sqrt(frob_sq) predicts sqrt(fsq_min) up to float32
        rounding -- unless the rounding moves the histogram argmax to another bin, which the bracket then misses."""
        if pre is None:
            self.ctx.set_frob_norm(1.0, 0.0)
        mn, mx, npos, counts, edges = self._range_hist(FIELD_FROB, strides, pre, finite_only=True)
        if npos == 0 or not np.isfinite(mx):
            return None
        t = float(min_triangle_otsu(counts, edges)) * self._one_pass_test_scale / division
        lo, hi = np.float32(t * t * (1.0 - self.one_pass_margin)), np.float32(t * t * (1.0 + self.one_pass_margin))
        if not (np.isfinite(lo) and np.isfinite(hi) and hi > 0):
            return None
        return float(lo), float(hi), (np.float32(mn), np.float32(mx))

    @staticmethod
    def _normalised_range(raw_range, max_abs):
        """(min, max) of the positive NL_FIELD_FROB samples for the exact normalisation, derived from the range the
        bracket round measured with max_abs := 1: x -> x / max_abs is monotone in float32, so min and max commute with
        it.  None (measure it) when something underflows to 0 or overflows."""
        with np.errstate(all="ignore"):
            mn, mx = raw_range[0] / np.float32(max_abs), raw_range[1] / np.float32(max_abs)
        return (mn, mx) if (mn > 0 and np.isfinite(mx)) else None

    # ---- the scales of a frame -------------------------------------------------------------------------------------------------------
    def compute_vesselness(self, frame, p: FilterParams, mask: bool = True, finish: bool = True):
        """filtering.py:806-853 + 926: leaves `vesselness * masks` on the device; returns #voxels > 0.
        finish=False stops before the product is materialised (see filter()); returns None then."""
        plan, _ = self._run_scales(frame, p, mask)
        return self._finish_frame(plan, mask) if finish else None

    def _run_scales(self, frame, p: FilterParams, mask: bool, tail_field=None):
        """Every scale of a frame (filtering.py:806-853), on the device-resident chain where it applies and the synchronous way where
        it does not, or where the chain met a condition it leaves to the host.  tail_field: the field whose percentile threshold the
        caller takes next (filter()); the chain then starts that epilogue under its own wait.  -> (plan, ChainTail)."""
        max_samples = int(p.max_threshold_samples) if p.max_threshold_samples is not None else 0
        if max_samples <= 0:
            raise ValueError("max_threshold_samples must be a positive integer")
        self._restart_frame(frame, p)
        plan = self._frame_plan(p, max_samples)
        tail = None
        if self._chain_usable(p, mask):
            tail = self._scales_on_the_device(plan, tail_field)
            if tail is None:
                # a condition the device-resident chain leaves to the host turned up: the frame is redone, synchronously
                self.chain_fallbacks += 1
                self._restart_frame(frame, p)
        if tail is None:
            self._scales_synchronously(plan, mask)
            tail = ChainTail()
        self._settle_mask_counts()
        return plan, tail

    def _scales_synchronously(self, plan: FramePlan, mask: bool):
        """The sigma loop with every threshold decided on the host, between the passes (one wait per decision)."""
        counts = _DeferredMaskCount(self)
        # Hessian statistics and vesselness candidates in ONE walk where the mask threshold can be bracketed beforehand
        want_bracket = bool(self.one_pass and mask and plan.division and plan.frob_thresh is None)
        ahead = False        # the cascade step of the current scale was enqueued during the previous one
        for k, sigma in enumerate(plan.sigmas):
            ahead = self._next_gaussian(plan, k, ahead, self._gauss_ahead)
            gamma, frob_pre = self._scale_gamma(plan, want_bracket)
            max_abs, max_frob, walked = self._scale_statistics(plan, want_bracket, frob_pre, counts)
            thr, thr_cmp, nonempty = self._scale_mask_threshold(plan, mask, max_abs, max_frob, walked)
            count, hit = 0, False
            if nonempty:                                         # filtering.py:843-844
                count, hit = self._scale_walk(plan, 2.0 * (float(gamma) ** 2), thr_cmp, walked is not None, counts)
            self.trace.scales.append(ScaleTrace(float(sigma), float(gamma), max_abs, thr, count, not nonempty, hit))
            if hit:
                counts.settle()
                counts.defer(self.trace.scales[-1])      # its kernel overlaps the next scale's Gaussian; count read later
        counts.settle()
        if not mask and not self.two_d:
            # filtering.py:581: with h_mask all ones EVERY Hessian goes to numpy.linalg.eigvalsh, and LAPACK gives up on a matrix with a
            # NaN entry -- the reference's run ends in LinAlgError("Eigenvalues did not converge") (pinned: tests/golden nomask_nan_*).
            # The device solves in closed form and would return 0 there; it reports such a voxel instead and the same exception is raised.
            if self._reduce_sum(int(self.ctx.info("nan_hessian"))):
                raise np.linalg.LinAlgError("Eigenvalues did not converge")

    def _scale_gamma(self, plan: FramePlan, want_bracket: bool):
        """gamma (filtering.py:365-380, 839-840) -> (gamma, the raw Frobenius round of the bracket when it came along, else None):
        the gamma samples and the raw Frobenius samples of the bracket need nothing from each other: one round trip."""
        ctx = self.ctx
        pair = None
        if want_bracket and self._chain_hist and self._pair_hist:
            ctx.set_spacing(plan.spacing)
            ctx.set_frob_norm(1.0, 0.0)
            pair = ctx.sample_range_hist2(FIELD_GAUSS, FIELD_FROB, plan.strides, 256)
        gamma = self._threshold_from_field(FIELD_GAUSS, plan.strides, pre=None if pair is None else pair[0])
        if gamma is None or gamma <= 0:
            gamma = _EPS32
        return gamma, (None if pair is None else pair[1])

    def _scale_statistics(self, plan: FramePlan, want_bracket: bool, frob_pre, counts: _DeferredMaskCount):
        """Hessian statistics (filtering.py:555-562) and the normalisation they set -- taken together with the vesselness candidates
        when the mask threshold can be bracketed beforehand (nl_vesselness_spec), by a pass of their own otherwise.
        -> (max_abs, max_frob, walked): walked is the raw sample range of the bracket round when the one-pass walk stands (neither
        a +inf frob_sq nor a queue overflow), None when the scale goes the two-pass way."""
        ctx = self.ctx
        stats, walked = None, None
        if want_bracket:
            if frob_pre is None:
                ctx.set_spacing(plan.spacing)
            bracket = self._fsq_bracket(plan.strides, float(plan.division), frob_pre)
            if bracket is not None:
                counts.settle()
                vz0, vz1 = self._vess_range()
                ma, mf, inf_, ovf = ctx.vesselness_spec(plan.spacing, bracket[0], bracket[1], z0=vz0, z1=vz1)
                stats = self._reduce_stats(ma, mf, inf_, ovf, fused_call=True)    # nl_vesselness_spec reduces them itself on a fused communicator
                if not stats[2] and not stats[3]:
                    walked = bracket[2]
                if stats[2]:
                    stats = None     # a +inf frob_sq turned up: the one-pass walk only flags it (the largest finite
                                     # value comes from the statistics pass below), and the scale goes the two-pass way
        if stats is None:
            stats = self._reduce_stats(*ctx.hessian_stats(plan.spacing))
        max_abs32, max_fsq32, any_inf = stats[:3]
        max_abs = float(max_abs32)
        if max_abs <= 0:
            max_abs = 1.0
        with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
            max_frob = np.sqrt(np.float32(max_fsq32)) / np.float32(max_abs)   # float32, as the volume op
        ctx.set_frob_norm(max_abs, float(max_frob) if any_inf else 0.0)
        return max_abs, max_frob, walked

    def _scale_mask_threshold(self, plan: FramePlan, mask: bool, max_abs, max_frob, walked):
        """h_mask's threshold -> (thr for the trace, thr_cmp as the walk compares it, is any voxel above it?)."""
        if not mask:
            return None, np.float32(-np.inf), True               # h_mask = ones_like(image) (filtering.py:566-567)
        if not plan.division:
            return None, None, bool(max_frob > 0)                # mask = frob > 0 (filtering.py:428-430)
        if plan.frob_thresh is None:
            known = None if walked is None else self._normalised_range(walked, max_abs)
            t = self._threshold_from_field(FIELD_FROB, plan.strides, known)
            thr = 0.0 if t is None else t                        # filtering.py:433-439
        else:
            thr = float(plan.frob_thresh)
        thr_cmp = np.float32(thr / plan.division)                # weak python scalar vs float32 array
        return thr, thr_cmp, bool(max_frob > thr_cmp)

    def _scale_walk(self, plan: FramePlan, gamma_sq, thr_cmp, walked: bool, counts: _DeferredMaskCount):
        """The vesselness of a scale -> (h_mask count, hit): the candidates of the one-pass walk resolved where the exact threshold fell
        inside the bracket (hit: the count comes later, _DeferredMaskCount), the two-pass walk otherwise."""
        if walked and self.ctx.vesselness_resolve(gamma_sq, plan.alpha_sq, plan.beta_sq, thr_cmp):
            return 0, True
        counts.settle()
        vz0, vz1 = self._vess_range()
        return self._reduce_sum(self.ctx.vesselness_step(gamma_sq, plan.alpha_sq, plan.beta_sq, thr_cmp, z0=vz0, z1=vz1)), False

    # Device-resident threshold chain (csrc/chain.inc): the scale loop without a host round trip; NELLIE_DEVICE_CHAIN=0: off
    _device_chain = os.environ.get("NELLIE_DEVICE_CHAIN", "1") == "1"
    chain_fallbacks = 0

    def _chain_usable(self, p: FilterParams, mask: bool) -> bool:
        return bool(self._device_chain and (self.one_pass or self.two_d) and mask and p.frob_thresh is None and p.frob_thresh_division
                    and "chain_begin" in self._ctx_has and ("chain_available" not in self._ctx_has or self.ctx.chain_available())
                    and self._chain_reductions_on_device())

    def _chain_reductions_on_device(self) -> bool:
        return True            # one GPU: nothing to reduce (a Z-slab pipeline needs its fused communicator)

    def _scales_on_the_device(self, plan: FramePlan, tail_field):
        """The sigma loop with every threshold decided on the device (nl_chain_*): kernels only, ONE wait at the end.
        -> ChainTail: the trace is filled and the frame stands; None: the caller redoes the frame synchronously."""
        if not 1 <= len(plan.sigmas) <= 16:
            return None
        order = self._scale_order(plan.deltas)            # None: sigma order
        if order is None:
            self._scales_in_sigma_order(plan)
        else:
            self._scales_out_of_order(plan, order)
        return self._chain_epilogue(plan, tail_field)

    # tests: {sigma index: factor on that scale's predicted threshold} -- a bracket miss in one scale of the chain
    _chain_test_scales = {}

    def _chain_test_scale(self, k):
        return self._chain_test_scales.get(k, self._one_pass_test_scale)

    def _scales_in_sigma_order(self, plan: FramePlan):
        ctx = self.ctx
        n = len(plan.sigmas)
        ctx.chain_begin(n)
        # No cascade step runs ahead here: that device (sharded.py) fills the GPU while the host waits for a scale's collectives,
        # and the chain has no such waits -- beside the walk the step only competes with it (measured on a 128 x 2048 x 2048 slab:
        # 34.1 ms/step with a step running ahead, 29.9 without; the synchronous path: 31.6 / 30.4).
        # ... except on frames that stream from the caches (below 2^26 voxels: a config-5 frame).  There a scale's threshold kernels --
        # one wave or a 10^6-point lattice each, ten of them per scale -- leave the GPU idle for 0.12 ms of every 0.5 ms, and the next
        # cascade step, enqueued on the side stream, fills those holes (round 5: 2.70 -> see profiles/r05_c5_chain_ahead.txt).
        run_ahead = self._chain_ahead(int(np.prod(self.shape))) and not self.two_d
        ahead = False
        # images: two passes per scale, the raw round's "bracket" decides nothing (margin 1: nl_chain_scale)
        margin = 1.0 if self.two_d else self.one_pass_margin
        for k in range(n):
            ahead = self._next_gaussian(plan, k, ahead, run_ahead)
            vz0, vz1 = self._vess_range()
            ctx.chain_scale(plan.spacing, plan.strides, plan.alpha_sq, plan.beta_sq, float(plan.division), margin,
                            self._chain_test_scale(k), z0=vz0, z1=vz1)

    # ---- scales walked out of sigma order (csrc/nellie_hip.hip: nl_chain_begin_unordered) --------------------------
    # NELLIE_SCALE_ORDER, read per frame: unset / "auto" = most selective pending mask first, "sigma" = sigma order, "3,2,1,4,5" = that
    # order (1-based sigma indices), refused if it does not fit three Gaussian volumes.  Whole 3-D frames on one context whose cascade
    # steps are all fused; every other frame keeps sigma order.
    _scale_reorder_ok = True             # (a Z-slab pipeline: no)
    last_scale_order = None              # tests / tools: the walk order of the last frame (0-based), None in sigma order
    _all_steps_fused = {}

    def _scale_order(self, deltas):
        """None: sigma order.  "auto", or a schedulable 0-based permutation."""
        self.last_scale_order = None
        env = os.environ.get("NELLIE_SCALE_ORDER", "auto").strip().lower() or "auto"
        if env == "sigma" or not self._scale_reorder_ok or self.two_d or "chain_begin_unordered" not in self._ctx_has:
            return None
        if self._chain_ahead(int(np.prod(self.shape))):
            return None                  # (small frames: the next cascade step runs beside the walk, on the two free volumes)
        key = (tuple(deltas), os.environ.get("NELLIE_GAUSS_FUSED"))
        if key not in self._all_steps_fused:          # (asked once per cascade: the frame's first kernel waits for this function)
            self._all_steps_fused = {key: all(all(s > 0 for s in d) and self.ctx.gauss_step_fused(*[gaussian_weights(s) for s in d])
                                              for d in deltas)}
        if not self._all_steps_fused[key]:
            return None
        if env == "auto":
            return "auto"
        n = len(deltas)
        try:
            order = [int(t) - 1 for t in env.split(",")]
        except ValueError:
            raise ValueError(f"NELLIE_SCALE_ORDER={env!r}: expected auto, sigma or a permutation such as 3,2,1,4,5") from None
        if sorted(order) != list(range(n)):
            raise ValueError(f"NELLIE_SCALE_ORDER={env!r} is not a permutation of the frame's {n} scales (1..{n})")
        if not scale_order_fits(order):
            raise ValueError(f"NELLIE_SCALE_ORDER={env!r} cannot be scheduled inside three Gaussian volumes: a scale's walk can be "
                             f"delayed by two cascade steps at most")
        return order

    def _scales_out_of_order(self, plan: FramePlan, order):
        ctx = self.ctx
        n = len(plan.sigmas)
        ctx.chain_begin_unordered(n)
        division = float(plan.division)
        est = {}
        walked = []

        def step(k):                     # (always fused, every delta positive: _scale_order -- so never refused, never ahead)
            self._cascade_step(plan, k, False)
            ctx.chain_sample(k, plan.spacing, plan.strides, division, self.one_pass_margin, self._chain_test_scale(k))

        def walk(k):
            vz0, vz1 = self._vess_range()
            ctx.chain_walk(k, plan.spacing, plan.strides, plan.alpha_sq, plan.beta_sq, division, z0=vz0, z1=vz1)
            walked.append(k)

        def choose(pending, steps_left):
            # the smallest forecast mask fraction; ties and missing forecasts: sigma order.  A forecast costs one short wait, taken
            # only while a cascade step is still to come (the frame's last two walks are thin either way)
            if len(pending) > 1 and steps_left and any(k not in est for k in pending):
                for k, f in enumerate(ctx.chain_estimates()):
                    if f >= 0:
                        est[k] = float(f)
            if any(k not in est for k in pending):
                return min(pending)
            return min(pending, key=lambda k: (est[k], k))

        run_scale_schedule(n, None if order == "auto" else order, step, walk, choose)
        self.last_scale_order = walked

    def _chain_epilogue(self, plan: FramePlan, tail_field):
        """The chain's one wait -> ChainTail, or None when a scale raised a flag (the frame is redone)."""
        ctx = self.ctx
        # filter()'s percentile threshold reads lattice samples of the result: their compaction is enqueued BEFORE the wait, so it
        # runs while the host waits for the chain's records and repeats its decisions (one round trip less per frame)
        # Round 4: with the percentile selected on the device (nl_tail_enqueue) the WHOLE epilogue is enqueued before the wait -- the
        # host repeats the chain's decisions while the GPU masks the frame -- and no sample ever travels.
        dev_tail = tail_field is not None and self._device_tail_usable()
        tail = not dev_tail and self._tail_ok and tail_field is not None and "sample_gather_positive_begin" in self._ctx_has
        if dev_tail:
            ctx.chain_flush()
            ctx.tail_enqueue(plan.strides, 1.0)
        elif tail:
            ctx.chain_flush()
            ctx.sample_gather_positive_begin(tail_field, plan.strides)
        flags, gamma, max_abs, thr, counts = ctx.chain_finish()
        samples = ctx.sample_gather_positive_end() if tail else None
        self.last_chain_flags = [int(f) for f in flags]
        if not self._all_ranks_agree(not flags.any()):
            if dev_tail:
                self._finish_device_tail(commit=False)     # the frame is redone: what the epilogue computed from it is dropped
            return None
        if self.check_device_edges:
            for k in range(len(plan.sigmas)):
                for which in range(3):
                    _, edges, rng, _ = ctx.chain_log(k, which)
                    assert np.array_equal(edges, histogram_edges(rng[0], rng[1], 256)), "device-built histogram edges differ from numpy's"
        for k, sigma in enumerate(plan.sigmas):
            self.trace.scales.append(ScaleTrace(float(sigma), float(gamma[k]), float(max_abs[k]), float(thr[k]),
                                                self._reduce_mask_count(int(counts[k])), False, not self.two_d))
        return ChainTail(samples, dev_tail)

    def _all_ranks_agree(self, ok: bool) -> bool:
        return ok

    # NELLIE_CHAIN_AHEAD: unset = frames below 2^26 voxels on a single context; 0 / 1: never / always.  Read per frame (a test or
    # a tool that sets it after the import is heard); an instance attribute `_chain_ahead_env` overrides the environment.
    _chain_ahead_env = None

    def _chain_ahead(self, n_voxels: int) -> bool:
        env = self._chain_ahead_env if self._chain_ahead_env is not None else os.environ.get("NELLIE_CHAIN_AHEAD")
        if env is not None:
            return env == "1"
        return n_voxels < (1 << 26)

    def _finish_frame(self, plan: FramePlan, mask: bool):
        """The product `vesselness * masks` (filtering.py:926) once every scale is in."""
        ctx = self.ctx
        vz0, vz1 = self._vess_range()
        self.trace.n_positive = self._reduce_sum(ctx.filter_finish(vz0, vz1))
        if self.two_d:
            # filtering.py:927-930: blob response of the (by now fully blurred) frame, maximum with the vesselness
            for i, s in enumerate(plan.sigmas):
                w2, w0 = gaussian_derivative_weights(s, 2), gaussian_derivative_weights(s, 0)
                ctx.log2d_step(w2, w0, w2, w0, np.float32(float(s) ** 2), first=(i == 0), use_mask=mask)
            self.trace.n_positive = ctx.log2d_finish()
        return self.trace.n_positive

    def mask_volume(self, p: FilterParams):
        """filtering.py:952-967 on the device-resident frame."""
        strides = self._strides(int(p.max_threshold_samples))
        if self._device_percentile_usable():
            rec = self.ctx.mask_volume_dev(strides, 1.0)
            if rec["n_samples"] == 0:
                return None
            self._check_device_percentile(rec)
            self.trace.percentile_thr = float(rec["thr"])
            return rec["thr"]
        positive = self._positive_lattice_samples(FIELD_FRANGI, strides)
        if positive.size == 0:
            return None
        thr = percentile_of_samples(positive, 1)
        self.ctx.mask_volume(thr)
        self.trace.percentile_thr = float(thr)
        return thr

    # the device chain may gather the samples of the percentile threshold under its own wait (a single context: a slab pipeline
    # gathers them across ranks)
    _tail_ok = True
    _device_tail = os.environ.get("NELLIE_DEVICE_TAIL", "1") == "1"      # 0: the percentile threshold on the host (round 3)

    def _device_percentile_usable(self) -> bool:
        """The percentile selected on the device: needs the entry points and the host's repetition of numpy's interpolation to be
        the installed numpy's (percentile_of_samples checks that once per process)."""
        global _FAST_PERCENTILE
        if _FAST_PERCENTILE is None:
            percentile_of_samples(np.array([1.0, 2.0], np.float32), 1)
        return bool(self._device_tail and _FAST_PERCENTILE and "mask_volume_dev" in self._ctx_has and self._tail_reductions_on_device())

    def _device_tail_usable(self) -> bool:
        """... and the whole fused epilogue enqueued without a wait (nl_tail_enqueue): 3-D frames."""
        return bool(self._device_percentile_usable() and not self.two_d and "tail_enqueue" in self._ctx_has)

    def _check_device_percentile(self, rec):
        thr, gamma = percentile_from_order_statistics(rec["n_samples"], rec["a"], rec["b"], 1)
        if not (np.float32(thr) == rec["thr"] and np.float32(gamma) == rec["gamma"] and rec["a"] <= rec["b"]):
            raise RuntimeError(f"device percentile {rec} differs from numpy's rule ({thr}, {gamma})")

    def _tail_reductions_on_device(self) -> bool:
        return True            # one GPU: nothing to reduce (a Z-slab pipeline needs its fused communicator)

    def _finish_device_tail(self, commit: bool):
        """The one place an epilogue that nl_tail_enqueue started ends.  commit: waits for it, checks the device's interpolation
        against numpy's rule, fills the trace -> positive voxels, or None when there was no positive sample (the caller takes the
        plain path).  Not commit (the frame is redone, or no scale was evaluated): what it computed is dropped -> None."""
        rec = self.ctx.tail_finish(commit=commit)
        if not commit or rec["n_samples"] == 0:
            return None
        self._check_device_percentile(rec)
        self.trace.percentile_thr = float(rec["thr"])
        self.trace.n_positive = self._reduce_fused_count(rec["n_positive"])
        return self.trace.n_positive

    _fused_epilogue = True      # (a Z-slab pipeline on a context without nl_mask_volume_fused keeps the two-step epilogue)
    # Enqueue the cascade step of scale s+1 on the side stream beside the Hessian walk of scale s.  Exact either way.
    # Off by default: at 1024^3 it buys ~1 % (two full-GPU kernels mostly take turns) and it blurs per-kernel timings.
    _gauss_ahead = os.environ.get("NELLIE_GAUSS_AHEAD", "0") == "1"

    def filter(self, frame, p: FilterParams, mask: bool = True, remove_edges: bool = False):
        """filtering.py:1012-1018: _run_frame, then _mask_volume when the frame has signal.
        Common case in one go: the percentile threshold only needs lattice samples of `vesselness * masks`, which
        can be read through the mask bits, so the product is never written just to be thresholded and rewritten
        (nl_mask_volume_fused).  No positive sample, no evaluated scale, 2-D or a slab: the two plain steps."""
        if remove_edges:                     # filtering.py:931-932: between the product and _mask_volume
            self.compute_vesselness(frame, p, mask=mask)
            npos = self.trace.n_positive = self._reduce_sum(self.ctx.remove_edges(15))
            if npos > 0:
                self.mask_volume(p)
            return npos
        if not self._fused_epilogue or self.two_d:
            npos = self.compute_vesselness(frame, p, mask=mask)
        else:
            plan, tail = self._run_scales(frame, p, mask, FIELD_VESSELNESS if (self._tail_ok or self._device_tail_usable()) else None)
            evaluated = any(not sc.skipped for sc in self.trace.scales)
            positive = tail.samples
            if tail.pending or (evaluated and positive is None and self._device_tail_usable()):
                if not tail.pending:
                    self.ctx.tail_enqueue(plan.strides, 1.0)
                npos = self._finish_device_tail(commit=evaluated)       # (every scale skipped: nothing to commit)
                if npos is not None:
                    return npos
                positive = np.zeros(0, np.float32)              # no positive sample: the plain path below
            if evaluated:
                if positive is None:
                    positive = self._positive_lattice_samples(FIELD_VESSELNESS, plan.strides)
                if positive.size > 0:
                    thr = percentile_of_samples(positive, 1)
                    self.trace.percentile_thr = float(thr)
                    self.trace.n_positive = self._reduce_fused_count(self.ctx.mask_volume_fused(thr))
                    return self.trace.n_positive
            npos = self._finish_frame(plan, mask)
        if npos > 0:      # float(sum(frame)) > 0 for a non-negative frame
            self.mask_volume(p)
        return npos

    def download_frangi(self, out=None):
        return self.ctx.filter_store(out=out)

    # ------------------------------------------------------------------ Label
    def upload_frangi(self, frangi):
        self.ctx.label_load_frangi(self._as_frame(np.asarray(frangi, dtype=np.float32)))

    def frangi_threshold(self, max_samples=1_000_000, nbins=256):
        """labelling.py:385-455 on the device-resident Frangi frame (no mask arguments)."""
        n = int(np.prod(self.shape))
        if n == 0:
            return None
        max_samples = max(1, int(max_samples))
        step = max(n // max_samples, 1)
        offsets = (0, step // 2) if step > 1 and step // 2 > 0 else (0,)
        values = np.zeros(0, np.float32)
        found = False
        for offset in offsets:
            values = self._positive_flat_samples(FIELD_FRANGI, offset, step)
            if values.size > 0 or step == 1:
                found = True
                break
        if not found:
            full = self._gather(self.ctx.flat_sample_gather(FIELD_FRANGI, 0, 1))     # rare: every strided sample empty
            if full.size == 0 or float(full.max()) <= 0:
                values = values[:0]
            else:
                values = full[full > 0]
        if values.size == 0:
            return None
        return log10_min_triangle_otsu(values, nbins)

    def label(self, frangi_thresh, min_area, fill_holes=True):
        """labelling.py:467-509; returns the number of labels.  Labels stay on the device."""
        self.trace.label_thr = None if frangi_thresh is None else float(frangi_thresh)
        self.trace.n_labels = self.ctx.label_run(frangi_thresh, int(min_area), fill_holes)
        return self.trace.n_labels

    # ------------------------------------------------------------------ Markers (the stage after Label)
    def markers(self, dim_res, labels=None, intensity=None, min_radius_um=0.20, max_radius_um=1, num_sigma=5,
                peak_min_distance=2, use_image=None):
        """mocap_marking.py:648-703 on the device; returns the number of markers.  labels / intensity default to what
        Label and load_input left on the device.  use_image: the float32 image the LoG runs on (use_im='frangi',
        :675-679); None = the distance image (use_im='distance').  2-D pipelines follow the reference's `no_z`
        branch (sigma_vec = (s, s), :323-324).  Products: download_markers()."""
        sigmas, max_r_px = marker_sigmas(dim_res, min_radius_um, max_radius_um, num_sigma)
        ctx = self.ctx
        ctx.markers_begin(None if labels is None else self._as_frame(labels), None if intensity is None else self._as_frame(intensity))
        n_mask = ctx.markers_distance(np.float32(max_r_px * 2.0))
        if n_mask > 0:                                  # empty mask: no markers, zero distance and border (:662-667)
            if use_image is not None:
                ctx.markers_use_image(self._as_frame(use_image))
            zr = None if self.two_d else z_ratio_of(dim_res)
            for s in sigmas:
                sv = float(s)
                w2, w0 = gaussian_derivative_weights(sv, 2), gaussian_derivative_weights(sv, 0)
                if self.two_d:
                    ctx.markers_log_step(None, None, w2, w0, w2, w0, np.float32(sv ** 2))
                else:
                    wz2, wz0 = gaussian_derivative_weights(sv / zr, 2), gaussian_derivative_weights(sv / zr, 0)
                    ctx.markers_log_step(wz2, wz0, w2, w0, w2, w0, np.float32(sv ** 2))
        return ctx.markers_finish(int(peak_min_distance))

    def download_markers(self):
        """(marker uint8, distance float32, border uint8)."""
        return self.ctx.markers_store()

    def download_labels(self, out=None):
        return self.ctx.label_store(out=out)


_FAST_PERCENTILE = None     # None: not checked yet; True / False: the shortcut below reproduces this numpy's np.percentile / does not


def _percentile_shortcut(values, q):
    """np.percentile(values, q) (method 'linear') of a 1-D float32 array without NaN, as numpy >= 2.0 evaluates it for float32
    input -- q / float32(100), virtual index (n - 1) * q in float32, _lerp in float32 -- with ONE selection instead of numpy's
    four-point partition plus its wrappers (0.4 ms on 3 * 10^4 samples, during which the GPU waits; filtering.py:957-962)."""
    n = values.size
    qf = np.true_divide(q, np.float32(100))
    vi = (n - 1) * qf
    if vi >= n - 1:
        lo = hi = n - 1
    else:
        lo = int(np.floor(vi))
        hi = lo + 1
    gamma = np.float32(np.float64(vi) - lo)
    part = np.partition(values, lo)
    a = part[lo]
    b = part[lo + 1:].min() if hi != lo else a          # the next order statistic: the smallest of what lies above the pivot
    diff = b - a
    if gamma >= 0.5:
        return b - diff * (1 - gamma)
    return a + diff * gamma


def percentile_from_order_statistics(n, a, b, q):
    """np.percentile of n float32 values whose order statistics at floor((n - 1) q / 100) and the next index are a and b: the
    interpolation of _percentile_shortcut (numpy's float32 'linear' rule).  -> (thr, gamma); the host's check of the device's."""
    qf = np.true_divide(q, np.float32(100))
    vi = (n - 1) * qf
    lo = n - 1 if vi >= n - 1 else int(np.floor(vi))
    gamma = np.float32(np.float64(vi) - lo)
    a, b = np.float32(a), np.float32(b)
    diff = b - a
    return (b - diff * (1 - gamma) if gamma >= 0.5 else a + diff * gamma), gamma


def _shortcut_matches_numpy():
    rng = np.random.default_rng(12345)
    for n in (1, 2, 3, 7, 100, 101, 1000, 4097):
        for scale in (1.0, 1e-6):
            v = (rng.random(n, dtype=np.float32) * np.float32(scale)).astype(np.float32)
            for q in (1, 50, 99):
                x, y = _percentile_shortcut(v, q), np.percentile(v, q)
                if type(x) is not type(y) or not (x == y):
                    return False
    return True


def percentile_of_samples(values, q):
    """np.percentile(values, q) for the positive lattice samples (1-D float32, no NaN): by the shortcut when it reproduces the
    installed numpy bit for bit and in type on a set of probes (checked once per process), by numpy otherwise."""
    global _FAST_PERCENTILE
    if _FAST_PERCENTILE is None:
        try:
            _FAST_PERCENTILE = bool(_shortcut_matches_numpy())
        except Exception:
            _FAST_PERCENTILE = False
    if _FAST_PERCENTILE and isinstance(values, np.ndarray) and values.dtype == np.float32 and values.ndim == 1 and values.size:
        return _percentile_shortcut(values, q)
    return np.percentile(values, q)


def log10_min_triangle_otsu(values, nbins=256):
    """labelling.py:448-455: thresholds in the log10 domain, mapped back, minimum of the two.  The reference histograms the same
    log values twice (once per threshold); one histogram serves both here -- same counts, same edges, same results."""
    log_values = np.log10(values)
    if log_values.dtype == np.float32 and log_values.size:
        triangle, otsu = hipnative.host_hist_thresholds(log_values, nbins)      # numpy's histogram arithmetic, one library call
    else:
        from nellie_amd.utils.gpu_functions import _host_histogram
        counts, edges = _host_histogram(log_values, nbins)
        triangle, otsu = hipnative.hist_thresholds(counts, edges)
    triangle = 10 ** triangle
    otsu = 10 ** otsu
    return min(triangle, otsu)
