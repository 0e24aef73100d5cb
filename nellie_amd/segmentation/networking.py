"""
nellie.segmentation.networking.Network on the MI355X HIP engine.

`Network` is the stage: it reads im_instance_label and im_preprocessed and writes im_skel, im_pixel_class and im_skel_relabelled, as the
reference's class of the same name does (networking.py:828-851, :902-931).  By default the one host call per frame is the thinning
(`skimage.morphology.skeletonize`, networking.py:394-409, or the `skeletonize` callable given); labels, thinning mask and Frangi frame
then go up once.  With skeletonize="hip" (3-D frames) the thinning runs on the device too (segmentation/thinning.py, csrc/thin.inc):
labels and Frangi frame go up, no mask, and nothing of skimage is imported.  On the device

  skel    = labels * mask                                                                    (:408)
  clean   `_remove_connected_label_pixels` (:261-296)
  seed    `_add_missing_skeleton_labels` (:342-387)
  classes `_get_pixel_class` (:634-683): 1 isolated, 2 tip, 3 edge, 4 junction; `_get_branch_skel_labels` (:758-800): 26- (2-D: 8-)
          connected labels of the skeleton without its junctions, int32 ids in scipy's raster order
  relabel `_relabel_objects` (:485-577): per object, the feature transform of its own branch voxels in its bounding box

run, and the three products come down once.  All of it is bit-identical to the reference's numpy / scipy path, with one documented
difference: where the Frangi maximum of a label without skeleton is taken more than once, the reference's pick comes out of an
unstable argsort and follows no rule; here the lowest raster index wins and NaN ranks above every number.

`HipNetworkKernels` keeps the two class methods as a mixin for the reference's own class,

    class Network(HipNetworkKernels, nellie.segmentation.networking.Network): pass

(same names, same arguments, numpy arrays in and out).  There is no CPU engine behind any of this: `force_cpu=True`, device="cpu" and a
missing HIP device raise.
"""
from __future__ import annotations

import zlib

import numpy as np

from nellie_amd import hipnative
from nellie_amd.stage import Held, flush, frame_count, open_outputs, require_gpu, resolve_device, spacing_of
from nellie_amd.utils.base_logger import logger


def _ctx_shape(shape):
    shape = tuple(int(s) for s in shape)
    if len(shape) == 2:
        return (1,) + shape
    if len(shape) == 3:
        return shape
    raise ValueError(f"expected a 2-D image or a 3-D volume, got shape {shape}")


class HipNetworkKernels:
    """Mixin / helper holding one HIP context per frame shape."""

    _held_ctx = None                      # a Held of this object's own from the first context on (a mixin has no constructor)
    device_index = 0

    def _hip_context(self, shape):
        require_gpu()
        key = (_ctx_shape(shape), int(getattr(self, "device_index", 0) or 0))
        if self._held_ctx is None:
            self._held_ctx = Held()
        if self._held_ctx.key != key:
            self.close()
        return self._held_ctx.get(key, lambda: hipnative.Context(key[0], device=key[1]))

    def close(self):
        if self._held_ctx is not None:
            self._held_ctx.close()

    @staticmethod
    def _no_cpu(force_cpu):
        if force_cpu:
            raise RuntimeError("nellie_amd provides the MI355X HIP backend only: force_cpu=True is not available "
                               "(use the reference implementation on CPU)")

    def _get_pixel_class(self, skel, force_cpu: bool = False):
        """uint8 classes: 0 background, 1 isolated, 2 tips, 3 edges, 4 junctions (clipped) -- networking.py:634-683."""
        self._no_cpu(force_cpu)
        skel = np.asarray(skel)
        ctx = self._hip_context(skel.shape)
        # skel_mask = skel > 0: any integer / float dtype reduces to its sign here
        if skel.dtype != np.int32:
            skel = (skel > 0).astype(np.int32)
        out, self.n_skeleton_voxels = ctx.skel_pixel_class(skel)
        self._pixel_class_resident = out
        self._pixel_class_crc = zlib.crc32(np.ascontiguousarray(out).view(np.uint8))
        return out

    def _get_branch_skel_labels(self, pixel_class, force_cpu: bool = False):
        """int32 connected components of (pixel_class > 0) & (pixel_class != 4) -- networking.py:758-800."""
        self._no_cpu(force_cpu)
        pc = np.asarray(pixel_class)
        ctx = self._hip_context(pc.shape)
        resident = getattr(self, "_pixel_class_resident", None)
        checksum = getattr(self, "_pixel_class_crc", None)
        self._pixel_class_resident = None
        # the array the previous call returned, UNCHANGED (the caller may have cleaned junctions in place): its bits are
        # still on the device.  Identity alone is not enough; the checksum costs a fraction of the upload it saves.
        if resident is pixel_class and checksum is not None and checksum == zlib.crc32(np.ascontiguousarray(pc).view(np.uint8)):
            labels, self.n_branches = ctx.skel_branch_labels(None)
            return labels.reshape(pc.shape)
        if pc.dtype != np.uint8:
            pc = np.where(pc == 4, 4, (pc > 0).astype(np.uint8)).astype(np.uint8)
        labels, self.n_branches = ctx.skel_branch_labels(pc)
        return labels


def pixel_class(skel, device=0):
    """Function form of `Network._get_pixel_class` (networking.py:672-683)."""
    k = HipNetworkKernels()
    k.device_index = device
    try:
        return k._get_pixel_class(skel)
    finally:
        k.close()


def branch_skel_labels(pixel_class_im, device=0):
    """Function form of `Network._get_branch_skel_labels` (networking.py:758-800)."""
    k = HipNetworkKernels()
    k.device_index = device
    try:
        return k._get_branch_skel_labels(pixel_class_im)
    finally:
        k.close()


def relabel_objects(branch_skel_labels, label_frame, scaling, scratch_voxels=None, device=0):
    """Function form of `Network._relabel_objects` (networking.py:485-577) with `scaling` in the role of `self.scaling` -> uint32."""
    require_gpu()
    labels = np.asarray(label_frame)
    with hipnative.Context(_ctx_shape(labels.shape), device=device) as ctx:
        ctx.network_relabel_load(labels, branch_skel_labels)
        ctx.network_relabel(scaling, scratch_voxels)
        return ctx.network_fetch(branch=False, pixel_class=False)[2]


HIP_THINNING = "hip"


def _check_thinning(skeletonize, im_info):
    """The `skeletonize` keyword, judged before any file is created: None (skimage's), a callable, or "hip" on a 3-D im_info."""
    if skeletonize is None or callable(skeletonize):
        return
    if not isinstance(skeletonize, str) or skeletonize != HIP_THINNING:
        raise ValueError(f"skeletonize={skeletonize!r}: expected None (skimage.morphology.skeletonize), a callable or {HIP_THINNING!r}")
    if getattr(im_info, "no_z", False):
        raise NotImplementedError("skeletonize='hip' is the 3-D thinning: for a 2-D image skimage runs another rule, which is not "
                                  "provided on the device -- pass skeletonize=None (skimage's) or a callable")


def _import_skeletonize():
    try:
        from skimage.morphology import skeletonize
    except Exception as exc:  # noqa: BLE001  (a broken install is as absent as a missing one)
        raise ImportError("Network needs a thinning: scikit-image (skimage.morphology.skeletonize) cannot be imported; install it or "
                          "pass skeletonize=<callable(bool ndarray) -> bool ndarray> to Network") from exc
    return skeletonize


class Network:
    """
    The reference's constructor (networking.py:50-60) plus `device_index`, `skeletonize` and `scratch_voxels`.

    low_memory, max_chunk_voxels   accepted and ignored: they select the reference's chunked and per-object CPU paths, whose results
                                   equal the whole-frame ones; here a frame is always processed whole on the device, and the
                                   per-object thinning of low_memory is not provided.
    skeletonize                    callable(mask: bool ndarray) -> bool ndarray of the same shape; None: skimage.morphology.skeletonize,
                                   imported when run() starts (ImportError, naming this keyword, before any file is created); "hip":
                                   the 3-D thinning on the device, skimage's result voxel for voxel (NotImplementedError on a 2-D
                                   im_info, before any file is created).
    rounds_per_sync                "hip" only: rounds of the thinning's re-check launched between two read-backs (None: the library's
                                   default); it changes no result.
    scratch_voxels                 box voxels one batch of the relabelling may hold (8 bytes each); None: half of the free HBM.  Never less
                                   than one frame.
    `kernel_ms` holds one dict per frame of the last run: clean, seed, classes, relabel (ms on the stream, transfers excluded), and
    "thin" in "hip" mode, where `frame_stats` also gains the thinning's seven counts as thin_*.
    """

    def __init__(self, im_info, num_t=None, min_radius_um=0.20, max_radius_um=1, viewer=None, device="auto", low_memory: bool = False,
                 max_chunk_voxels: int = int(1e6), device_index=0, skeletonize=None, scratch_voxels=None, rounds_per_sync=None):
        self.im_info = im_info
        self.device = device
        self.device_type = resolve_device(device)
        self.device_index = int(device_index or 0)
        self.low_memory = low_memory
        self.max_chunk_voxels = int(max_chunk_voxels)
        self.num_t = num_t
        if num_t is None and not im_info.no_t:
            self.num_t = im_info.shape[im_info.axes.index("T")]
        if not im_info.no_z:
            self.z_ratio = im_info.dim_res["Z"] / im_info.dim_res["X"]
        self.min_radius_um = max(min_radius_um, im_info.dim_res["X"])
        self.max_radius_um = max_radius_um
        self.min_radius_px = self.min_radius_um / im_info.dim_res["X"]
        self.max_radius_px = self.max_radius_um / im_info.dim_res["X"]
        self.scaling = spacing_of(im_info)
        self.skeletonize = skeletonize
        self.scratch_voxels = scratch_voxels
        self.rounds_per_sync = rounds_per_sync
        self.shape = ()
        self.im_frangi_memmap = self.label_memmap = self.pixel_class_memmap = self.skel_memmap = self.skel_relabelled_memmap = None
        self.viewer = viewer
        self.kernel_ms = []
        self.frame_stats = []                # per frame: max_label, n_removed, n_seeded, n_skel, n_branches, n_objects, box_volume, n_batches
                                             # ("hip" thinning: and thin_n_in, thin_n_out, thin_outer, thin_subiters, thin_rounds, ...)
        self._held = Held()
        self._thin = None                    # the thinning in use: `skeletonize`, or skimage's once it has been imported

    def close(self):
        self._held.close()

    def _get_t(self):
        self.num_t = frame_count(self.im_info, self.num_t)

    def _allocate_memory(self):
        paths = self.im_info.pipeline_paths
        self.label_memmap = self.im_info.get_memmap(paths["im_instance_label"])
        self.im_frangi_memmap = self.im_info.get_memmap(paths["im_preprocessed"])
        self.shape = self.label_memmap.shape
        self.skel_memmap, self.pixel_class_memmap, self.skel_relabelled_memmap = open_outputs(
            self.im_info, [(paths["im_skel"], "int32", "skeleton image"), (paths["im_pixel_class"], "uint8", "pixel class image"),
                           (paths["im_skel_relabelled"], "uint32", "skeleton relabelled image")], creator=True)

    def _skeleton_mask(self, label_frame):
        mask = np.asarray(self._thin(label_frame > 0))
        if mask.shape != label_frame.shape:
            raise ValueError(f"skeletonize returned shape {mask.shape} for a frame of shape {label_frame.shape}")
        return mask != 0

    def frame(self, label_frame, frangi_frame, skel_mask=None):
        """networking.py:828-851 on arrays -> (branch skeleton labels int32, pixel classes uint8, relabelled uint32).  skel_mask: the
        thinning's result when the caller has it, else `skeletonize` runs on label_frame > 0."""
        require_gpu()
        labels = np.asarray(label_frame)
        frangi = np.asarray(frangi_frame)
        if labels.ndim != len(self.scaling):
            raise ValueError(f"expected a {len(self.scaling)}-D frame, got shape {labels.shape}")
        if frangi.shape != labels.shape:
            raise ValueError(f"frangi frame shape {frangi.shape} does not match the labels' {labels.shape}")
        on_device = skel_mask is None and isinstance(self.skeletonize, str)
        if on_device:
            _check_thinning(self.skeletonize, self.im_info)
        elif skel_mask is None:
            if self._thin is None:
                self._thin = self.skeletonize or _import_skeletonize()
            skel_mask = self._skeleton_mask(labels)
        key = (_ctx_shape(labels.shape), self.device_index)
        ctx = self._held.get(key, lambda: hipnative.Context(key[0], device=key[1]))
        thin_ms = None
        if on_device:
            stats = dict(max_label=ctx.network_load_thin(labels, frangi, self.rounds_per_sync))
            counts, thin_ms = ctx.thin_info()
            stats.update(("thin_" + k, v) for k, v in counts.items())
        else:
            stats = dict(max_label=ctx.network_load(labels, skel_mask, frangi))
        stats["n_removed"], stats["n_seeded"] = ctx.network_clean_seed()
        stats["n_skel"], stats["n_branches"] = ctx.network_classes()
        stats["n_objects"], stats["box_volume"], stats["n_batches"] = ctx.network_relabel(self.scaling, self.scratch_voxels)
        out = ctx.network_fetch()
        self.kernel_ms.append(ctx.network_kernel_ms() if thin_ms is None else dict(ctx.network_kernel_ms(), thin=thin_ms))
        self.frame_stats.append(stats)
        return out

    def _run_frame(self, t):
        logger.info(f"Running network analysis, volume {t}/{self.num_t - 1}")
        return self.frame(np.asarray(self.label_memmap[t]), np.asarray(self.im_frangi_memmap[t]))

    def _run_networking(self):
        self.kernel_ms, self.frame_stats = [], []
        for t in range(self.num_t):
            if self.viewer is not None:
                self.viewer.status = f"Extracting branches. Frame: {t + 1} of {self.num_t}."
            skel, pixel_class, skel_relabelled = self._run_frame(t)
            if self.im_info.no_t or self.num_t == 1:
                self.skel_memmap[:] = skel
                self.pixel_class_memmap[:] = pixel_class
                self.skel_relabelled_memmap[:] = skel_relabelled
            else:
                self.skel_memmap[t] = skel
                self.pixel_class_memmap[t] = pixel_class
                self.skel_relabelled_memmap[t] = skel_relabelled

    def run(self):
        logger.info("Running Network (HIP).")
        _check_thinning(self.skeletonize, self.im_info)                 # before any file exists, like the import
        self._thin = None if isinstance(self.skeletonize, str) else self.skeletonize or _import_skeletonize()
        require_gpu()
        self._get_t()
        self._allocate_memory()
        try:
            self._run_networking()
            flush(self.skel_memmap, self.pixel_class_memmap, self.skel_relabelled_memmap)
        finally:
            self.close()
