"""
The 3-D thinning on the MI355X HIP engine: `skimage.morphology.skeletonize` of a volume (Lee, Kashyap & Chu 1994 as skimage 0.18.3 runs
it; the reference's `_skeletonize`, networking.py:394-409), voxel for voxel.

    skeletonize(mask) -> bool ndarray of mask's shape            # == skimage.morphology.skeletonize(mask) > 0

`Network(..., skeletonize="hip")` runs the same kernels on the labels it uploads anyway (csrc/thin.inc holds the algorithm, the rule
that makes its sequential re-check parallel, and the kernels; DESIGN.md has the measurements).  3-D only: for a 2-D image skimage runs
another rule (its Zhang variant), which is not provided -- NotImplementedError.  There is no CPU engine behind this.
"""
from __future__ import annotations

import numpy as np

from nellie_amd import hipnative
from nellie_amd.stage import require_gpu


def _as_mask(mask):
    mask = np.asarray(mask)
    if mask.ndim != 3:
        raise NotImplementedError(f"skeletonize on the device is the 3-D thinning; got shape {mask.shape}: for a 2-D image skimage runs "
                                  "another rule -- use skimage.morphology.skeletonize (Network: skeletonize=None or a callable)")
    if mask.dtype != np.bool_ and mask.dtype.kind not in "iu":
        raise TypeError(f"skeletonize takes a bool or integer array, not {mask.dtype}")
    if 0 in mask.shape:
        raise ValueError(f"empty volume {mask.shape}")
    return mask if mask.dtype == np.bool_ else mask != 0


def skeletonize(mask, device=0, rounds_per_sync=None, with_info=False):
    """bool or integer ndarray (non-zero = foreground) of shape (Z, Y, X) -> bool skeleton of the same shape; the input is not modified.
    rounds_per_sync: rounds launched between two read-backs (None: the library's default; no effect on the result).
    with_info: -> (skeleton, dict of the seven counts n_in, n_out, outer, subiters, rounds, candidates, removed, plus ms)."""
    mask = _as_mask(mask)
    require_gpu()
    with hipnative.Context(mask.shape, device=device) as ctx:
        out = ctx.thin(mask, rounds_per_sync)
        if not with_info:
            return out
        counts, ms = ctx.thin_info()
        return out, dict(counts, ms=ms)
