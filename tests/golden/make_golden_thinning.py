#!/usr/bin/env python3
"""Records tests/golden/thinning/*.npz: masks, what skimage.morphology.skeletonize makes of them, and the restatement's counts.

Run by hand with an interpreter that has numpy and scikit-image (the fixtures in the tree were recorded with skimage 0.18.3); nothing
else of this package is needed:

    python tests/golden/make_golden_thinning.py

Before a file is written both forms of tests/thinning_restatement.py must equal skimage voxel for voxel on its mask.  Each file holds
shape, mask_bits and skel_bits (np.packbits of the raveled volumes), the restatement's counts (outer, subiters, candidates, removed,
max_candidates, rounds, max_rounds) and skimage_version.  The network cases are `labels > 0` of the 3-D scenes of tests/golden/network_steps/.
"""
import glob
import os
import sys

import numpy as np
import skimage
from skimage.morphology import skeletonize

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import thinning_restatement as rs  # noqa: E402

OUT = os.path.join(HERE, "thinning")


def framed(shape, block):
    """A solid block centred in a frame of zeros."""
    m = np.zeros(shape, bool)
    lo = [(s - b) // 2 for s, b in zip(shape, block)]
    m[tuple(slice(a, a + b) for a, b in zip(lo, block))] = True
    return m


def dilate(m, r):
    """Dilation by the ball of radius r, zero outside the frame."""
    out = np.zeros_like(m)
    pts = np.argwhere(m)
    rr = np.arange(-r, r + 1)
    for off in np.argwhere(np.add.outer(np.add.outer(rr * rr, rr * rr), rr * rr) <= r * r) - r:
        q = pts + off
        q = q[((q >= 0) & (q < m.shape)).all(1)]
        out[tuple(q.T)] = True
    return out


def tubes(rng, n, walks, radius):
    line = np.zeros((n, n, n), bool)
    for _ in range(walks):
        d = np.cumsum(rng.integers(-1, 2, (n, 3)), axis=0) + rng.integers(0, n, 3)
        d = d[((d >= 0) & (d < n)).all(1)]
        line[tuple(d.T)] = True
    return dilate(line, radius)


def cases():
    rng = np.random.default_rng(1994)
    yield "box", framed((12, 36, 40), (6, 30, 34))
    z, y, x = np.ogrid[:30, :30, :30]
    yield "ball", (z - 15) ** 2 + (y - 15) ** 2 + (x - 15) ** 2 <= 13 * 13
    yield "bar_x", framed((5, 5, 202), (3, 3, 200))
    yield "bar_y", framed((5, 152, 5), (3, 150, 3))
    yield "bar_z", framed((122, 5, 5), (120, 3, 3))
    yield "plate", framed((3, 22, 72), (1, 20, 70))
    yield "full", np.ones((5, 6, 7), bool)
    yield "plane", rng.random((1, 20, 24)) < 0.7
    yield "one", np.ones((1, 1, 1), bool)
    yield "two", np.ones((1, 1, 2), bool)
    yield "empty", np.zeros((6, 20, 24), bool)
    hollow = framed((13, 14, 15), (11, 12, 13))
    hollow &= ~framed((13, 14, 15), (5, 6, 7))
    yield "hollow", hollow
    yield "noise", rng.random((9, 10, 70)) < 0.6
    yield "tubes_r2", tubes(rng, 40, 5, 2)
    yield "tubes_r4", tubes(rng, 40, 3, 4)
    yield "odd", dilate(rng.random((11, 33, 45)) < 0.02, 2)
    # more foreground voxels, and more candidates in one sub-iteration, than one launch has threads (1024 workgroups of 256): the
    # kernels' stride loops take more than one trip.  A 16^3 tile of noise repeated, so that the file stays small.
    yield "large_tiled_noise", np.tile(rng.random((16, 16, 16)) < 0.6, (6, 12, 12))
    for path in sorted(glob.glob(os.path.join(HERE, "network_steps", "*.npz"))):
        labels = np.load(path)["labels"]
        if labels.ndim == 3:
            yield os.path.basename(path)[:-4], labels > 0


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, mask in cases():
        mask = np.ascontiguousarray(mask, bool)
        want = skeletonize(mask) > 0
        seq, s_seq = rs.thin_sequential(mask)
        par, s_par = rs.thin_rounds(mask)
        assert np.array_equal(seq, want), f"{name}: the sequential restatement differs from skimage"
        assert np.array_equal(par, want), f"{name}: the round-parallel restatement differs from skimage"
        assert all(s_seq[k] == s_par[k] for k in s_seq), (name, s_seq, s_par)
        np.savez_compressed(os.path.join(OUT, name + ".npz"), shape=np.array(mask.shape, np.int64), mask_bits=np.packbits(mask.ravel()),
                            skel_bits=np.packbits(want.ravel()), skimage_version=np.array(skimage.__version__),
                            **{k: np.int64(v) for k, v in s_par.items()})
        print(f"{name:24s} {str(mask.shape):16s} in {int(mask.sum()):7d} out {int(want.sum()):6d} {s_par}", flush=True)


if __name__ == "__main__":
    main()
