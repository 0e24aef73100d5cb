"""Writes tests/golden/solidity/*.npz: label frames with, per region, the voxel count, the convex count and the solidity
(tests/solidity_restatement.py).  Run by hand:  python tests/golden/make_golden_solidity.py

Before a file is written, the float rule through scipy's ConvexHull (a) and the exact integer count (b) must agree on every
region, and in a scene not built to be degenerate at least three quarters of the regions must have a non-zero count.  Where skimage
imports, `regionprops(labels, spacing=...)[i].solidity` must equal the stored value bit for bit and `skimage_version` records the
version; where it does not, `skimage_version` is "not checked".
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import solidity_restatement as sr  # noqa: E402

OUT = os.path.join(HERE, "solidity")


def ball(shape, centre, radius):
    g = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1)
    return ((g - np.asarray(centre)) ** 2).sum(axis=-1) <= radius * radius


def shapes_3d():
    lab = np.zeros((14, 20, 26), np.int32)
    for k, p in enumerate([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)]):
        lab[1 + p[0], 1 + p[1], 1 + p[2]] = 3                      # the four-voxel tetrahedron
    lab[1:6, 5:10, 1:6] = 5                                        # a cube ...
    lab[2:5, 6:9, 2:5] = 0                                         # ... hollowed: a shell
    lab[3, 7, 3] = 9                                               # with a voxel of another label inside
    lab[8:13, 1:8, 1:3] = 12                                       # a C: three bars
    lab[8:13, 1:3, 3:8] = 12
    lab[8:13, 6:8, 3:8] = 12
    lab[ball(lab.shape, (6, 13, 18), 5.3)] = 20
    lab[12, 10:14, 10] = 40
    lab[13, 12, 9:13] = 40                                         # a cross over two planes
    return lab, np.array([0.3, 0.1, 0.1])


def degenerate_3d():
    lab = np.zeros((8, 10, 12), np.int16)
    lab[0, 0, 0] = 1                                               # a voxel
    lab[2, 2, 2:4] = 2                                             # a pair
    lab[4, 4, 4:7] = 3                                             # a collinear triple
    lab[6, 1:3, 8:10] = 4                                          # a 2 x 2 plate
    for k in range(4):                                             # a plate in the plane z = x: rank 2, not axis-aligned
        lab[k, 6:9, k] = 7
    lab[5:8, 6:9, 0:2] = 11                                        # and one solid block
    return lab, np.array([0.25, 0.1, 0.1])


def random_3d():
    rng = np.random.default_rng(24)
    lab = np.zeros((10, 24, 28), np.uint16)
    for k in range(14):
        c = rng.integers(0, [10, 24, 28])
        m = ball(lab.shape, c, rng.uniform(1.2, 4.0)) & (rng.random(lab.shape) < 0.7)
        lab[m & (lab == 0)] = 2 * k + 3
    return lab, np.array([0.29, 0.11, 0.13])


def shapes_2d():
    lab = np.zeros((24, 30), np.int32)
    lab[0, 0] = 1
    lab[2, 2:4] = 2
    lab[4, 4:7] = 3
    lab[6:8, 8:10] = 4
    lab[9, 1] = lab[10, 1] = lab[9, 2] = 6
    lab[12:20, 2:10] = 8
    lab[14:18, 4:10] = 0                                           # a C
    lab[ball(lab.shape, (12, 20), 7.4)] = 15
    lab[ball(lab.shape, (12, 20), 4.2)] = 0                        # a ring
    for k in range(6):
        lab[18 + k, 12 + 2 * k:14 + 2 * k] = 21                    # a staircase
    return lab, np.array([0.1, 0.1])


def random_2d():
    rng = np.random.default_rng(25)
    lab = np.zeros((40, 44), np.uint8)
    for k in range(18):
        c = rng.integers(0, [40, 44])
        m = ball(lab.shape, c, rng.uniform(0.8, 5.0)) & (rng.random(lab.shape) < 0.75)
        lab[m & (lab == 0)] = 3 * k + 2
    return lab, np.array([0.2, 0.07])


SCENES = {"shapes_3d": (shapes_3d, False), "degenerate_3d": (degenerate_3d, True), "random_3d": (random_3d, False),
          "shapes_2d": (shapes_2d, False), "random_2d": (random_2d, False)}


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, (make, degenerate) in SCENES.items():
        labels, spacing = make()
        regs = sr.regions_of(labels)
        exact = np.array([sr.count_exact(c, e) for _, c, e in regs], np.int64)
        for (l, c, e), want in zip(regs, exact):
            got = sr.count_float(c, e)
            assert got == want, f"{name}: region {l}: float rule {got}, exact {want}"
        region_labels = np.array([r[0] for r in regs], np.int64)
        n = np.array([len(r[1]) for r in regs], np.int64)
        solidity = sr.solidity_of(n, exact, spacing)
        if not degenerate:
            assert 4 * np.count_nonzero(exact) >= 3 * len(exact), f"{name}: too many flat regions"
        version = "not checked"
        try:
            import skimage
            from skimage import measure
        except ImportError:
            pass
        else:
            props = measure.regionprops(labels.astype(np.int64), spacing=tuple(spacing))
            assert [p.label for p in props] == list(region_labels)
            with np.errstate(all="ignore"):
                sk = np.array([p.solidity for p in props], np.float64)
            assert sk.tobytes() == solidity.tobytes(), f"{name}: skimage's solidity differs"
            version = skimage.__version__
        np.savez_compressed(os.path.join(OUT, name + ".npz"), labels=labels, spacing=spacing, region_labels=region_labels, n=n,
                            convex_count=exact, solidity=solidity, skimage_version=np.array(version))
        print(name, labels.shape, len(regs), "regions,", int((exact == 0).sum()), "flat, skimage:", version)


if __name__ == "__main__":
    main()
