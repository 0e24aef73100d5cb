"""
numpy restatement of the Network stage behind the thinning (reference nellie/segmentation/networking.py:828-851), step by step:

  clean     `_remove_connected_label_pixels` (:261-296)
  seed      `_add_missing_skeleton_labels` (:342-387), with the device's rule for equal maxima: NaN ranks above every number and
            among equals the lowest raster index wins (the reference's pick follows no rule; the fixtures keep every maximum unique)
  classes   `_get_pixel_class` (:672-683) and `_get_branch_skel_labels` (:758-800)
  relabel   `_relabel_objects` (:485-577), with scipy's feature transform written out line by line (`feature_transform`): the
            separable Voronoi transform behind scipy.ndimage.distance_transform_edt(return_indices=True), whose choice among
            equidistant seeds is part of the result.

Nothing here imports the package under test or the reference.
"""
import numpy as np
from scipy import ndimage as ndi


def clean(skel, ndim):
    """Zero the skeleton voxels whose 3^ndim neighbourhood (centre included, outside = background) holds two different labels;
    voxels on a face of the frame are kept."""
    skel = np.asarray(skel)
    size = (3,) * ndim
    mx = ndi.maximum_filter(skel, size=size, mode="constant", cval=0)
    big = 1 << 40                       # above every int32 label, exact as the float64 the filter takes its cval through
    nobg = np.where(skel == 0, big, skel.astype(np.int64))
    mn = ndi.minimum_filter(nobg, size=size, mode="constant", cval=big)
    mn = np.where(mn == big, 0, mn)
    ambiguous = (skel > 0) & (mn > 0) & (mx > 0) & (mn != mx)
    inner = np.zeros(skel.shape, bool)
    inner[(slice(1, -1),) * ndim] = True
    return np.where(ambiguous & inner, 0, skel)


def seed_rank(frangi, nan_highest=True, zeros_equal=True):
    """Sort key of the seeding rule: larger is better; NaN above every number, -0.0 equal to 0.0.
    nan_highest=False, zeros_equal=False: other rules (NaN below every number; -0.0 below 0.0), which the tests must tell apart."""
    f = np.asarray(frangi, np.float32).ravel()
    if zeros_equal:
        f = f + np.float32(0.0)
    u = f.view(np.uint32).astype(np.uint64)
    key = np.where(u & 0x80000000, ~u & 0xFFFFFFFF, u | 0x80000000)
    return np.where(np.isnan(f), 0xFFFFFFFF if nan_highest else 0, key).astype(np.uint64)


def seed(skel_clean, labels, frangi, lowest_index=True, nan_highest=True, zeros_equal=True):
    """Every label > 0 without a voxel in skel_clean gets one at the maximum of frangi over its voxels.  The three keywords are the
    rule among equal maxima, NaNs and signed zeros; the defaults are the device's."""
    out = np.array(skel_clean, copy=True)
    lab = np.asarray(labels).ravel()
    have = np.unique(out)
    missing = np.setdiff1d(np.unique(lab), have)
    missing = missing[missing > 0]
    if missing.size == 0:
        return out, 0
    rank = seed_rank(frangi, nan_highest, zeros_equal)
    flat = out.reshape(-1)
    for L in missing:
        idx = np.flatnonzero(lab == L)
        r = rank[idx]
        flat[idx[np.flatnonzero(r == r.max())[0 if lowest_index else -1]]] = L
    return out, int(missing.size)


def unique_maxima(labels, frangi):
    """True when, for every label > 0, the maximum of frangi over the label's voxels is taken once and is no NaN."""
    lab = np.asarray(labels).ravel()
    fr = np.asarray(frangi).ravel()
    for L in np.unique(lab):
        if L <= 0:
            continue
        v = fr[lab == L]
        if np.isnan(v).any() or int((v == v.max()).sum()) != 1:
            return False
    return True


def pixel_class(skel, ndim):
    m = (np.asarray(skel) > 0).astype(np.uint8)
    s = ndi.convolve(m, np.ones((3,) * ndim), mode="constant", cval=0) * m
    s[s > 4] = 4
    return s.astype(np.uint8)


def branch_skel_labels(pc, ndim):
    lab, _ = ndi.label((pc > 0) & (pc != 4), structure=np.ones((3,) * ndim))
    return lab.astype(np.int32)


# ---- scipy's feature transform, line by line ------------------------------------------------------------------------------------------

def _voronoi_line(feat, coor, d, s):
    """One line along axis d.  feat: (len, rank) int64 features of the line's voxels (feat[:, 0] < 0: none), rewritten in place;
    coor: the line's coordinates on the other axes (entry d unused); s: spacing."""
    n, rank = feat.shape
    f = feat.copy()
    g = []
    for i in range(n):
        if f[i, 0] < 0:
            continue
        fd = float(f[i, d])
        wR = 0.0
        for j in range(rank):
            if j != d:
                tw = float(f[i, j] - coor[j]) * s[j]
                wR += tw * tw
        while len(g) >= 2:
            i1, i2 = g[-1], g[-2]
            f1 = float(f[i1, d])
            a = (f1 - float(f[i2, d])) * s[d]
            b = (fd - f1) * s[d]
            c = a + b
            uR = vR = 0.0
            for j in range(rank):
                if j != d:
                    tu = float(f[i2, j] - coor[j]) * s[j]
                    tv = float(f[i1, j] - coor[j]) * s[j]
                    uR += tu * tu
                    vR += tv * tv
            if c * vR - b * uR - a * wR - a * b * c <= 0.0:
                break
            g.pop()
        g.append(i)
    if not g:
        return
    top, l = len(g) - 1, 0

    def dist(k, i):
        acc = 0.0
        for j in range(rank):
            t = float(f[g[k], j] - (i if j == d else coor[j])) * s[j]
            acc += t * t
        return acc
    for i in range(n):
        d1 = dist(l, i)
        while l < top:
            d2 = dist(l + 1, i)
            if d1 <= d2:
                break
            d1 = d2
            l += 1
        feat[i] = f[g[l]]


def feature_transform(seeds, sampling):
    """Indices (rank, *shape) int32 of the seed scipy.ndimage.distance_transform_edt(~seeds, sampling, return_indices=True) picks
    for every voxel; -1 everywhere when there is no seed."""
    seeds = np.asarray(seeds, bool)
    rank = seeds.ndim
    s = [float(v) for v in sampling]
    shape = seeds.shape
    feat = np.full(shape + (rank,), -1, np.int64)
    idx = np.nonzero(seeds)
    for j in range(rank):
        feat[idx + (j,)] = idx[j]
    for d in range(rank):
        others = [a for a in range(rank) if a != d]
        for pos in np.ndindex(*[shape[a] for a in others]):
            coor = [0] * rank
            sl = [slice(None)] * rank
            for a, p in zip(others, pos):
                coor[a] = p
                sl[a] = p
            line = feat[tuple(sl)]                       # a view: (len, rank)
            _voronoi_line(line, coor, d, s)
    return np.moveaxis(feat, -1, 0).astype(np.int32)


def relabel(branch, labels, sampling, transform=feature_transform):
    """`_relabel_objects`: per object, in its bounding box, every voxel takes the branch label of the seed the feature transform of
    the object's own seeds picks.  Also returns the number of objects with a seed and the sum of their box volumes."""
    labels = np.asarray(labels)
    branch = np.asarray(branch)
    out = np.zeros(labels.shape, np.uint32)
    n_obj = vol = 0
    if labels.size == 0 or int(labels.max()) <= 0:
        return out, n_obj, vol
    for k, sl in enumerate(ndi.find_objects(labels.astype(np.int32))):
        if sl is None:
            continue
        L = k + 1
        obj = labels[sl] == L
        seeds = (branch[sl] > 0) & obj
        if not seeds.any():
            continue
        n_obj += 1
        vol += int(obj.size)
        ind = transform(seeds, sampling)
        near = branch[sl][tuple(ind)]
        sub = out[sl]
        sub[obj] = near[obj].astype(np.uint32)
    return out, n_obj, vol


def scipy_transform(seeds, sampling):
    return ndi.distance_transform_edt(~np.asarray(seeds, bool), sampling=sampling, return_distances=False, return_indices=True)


def frame(labels, skel_mask, frangi, sampling, transform=feature_transform):
    """Steps 1-5 on one frame -> dict of every intermediate and the three products."""
    labels = np.asarray(labels)
    ndim = labels.ndim
    lab = labels.astype(np.int32)
    skel = lab * np.asarray(skel_mask, bool)
    skel_clean = clean(skel, ndim)
    skel_seeded, n_seeded = seed(skel_clean, lab, frangi)
    skel_pre = (skel_seeded > 0) * lab
    pc = pixel_class(skel_pre, ndim)
    branch = branch_skel_labels(pc, ndim)
    relabelled, n_obj, vol = relabel(branch, lab, sampling, transform)
    return dict(skel=skel, skel_clean=skel_clean, skel_seeded=skel_seeded, n_seeded=n_seeded, skel_pre=skel_pre, pixel_class=pc,
                branch=branch, relabelled=relabelled, n_objects=n_obj, box_volume=vol)
