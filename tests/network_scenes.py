"""Seeded scenes for the Network stage behind the thinning: labelled tubes around random walks, whose walks stand in for the thinning
(skimage is not available where the fixtures are made), plus the hand-built relabel scenes of tests/test_hip_network_steps.py."""
import numpy as np
from scipy import ndimage as ndi


def unique_frangi(rng, shape):
    """float32 values, all different (so every label's maximum is unique), in (0, 1]."""
    n = int(np.prod(shape))
    assert n < 1 << 24
    return ((rng.permutation(n).astype(np.float32) + 1) / np.float32(n)).reshape(shape)


def _walk(rng, shape, start, steps, keep_dir=0.7):
    ndim = len(shape)
    pos = np.array(start)
    out = [tuple(pos)]
    d = rng.integers(-1, 2, ndim)
    for _ in range(steps):
        if rng.random() > keep_dir or not d.any():
            d = rng.integers(-1, 2, ndim)
        nxt = pos + d
        if ((nxt < 0) | (nxt >= shape)).any():
            d = -d
            nxt = pos + d
            if ((nxt < 0) | (nxt >= shape)).any():
                continue
        pos = nxt
        out.append(tuple(pos))
    return out


def walks_scene(rng, shape, n_obj=6, steps=25, branches=2, radius=1, drop=0, blocks=0, touching=False):
    """labels (int32), skeleton mask (bool), frangi (float32).  Object k + 1 is the dilation of a random walk with side walks, painted
    in order where nothing is painted yet; the mask is the walks' own voxels inside their object.
    drop     the first `drop` objects lose their mask (the seed step has to give them a voxel)
    blocks   that many extra objects whose mask is a 2^ndim block: every voxel a junction, so no branch and no seed for the relabelling
    touching object 2 is a shifted copy of object 1, one voxel away: skeleton voxels of two labels in one neighbourhood"""
    shape = tuple(shape)
    ndim = len(shape)
    labels = np.zeros(shape, np.int32)
    mask = np.zeros(shape, bool)
    struct = ndi.generate_binary_structure(ndim, ndim)
    paths = []
    for k in range(n_obj):
        if touching and k == 1:
            shift = np.zeros(ndim, int)
            shift[-1] = 1
            vox = [tuple(np.clip(np.array(p) + shift, 0, np.array(shape) - 1)) for p in paths[0]]
        else:
            start = [int(rng.integers(0, s)) for s in shape]
            vox = _walk(rng, shape, start, steps)
            for _ in range(branches):
                vox += _walk(rng, shape, vox[int(rng.integers(0, len(vox)))], steps // 3)
        paths.append(vox)
        line = np.zeros(shape, bool)
        line[tuple(np.array(vox).T)] = True
        body = ndi.binary_dilation(line, struct, iterations=radius) if radius else line
        if touching and k == 0:
            body = line                                  # thin, so that object 2's walk lies beside it, not inside it
        new = body & (labels == 0)
        labels[new] = k + 1
        if k >= drop:
            mask |= line & (labels == k + 1)
    for b in range(blocks):
        L = int(labels.max()) + 1
        for _ in range(200):
            c = [int(rng.integers(1, max(2, s - 4))) for s in shape]
            sl = tuple(slice(a, a + 4) for a in c)
            if labels[sl].shape == (4,) * ndim and not labels[sl].any():
                labels[sl] = L
                mask[tuple(slice(a + 1, a + 3) for a in c)] = True
                break
    return labels, mask, unique_frangi(rng, shape)


def irregular_seeds(rng, n, lo=3, hi=40):
    """Positions 0 <= p < n at irregular gaps."""
    out, p = [], int(rng.integers(0, lo + 1))
    while p < n:
        out.append(p)
        p += int(rng.integers(lo, hi))
    return out


def network_im_info(labels_t, frangi_t, spacing, no_t=False):
    """tests/fakes.ArrayImInfo with Network's inputs in place and its three output paths; `created` lists the files made."""
    from fakes import ArrayImInfo, _mem
    ndim = len(spacing)
    info = ArrayImInfo(labels_t, dict(zip("ZYX"[3 - ndim:], spacing), T=1.0), no_z=ndim == 2)
    info.no_t = no_t
    info.pipeline_paths.update(im_skel="skel", im_pixel_class="pixel_class", im_skel_relabelled="skel_relabelled")
    info.store["labels"] = _mem(labels_t)
    info.store["frangi"] = _mem(frangi_t)
    info.created = []
    allocate = info.allocate_memory

    def allocate_memory(path, *a, **kw):
        info.created.append(path)
        return allocate(path, *a, **kw)
    info.allocate_memory = allocate_memory
    return info


# ---- scenes at the sizes where the Network kernels stride and their tables grow (tests/test_hip_network_scale.py) -------------------------
TRIP_2048 = 2048 * 256            # voxels one launch of nw_skel_kernel / nw_minmax_kernel covers
TRIP_8192 = 8192 * 256            # the same for nw_clean_kernel, nw_has_kernel and nw_best_kernel: at or above it lies the "last trip"


def _paint_in_crop(labels, mask, vox, label, radius, masked, struct):
    """walks_scene's painting of one object, inside the crop around its walk: the dilation never sees the whole frame."""
    v = np.array(vox)
    lo = np.maximum(v.min(0) - radius, 0)
    hi = np.minimum(v.max(0) + radius + 1, labels.shape)
    crop = tuple(slice(int(a), int(b)) for a, b in zip(lo, hi))
    line = np.zeros(tuple(int(b - a) for a, b in zip(lo, hi)), bool)
    line[tuple((v - lo).T)] = True
    body = ndi.binary_dilation(line, struct, iterations=radius) if radius else line
    sub = labels[crop]
    sub[body & (sub == 0)] = label
    if masked:
        mask[crop] |= line & (sub == label)


def _straight(start, step, count):
    return [tuple(int(a + i * d) for a, d in zip(start, step)) for i in range(count)]


def wide_planted(shape):
    """The objects a wide scene holds on purpose -> list of (name, voxels, radius, masked).  In raster order the last trip of the
    8192-workgroup kernels begins at TRIP_8192; its first whole row is `y8` (2-D) or row `y8` of plane nz - 2 (3-D)."""
    nx = shape[-1]
    if len(shape) == 3:
        nz, ny, _ = shape
        assert (nz - 2) * ny * nx < TRIP_8192 < (nz - 1) * ny * nx and 6 * ny * nx > TRIP_2048
        y8 = -(-(TRIP_8192 - (nz - 2) * ny * nx) // nx)
        assert y8 + 110 < ny
        return [("largest", _straight((nz - 1, y8 + 80, 20), (0, 0, 1), 40), 1, True),           # (a)
                ("seeded_last", _straight((nz - 1, y8 + 100, 100), (0, 0, 1), 40), 1, False),    # (b)
                ("spanning", _straight((0, ny // 2, 200), (1, 0, 0), nz), 1, False),             # (c)
                ("touch_a", _straight((nz - 2, y8 + 30, 50), (0, 0, 1), 30), 0, True),           # (d): an inner plane
                ("touch_b", _straight((nz - 2, y8 + 31, 50), (0, 0, 1), 30), 0, True),
                ("along_x", _straight((10, 50, 30), (0, 0, 1), 111), 1, True),                   # (e) (f) (h) (k): crosses x = 63|64, 127|128
                ("across_planes", _straight((4, 80, 54), (1, 0, 1), 16), 1, True),               # (g): x = 63 -> 64 while z goes up
                ("left_edge", _straight((8, 120, 0), (0, 0, 1), 13), 1, True),                   # (i)
                ("right_edge", _straight((8, 130, nx - 13), (0, 0, 1), 13), 1, True),
                ("column", _straight((0, 220, 100), (1, 0, 0), nz), 1, True)]                    # (j)
    ny, _ = shape
    y8 = -(-TRIP_8192 // nx)
    assert y8 + 90 < ny and 101 * nx < TRIP_2048
    return [("largest", _straight((y8 + 50, 20), (0, 1), 40), 1, True),
            ("seeded_last", _straight((y8 + 70, 100), (0, 1), 40), 1, False),
            ("spanning", _straight((100, 700), (1, 0), y8 + 80 - 100), 1, False),
            ("touch_a", _straight((y8 + 20, 50), (0, 1), 30), 0, True),
            ("touch_b", _straight((y8 + 21, 50), (0, 1), 30), 0, True),
            ("along_x", _straight((50, 30), (0, 1), 111), 1, True),
            ("across_rows", _straight((80, 54), (1, 1), 16), 1, True),
            ("left_edge", _straight((120, 0), (0, 1), 13), 1, True),
            ("right_edge", _straight((130, nx - 13), (0, 1), 13), 1, True),
            ("column", _straight((0, 900), (1, 0), 30), 1, True)]


def wide_scene(shape, seed, n_obj=450, steps=150, keep_dir=0.92, branches=2):
    """labels (int32), skeleton mask (bool), frangi (float32) for a frame above TRIP_8192 voxels.  Object k carries label 3k + 1 (gaps; the
    largest above 1024, where the per-label table starts).  The planted objects (wide_planted) are painted first and keep their shape; the
    one named "largest" carries the largest label.  The others are walks_scene's tubes around long walks, every second one without mask;
    the Frangi maximum of "spanning" is moved into the last trip (a swap: the values stay all different)."""
    shape = tuple(shape)
    ndim = len(shape)
    rng = np.random.default_rng(seed)
    labels = np.zeros(shape, np.int32)
    mask = np.zeros(shape, bool)
    struct = ndi.generate_binary_structure(ndim, ndim)
    planted = wide_planted(shape)
    free = list(range(n_obj - 1))
    ids = {}
    for name, vox, radius, masked in planted:
        k = n_obj - 1 if name == "largest" else free.pop(int(rng.integers(0, len(free))))
        ids[name] = 3 * k + 1
        _paint_in_crop(labels, mask, vox, ids[name], radius, masked, struct)
    for k in free:
        start = [int(rng.integers(0, s)) for s in shape]
        vox = _walk(rng, shape, start, steps, keep_dir)
        for _ in range(branches):
            vox += _walk(rng, shape, vox[int(rng.integers(0, len(vox)))], steps // 3, keep_dir)
        _paint_in_crop(labels, mask, vox, 3 * k + 1, 1, bool(k % 2), struct)
    frangi = unique_frangi(rng, shape)
    fr, lab = frangi.reshape(-1), labels.reshape(-1)
    own = np.flatnonzero(lab == ids["spanning"])
    top, late = own[np.argmax(fr[own])], own[own >= TRIP_8192][-1]
    fr[top], fr[late] = fr[late], fr[top]
    return labels, mask, frangi, ids


WIDE = {"wide_3d": dict(shape=(24, 300, 310), spacing=(0.29, 0.11, 0.11), seed=31, steps=100),
        "wide_2d": dict(shape=(1500, 1500), spacing=(0.107, 0.083), seed=32, steps=320, keep_dir=0.95)}


def seed_rule_scene(shape):
    """labels (int32) and frangi (float32) for the seeding rule, nothing else decides: with an empty mask every label is seeded.  Each
    label is three runs of `run` voxels in raster order -- early, middle, late; in a frame above TRIP_8192 voxels the early runs lie
    below TRIP_2048 and the late ones in the last trip -- whose Frangi values are set by hand.  -> labels, frangi, {case: label}."""
    shape = tuple(shape)
    n = int(np.prod(shape))
    run = 20
    cases = ["tie3_late", "tie3_span", "nan_among_larger", "two_nans", "minus_zero_first", "plus_zero_first", "all_negative", "plus_inf",
             "only_minus_inf", "subnormals", "one_voxel"]
    if n > TRIP_8192:
        bases = (1000, n // 2, TRIP_8192 + 1000)
        assert bases[0] + run * len(cases) < TRIP_2048
    else:
        bases = (0, n // 3, 2 * n // 3)
    assert bases[2] + run * len(cases) <= n and run * len(cases) <= bases[1] - bases[0]
    labels = np.zeros(n, np.int32)
    frangi = np.zeros(n, np.float32)
    rng = np.random.default_rng(n)
    f32 = np.float32
    which = {}
    for j, case in enumerate(cases):
        L = which[case] = 2 * j + 3
        p = np.concatenate([np.arange(b + j * run, b + (j + 1) * run) for b in bases])       # raster order: early, middle, late
        if case == "one_voxel":
            p = p[run + 7:run + 8]
        labels[p] = L
        low = ((rng.permutation(p.size) + 1) / f32(2 * p.size)).astype(f32)                   # all different, in (0, 0.5]
        if case == "tie3_late":
            v = low
            v[[2 * run + 1, 2 * run + 4, 2 * run + 9]] = 0.75
        elif case == "tie3_span":
            v = low
            v[[run - 1, run + 3, 2 * run + 5]] = 0.75                                         # large frame: below TRIP_2048 ... in the last trip
        elif case == "nan_among_larger":
            v = low + f32(10.0)
            v[run + 2] = np.nan
        elif case == "two_nans":
            v = low
            v[run + 1] = np.nan
            v[2 * run + 1] = -np.float32(np.nan)                                              # another bit pattern, the same rank
        elif case in ("minus_zero_first", "plus_zero_first"):
            v = -low
            v[5], v[run + 5] = (-0.0, 0.0) if case == "minus_zero_first" else (0.0, -0.0)
        elif case == "all_negative":
            v = -low - f32(1.0)
            v[2 * run + 6] = -0.5
        elif case == "plus_inf":
            v = low * f32(3e38)
            v[2 * run + 3] = np.inf
        elif case == "only_minus_inf":
            v = np.full(p.size, -np.inf, f32)
        elif case == "subnormals":
            v = ((rng.permutation(p.size).astype(np.int32) - p.size // 2) * 3).astype(np.int32)    # bit patterns of tiny magnitudes
            v = np.where(v < 0, (-v).astype(np.uint32) | np.uint32(0x80000000), v.astype(np.uint32)).astype(np.uint32).view(f32)
            top = int(np.argmax(v))
            v[[top, run + 4]] = v[[run + 4, top]]                                             # the largest away from the label's first voxel
        else:
            v = low
        frangi[p] = v
    return labels.reshape(shape), frangi.reshape(shape), which


SEED_RULE_SMALL, SEED_RULE_LARGE = (3, 5, 70), (24, 300, 310)


def table_growth_frames(shape=(6, 40, 70)):
    """Four frames for one handle: the largest labels are 40, 5000, 40 and 70000, so the per-label table (1024 labels at first) grows
    twice and serves a small frame in between.  Frames 2 and 3 share the ids 3, 7, 12 and 20: 3 and 12 have no mask in frame 2 and one
    in frame 3, 7 and 20 the other way round.  -> list of (labels, mask, frangi)."""
    plans = [([2, 5, 9, 17, 28, 40], 2), ([3, 12, 2600, 5000, 7, 20, 33, 1500], 4), ([7, 20, 3, 12, 33, 40], 2),
             ([4, 900, 1025, 70000, 65536, 30000, 11, 50000], 4)]
    frames = []
    for t, (ids, drop) in enumerate(plans):
        rng = np.random.default_rng([t, 41])
        labels, mask, frangi = walks_scene(rng, shape, n_obj=len(ids), drop=drop)
        lut = np.zeros(len(ids) + 1, np.int32)
        lut[1:] = ids
        frames.append((lut[labels], mask, frangi))
    return frames
