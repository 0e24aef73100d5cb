"""Scenes of the Label path tests (test_label_scenes_cpu.py asserts what each one is built to reach, test_hip_label_paths.py runs
them on the device).  Every builder returns a bool mask and is seeded; numpy only, except `stages`, which restates the pipeline with
scipy.  The run-level Label keeps its runs in scratch of `cap = n // 2` entries: a run set beyond it, at any of the three labellings
of a frame (background for the hole fill, foreground before the area filter, foreground after the majority filter), sends the frame
to the voxel-level kernels -- as do rows of more than 65535 voxels, whose ends do not fit a run's 16-bit fields."""
import numpy as np

THR = np.float32(0.25)
PATH_RUNS, PATH_WIDE, PATH_OVERFLOW, PATH_FORCED = 0, 1, 2, 3       # nl_ctx_info "last_label_path"


def runs(mask):
    """maximal x-runs of a mask"""
    m = np.asarray(mask, bool)
    starts = m.copy()
    starts[..., 1:] &= ~m[..., :-1]
    return int(starts.sum())


def cap(mask):
    return int(np.asarray(mask).size) // 2


def frangi_of(mask, seed=0):
    """what the tests upload: the mask times values above the threshold"""
    return mask.astype(np.float32) * np.random.default_rng(seed).uniform(0.5, 1.0, mask.shape).astype(np.float32)


def scipy_stage_masks(mask, min_area, fill):
    """(mask the first labelling sees, mask after the area and majority filters): labelling.py:484-505 with scipy"""
    from scipy import ndimage as ndi
    m1 = ndi.binary_fill_holes(mask) if fill else np.asarray(mask, bool)
    lab, _ = ndi.label(m1, structure=np.ones((3, 3, 3)))
    areas = np.bincount(lab.ravel())
    keep = areas >= min_area
    keep[0] = False
    m2 = ndi.uniform_filter(keep[lab].astype(np.float32), size=3, mode="reflect") > 0.5
    return m1, m2


def stages(mask, min_area, fill):
    """runs of (the background, the mask before the first labelling, the mask after the majority filter): what the three
    build_components calls of a frame are asked to hold"""
    m1, m2 = scipy_stage_masks(mask, min_area, fill)
    return runs(~np.asarray(mask, bool)), runs(m1), runs(m2)


def scipy_labels(mask, min_area, fill):
    """the whole pipeline with scipy: (int32 labels, count)"""
    from scipy import ndimage as ndi
    _, m2 = scipy_stage_masks(mask, min_area, fill)
    lab, n = ndi.label(m2, structure=np.ones((3, 3, 3)))
    return lab.astype(np.int32), int(n)


def oracle_labels(fr, min_area, fill):
    """the project's oracle on an uploaded frame: int32 labels"""
    from oracle import nellie_oracle as orc
    if fill:
        return orc.get_labels(fr, THR, min_area)[1]
    lab = orc.label26(fr > THR)
    counts = np.bincount(lab.ravel())
    keep = counts >= min_area
    keep[0] = False
    return orc.label26(orc.majority3(keep[lab]))


def expected_path(mask, min_area, fill):
    """the path nl_label_run takes by the capacity rule, from the scipy restatement of the stages"""
    if mask.shape[2] > 65535:
        return PATH_WIDE
    bg, first, last = stages(mask, min_area, fill)
    over = (fill and bg > cap(mask)) or first > cap(mask) or last > cap(mask)
    return PATH_OVERFLOW if over else PATH_RUNS


def ordinary(shape, seed=1):
    """a frame of the kind the suite already labels: Bernoulli noise, a quarter of the capacity"""
    return np.random.default_rng(seed).random(shape) < 0.3


# ------------------------------------------------------------------------------------------------ a, b, c: the capacity
OVERFLOW_FG_SHAPES = ((6, 9, 5), (4, 7, 131), (2, 3, 4097))


def overflow_fg(shape):
    """foreground at every even x of an odd-width frame: (nx + 1) / 2 runs per row, the background (nx - 1) / 2"""
    assert shape[2] % 2 == 1
    m = np.zeros(shape, bool)
    m[..., ::2] = True
    return m


OVERFLOW_BG_CASES = (((12, 20, 9), (3, 3, 2), (5, 5, 5)), ((10, 16, 131), (3, 5, 2), (5, 5, 5)))


def overflow_bg(shape, box_lo, box_size):
    """foreground at every odd x (the background then has the surplus runs) plus a closed hollow box, walls one voxel thick"""
    assert shape[2] % 2 == 1
    m = np.zeros(shape, bool)
    m[..., 1::2] = True
    z, y, x = box_lo
    dz, dy, dx = box_size
    m[z:z + dz, y:y + dy, x:x + dx] = True
    m[z + 1:z + dz - 1, y + 1:y + dy - 1, x + 1:x + dx - 1] = False
    return m


AT_CAPACITY_EVEN_SHAPES = ((4, 6, 8), (3, 5, 130))
AT_CAPACITY_ODD_SHAPE = (4, 7, 131)


def at_capacity_even(shape):
    """even width: foreground and background runs both equal n / 2, every scratch array exactly full"""
    assert shape[2] % 2 == 0
    m = np.zeros(shape, bool)
    m[..., ::2] = True
    return m


def at_capacity_odd(shape, surplus, seed=3):
    """the odd-width comb with interior teeth removed, one voxel each, until runs == n // 2 + surplus"""
    m = overflow_fg(shape)
    rng = np.random.default_rng(seed)
    teeth = np.argwhere(m[..., 1:-1]) + (0, 0, 1)                 # a tooth voxel with neighbours on both sides in x
    k = runs(m) - (m.size // 2 + surplus)
    assert 0 <= k <= len(teeth)
    for z, y, x in teeth[rng.permutation(len(teeth))[:k]]:
        m[z, y, x] = False
    return m


# ------------------------------------------------------------------------------------------------ d: row widths
RULER_WIDTHS = (64, 65, 129, 257, 513, 1025, 2049, 1920, 1921, 4096, 4097, 65535, 65536, 65537)
RULER_WIDTHS_SMALL = tuple(w for w in RULER_WIDTHS if w <= 4097)


def _random_runs(rng, nx):
    row = np.zeros(nx, bool)
    edges = np.cumsum(rng.integers(1, 40, nx // 10 + 8))
    edges = edges[edges < nx]
    for a, b in zip(edges[0::2], edges[1::2]):
        row[a:b] = True
    return row


def ruler(nx, seed=7):
    """(3, 4, nx): runs at the places where the run kernels change over.  The four corner rows carry the marks (they are no
    6-neighbours of the cavity rows), the other rows the walls of the cavities in plane 1, rows 1 and 2."""
    assert nx >= 64
    rng = np.random.default_rng(seed + nx)
    m = np.zeros((3, 4, nx), bool)
    for z in range(3):
        for y in range(4):
            m[z, y] = _random_runs(rng, nx)

    def put(z, y, a, b, value=True):
        a, b = max(a, 0), min(b, nx)
        if a < b:
            m[z, y, a:b] = value
    last = 64 * ((nx - 1) // 64)                                   # the last word boundary below nx
    m[1, 0] = True                                                 # one run [0, nx)
    put(0, 0, nx - 200, nx, False)
    m[0, 0, max(nx - 200, 0)::2] = True                            # a comb over the last 200 voxels
    for b in sorted({64, last} - {0}):
        for z, y in ((0, 3), (2, 3), (2, 0)):
            put(z, y, b - 24, b + 24, False)
        put(0, 3, b - 20, b)                                       # ends at b - 1
        put(2, 3, b, b + 15)                                       # starts at b
        put(2, 0, b - 10, b + 10)                                  # crosses b - 1 | b
    put(2, 3, 0, 3, False), put(2, 3, nx - 3, nx, False)
    m[2, 3, 0] = m[2, 3, nx - 1] = True                            # single voxels at both ends
    walls = ((0, 1), (0, 2), (2, 1), (2, 2), (1, 0), (1, 3), (1, 1), (1, 2))
    for z, y in walls:
        put(z, y, 58, 73)
        put(z, y, nx - 14, nx)
    put(1, 1, 60, 71, False), put(1, 2, 60, 71, False)             # closed across x = 60..70 (open where the frame ends before 71)
    put(1, 1, nx - 10, nx - 1, False)                              # closed, ends at x = nx - 2
    put(1, 2, nx - 1, nx, False)                                   # open through x = nx - 1: not a hole
    return m


# ------------------------------------------------------------------------------------------------ e: topology
def comb_last_plane(shape=(9, 68, 21)):
    """teeth three rows thick, three apart, that meet only in the last plane"""
    m = np.zeros(shape, bool)
    m[:, (np.arange(shape[1]) % 6) < 3, :] = True
    m[-1] = True
    return m


def comb_last_row(shape=(15, 66, 21)):
    """teeth three planes thick that meet only in the last row of every plane"""
    m = np.zeros(shape, bool)
    m[(np.arange(shape[0]) % 6) < 3] = True
    m[:, -1, :] = True
    return m


def serpentine(shape=(7, 65, 24)):
    """one 1-voxel path through every other row of every other plane, a block at each end: one component, or the area is wrong"""
    nz, ny, nx = shape
    assert nz % 4 == 3 and ny % 2 == 1 and nx > 12
    m = np.zeros(shape, bool)
    k = 0
    for p, z in enumerate(range(0, nz, 2)):
        ys = list(range(0, ny, 2))
        if p % 2:
            ys.reverse()
        for j, y in enumerate(ys):
            m[z, y, 8:] = True
            end = nx - 1 if k % 2 == 0 else 8
            if j + 1 < len(ys):
                m[z, (y + ys[j + 1]) // 2, end] = True             # to the next row of the plane
            elif z + 2 < nz:
                m[z + 1, y, end] = True                            # to the next plane
            k += 1
    assert k % 2 == 0                                              # the path ends at (nz - 1, 0, 8)
    m[0:3, 0:5, 0:5] = True
    m[0, 0, 5:8] = True
    m[nz - 3:nz, 0:5, 0:5] = True
    m[nz - 1, 0, 5:8] = True
    return m


def nested_shells(shape=(20, 66, 22)):
    """a shell inside the cavity of a shell, walls two voxels thick, across rows 31 | 32"""
    m = np.zeros(shape, bool)
    m[1:19, 24:42, 2:20] = True
    m[3:17, 26:40, 4:18] = False
    m[5:15, 28:38, 6:16] = True
    m[7:13, 30:36, 8:14] = False
    return m


def pierced(shape=(12, 66, 30)):
    """two blocks with a 3 x 3 x 3 cavity: one reached by a tunnel that ends diagonally next to the cavity (still a hole), one by a
    face-connected 1-voxel tunnel from the frame's x = 0 face (not a hole)"""
    m = np.zeros(shape, bool)
    for y0, diagonal in ((27, True), (48, False)):
        m[2:11, y0:y0 + 9, 0:12] = True
        m[5:8, y0 + 3:y0 + 6, 6:9] = False                        # the cavity
        if diagonal:
            m[4, y0 + 2, 0:6] = False                             # ends at (4, y0 + 2, 5): a diagonal neighbour of (5, y0 + 3, 6)
        else:
            m[6, y0 + 4, 0:6] = False                             # ends at (6, y0 + 4, 5): a face neighbour of (6, y0 + 4, 6)
    return m


def face_boxes(shape=(30, 66, 30)):
    """per frame face: a box whose missing wall lies on the face (open: not filled), beside the same box one voxel inside (filled)"""
    m = np.zeros(shape, bool)
    spots = {0: ((27, 13), (35, 13)), 1: ((9, 13), (17, 13)), 2: ((9, 30), (17, 30))}      # (open, closed) in the other two axes
    for axis in range(3):
        others = [a for a in range(3) if a != axis]
        for high in (False, True):
            for is_open, spot in zip((True, False), spots[axis]):
                lo, hi = [0, 0, 0], [0, 0, 0]
                for a, s in zip(others, spot):
                    lo[a], hi[a] = s, s + 5
                n = shape[axis]
                if is_open:
                    lo[axis], hi[axis] = (n - 4, n + 1) if high else (-1, 4)
                else:
                    lo[axis], hi[axis] = (n - 5, n) if high else (0, 5)
                sl = tuple(slice(max(a, 0), min(b, s)) for a, b, s in zip(lo, hi, shape))
                cav = tuple(slice(max(a + 1, 0), min(b - 1, s)) for a, b, s in zip(lo, hi, shape))
                m[sl] = True
                m[cav] = False
    return m


def fan(shape=(9, 66, 24)):
    """a sheet (planes 3..5, one component per plane) over five bars and under five bars: a component of plane 3 meets five
    components of plane 2, and five components of plane 6 meet one of plane 5.  The sheet crosses rows 31 | 32."""
    m = np.zeros(shape, bool)
    bars = (np.arange(shape[1]) % 14) < 3
    bars[:2] = False
    m[0:3, bars, 2:-2] = True
    m[3:6, 2:-2, 2:-2] = True
    m[6:9, bars, 2:-2] = True
    return m


TOPOLOGY = {"comb_last_plane": comb_last_plane, "comb_last_row": comb_last_row, "serpentine": serpentine,
            "nested_shells": nested_shells, "pierced": pierced, "face_boxes": face_boxes, "fan": fan}


# ------------------------------------------------------------------------------------------------ f: many small objects
SPECKS_MIN_AREA = 40
SPECKS_SLAB_ROWS = tuple(range(2, 60, 6))      # ten slabs: their runs lie scattered among the specks' runs, whose roots fill the table


def specks(shape=(8, 66, 260), seed=13):
    """isolated objects of 1, 2 and 3 voxels on a lattice (x >= 16), two of them across adjacent rows, and in x < 14 ten slabs of
    SPECKS_MIN_AREA - 1, SPECKS_MIN_AREA and SPECKS_MIN_AREA + 1 voxels over two planes each.  Nothing else survives the majority
    filter: a slab whose area was summed wrongly -- its runs mostly miss rl_area_kernel's full table -- shows in the labels."""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    m = np.zeros(shape, bool)
    for z in range(0, nz, 2):
        for y in range(0, ny - 1, 3):
            for x in range(16, nx - 1, 4):
                kind = rng.integers(1, 4)
                m[z, y, x] = True
                if kind >= 2:
                    m[z, y + 1, x] = True
                if kind == 3:
                    m[z, y, x + 1] = True
    for k, y0 in enumerate(SPECKS_SLAB_ROWS):                      # 2 x 4 x 5 = 40 voxels, one fewer, one more, in turn
        m[3:5, y0:y0 + 4, 4:9] = True
        if k % 3 == 0:
            m[3, y0, 4] = False
        if k % 3 == 2:
            m[3, y0, 9] = True
    return m


def speck_window_components(mask, window=4096):
    """distinct components among the first `window` runs, in raster order"""
    from scipy import ndimage as ndi
    lab, _ = ndi.label(mask, structure=np.ones((3, 3, 3)))
    starts = mask.copy()
    starts[..., 1:] &= ~mask[..., :-1]
    return int(np.unique(lab[starts][:window]).size)


def critical_min_areas(mask):
    """(1, A, A + 1) with A the largest component's area, with and without the hole fill: at A it stays, at A + 1 it goes -- a union-find that splits it shows"""
    from scipy import ndimage as ndi
    out = {1}
    for fill in (True, False):
        m1 = ndi.binary_fill_holes(mask) if fill else mask
        lab, _ = ndi.label(m1, structure=np.ones((3, 3, 3)))
        a = int(np.bincount(lab.ravel())[1:].max())
        out |= {a, a + 1}
    return tuple(sorted(out))


# ------------------------------------------------------------------------------------------------ the case lists
def capacity_cases():
    """(name, mask, min_areas, expected path, stage that overflows or None) of groups a, b, c"""
    out = []
    for shape in OVERFLOW_FG_SHAPES:
        out.append(("overflow_fg-%dx%dx%d" % shape, overflow_fg(shape), (1, 2, 3, 5), PATH_OVERFLOW, "first labelling"))
    for shape, lo, size in OVERFLOW_BG_CASES:
        out.append(("overflow_bg-%dx%dx%d" % shape, overflow_bg(shape, lo, size), (1, 2, 3, 5), None, "hole fill"))
    for shape in AT_CAPACITY_EVEN_SHAPES:
        out.append(("at_capacity_even-%dx%dx%d" % shape, at_capacity_even(shape), (1, 2, 3, 5), PATH_RUNS, None))
    out.append(("at_capacity_odd+1", at_capacity_odd(AT_CAPACITY_ODD_SHAPE, 1), (1, 5), PATH_OVERFLOW, "first labelling"))
    out.append(("at_capacity_odd+0", at_capacity_odd(AT_CAPACITY_ODD_SHAPE, 0), (1, 5), PATH_RUNS, None))
    return out


def topology_cases():
    """(name, mask, min_areas) of groups e and f; every one stays on the run-level path"""
    out = [(name, build(), critical_min_areas(build())) for name, build in TOPOLOGY.items()]
    out.append(("specks", specks(), (1, 2, 3, SPECKS_MIN_AREA, SPECKS_MIN_AREA + 1)))
    return out
