"""The 3-D thinning of Lee, Kashyap & Chu (1994) as skimage 0.18.3's `skeletonize` runs it on a volume, restated in numpy / Python:
the sequential form, and the round-parallel form the HIP engine runs (csrc/thin.inc).  tests/golden/make_golden_thinning.py holds both
against skimage voxel for voxel before it records a fixture; tests/test_thinning_cpu.py holds them against the fixtures.

Axes are (z, y, x); outside the frame is background.  The 3x3x3 neighbourhood of a voxel is a 27-bit word, bit
(dz + 1) * 9 + (dy + 1) * 3 + (dx + 1); bit 13 is the voxel itself.

    unchanged = 0
    while unchanged < len(DIRS):
        unchanged = 0
        for d in DIRS:
            C = the voxels that are set, whose neighbour at d is background, that are no endpoint, Euler-invariant and simple --
                all judged on the image as the sub-iteration finds it -- in raster order
            for v in C: if v is (still) simple: delete it           # the component test alone, on the image as it stands by then
            if nothing was deleted: unchanged += 1

A frame of one plane (nz == 1) is skimage's 2-D case: DIRS is then its first four entries only, and the loop ends when all four leave
the image unchanged.
"""
import functools
import itertools

import numpy as np

DIRS = ((0, -1, 0), (0, 1, 0), (0, 0, 1), (0, 0, -1), (1, 0, 0), (-1, 0, 0))
OFFSETS = tuple(itertools.product((-1, 0, 1), repeat=3))              # bit k <-> OFFSETS[k]
CENTRE = 13
NEIGHBOURS = (1 << 27) - 1 - (1 << CENTRE)
# 26-adjacency inside the block, the centre left out
ADJ = tuple(sum(1 << j for j, q in enumerate(OFFSETS) if j != k and j != CENTRE and max(abs(a - b) for a, b in zip(p, q)) <= 1)
            if k != CENTRE else 0 for k, p in enumerate(OFFSETS))
# the cells of the centre cube's boundary: the cell at offset o (1 non-zero component: a face, 2: an edge, 3: a vertex) also belongs to
# the neighbours whose offset is o with some components zeroed
CELLS = tuple((-1 if sum(map(abs, o)) == 2 else 1,
               sum(1 << j for j, q in enumerate(OFFSETS) if j != CENTRE and all(b in (0, a) for a, b in zip(o, q))))
              for k, o in enumerate(OFFSETS) if k != CENTRE)


def popcount(words):
    w = np.asarray(words, np.uint32).copy()
    n = np.zeros(w.shape, np.int32)
    while w.any():
        n += (w & 1).astype(np.int32)
        w >>= 1
    return n


def is_endpoint(word):
    """The centre and exactly one neighbour."""
    return bin(int(word)).count("1") == 2


@functools.lru_cache(maxsize=None)
def simple(word):
    """The set neighbours, centre excluded, form at most one 26-connected component inside the block."""
    mask = int(word) & NEIGHBOURS
    if not mask:
        return True
    reached = mask & -mask
    while True:
        grow = reached
        for k in range(27):
            if reached >> k & 1:
                grow |= ADJ[k] & mask
        if grow == reached:
            return reached == mask
        reached = grow


def _euler_characteristic(voxels):
    """Vertices - edges + faces - cubes of the union of closed unit cubes: a cell is the set of doubled coordinates of its centre."""
    cells = set()
    for z, y, x in voxels:
        for dz, dy, dx in OFFSETS:
            cells.add((2 * z + dz, 2 * y + dy, 2 * x + dx))
    chi = 0
    for c in cells:
        dim = sum(1 for v in c if v % 2 == 0)                       # even coordinate: the cell extends along that axis
        chi += -1 if dim % 2 else 1
    return chi


@functools.lru_cache(maxsize=None)
def euler_invariant(word):
    """Removing the centre leaves the Euler characteristic of the block's cell complex unchanged (by the definition)."""
    word = int(word)
    vox = [o for k, o in enumerate(OFFSETS) if word >> k & 1 and k != CENTRE]
    return _euler_characteristic(vox + [(0, 0, 0)]) == _euler_characteristic(vox)


def simple_v(words):
    mask = np.asarray(words, np.uint32) & np.uint32(NEIGHBOURS)
    reached = mask & (~mask + np.uint32(1))
    while True:
        grow = reached.copy()
        for k in range(27):
            if k != CENTRE:
                grow |= np.where(reached >> np.uint32(k) & np.uint32(1), np.uint32(ADJ[k]), np.uint32(0)) & mask
        if np.array_equal(grow, reached):
            return reached == mask
        reached = grow


def euler_invariant_v(words):
    """The same quantity cell by cell: the centre cube brings its own cube (-1) and every boundary cell no neighbour already has."""
    w = np.asarray(words, np.uint32)
    delta = np.full(w.shape, -1, np.int32)
    for sign, sharers in CELLS:
        delta += sign * ((w & np.uint32(sharers)) == 0)
    return delta == 0


def words_at(padded, coords):
    """27-bit neighbourhood words of the voxels `coords` (k, 3; unpadded coordinates) of a volume padded by one."""
    z, y, x = (coords[:, a] + 1 for a in range(3))
    w = np.zeros(len(coords), np.uint32)
    for k, (dz, dy, dx) in enumerate(OFFSETS):
        w |= padded[z + dz, y + dy, x + dx].astype(np.uint32) << np.uint32(k)
    return w


def candidates(padded, d):
    """Step (1) of a sub-iteration, in raster order (np.argwhere's)."""
    inner = padded[1:-1, 1:-1, 1:-1]
    nb = padded[1 + d[0]:padded.shape[0] - 1 + d[0], 1 + d[1]:padded.shape[1] - 1 + d[1], 1 + d[2]:padded.shape[2] - 1 + d[2]]
    c = np.argwhere(inner & ~nb)
    if not len(c):
        return c
    w = words_at(padded, c)
    keep = popcount(w) != 2
    keep[keep] &= euler_invariant_v(w[keep])
    keep[keep] &= simple_v(w[keep])
    return c[keep]


def _prepare(mask):
    """-> the volume padded by one, and the directions of a frame of this shape."""
    mask = np.asarray(mask)
    if mask.ndim != 3:
        raise ValueError("the restatement is of the 3-D thinning")
    return np.pad(mask != 0, 1), DIRS[:4] if mask.shape[0] == 1 else DIRS


def thin_sequential(mask):
    """-> (skeleton bool, stats): the algorithm as written above."""
    p, dirs = _prepare(mask)
    stats = dict(outer=0, subiters=0, candidates=0, removed=0, max_candidates=0)
    unchanged = 0
    while unchanged < len(dirs):
        unchanged = 0
        stats["outer"] += 1
        for d in dirs:
            stats["subiters"] += 1
            cand = candidates(p, d)
            stats["candidates"] += len(cand)
            stats["max_candidates"] = max(stats["max_candidates"], len(cand))
            removed = 0
            for z, y, x in cand + 1:
                word = 0
                block = p[z - 1:z + 2, y - 1:y + 2, x - 1:x + 2].ravel()
                for k in np.flatnonzero(block):
                    word |= 1 << int(k)
                if simple(word):
                    p[z, y, x] = False
                    removed += 1
            stats["removed"] += removed
            unchanged += removed == 0
    return p[1:-1, 1:-1, 1:-1].copy(), stats


# the 13 neighbours that precede a voxel in raster order
PRECEDING = tuple(o for o in OFFSETS if o < (0, 0, 0))


def thin_rounds(mask):
    """-> (skeleton bool, stats): the re-check in rounds.  A candidate is ready when none of the 13 neighbours that precede it in raster
    order is an undecided candidate; all ready candidates of a round decide at once on the image the earlier rounds left.
    stats adds `rounds` (summed over the thinning) and `max_rounds` (of one sub-iteration); `max_candidates` is the longest list C."""
    p, dirs = _prepare(mask)
    stats = dict(outer=0, subiters=0, candidates=0, removed=0, max_candidates=0, rounds=0, max_rounds=0)
    undecided = np.zeros(p.shape, bool)
    unchanged = 0
    while unchanged < len(dirs):
        unchanged = 0
        stats["outer"] += 1
        for d in dirs:
            stats["subiters"] += 1
            todo = candidates(p, d)
            stats["candidates"] += len(todo)
            stats["max_candidates"] = max(stats["max_candidates"], len(todo))
            undecided[tuple((todo + 1).T)] = True
            removed = rounds = 0
            while len(todo):
                rounds += 1
                z, y, x = (todo[:, a] + 1 for a in range(3))
                ready = np.ones(len(todo), bool)
                for dz, dy, dx in PRECEDING:
                    ready &= ~undecided[z + dz, y + dy, x + dx]
                now = todo[ready]
                gone = now[simple_v(words_at(p, now))]
                p[tuple((gone + 1).T)] = False
                undecided[tuple((now + 1).T)] = False
                removed += len(gone)
                todo = todo[~ready]
            stats["rounds"] += rounds
            stats["max_rounds"] = max(stats["max_rounds"], rounds)
            stats["removed"] += removed
            unchanged += removed == 0
    return p[1:-1, 1:-1, 1:-1].copy(), stats


def all_words_up_to(k_max):
    """Every neighbourhood with the centre set and at most k_max set neighbours."""
    bits = [k for k in range(27) if k != CENTRE]
    out = []
    for k in range(k_max + 1):
        for combo in itertools.combinations(bits, k):
            out.append((1 << CENTRE) | sum(1 << b for b in combo))
    return np.array(out, np.uint32)
