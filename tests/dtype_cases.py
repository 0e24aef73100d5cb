"""The dtype matrix of the library's entry points: which element types there are, the values of each type at which a conversion or
a predicate goes wrong, frames that hold those values at the places a kernel's indexing goes wrong, and references that do not rest
on the code under test.  Pure numpy and Python integers; nothing here touches the device."""
from fractions import Fraction

import numpy as np

from nellie_amd import hipnative

ALL = list(hipnative.DTYPE_CODES)                       # iterated, not copied: an eleventh dtype extends every test
HOST_CAST = [np.dtype(np.float16), np.dtype(bool), np.dtype(">u2"), np.dtype(">f4")]      # converted by the binding, not the library
INTEGERS = [d for d in ALL if d.kind in "iu"]
FLOATS = [d for d in ALL if d.kind == "f"]
F32_MAX = float(np.finfo(np.float32).max)


def ids(dtypes):
    return [np.dtype(d).str.strip("<|=").replace(">", "be_") for d in dtypes]


def _int_edges(dtype):
    info = np.iinfo(dtype)
    bits = dtype.itemsize * 8
    vals = [info.min, info.max, 0, 1]
    if dtype.kind == "i":
        vals += [-1]
    if bits >= 32:
        # float32 holds 24 bits: 2**24 + 1 lies halfway and goes down to the even neighbour, 2**24 + 3 halfway and goes up
        ties = [2 ** 24 + 1, 2 ** 24 + 3]
        # the same one binade below the type's maximum (float32 spacing there: 2**(top - 23)), and one either side of each tie
        top = bits - (2 if dtype.kind == "i" else 1)
        half = 2 ** (top - 24)
        for tie in (2 ** top + half, 2 ** top + 3 * half):
            ties += [tie - 1, tie, tie + 1]
        vals += ties + ([-t for t in ties] if dtype.kind == "i" else [])
    if bits == 64:
        vals += [2 ** 53 + 1]
        if dtype.kind == "u":
            # direct conversion gives 2**63 + 2**40; through float64 the 1 is lost first, the tie then goes down to 2**63
            vals += [2 ** 63 + 2 ** 39 + 1, 2 ** 63, 2 ** 63 + 1, 2 ** 64 - 2 ** 39, 2 ** 64 - 2 ** 39 - 1]
        else:
            vals += [2 ** 62 + 2 ** 38 + 1, -(2 ** 62 + 2 ** 38 + 1), -(2 ** 53 + 1)]
    assert all(info.min <= v <= info.max for v in vals)
    return np.array(sorted(set(vals)), dtype=object).astype(dtype)


def _float_edges(dtype):
    fi = np.finfo(dtype)
    t = dtype.type
    tiny = np.nextafter(t(0), t(1))                     # the smallest denormal
    vals = [fi.min, fi.max, t(0), t(1), t(-1), t(-0.0), tiny, -tiny, fi.tiny, t(np.nan), t(np.inf), t(-np.inf)]
    if dtype == np.float64:
        # float32 denormals, underflow to +-0, overflow to +-inf, exact float32 ties (down to even, up to even)
        vals += [1e-40, -1e-40, 1e-46, -1e-46, 3.5e38, -3.5e38, 1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, -(1.0 + 2.0 ** -24),
                 F32_MAX + 2.0 ** 102, np.nextafter(F32_MAX + 2.0 ** 103, 0.0), F32_MAX + 2.0 ** 103,      # below / at the overflow tie
                 2.0 ** -150, np.nextafter(2.0 ** -150, 1.0), 2.0 ** -149 + 2.0 ** -150]                  # ties among the denormals
    return np.array(vals, dtype=dtype)


def edge_values(dtype, finite=False):
    """The values every frame of that dtype must hold.  finite: only those that stay finite in float32."""
    dtype = np.dtype(dtype)
    v = _int_edges(dtype) if dtype.kind in "iu" else _float_edges(dtype)
    if finite and dtype.kind == "f":
        v = v[np.isfinite(v) & (np.abs(v) <= F32_MAX)]
    return v


def random_values(dtype, n, rng, finite=False):
    """Uniformly random bits over the whole range of the type."""
    dtype = np.dtype(dtype)
    v = rng.integers(0, 256, size=n * dtype.itemsize, dtype=np.uint8).view(dtype).copy()
    if finite and dtype.kind == "f":
        bad = ~(np.isfinite(v) & (np.abs(v) <= F32_MAX))
        v[bad] = (rng.standard_normal(int(bad.sum())) * 1000).astype(dtype)
    return v


def anchors(shape):
    """Flat indices of the first voxel, the last voxel of the first row, the first voxel of the last plane and the last voxel."""
    n = int(np.prod(shape))
    plane = int(np.prod(shape[1:]))
    return [0, shape[-1] - 1, n - plane, n - 1]


def frame(dtype, shape, seed, finite=False):
    """Random bits with every edge value somewhere, and edge values (which ones turns with the seed) at the four anchors."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    edges = edge_values(dtype, finite)
    flat = random_values(dtype, n, rng, finite)
    at = anchors(shape)
    free = np.setdiff1d(np.arange(n), at)
    assert len(free) >= len(edges), "frame too small for its edge values"
    flat[rng.choice(free, size=len(edges), replace=False)] = edges
    for j, i in enumerate(at):
        flat[i] = edges[(seed + j) % len(edges)]
    return flat.reshape(shape)


def sparse_frame(dtype, shape, seed, extra=12, finite=False):
    """Zeros with every edge value and `extra` random ones at random places, a 1 in the first and in the last voxel: label, class
    and mask frames, where most voxels are background."""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    vals = np.concatenate([edge_values(dtype, finite), random_values(dtype, extra, rng, finite)])
    flat = np.zeros(n, dtype)
    flat[rng.choice(np.arange(1, n - 1), size=len(vals), replace=False)] = vals
    flat[0] = flat[n - 1] = 1
    return flat.reshape(shape)


def host_cast_frame(dtype, shape, seed):
    """A frame of a dtype the binding converts itself; big-endian ones hold the little-endian frame's values."""
    dtype = np.dtype(dtype)
    if dtype == bool:
        return np.random.default_rng(seed).integers(0, 2, shape).astype(bool)
    if dtype == np.float16:
        f = np.random.default_rng(seed).integers(0, 2 ** 16, shape, dtype=np.uint16).view(np.float16)
        f.reshape(-1)[anchors(shape)] = np.array([np.finfo(np.float16).max, -0.0, np.nextafter(np.float16(0), np.float16(1)), np.nan], np.float16)
        return f
    return frame(dtype.newbyteorder("<"), shape, seed).astype(dtype)


def strided_views(a):
    """(name, non-contiguous array of a's shape and values): every other element of a wider buffer, and Fortran order."""
    wide = np.zeros(a.shape[:-1] + (2 * a.shape[-1],), a.dtype)
    wide[..., ::2] = a
    return [("step2", wide[..., ::2]), ("fortran", np.asfortranarray(a))]


def same_bits(a, b):
    """Equality of bits with every NaN equal to every NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    u = {2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    nan = np.isnan(a)
    return bool(np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(u)[~nan], b.view(u)[~nan]))


# --------------------------------------------------------------------------------------------- exact references
def exact_f32(v):
    """The float32 nearest to the int or Fraction v, ties to even: integer arithmetic only."""
    q = Fraction(v)
    if q == 0:
        return np.float32(0.0)
    sign, q = (1 if q < 0 else 0), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    assert Fraction(2) ** e <= q < Fraction(2) ** (e + 1)
    e = max(e, -126)                                    # the denormals share the smallest normal exponent
    scaled = q / Fraction(2) ** (e - 23)                # in units of the last place
    m = scaled.numerator // scaled.denominator
    rest = scaled - m
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and m % 2 == 1):
        m += 1
    if m == 2 ** 24:
        m, e = 2 ** 23, e + 1
    if e > 127:
        bits = 0x7F800000
    elif m < 2 ** 23:
        bits = m                                        # denormal (or zero)
    else:
        bits = ((e + 127) << 23) | (m - 2 ** 23)
    return np.array([bits | (sign << 31)], np.uint32).view(np.float32)[0]


def exact_f64_then_f32(v):
    """v -> float64 -> float32 for a Python int: what a conversion through double gives."""
    return np.float32(np.float64(float(v)))


def mask_reference(orig, thresh):
    """`orig > thresh` as numpy itself evaluates it."""
    with np.errstate(invalid="ignore", over="ignore"):
        return orig > thresh


THRESHOLD_FORMS = (float, int, np.float32, np.float64, np.int64)


def thresholds(dtype):
    """[(name, threshold)] for an image of that dtype: equal to an element, one step either side of it, and 0.1, which float32
    does not hold; each in every form of THRESHOLD_FORMS that can express it."""
    dtype = np.dtype(dtype)
    out = []
    if dtype.kind in "iu":
        info = np.iinfo(dtype)
        bases = {1, info.max - 1, info.min + 1}
        if dtype.itemsize >= 4:
            bases |= {2 ** 24 + 1}
        if dtype.itemsize == 8:
            bases |= {2 ** 53 + 1, 2 ** 53, (2 ** 63 + 2 ** 39 + 1) if dtype.kind == "u" else 2 ** 62 + 2 ** 38 + 1}
        ints = sorted({b + d for b in bases for d in (-1, 0, 1)} | {info.min - 1, info.max + 1})
        for t in ints:
            out.append((f"int:{t}", int(t)))
            if -2 ** 63 <= t < 2 ** 63:
                out.append((f"i64:{t}", np.int64(t)))
        floats = sorted({float(b) for b in bases})
    else:
        elems = [dtype.type(v) for v in (1.0, -0.0, np.nextafter(dtype.type(0), dtype.type(1)), 1.0 + 3 * 2.0 ** -24 if dtype == np.float64 else 1.5)]
        floats = [float(e) for e in elems]
        for t in (0, 1, -1, 2):
            out += [(f"int:{t}", t), (f"i64:{t}", np.int64(t))]
    for f in floats:
        for name, form in (("float", float), ("f32", np.float32), ("f64", np.float64)):
            c = form(f)
            lo, hi = (np.nextafter(c, form(-np.inf)), np.nextafter(c, form(np.inf))) if form is not float else \
                (float(np.nextafter(f, -np.inf)), float(np.nextafter(f, np.inf)))
            out += [(f"{name}:{float(t)!r}", t) for t in (lo, c, hi)]
    out += [("float:0.1", 0.1), ("f32:0.1", np.float32(0.1)), ("f64:0.1", np.float64(0.1)), ("f64:nan", np.float64(np.nan))]
    return out
