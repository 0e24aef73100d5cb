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
