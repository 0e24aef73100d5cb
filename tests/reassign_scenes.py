"""Synthetic scenes for the voxel-reassignment tests and goldens, test infrastructure only: blobs and tubes that drift by a
fractional number of voxels per frame, object ids permuted per frame, branch labels a strict subset of the object voxels, flow
rows [t, pos, vec, cost] at random labelled voxels (vector = the object's drift plus noise, random float32 costs)."""
import numpy as np


def _raster(shape, s, kind, p, size_um, axis_dir, half_len_um):
    grid = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij"), axis=-1)
    rel = (grid - p) * s
    if kind == "tube":
        along = np.clip(rel @ axis_dir, -half_len_um, half_len_um)
        rel = rel - along[..., None] * axis_dir
    return (rel ** 2).sum(axis=-1) <= size_um ** 2


def make_scene(rng, shape, T, spacing, n_obj=6, drift_um=0.16, rows_per_obj=12, noise=0.3, integer_flow=False, appear=False,
               vanish=False, converge=False, empty_t=None, no_flow_t=None, size_um=(0.3, 0.45), x_share=1.0, mismatch=0.5):
    """-> branch (T, ...) int32, obj (T, ...) int32, flow (n, 2 D + 2) float64.  x_share < 1 keeps the ordinary objects in the
    low part of the last axis (`appear` puts its object, which has no flow row, at the far end).  integer_flow: every vector is
    the object's drift rounded to whole voxels, and the drift itself is within `mismatch` voxels of that whole number."""
    s = np.asarray(spacing, np.float64)
    D = len(shape)
    objs = []
    for k in range(n_obj):
        size = rng.uniform(*size_um)
        pad = size / s + 1.0 + 1.5 * T * drift_um / s
        hi = np.asarray(shape, np.float64) - 1 - pad
        hi[-1] = (shape[-1] - 1) * x_share - pad[-1]
        lo = np.minimum(pad, hi)
        u = rng.normal(size=D)
        objs.append(dict(kind="tube" if k % 2 else "blob", p0=rng.uniform(lo, np.maximum(lo, hi)), size=size * (0.6 if k % 2 else 1.0),
                         dir=u / np.linalg.norm(u), half=rng.uniform(0.3, 0.7), drift=rng.uniform(-drift_um, drift_um, D) / s,
                         frames=range(T), flow=True, same_as=k))
    if integer_flow:
        for o in objs:
            o["drift"] = np.round(o["drift"]) + rng.uniform(-mismatch, mismatch, D)
    if vanish:
        objs[0]["frames"] = range(0, T // 2)
    if converge and n_obj >= 2:                          # object 1 runs into object 0 and carries its id from frame 2 on
        a, b = objs[0], objs[1]
        b.update(kind=a["kind"], size=a["size"], dir=a["dir"], half=a["half"])
        off = np.zeros(D)
        off[-2] = 2.0 * a["size"] / s[-2] + 2.0
        b["p0"] = a["p0"] + off
        a["drift"], b["drift"] = off / (2.0 * 2.2), -off / (2.0 * 2.2)
        b["merge_from"] = 2
    if appear:
        p = (np.asarray(shape, np.float64) - 1) / 2.0
        p[-1] = shape[-1] - 1 - 0.4 / s[-1] - 1.0
        objs.append(dict(kind="blob", p0=p, size=0.35, dir=None, half=0.0, drift=np.zeros(D), frames=range(1, T), flow=False,
                         same_as=n_obj))
    K = len(objs)
    branch, obj = np.zeros((T,) + tuple(shape), np.int32), np.zeros((T,) + tuple(shape), np.int32)
    rows = []
    for t in range(T):
        if t == empty_t:
            continue
        perm_o, perm_b = rng.permutation(K) + 1, rng.permutation(K) + 1 + K
        for k, o in enumerate(objs):
            if t not in o["frames"]:
                continue
            p = o["p0"] + t * o["drift"]
            ident = 0 if t >= o.get("merge_from", T + 1) else k
            body = _raster(shape, s, o["kind"], p, o["size"], o["dir"], o["half"])
            core = _raster(shape, s, o["kind"], p, o["size"] * 0.55, o["dir"], o["half"])
            obj[t][body] = perm_o[ident]
            branch[t][body] = 0
            branch[t][core] = perm_b[ident]
            vox = np.argwhere(body)
            if o["flow"] and t < T - 1 and t != no_flow_t and len(vox):
                pick = vox[rng.choice(len(vox), min(rows_per_obj, len(vox)), replace=False)].astype(np.float64)
                if integer_flow:
                    vec = np.tile(np.round(o["drift"]), (len(pick), 1))
                else:
                    vec = o["drift"] + rng.uniform(-noise, noise, pick.shape)
                cost = rng.random(len(pick)).astype(np.float32).astype(np.float64)
                rows.append(np.column_stack([np.full(len(pick), float(t)), pick, vec, cost]))
        branch[t][obj[t] == 0] = 0
    flow = np.concatenate(rows) if rows else np.zeros((0, 2 * D + 2))
    return branch, obj, flow
