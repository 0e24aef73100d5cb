"""
Captures tests/golden/flow/flow_*.npz from the reference's FlowInterpolator (cKDTree on the CPU):

    python tests/golden/make_golden_flow.py /path/to/nellie-reference

Each fixture holds a flow_vector_array (float64 rows [t, (z,) y, x, (vz,) vy, vx, cost]), spacing, dt, max_distance_um, the
query coordinates, t, the direction and what the reference's interpolate_coord returned (`ref`, shape (0, D) included); the
track fixtures hold start / end frames and the reference's tracks and frame_num instead.  Spacings are not round, and a seed
for which any (query, row) pair has a squared distance within 1e-9 relative of r*r is replaced by the next one (asserted), so
that membership never rests on cKDTree's node pruning.
"""
import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402
import flow_interpolation_restatement as rs  # noqa: E402

ISO, ANISO, ANISO2, ISO_2D, ANISO_2D = (0.107,) * 3, (0.29, 0.0973, 0.0973), (0.211, 0.083, 0.083), (0.0973, 0.0973), (0.107, 0.083)

# name: shape, spacing, dt, max_distance_um, rows per frame, forward, t, queries, extras
CASES = {
    "flow_3d_iso_forward": dict(shape=(12, 40, 40), spacing=ISO, rows=150, forward=True, t=1, queries="mask"),
    "flow_3d_iso_backward": dict(shape=(12, 40, 40), spacing=ISO, rows=150, forward=False, t=2, queries="mask"),
    "flow_3d_aniso_forward": dict(shape=(8, 44, 40), spacing=ANISO, rows=140, forward=True, t=0, queries="mask"),
    "flow_3d_aniso_backward": dict(shape=(10, 36, 44), spacing=ANISO2, rows=160, forward=False, t=1, queries="mask"),
    "flow_2d_forward": dict(shape=(70, 64), spacing=ISO_2D, rows=120, forward=True, t=1, queries="mask"),
    "flow_2d_backward": dict(shape=(64, 72), spacing=ANISO_2D, rows=130, forward=False, t=1, queries="mask"),
    "flow_3d_t_without_rows": dict(shape=(8, 24, 24), spacing=ISO, rows=60, forward=True, t=2, queries="mask", empty_t=2),
    "flow_2d_t_without_rows_backward": dict(shape=(40, 40), spacing=ISO_2D, rows=50, forward=False, t=3, queries="mask", empty_t=2),
    "flow_3d_marker_queries": dict(shape=(10, 32, 32), spacing=ISO, rows=120, forward=True, t=1, queries="markers"),
    "flow_2d_marker_queries_backward": dict(shape=(60, 60), spacing=ISO_2D, rows=100, forward=False, t=2, queries="markers"),
    "flow_3d_wide_radius": dict(shape=(12, 36, 36), spacing=ANISO, rows=150, forward=True, t=1, queries="mask", dt=1.7),
    "flow_3d_max_distance_1um": dict(shape=(10, 30, 30), spacing=ISO, rows=60, forward=False, t=1, queries="mask", maxd=1.0),
    "flow_3d_empty_queries": dict(shape=(8, 24, 24), spacing=ISO, rows=60, forward=True, t=1, queries="empty"),
    "flow_3d_max_k_1": dict(shape=(16, 60, 60), spacing=ISO, rows=8, forward=True, t=1, queries="mask", separated=True),
    "flow_3d_nan_rows": dict(shape=(10, 32, 32), spacing=ANISO2, rows=120, forward=True, t=1, queries="mask", nan_rows=True),
    "flow_3d_fractional": dict(shape=(10, 32, 32), spacing=ISO, rows=120, forward=False, t=1, queries="fractional"),
    "flow_3d_tracks": dict(shape=(10, 28, 28), spacing=ISO, rows=260, tracks=True, maxd=1.0),
    "flow_2d_tracks": dict(shape=(48, 52), spacing=ANISO_2D, rows=220, tracks=True, maxd=1.0),
}
T = 4


def make_flow(rng, shape, rows, empty_t=None, separated=False, r=0.5, spacing=None, vmax=4):
    """rows of T - 1 frame pairs: random integer positions, vectors within +-vmax voxels, float32 costs in [0, 1]; a fifth of
    the rows are repeated with another vector and cost (one marker as a row- and as a column-based candidate), and two rows
    share one position and one vector"""
    D = len(shape)
    out = []
    for t in range(T - 1):
        if t == empty_t:
            continue
        if separated:                                  # no two rows within 2 r of each other, in either direction
            pos = []
            while len(pos) < rows:
                p = np.array([rng.integers(0, s) for s in shape], float)
                if all(np.sqrt((((p - q) * spacing) ** 2).sum()) > 2.2 * r for q in pos):
                    pos.append(p)
            pos = np.array(pos)
        else:
            pos = np.column_stack([rng.integers(0, s, rows) for s in shape]).astype(float)
        vec = rng.integers(-vmax, vmax + 1, (rows, D)).astype(float)
        cost = rng.random(rows).astype(np.float32).astype(float)
        if not separated:
            dup = rng.choice(rows, rows // 5, replace=False)
            pos = np.concatenate([pos, pos[dup], pos[:1]])
            vec = np.concatenate([vec, rng.integers(-vmax, vmax + 1, (len(dup), D)).astype(float), vec[:1]])
            cost = np.concatenate([cost, rng.random(len(dup)).astype(np.float32).astype(float), rng.random(1).astype(np.float32).astype(float)])
        out.append(np.column_stack([np.full(len(pos), float(t)), pos, vec, cost]))
    return np.concatenate(out)


def make_queries(rng, kind, shape, flow, t, forward, nan_rows=False, first_near=False):
    D = len(shape)
    if kind == "empty":
        return np.zeros((0, D))
    if kind == "markers":                              # every check coordinate itself (d == 0, repeated rows included) and some voxels
        _, cc = rs.select_rows(flow, t, forward, D)
        extra = np.argwhere(rng.random(shape) < 0.02).astype(float)
        return np.concatenate([cc, extra])
    if kind == "fractional":
        n = 3000
        return np.column_stack([rng.uniform(-1.0, s, n) for s in shape])
    q = np.argwhere(rng.random(shape) < (0.15 if D == 3 else 0.6)).astype(float)
    if first_near:                                     # row 0 has a neighbour: the one row the reference fills when max_k == 1
        q[0] = rs.select_rows(flow, t, forward, D)[1][0] + 1.0
    if nan_rows:                                       # four NaN rows; the array ends in rows that have neighbours (check coordinates),
        q = np.concatenate([q, rs.select_rows(flow, t, forward, D)[1][:6]])      # the ones the reference then leaves NaN
        q[[0, 5, len(q) // 2, len(q) - 40]] = np.nan
    return q


def reference_im(flow, shape, spacing, dt):
    D = len(shape)
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "flow.npy")
    np.save(path, flow)
    axes = "TYX" if D == 2 else "TZYX"
    dim_res = dict(zip(axes[1:], spacing))
    dim_res["T"] = dt
    stack = np.zeros((T,) + tuple(shape), np.uint8)
    return SimpleNamespace(no_t=False, no_z=D == 2, shape=stack.shape, axes=axes, dim_res=dim_res, im_path="im",
                           pipeline_paths={"flow_vector_array": path}, get_memmap=lambda p: stack)


def main():
    make_golden.REF = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else make_golden.REF
    make_golden._import_reference()
    from nellie.tracking import flow_interpolation as ref
    os.makedirs(os.path.join(HERE, "flow"), exist_ok=True)
    for name, case in CASES.items():
        shape, spacing = case["shape"], case["spacing"]
        dt, maxd = case.get("dt", 1.0), case.get("maxd", 0.5)
        r = max(maxd * dt, 0.5)
        seed = 0
        while True:
            rng = np.random.default_rng([seed, len(name)])
            flow = make_flow(rng, shape, case["rows"], case.get("empty_t"), case.get("separated", False), r, spacing, case.get("vmax", 4))
            im = reference_im(flow, shape, spacing, dt)
            out = dict(flow=flow, spacing=np.asarray(spacing, float), dt=np.float64(dt), max_distance_um=np.float64(maxd),
                       seed=np.int64(seed))
            if case.get("tracks"):
                start = np.argwhere(rng.random(shape) < (0.03 if len(shape) == 3 else 0.1)).astype(float)
                far = np.full((5, len(shape)), 500.0)                   # lost at once; at the end, where the reference's loop over the
                start = np.concatenate([start, far])                    # good rows is not disturbed by NaN rows
                margin = np.inf
                for fwd in (True, False):
                    a, b = (0, 3) if fwd else (3, 1)
                    c_ref, c_rs = start.copy(), start.copy()
                    fn = ref.interpolate_all_forward if fwd else ref.interpolate_all_backward
                    tracks, props = fn(c_ref, a, b, im, min_track_num=7, max_distance_um=maxd)
                    _, _, m = rs.interpolate_all(flow, spacing, r, c_rs, a, b, fwd, min_track_num=7)
                    margin = min(margin, m)
                    # a coordinate lost in the middle of the array makes the reference drop the last good rows of every later
                    # frame (its loop over the good rows): such a seed is not a statement of the intent and is replaced
                    if np.isnan(c_ref[:-5]).any() or not np.isnan(c_ref[-5:]).all():
                        margin = -1.0
                    key = "forward" if fwd else "backward"
                    out.update({f"tracks_{key}": np.asarray(tracks, float), f"frame_num_{key}": np.asarray(props["frame_num"], np.int64),
                                f"coords_{key}": c_ref, f"range_{key}": np.asarray([a, b], np.int64)})
                out["start"] = start
                info = f"{len(start)} coordinates, {len(out['tracks_forward'])} + {len(out['tracks_backward'])} track rows"
            else:
                q = make_queries(rng, case["queries"], shape, flow, case["t"], case["forward"], case.get("nan_rows", False), case.get("separated", False))
                fi = ref.FlowInterpolator(im, max_distance_um=maxd, forward=case["forward"])
                assert fi.max_distance_um == r
                res = np.asarray(fi.interpolate_coord(q.copy(), case["t"]), float)
                _, k, _, margin = rs.interpolate_coord(flow, spacing, r, q, case["t"], case["forward"])
                out.update(queries=q, t=np.int64(case["t"]), forward=np.bool_(case["forward"]), ref=res.reshape(-1, len(shape)))
                info = f"{len(q)} queries, {int((k > 0).sum())} with neighbours, max k {int(k.max(initial=0))}, ref {res.shape}"
            if margin > 1e-9:
                break
            seed += 1
        assert margin > 1e-9, name                      # no query of the fixture has a neighbour on the radius
        out["margin"] = np.float64(margin)
        path = os.path.join(HERE, "flow", name + ".npz")
        np.savez_compressed(path, **out)
        print(f"{name}: seed {seed}, {len(flow)} flow rows, {info}, margin {margin:.3g}, {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
