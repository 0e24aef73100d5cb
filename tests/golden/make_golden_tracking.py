"""
Captures tests/golden/tracking/tracking_*.npz (a directory of their own: the Filter cases are every top-level fixture) from the reference's HuMomentTracking (numpy path, device="cpu"):

    python tests/golden/make_golden_tracking.py /path/to/nellie-reference

Each fixture holds the T-stack it was made from (intensity, frangi, distance, marker), the reference's per-frame coordinates,
stats and log-Hu features (rows of all frames, `counts` per frame) and its flow_vector_array.  A seed whose dense costs put a
row's or a column's best and second-best within 2 float16 ulp of each other is replaced by the next one, so that exact
end-to-end equality rests on a margin.
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
import hu_tracking_restatement as rs  # noqa: E402

# name: (shape per frame, T, dtype, spacing (Z,)Y,X, dt, mode, max_dense_pairs, markers per frame, extras)
CASES = {
    "tracking_3d_u16_auto_dense": ((10, 22, 24), 3, np.uint16, (0.1, 0.1, 0.1), 1.0, "auto", int(1e7), (30, 30, 30), {}),
    "tracking_3d_f32_sparse_aniso": ((8, 24, 26), 3, np.float32, (0.3, 0.1, 0.1), 0.7, "sparse", int(1e7), (35, 30, 35), {}),
    "tracking_3d_u16_auto_sparse": ((9, 20, 22), 4, np.uint16, (0.2, 0.1, 0.1), 2.0, "auto", 100, (0, 28, 25, 30), {}),
    "tracking_3d_u16_dense_wrap": ((7, 16, 18), 4, np.uint16, (0.15, 0.1, 0.1), 1.0, "dense", int(1e7), (25, 0, 22, 24),
                                   {"bright": True, "faces": True}),
    "tracking_3d_u8_dense": ((8, 18, 20), 3, np.uint8, (0.1, 0.1, 0.1), 1.0, "dense", int(1e7), (20, 24, 22), {"faces": True}),
    "tracking_2d_u16_dense": ((60, 64), 3, np.uint16, (0.1, 0.1), 0.5, "dense", int(1e7), (40, 45, 40), {"faces": True}),
    "tracking_2d_f32_sparse": ((56, 60), 4, np.float32, (0.12, 0.1), 1.0, "sparse", int(1e7), (40, 0, 38, 42), {}),
    "tracking_2d_u8_auto_sparse": ((50, 52), 3, np.uint8, (0.1, 0.1), 1.0, "auto", 500, (0, 40, 44), {}),
    # float32 intensities of 1000 +- 10 (a camera offset: the variance's sumsq - s^2/c cancels), distances up to 5 (R = 21)
    "tracking_3d_f32_lowcontrast": ((10, 22, 24), 3, np.float32, (0.1, 0.1, 0.1), 1.0, "dense", int(1e7), (30, 28, 32),
                                    {"lowcontrast": True, "dist_hi": 26}),
    # distances up to 15 (R = 61) on a frame thinner than R in z: every ROI is clipped and its padding joins the projections
    "tracking_3d_u16_bigroi": ((9, 28, 30), 3, np.uint16, (0.2, 0.1, 0.1), 1.0, "dense", int(1e7), (8, 7, 8),
                               {"faces": True, "dist_hi": 226}),
    # one marker per frame at distance 30.9 (radius 62, R = 125, the feature kernel's largest tile), the rest small
    "tracking_2d_f32_bigroi_sparse": ((60, 64), 3, np.float32, (0.1, 0.1), 1.0, "sparse", int(1e7), (30, 32, 28),
                                      {"big": 30.9}),
}


def make_stack(shape, T, dtype, n_markers, seed, bright=False, faces=False, lowcontrast=False, dist_hi=10, big=None):
    rng = np.random.default_rng(seed)
    ints, frs, dists, marks = [], [], [], []
    for t in range(T):
        if dtype == np.float32 and lowcontrast:
            im = rng.uniform(990.0, 1010.0, shape).astype(np.float32)
        elif dtype == np.float32:
            im = (rng.gamma(2.0, 300.0, shape) - 150.0).astype(np.float32)          # textured, some negatives
        elif dtype == np.uint8:
            im = rng.integers(0, 256, shape).astype(np.uint8)
        else:
            lo = 40000 if bright else 0
            im = rng.integers(lo, 65536 if bright else 5000, shape).astype(np.uint16)
        im[rng.random(shape) < 0.15] = 0
        fr = (rng.gamma(1.5, 2.0, shape) * (rng.random(shape) < 0.7)).astype(np.float32)
        dist = np.sqrt(rng.integers(0, dist_hi, shape)).astype(np.float32)
        mk = np.zeros(shape, np.uint8)
        n = n_markers[t]
        if n:
            flat = rng.choice(int(np.prod(shape)), size=n, replace=False)
            mk.flat[flat] = 1
            if faces:                                        # markers on every face (clipped ROIs)
                for ax in range(len(shape)):
                    for end in (0, shape[ax] - 1):
                        p = [int(rng.integers(0, s)) for s in shape]
                        p[ax] = end
                        mk[tuple(p)] = 1
            if big is not None:                              # one marker with a large radius, away from the others
                p = tuple(int(rng.integers(1, s - 1)) for s in shape)
                mk[tuple(slice(c - 1, c + 2) for c in p)] = 0
                mk[p] = 1
                dist[p] = big
        ints.append(im); frs.append(fr); dists.append(dist); marks.append(mk)
    return np.stack(ints), np.stack(frs), np.stack(dists), np.stack(marks)


def reference_run(HMT, stack, spacing, dt, mode, max_dense_pairs):
    intensity, frangi, distance, marker = stack
    two_d = intensity.ndim == 3
    tmp = tempfile.mkdtemp()
    paths = {"im_instance_label": "lab", "im_preprocessed": "fr", "im_marker": "mk", "im_distance": "dist",
             "flow_vector_array": os.path.join(tmp, "flow.npy")}
    arrays = {"im": intensity, "lab": np.zeros(intensity.shape, np.int32), "fr": frangi, "mk": marker, "dist": distance}
    axes = "TYX" if two_d else "TZYX"
    dim_res = dict(zip(axes[1:], spacing))
    dim_res["T"] = dt
    im = SimpleNamespace(no_t=False, no_z=two_d, shape=intensity.shape, axes=axes, dim_res=dim_res, pipeline_paths=paths,
                         im_path="im", get_memmap=lambda p: arrays[p])
    tr = HMT(im, device="cpu", mode=mode, max_dense_pairs=max_dense_pairs)
    tr._set_backend("cpu")
    tr._get_t()
    tr._allocate_memory()
    feats = [tr._get_frame_features(t) for t in range(intensity.shape[0])]
    tr._run_hu_tracking()
    return feats, np.load(paths["flow_vector_array"]), tr.max_distance_um


def tight(feats, maxd):
    """a row's or a column's best and second-best dense cost within 2 float16 ulp"""
    for a, b in zip(feats[1:], feats[:-1]):
        if len(a.coords_voxel) == 0 or len(b.coords_voxel) == 0:
            continue
        c = rs.dense_costs(a.coords_phys, b.coords_phys, a.stats, b.stats, a.hu, b.hu, maxd)
        if c is None:
            continue
        c = c.astype(np.float32)
        for m in (c, c.T):
            if m.shape[1] < 2:
                continue
            s = np.sort(m, axis=1)
            fin = np.isfinite(s[:, 0]) & (s[:, 0] <= 1.0)
            ulp = np.spacing(np.abs(s[:, 0]).astype(np.float16)).astype(np.float32)
            if np.any(fin & (s[:, 1] - s[:, 0] <= 2 * ulp)):
                return True
    return False


def dense_roi_path(stack, max_voxels=int(5e7)):
    """the reference's dense ROI path (the one this port follows) holds N * R^d <= max_dense_roi_voxels_cpu in every frame"""
    intensity, _, distance, marker = stack
    for t in range(intensity.shape[0]):
        m = marker[t] > 0
        if m.any():
            R = int(np.ceil((rs._max3(distance[t]) * np.float32(2))[m].max())) * 2 + 1
            if int(m.sum()) * R ** marker[t].ndim > max_voxels:
                return False
    return True


def main():
    make_golden.REF = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else make_golden.REF
    make_golden._import_reference()
    from nellie.tracking.hu_tracking import HuMomentTracking
    for name, (shape, T, dtype, spacing, dt, mode, mdp, nmk, extra) in CASES.items():
        seed = 0
        while True:
            stack = make_stack(shape, T, dtype, nmk, seed, **extra)
            assert dense_roi_path(stack), name
            feats, flow, maxd = reference_run(HuMomentTracking, stack, spacing, dt, mode, mdp)
            if not tight(feats, maxd):
                break
            seed += 1
        nh = 6 if len(shape) == 2 else 18
        out = dict(intensity=stack[0], frangi=stack[1], distance=stack[2], marker=stack[3], spacing=np.asarray(spacing, float),
                   dt=np.float64(dt), mode=np.array(mode), max_dense_pairs=np.int64(mdp), seed=np.int64(seed),
                   counts=np.array([len(f.coords_voxel) for f in feats], np.int64),
                   coords=np.concatenate([f.coords_voxel.reshape(-1, len(shape)) for f in feats]).astype(np.int64),
                   stats=np.concatenate([np.asarray(f.stats, np.float32).reshape(-1, 4) for f in feats]),
                   hu=np.concatenate([np.asarray(f.hu, np.float64).reshape(-1, nh) for f in feats]),
                   flow=flow)
        os.makedirs(os.path.join(HERE, "tracking"), exist_ok=True)
        path = os.path.join(HERE, "tracking", name + ".npz")
        np.savez_compressed(path, **out)
        print(f"{name}: seed {seed}, markers {out['counts'].tolist()}, {len(flow)} rows, {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
