"""One frame of the voxel level of the hierarchy at 128 x 512 x 512 (nellie_amd/synthetic.py): labelled voxels, nodes, device time
per part (load and compaction, flow, pivot, motility, node assignment) and the wall time of the frame.

    python tools/bench_voxels.py [--shape 128 512 512] [--rows 20000] [--repeat 5]

The scene is that of tools/bench_reassign.py: the voxels of a synthetic volume above 130 are components (ids by 32-voxel blocks),
those above 170 branches; every 40th branch voxel is a node whose radius is 1 .. 4 voxels.  T = 3 with the same labels in every
frame and flow rows at random labelled voxels of frames 0 and 1, so the measured frame (t = 1) has both directions.
"""
import argparse
import json
import os
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def make_frame(shape, rows, seed=4567):
    from nellie_amd.synthetic import make_volume
    vol = make_volume(shape, seed)
    zz, yy, xx = np.meshgrid(*[np.arange(n) // 32 for n in shape], indexing="ij", sparse=True)
    ids = (1 + zz * 10007 + yy * 101 + xx).astype(np.int32)
    comp = np.where(vol > 130, ids, 0).astype(np.int32)
    branch = np.where(vol > 170, ids + 5, 0).astype(np.int32)
    rng = np.random.default_rng(seed)
    core = np.flatnonzero(branch.ravel() > 0)[::40]
    pixel_class = np.zeros(shape, np.uint8)
    distance = np.zeros(shape, np.float32)
    pixel_class.ravel()[core] = 2
    distance.ravel()[core] = rng.uniform(1.0, 4.0, len(core)).astype(np.float32)
    vox = np.argwhere(comp > 0)
    flow = []
    for t in range(2):
        pos = vox[rng.choice(len(vox), min(rows, len(vox)), replace=False)].astype(np.float64)
        vec = np.asarray((1.0, 2.0, -1.0)) + rng.uniform(-0.3, 0.3, pos.shape)
        flow.append(np.column_stack([np.full(len(pos), float(t)), pos, vec, rng.random(len(pos)).astype(np.float32)]))
    struct = (vol.astype(np.float32) / np.float32(255.0)) * (comp > 0)
    return vol, struct, comp, branch, pixel_class, distance, np.concatenate(flow)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=(128, 512, 512))
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    from nellie_amd import build, hipnative
    from nellie_amd.feature_extraction import Voxels
    from nellie_amd.tracking.flow_interpolation import FlowInterpolator
    build.build(verbose=False)
    shape = tuple(a.shape)
    vol, struct, comp, branch, pixel_class, distance, flow = make_frame(shape, a.rows)
    T, t = 3, 1
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "flow.npy")
        np.save(path, flow)
        im = SimpleNamespace(no_t=False, no_z=False, shape=(T,) + shape, axes="TZYX", dim_res=dict(Z=0.29, Y=0.0973, X=0.0973, T=1.0), im_path="im",
                             pipeline_paths={"flow_vector_array": path}, get_memmap=lambda p, read_mode="r+": np.zeros((T, 4, 4, 4), np.uint8),
                             file_info=SimpleNamespace(filename_no_ext="bench"))
        stack = lambda x: [x] * T   # noqa: E731
        h = SimpleNamespace(im_info=im, num_t=T, spacing=(0.29, 0.0973, 0.0973), viewer=None, label_components=stack(comp), label_branches=stack(branch),
                            im_raw=stack(vol), im_struct=stack(struct), im_pixel_class=stack(pixel_class), im_distance=stack(distance),
                            skip_nodes=False, enable_motility=True, flow_interpolator_fw=FlowInterpolator(im),
                            flow_interpolator_bw=FlowInterpolator(im, forward=False))
        v = Voxels(h)
        v._engine, v._flow = hipnative.VoxelFeatures(shape, h.spacing, 1.0), (h.flow_interpolator_fw, h.flow_interpolator_bw)
        walls, parts = [], []
        for _ in range(a.repeat + 1):                     # the first run warms up (allocations, code objects)
            for name in list(vars(v)):
                if isinstance(getattr(v, name), list) and name not in ("stats_to_aggregate", "features_to_save", "_own_interpolators"):
                    setattr(v, name, [])
            t0 = time.perf_counter()
            v._run_frame(t)
            walls.append(time.perf_counter() - t0)
            parts.append(v.kernel_ms[0])
        n_vox, n_nodes, n_pairs = len(v.coords[0]), len(v.node_voxel_idxs[0]), int(v.node_labels_csr[0][0][-1])
        with_flow = int((~np.isnan(v.vec12[0][:, 0])).sum())
        v.close()
        h.flow_interpolator_fw.close()
        h.flow_interpolator_bw.close()
    walls, parts = walls[1:], parts[1:]
    out = dict(tool="bench_voxels", shape=list(shape), device=hipnative.load().device_name(0), flow_rows_per_direction=int(a.rows),
               labelled_voxels=n_vox, voxels_with_forward_flow=with_flow, nodes=n_nodes, node_voxel_pairs=n_pairs,
               kernel_ms={k: float(np.median([p[k] for p in parts])) for k in parts[0]},
               kernel_ms_total=float(np.median([sum(p.values()) for p in parts])), wall_ms_per_frame=float(np.median(walls) * 1e3),
               wall_ms_all=[round(w * 1e3, 2) for w in walls], repeat=a.repeat,
               note="wall = one frame of Voxels: uploads, kernels, downloads and the split of both node lists into Python lists")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
