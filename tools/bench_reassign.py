"""One frame pair of voxel reassignment at 128 x 512 x 512 (nellie_amd/synthetic.py): labelled-voxel count, device time and wall
time per pair, appended to profiles/reassign_bench.jsonl.

    python tools/bench_reassign.py [--shape 128 512 512] [--rows 20000] [--repeat 5] [--no-append]

Frame 0: the voxels of a synthetic volume above 130 are objects (ids by 32-voxel blocks), those above 170 branches.  Frame 1 is
frame 0 moved by (1, 2, -1) voxels.  The flow rows sit at random labelled voxels and carry that vector plus +-0.3 voxels of noise.
"""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def make_pair(shape, rows, seed=4567):
    from nellie_amd.synthetic import make_volume
    vol = make_volume(shape, seed)
    zz, yy, xx = np.meshgrid(*[np.arange(n) // 32 for n in shape], indexing="ij", sparse=True)
    ids = (1 + zz * 10007 + yy * 101 + xx).astype(np.int32)
    obj0 = np.where(vol > 130, ids, 0).astype(np.int32)
    branch0 = np.where(vol > 170, ids + 5, 0).astype(np.int32)
    shift = (1, 2, -1)
    obj = np.stack([obj0, np.roll(obj0, shift, axis=(0, 1, 2))])
    branch = np.stack([branch0, np.roll(branch0, shift, axis=(0, 1, 2))])
    rng = np.random.default_rng(seed)
    vox = np.argwhere(obj0 > 0)
    pos = vox[rng.choice(len(vox), min(rows, len(vox)), replace=False)].astype(np.float64)
    vec = np.asarray(shift, np.float64) + rng.uniform(-0.3, 0.3, pos.shape)
    flow = np.column_stack([np.zeros(len(pos)), pos, vec, rng.random(len(pos)).astype(np.float32)])
    return branch, obj, flow


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=(128, 512, 512))
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-append", action="store_true")
    a = ap.parse_args()
    from nellie_amd import build, hipnative
    from nellie_amd.tracking.voxel_reassignment import VoxelReassigner
    build.build(verbose=False)
    shape = tuple(a.shape)
    branch, obj, flow = make_pair(shape, a.rows)
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        stacks = {"im_skel_relabelled": branch, "im_instance_label": obj}
        paths = {k: k for k in ("im_skel_relabelled", "im_instance_label", "im_branch_label_reassigned", "im_obj_label_reassigned")}
        paths["flow_vector_array"] = os.path.join(tmp, "flow.npy")
        paths["voxel_matches"] = os.path.join(tmp, "matches.npy")
        np.save(paths["flow_vector_array"], flow)

        def allocate_memory(path, dtype="float", data=None, description="", return_memmap=False, read_mode="r+"):
            stacks[path] = np.zeros(obj.shape, dtype)
            return stacks[path]
        im = SimpleNamespace(no_t=False, no_z=False, shape=obj.shape, axes="TZYX", dim_res=dict(Z=0.29, Y=0.0973, X=0.0973, T=1.0), im_path="im",
                             pipeline_paths=paths, get_memmap=lambda p, read_mode="r+": stacks.get(p, np.zeros((2, 4, 4, 4), np.uint8)),
                             allocate_memory=allocate_memory)
        walls, kernels = [], []
        for _ in range(a.repeat + 1):                     # the first run warms up (allocations, code objects)
            vr = VoxelReassigner(im)
            t0 = time.perf_counter()
            vr.run()
            walls.append(time.perf_counter() - t0)
            kernels.append(vr.kernel_ms[0])
            vr.close()
        assigned = int((stacks["im_obj_label_reassigned"][1] > 0).sum())
    walls, kernels = walls[1:], kernels[1:]
    out = dict(tool="bench_reassign", shape=list(shape), device=hipnative.load().device_name(0), flow_rows=int(len(flow)),
               labelled_voxels=[int((obj[t] > 0).sum()) for t in range(2)], assigned_object_voxels=assigned,
               kernel_ms_per_pair=float(np.median(kernels)), wall_ms_per_pair=float(np.median(walls) * 1e3),
               kernel_ms_all=[round(k, 3) for k in kernels], wall_ms_all=[round(w * 1e3, 2) for w in walls], repeat=a.repeat,
               note="wall = VoxelReassigner.run() of a T = 2 stack: both uploads, the pair, both downloads and the host scatter")
    print(json.dumps(out))
    if not a.no_append:
        os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
        with open(os.path.join(REPO, "profiles", "reassign_bench.jsonl"), "a") as f:
            f.write(json.dumps(out) + "\n")


if __name__ == "__main__":
    main()
