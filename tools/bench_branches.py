"""One frame of the branch level of the hierarchy at 128 x 512 x 512 (nellie_amd/synthetic.py): skeleton voxels, branches, regions,
device time per part (skeleton list, degree and edge counts, radii, per-label lists, region sums, aggregation) and the wall time
of the frame.

    python tools/bench_branches.py [--shape 128 512 512] [--repeat 5] [--no-reassigned]

The scene is that of tools/bench_voxels.py: the skeleton is its node voxels (every 40th branch voxel) carrying their branch label,
the border the background voxels that touch a component voxel along an axis, the reassigned labels the branch labels modulo 97.
`voxels` and `nodes` are plain objects: the labelled voxels and the nodes in raster order with their branch labels and random
statistics (eleven float32 ones per voxel, four float64 ones per node), which is all that Branches reads of them.
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
sys.path.insert(0, os.path.join(REPO, "tools"))

VOXEL_STATS = ["linear_vel", "angular_vel", "linear_acc", "angular_acc", "rel_linear_vel", "rel_angular_vel", "rel_linear_acc", "rel_angular_acc",
               "rel_directionality", "structure", "intensity"]
NODE_STATS = ["divergence", "convergence", "vergere", "node_thickness"]


def level(rng, labels, names, dtype, key):
    return SimpleNamespace(stats_to_aggregate=list(names), **{key: [labels]}, **{s: [rng.standard_normal(len(labels)).astype(dtype)] for s in names})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=(128, 512, 512))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-reassigned", action="store_true")
    a = ap.parse_args()
    from bench_nodes import shell
    from bench_voxels import make_frame
    from nellie_amd import build, hipnative
    from nellie_amd.feature_extraction import Branches
    build.build(verbose=False)
    shape = tuple(a.shape)
    _, _, comp, branch, pixel_class, _, _ = make_frame(shape, 1)
    skel = np.where(pixel_class > 0, branch, 0).astype(np.int32)
    border = shell(comp)
    reassigned = None if a.no_reassigned else (branch % 97).astype(np.int32)
    spacing = (0.29, 0.0973, 0.0973)
    rng = np.random.default_rng(1)
    im = SimpleNamespace(no_t=False, no_z=False, file_info=SimpleNamespace(filename_no_ext="bench"))
    h = SimpleNamespace(im_info=im, num_t=1, spacing=spacing, viewer=None, im_skel=[skel], label_components=[comp], label_branches=[branch],
                        im_border_mask=[border], im_branch_reassigned=None if reassigned is None else [reassigned], skip_nodes=False, low_memory=False,
                        voxels=level(rng, branch[comp > 0], VOXEL_STATS, np.float32, "branch_labels"),
                        nodes=level(rng, branch[pixel_class > 0], NODE_STATS, np.float64, "branch_label"))
    branches = Branches(h)
    branches._engine = hipnative.BranchFeatures(shape, spacing)
    branches._aggregator = hipnative.NodeFeatures()
    lists = [k for k, v in vars(branches).items() if isinstance(v, list) and k not in ("stats_to_aggregate", "features_to_save")]
    walls, parts = [], []
    for _ in range(a.repeat + 1):                         # the first run warms up (allocations, code objects)
        for name in lists:
            setattr(branches, name, [])
        t0 = time.perf_counter()
        branches._run_frame(0)
        walls.append(time.perf_counter() - t0)
        parts.append(branches.kernel_ms[0])
    out = dict(tool="bench_branches", shape=list(shape), device=hipnative.load().device_name(0), skeleton_voxels=len(branches.branch_idxs[0]),
               branches=len(branches.branch_label[0]), regions=len(branches.region_label[0]), region_voxels=int((branch > 0).sum()),
               largest_region=int(np.bincount(branch[branch > 0]).max()), labelled_voxels=int((comp > 0).sum()), border_voxels=int(border.sum()),
               reassigned=reassigned is not None)
    branches.close()
    walls, parts = walls[1:], parts[1:]
    out.update(kernel_ms={k: float(np.median([p[k] for p in parts])) for k in parts[0]},
               kernel_ms_total=float(np.median([sum(p.values()) for p in parts])), wall_ms_per_frame=float(np.median(walls) * 1e3),
               wall_ms_all=[round(w * 1e3, 2) for w in walls], repeat=a.repeat,
               note="wall = one frame of Branches: uploads of five frames, kernels, downloads, one stable sort per level for the groups, "
                    "fifteen statistics aggregated, the per-branch numpy; regions = sums plus the most frequent reassigned label")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
