"""One frame of the organelle level of the hierarchy at 128 x 512 x 512 (nellie_amd/synthetic.py): components, the largest one,
device time per part (region sums, aggregation) and the wall time of the frame; and, apart from that, the `regions` part alone on
the component-label frame without reassigned labels (so no sort), per voxel (rows=False) and by row runs (rows=True) alternating
in one process: the median of `--repeat` runs after a warm-up, with their smallest and largest.

    python tools/bench_components.py [--shape 128 512 512] [--repeat 5] [--no-reassigned] [--network Z Y X]

The scene is that of tools/bench_voxels.py; the reassigned labels are the component labels modulo 97.  `voxels`, `nodes` and
`branches` are plain objects: the labelled voxels, the nodes and one branch per branch label with their component labels and random
statistics, which is all that Components reads of them.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=(128, 512, 512))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-reassigned", action="store_true")
    ap.add_argument("--network", type=int, nargs=3, default=None, metavar=("Z", "Y", "X"),
                    help="time the regions part alone on one box-shaped component of this extent in the middle of the frame as well")
    a = ap.parse_args()
    from bench_branches import NODE_STATS, VOXEL_STATS, level
    from bench_voxels import make_frame
    from nellie_amd import build, hipnative
    from nellie_amd.feature_extraction import Components
    from nellie_amd.feature_extraction.components import REGION_STATS
    build.build(verbose=False)
    shape = tuple(a.shape)
    _, _, comp, branch, pixel_class, _, _ = make_frame(shape, 1)
    reassigned = None if a.no_reassigned else (comp % 97).astype(np.int32)
    spacing = (0.29, 0.0973, 0.0973)
    rng = np.random.default_rng(1)
    _, first = np.unique(branch[comp > 0], return_index=True)     # one branch per branch label, in the component of its first voxel
    branch_stats = ["branch_length", "branch_thickness", "branch_aspect_ratio", "branch_tortuosity", "branch_area", "branch_axis_length_maj",
                    "branch_axis_length_min", "branch_extent", "branch_solidity", "reassigned_label"]
    im = SimpleNamespace(no_t=False, no_z=False, file_info=SimpleNamespace(filename_no_ext="bench"))
    h = SimpleNamespace(im_info=im, num_t=1, spacing=spacing, viewer=None, label_components=[comp], im_obj_reassigned=None if reassigned is None else [reassigned],
                        skip_nodes=False, low_memory=False, voxels=level(rng, comp[comp > 0], VOXEL_STATS, np.float32, "component_labels"),
                        nodes=level(rng, comp[pixel_class > 0], NODE_STATS, np.float64, "component_label"),
                        branches=level(rng, comp[comp > 0][first], branch_stats, np.float64, "component_label"))
    components = Components(h)
    components._engine = hipnative.BranchFeatures(shape, spacing)
    components._aggregator = hipnative.NodeFeatures()
    lists = [k for k, v in vars(components).items() if isinstance(v, list) and k not in ("stats_to_aggregate", "features_to_save")]
    walls, parts = [], []
    for _ in range(a.repeat + 1):                         # the first run warms up (allocations, code objects)
        for name in lists:
            setattr(components, name, [])
        t0 = time.perf_counter()
        components._run_frame(0)
        walls.append(time.perf_counter() - t0)
        parts.append(components.kernel_ms[0])
    sizes = np.bincount(comp[comp > 0])
    out = dict(tool="bench_components", shape=list(shape), device=hipnative.load().device_name(0), components=len(components.component_label[0]),
               largest_component=int(sizes.max()), component_voxels=int((comp > 0).sum()), nodes=int((pixel_class > 0).sum()), branches=len(first),
               reassigned=reassigned is not None)
    assert all(len(getattr(components, k)[0]) == out["components"] for k in REGION_STATS)
    eng = components._engine

    def time_alone(frame):
        alone, sums = {False: [], True: []}, {}
        for i in range(a.repeat + 1):                     # rows=False and rows=True alternating; the first pair warms up
            for rows in (False, True):
                eng.regions(frame, None, rows=rows)
                sums[rows] = eng.fetch_regions()[1]
                if i:
                    alone[rows].append(eng.kernel_ms_parts()["regions"])
        assert np.array_equal(sums[False], sums[True])
        return {("rows" if rows else "per_voxel"): dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for rows, v in alone.items()}
    out["regions_alone_ms"] = time_alone(comp)
    if a.network:
        box = np.zeros(shape, comp.dtype)
        box[tuple(slice((s - e) // 2, (s - e) // 2 + e) for s, e in zip(shape, a.network))] = 1
        out.update(network_voxels=int(box.sum()), network_regions_alone_ms=time_alone(box))
    components.close()
    walls, parts = walls[1:], parts[1:]
    out.update(kernel_ms={k: float(np.median([p[k] for p in parts])) for k in parts[0]},
               kernel_ms_total=float(np.median([sum(p.values()) for p in parts])), wall_ms_per_frame=float(np.median(walls) * 1e3),
               wall_ms_all=[round(w * 1e3, 2) for w in walls], repeat=a.repeat,
               note="wall = one frame of Components: uploads of two frames, kernels, downloads, one stable sort per child for the groups, "
                    "twenty-four statistics aggregated, the per-component numpy; regions = label ranking, sums and the most frequent "
                    "reassigned label; regions_alone = label ranking and sums without reassigned labels")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
