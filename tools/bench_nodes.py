"""One frame of the node level of the hierarchy at 128 x 512 x 512 (nellie_amd/synthetic.py): nodes, the longest voxel list L,
device time per part (node list, thickness, node statistics, aggregation) and the wall time of the frame.

    python tools/bench_nodes.py [--shape 128 512 512] [--rows 20000] [--repeat 5]

The scene is that of tools/bench_voxels.py, whose frame t = 1 is run through `Voxels` once; its output is the `voxels` that `Nodes`
reads.  The border is the background voxels that touch a component voxel along an axis.
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
sys.path.insert(0, os.path.join(REPO, "tools"))


def shell(comp):
    on = comp > 0
    near = np.zeros_like(on)
    for ax in range(on.ndim):
        near[(slice(None),) * ax + (slice(1, None),)] |= on[(slice(None),) * ax + (slice(None, -1),)]
        near[(slice(None),) * ax + (slice(None, -1),)] |= on[(slice(None),) * ax + (slice(1, None),)]
    return (near & ~on).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=(128, 512, 512))
    ap.add_argument("--rows", type=int, default=20000)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    from bench_voxels import make_frame
    from nellie_amd import build, hipnative
    from nellie_amd.feature_extraction import Nodes, Voxels
    from nellie_amd.tracking.flow_interpolation import FlowInterpolator
    build.build(verbose=False)
    shape = tuple(a.shape)
    vol, struct, comp, branch, pixel_class, distance, flow = make_frame(shape, a.rows)
    border = shell(comp)
    T, t = 3, 1
    spacing = (0.29, 0.0973, 0.0973)
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "flow.npy")
        np.save(path, flow)
        im = SimpleNamespace(no_t=False, no_z=False, shape=(T,) + shape, axes="TZYX", dim_res=dict(Z=0.29, Y=0.0973, X=0.0973, T=1.0), im_path="im",
                             pipeline_paths={"flow_vector_array": path}, get_memmap=lambda p, read_mode="r+": np.zeros((T, 4, 4, 4), np.uint8),
                             file_info=SimpleNamespace(filename_no_ext="bench"))
        stack = lambda x: [x] * T   # noqa: E731
        h = SimpleNamespace(im_info=im, num_t=T, spacing=spacing, viewer=None, label_components=stack(comp), label_branches=stack(branch),
                            im_raw=stack(vol), im_struct=stack(struct), im_pixel_class=stack(pixel_class), im_distance=stack(distance),
                            skip_nodes=False, enable_motility=True, flow_interpolator_fw=FlowInterpolator(im),
                            flow_interpolator_bw=FlowInterpolator(im, forward=False))
        v = Voxels(h)
        v._engine, v._flow = hipnative.VoxelFeatures(shape, spacing, 1.0), (h.flow_interpolator_fw, h.flow_interpolator_bw)
        v._run_frame(t)                                   # every list of v has one entry: frame 0 below
        v.close()
        h.flow_interpolator_fw.close()
        h.flow_interpolator_bw.close()
    h = SimpleNamespace(im_info=im, num_t=1, spacing=spacing, viewer=None, label_components=[comp], label_branches=[branch], im_pixel_class=[pixel_class],
                        im_border_mask=[border], skip_nodes=False, low_memory=False, voxels=v)
    nodes = Nodes(h)
    nodes._engine = hipnative.NodeFeatures(shape, spacing)
    walls, parts = [], []
    for _ in range(a.repeat + 1):                         # the first run warms up (allocations, code objects)
        for name in ("time", "nodes", "aggregate_voxel_metrics", "z", "y", "x", "node_thickness", "divergence", "convergence", "vergere", "branch_label",
                     "component_label", "image_name", "longest", "kernel_ms"):
            setattr(nodes, name, [])
        t0 = time.perf_counter()
        nodes._run_frame(0)
        walls.append(time.perf_counter() - t0)
        parts.append(nodes.kernel_ms[0])
    n_nodes, longest, pairs = len(nodes.nodes[0]), nodes.longest[0], int(v.node_voxel_idxs_csr[0][0][-1])
    nodes.close()
    walls, parts = walls[1:], parts[1:]
    out = dict(tool="bench_nodes", shape=list(shape), device=hipnative.load().device_name(0), labelled_voxels=len(v.coords[0]), nodes=n_nodes,
               node_voxel_pairs=pairs, longest_list=longest, border_voxels=int(border.sum()),
               kernel_ms={k: float(np.median([p[k] for p in parts])) for k in parts[0]},
               kernel_ms_total=float(np.median([sum(p.values()) for p in parts])), wall_ms_per_frame=float(np.median(walls) * 1e3),
               wall_ms_all=[round(w * 1e3, 2) for w in walls], repeat=a.repeat,
               note="wall = one frame of Nodes: uploads of four frames, the voxel lists, coordinates, vectors and eleven statistics, kernels, downloads; "
                    "aggregation = eleven statistics")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
