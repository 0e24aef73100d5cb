#!/usr/bin/env python3
"""Network stage's two dense steps (pixel classes, branch labels) on a synthetic skeleton image.
    python tools/bench_network.py [Z Y X]          default 1024^3 (a 128^3 random-walk skeleton tiled)
Times include the H2D of the int32 skeleton and the D2H of both products (the C-ABI hands over host arrays);
`kernel_ms` is the HIP-event time of the device work alone.

    python tools/bench_network.py --frame [N] [--walks W] [--no-host]
The whole stage behind the thinning on one synthetic N^3 frame (default 256) of dilated random walks, the walks standing in for the
thinning: wall time through Network._run_frame (upload, the five steps, download) and the per-step stream times, best of three;
then, unless --no-host, the reference's per-object relabelling loop (find_objects + scipy's distance_transform_edt per object,
networking.py:485-577) on the same frame and host, once, and whether the two relabelled volumes are equal.

    python tools/bench_network.py --frame [N] --thin hip [--rounds-per-sync R] [--dump-skel FILE.npy]
The same frame with the thinning on the device (Network(skeletonize="hip")): the mask is the thinning of labels > 0, not the walks.
Reports kernel_ms["thin"], the thinning's seven counts and the wall time of _run_frame, best of three; --dump-skel saves the device's
mask.
    python tools/bench_network.py --frame [N] --dump-mask FILE.npy
Saves labels > 0 of that frame and stops (needs no device), so that skimage.morphology.skeletonize can be timed on the same mask by an
interpreter that has it, and its result compared with --dump-skel's."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from nellie_amd import hipnative
from nellie_amd.synthetic import make_skeleton


def walks_frame(n, walks, seed=7, steps=None, radius=2):
    """labels (int32: the 26-connected components of the dilated walks), the walks' voxels (bool), a Frangi stand-in (float32)."""
    from scipy import ndimage as ndi
    rng = np.random.default_rng(seed)
    steps = steps or n
    line = np.zeros((n, n, n), bool)
    for _ in range(walks):
        d = np.cumsum(rng.integers(-1, 2, (steps, 3)), axis=0) + rng.integers(0, n, 3)
        d = d[((d >= 0) & (d < n)).all(1)]
        line[tuple(d.T)] = True
    pts = np.argwhere(line)
    body = np.zeros_like(line)
    r = radius
    for off in np.argwhere(np.indices((2 * r + 1,) * 3).transpose(1, 2, 3, 0).__sub__(r).__pow__(2).sum(-1) <= r * r) - r:
        q = np.clip(pts + off, 0, n - 1)
        body[tuple(q.T)] = True
    labels, _ = ndi.label(body, structure=np.ones((3, 3, 3)))
    return labels.astype(np.int32), line, rng.random((n, n, n), dtype=np.float32)


def host_relabel(branch, labels, scaling):
    """The reference's loop (networking.py:485-577), scipy per object."""
    from scipy import ndimage as ndi
    out = np.zeros(labels.shape, np.uint32)
    n_obj = vol = 0
    for k, sl in enumerate(ndi.find_objects(labels)):
        if sl is None:
            continue
        obj = labels[sl] == k + 1
        seeds = (branch[sl] > 0) & obj
        if not seeds.any():
            continue
        n_obj += 1
        vol += obj.size
        ind = ndi.distance_transform_edt(~seeds, sampling=scaling, return_distances=False, return_indices=True)
        near = branch[sl][tuple(ind)]
        sub = out[sl]
        sub[obj] = near[obj].astype(np.uint32)
    return out, n_obj, vol


def bench_thin(argv, n, walks, labels, frangi, info):
    from nellie_amd.segmentation.networking import Network
    how = argv[argv.index("--thin") + 1]
    rps = int(argv[argv.index("--rounds-per-sync") + 1]) if "--rounds-per-sync" in argv else None
    net = Network(info, skeletonize=how, rounds_per_sync=rps)
    net.num_t = 1
    net.label_memmap, net.im_frangi_memmap = labels[None], frangi[None]
    wall = []
    for _ in range(3):
        t0 = time.perf_counter()
        net._run_frame(0)
        wall.append(time.perf_counter() - t0)
    best = min(range(3), key=lambda k: net.kernel_ms[k]["thin"])
    stats = net.frame_stats[best]
    res = {"frame": [n, n, n], "walks": walks, "thin": how, "rounds_per_sync": rps, "labels": int(labels.max()),
           "thin_ms_best": round(net.kernel_ms[best]["thin"], 3), "thin_ms_all": [round(k["thin"], 3) for k in net.kernel_ms],
           **{k: v for k, v in stats.items() if k.startswith("thin_")},
           "kernel_ms_best_thin_run": {k: round(v, 3) for k, v in net.kernel_ms[best].items()},
           "wall_ms_best": round(min(wall) * 1e3, 2), "wall_ms_all": [round(w * 1e3, 2) for w in wall],
           **{k: v for k, v in stats.items() if not k.startswith("thin_")},
           "note": "wall: Network._run_frame, thinning on the device; includes H2D of 8 B/voxel and D2H of 9 B/voxel, pageable"}
    if "--dump-skel" in argv:
        np.save(argv[argv.index("--dump-skel") + 1], net._held.obj.network_fetch_mask(labels.shape))
    net.close()
    print(json.dumps(res))


def bench_frame(argv):
    from types import SimpleNamespace
    from nellie_amd.segmentation.networking import Network
    n = int(argv[argv.index("--frame") + 1]) if len(argv) > argv.index("--frame") + 1 and argv[argv.index("--frame") + 1].isdigit() else 256
    walks = int(argv[argv.index("--walks") + 1]) if "--walks" in argv else max(4, n * n * n // 40000)
    labels, line, frangi = walks_frame(n, walks)
    if "--dump-mask" in argv:
        np.save(argv[argv.index("--dump-mask") + 1], labels > 0)
        print(json.dumps({"frame": [n, n, n], "walks": walks, "foreground": int((labels > 0).sum()), "saved": argv[argv.index("--dump-mask") + 1]}))
        return
    scaling = (0.29, 0.11, 0.11)
    info = SimpleNamespace(no_t=True, no_z=False, shape=(1, n, n, n), axes="TZYX", dim_res=dict(zip("ZYX", scaling), T=1.0))
    if "--thin" in argv:
        return bench_thin(argv, n, walks, labels, frangi, info)
    net = Network(info, skeletonize=lambda mask: line)
    net.num_t = 1
    net.label_memmap, net.im_frangi_memmap = labels[None], frangi[None]
    wall, products = [], None
    for _ in range(3):
        t0 = time.perf_counter()
        products = net._run_frame(0)
        wall.append(time.perf_counter() - t0)
    best = min(range(3), key=lambda k: net.kernel_ms[k]["relabel"])
    res = {"frame": [n, n, n], "walks": walks, "scaling": list(scaling), "labels": int(labels.max()), **net.frame_stats[-1],
           "wall_ms_best": round(min(wall) * 1e3, 2), "wall_ms_all": [round(w * 1e3, 2) for w in wall],
           "kernel_ms_best_relabel_run": {k: round(v, 3) for k, v in net.kernel_ms[best].items()},
           "post_thinning_stream_ms_best": round(min(sum(k.values()) for k in net.kernel_ms), 3),
           "note": "wall: Network._run_frame with the thinning replaced by a stored mask; includes H2D of 9 B/voxel and D2H of 9 B/voxel, pageable"}
    net.close()
    if "--no-host" not in argv:
        t0 = time.perf_counter()
        host, n_obj, vol = host_relabel(products[0], labels, scaling)
        res["host_relabel_loop_s"] = round(time.perf_counter() - t0, 3)
        res["host_equals_device"] = bool(np.array_equal(host, products[2]))
        assert (n_obj, vol) == (res["n_objects"], res["box_volume"])
    print(json.dumps(res))


if "--frame" in sys.argv:
    bench_frame(sys.argv)
    sys.exit(0)

shape = tuple(int(a) for a in sys.argv[1:4]) if len(sys.argv) >= 4 else (1024, 1024, 1024)
tile = make_skeleton((128, 128, 128), 7)
reps = [-(-s // 128) for s in shape]
skel = np.ascontiguousarray(np.tile(tile, reps)[:shape[0], :shape[1], :shape[2]])
ctx = hipnative.Context(shape)
wall, kern = [], []
for rep in range(3):
    ctx.prof_reset(); ctx.prof_enable(True)
    t0 = time.perf_counter()
    pc, n_skel = ctx.skel_pixel_class(skel)
    labels, n_branches = ctx.skel_branch_labels(None)
    wall.append(time.perf_counter() - t0)
    ctx.prof_enable(False)
    kern.append(ctx.prof_get("network")[0])
print(json.dumps({"shape": list(shape), "skeleton_voxels": n_skel, "branches": n_branches,
                  "classes": np.bincount(pc.ravel(), minlength=5).tolist(),
                  "wall_ms_best": round(min(wall) * 1e3, 2), "device_ms_best": round(min(kern), 3),
                  "note": "wall includes H2D of the int32 skeleton and D2H of uint8 classes + int32 labels from pageable memory"}))
ctx.close()
