"""The cost of the solidity columns on the organelle level's region call, per frame: the device time of the
region sums (what `Components` spends with solidity off) and, with solidity on, of the three device parts of the convex count (row
extremes, per-plane hulls, the count) with the host time of the hulls, and the wall time of both; medians of `--repeat` runs after a
warm-up, one JSON line per scene, appended to profiles/solidity_bench.jsonl with `--save`.

    python tools/bench_solidity.py [--shape 128 512 512] [--network 64 256 256] [--repeat 5] [--save]

Scenes: the component labels of tools/bench_components.py's frame (many organelles), and one organelle network: a lattice of
tubes, every node joined to its neighbours, at least 10^5 voxels in a single region.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))


def network(shape, pitch=16, radius=2):
    """one connected lattice of tubes along the three axes, bent a little so that no plane of it is flat"""
    z, y, x = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij", sparse=True)
    wob = lambda a, b: (3.0 * np.sin(a / 23.0) + 2.0 * np.cos(b / 17.0))
    near = lambda v, w: np.abs(((v + w) % pitch) - pitch / 2) <= radius
    tubes = (near(z, wob(x, y)) & near(y, wob(x, z))) | (near(z, wob(y, x)) & near(x, wob(y, z))) | (near(y, wob(z, x)) & near(x, wob(z, y)))
    return tubes.astype(np.int32)


def measure(eng, frame, repeat):
    runs = []
    for i in range(repeat + 1):                                    # the first run warms up (allocations, code objects)
        t0 = time.perf_counter()
        eng.regions(frame, None, rows=True)
        _, sums, _ = eng.fetch_regions()
        t1 = time.perf_counter()
        eng.convex()
        count, facets, rows = eng.fetch_convex(sizes=True)
        t2 = time.perf_counter()
        if i:
            runs.append(dict(eng.convex_ms_parts(), regions=eng.kernel_ms_parts()["regions"], wall_off=(t1 - t0) * 1e3, wall_on=(t2 - t0) * 1e3))
    med = {k: float(np.median([r[k] for r in runs])) for k in runs[0]}
    big = int(np.argmax(sums[0]))
    return dict(regions=int(sums.shape[1]), region_voxels=int(sums[0].sum()), largest_region=int(sums[0][big]), largest_region_facets=int(facets[big]),
                largest_region_box_rows=int(rows[big]), facets=int(facets.sum()), box_rows=int(rows.sum()), flat_regions=int((count == 0).sum()),
                device_ms=dict(regions=med["regions"], extremes=med["extremes"], planes=med["planes"], count=med["count"]), hull_host_ms=med["hull"],
                wall_ms=dict(solidity_off=med["wall_off"], solidity_on=med["wall_on"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", type=int, nargs=3, default=(128, 512, 512))
    ap.add_argument("--network", type=int, nargs=3, default=(64, 256, 256))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--save", action="store_true")
    a = ap.parse_args()
    from bench_voxels import make_frame
    from nellie_amd import build, hipnative
    build.build(verbose=False)
    spacing = (0.29, 0.0973, 0.0973)
    scenes = [("organelles", make_frame(tuple(a.shape), 1)[2]), ("network", network(tuple(a.network)))]
    lines = []
    for name, frame in scenes:
        with hipnative.BranchFeatures(frame.shape, spacing) as eng:
            out = dict(tool="bench_solidity", scene=name, shape=list(frame.shape), device=hipnative.load().device_name(0), repeat=a.repeat,
                       **measure(eng, frame, a.repeat))
        out["note"] = ("wall_off = regions(rows=True) and its download; wall_on adds convex() and its download: two device parts, the "
                       "download of two ints per box row, the hulls on the host, the upload of the facets, the count")
        lines.append(json.dumps(out))
        print(lines[-1], flush=True)
    if a.save:
        os.makedirs(os.path.join(REPO, "profiles"), exist_ok=True)
        with open(os.path.join(REPO, "profiles", "solidity_bench.jsonl"), "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
