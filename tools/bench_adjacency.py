"""The adjacency maps of one frame at a stated row count: the device path (nellie_amd.feature_extraction.adjacency_maps: uploads,
kernels, 16 bytes per edge back over PCIe) against the numpy restatement on the host (tests/adjacency_restatement.py, which is
vectorised; the reference's own v_n is a Python double loop and far slower than either).

    python tools/bench_adjacency.py [--rows 10000000] [--repeat 3] [--timeout 300]

Each side runs in a child process of its own under its own time limit and prints one JSON line; this process prints both and which
side won.  The frame is synthetic: `rows` voxels that all carry a component label, 30 % of them a branch label, 0 to 6 nodes each
(10 % none), rows / 50 nodes, rows / 200 branches and rows / 2000 components, labels unsorted.  Wall time is the median of `repeat`
runs after a warm-up; kernel_ms is the device time of the kernels alone (transfers excluded) of the median run.
"""
import argparse
import json
import os
import subprocess
import sys
import time
from types import SimpleNamespace

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def make_frame(rows, seed=1):
    rng = np.random.default_rng(seed)
    n_nodes, n_branches, n_comps = max(rows // 50, 1), max(rows // 200, 1), max(rows // 2000, 1)
    branch_ids, comp_ids = rng.permutation(n_branches) + 1, rng.permutation(n_comps) + 1
    vox_branch = rng.integers(1, n_branches + 1, rows).astype(np.int32)
    vox_branch[rng.random(rows) >= 0.3] = 0
    counts = rng.integers(1, 7, rows)
    counts[rng.random(rows) < 0.1] = 0
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    voxels = SimpleNamespace(time=[0], branch_labels=[vox_branch], component_labels=[rng.integers(1, n_comps + 1, rows).astype(np.int32)],
                             node_labels_csr=[(off, rng.integers(0, n_nodes, int(off[-1])))])
    nodes = SimpleNamespace(time=[0], branch_label=[rng.integers(0, n_branches + 1, n_nodes).astype(np.int32)],
                            component_label=[rng.integers(1, n_comps + 1, n_nodes).astype(np.int32)])
    branches = SimpleNamespace(time=[0], branch_label=[branch_ids], component_label=[rng.integers(1, n_comps + 1, n_branches).astype(np.int32)])
    return SimpleNamespace(skip_nodes=False, voxels=voxels, nodes=nodes, branches=branches, components=SimpleNamespace(component_label=[comp_ids]))


def host_lists(h):
    """the restatement on the CSR the device path is given (it does not split the node lists into one array per voxel first)"""
    import adjacency_restatement as ar
    v, n, b, c = h.voxels, h.nodes, h.branches, h.components
    return dict(v_b=[ar.pairs(v.branch_labels[0], 1)], v_n=[ar.expand(*v.node_labels_csr[0])], v_o=[ar.pairs(v.component_labels[0], 0)],
                n_b=[ar.lookup(n.branch_label[0], b.branch_label[0])], n_o=[ar.lookup(n.component_label[0], c.component_label[0])],
                b_o=[ar.lookup(b.component_label[0], c.component_label[0])])


def side(name, rows, repeat):
    h = make_frame(rows)
    walls, parts, out = [], [], None
    if name == "device":
        from nellie_amd import build
        from nellie_amd.feature_extraction import adjacency_maps
        build.build(verbose=False)
    for _ in range(repeat + 1):                                    # the first run warms up
        ms = {}
        t0 = time.perf_counter()
        out = adjacency_maps(h, kernel_ms=ms) if name == "device" else host_lists(h)
        walls.append(time.perf_counter() - t0)
        parts.append(ms)
    walls, parts = walls[1:], parts[1:]
    k = int(np.argsort(walls)[len(walls) // 2])
    res = dict(side=name, rows=rows, edges={key: int(len(v[0])) for key, v in out.items()}, wall_ms=round(walls[k] * 1e3, 2),
               wall_ms_all=[round(w * 1e3, 2) for w in walls])
    if name == "device":
        from nellie_amd import hipnative
        res.update(kernel_ms={key: round(v, 3) for key, v in parts[k].items()}, kernel_ms_total=round(sum(parts[k].values()), 3),
                   device=hipnative.load().device_name(0))
        import adjacency_restatement as ar
        assert ar.same_lists(out, host_lists(h))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds for each side")
    ap.add_argument("--side", choices=("device", "host"), default=None, help="run this side in this process")
    a = ap.parse_args()
    if a.side:
        side(a.side, a.rows, a.repeat)
        return
    results = {}
    for name in ("device", "host"):
        cmd = [sys.executable, os.path.abspath(__file__), "--side", name, "--rows", str(a.rows), "--repeat", str(a.repeat)]
        done = subprocess.run(cmd, timeout=a.timeout, check=True, capture_output=True, text=True)
        results[name] = json.loads(done.stdout.strip().splitlines()[-1])
        print(json.dumps(results[name]), flush=True)
    d, h = results["device"]["wall_ms"], results["host"]["wall_ms"]
    print(json.dumps(dict(tool="bench_adjacency", rows=a.rows, date=time.strftime("%Y-%m-%d"), device_wall_ms=d, host_wall_ms=h,
                          device_kernel_ms=results["device"]["kernel_ms_total"], winner="device" if d < h else "host",
                          ratio=round(max(d, h) / min(d, h), 2))))


if __name__ == "__main__":
    main()
