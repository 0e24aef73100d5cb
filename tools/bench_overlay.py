"""The analysis overlay of one frame: the device path (nellie_amd.feature_extraction.FeatureOverlay on files) against the sparse
numpy restatement on the host (tests/feature_overlay_restatement.py).

    python tools/bench_overlay.py [--frame 256] [--repeat 3] [--timeout 600] [--no-host]

The frame is the one of `tools/bench_network.py --frame N`: N^3 voxels, 419 random walks dilated by 2 voxels,
labelled by connected component.  Its labelled voxels get synthetic groups: the organelle of a voxel is its label, its branch one
of V / 40 at random, its nodes 0 to 6 of V / 50 at random; the tables hold one random column per level.  Each side runs in a child
process of its own under its own time limit and prints one JSON line per level.

Device, per level, best of `repeat` after a warm-up: the stream time of the value kernel and of the paint as float64 and as float32
(`kernel_ms`, transfers excluded), the paint's stored bytes per second, the wall time of frame() on a frame that is not resident
(upload of 4 B/voxel, mask, scan, groups, values, paint, download into pageable memory) and of frame() for another column of the
resident frame (column upload, values, paint, download).  Host: the sparse restatement of the same frame, once.  The literal dense
form is not run at this size; the line says what it would allocate."""
import argparse
import json
import os
import pickle
import subprocess
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
LEVELS = ("voxel", "node", "branch", "organelle")
TABLES = {"voxel": "features_voxels", "node": "features_nodes", "branch": "features_branches", "organelle": "features_organelles"}


def walks_frame(n, walks=419, seed=7, radius=2):
    """the labels of tools/bench_network.py's frame: the 26-connected components of `walks` random walks dilated by `radius`"""
    from scipy import ndimage as ndi
    rng = np.random.default_rng(seed)
    line = np.zeros((n, n, n), bool)
    for _ in range(walks):
        d = np.cumsum(rng.integers(-1, 2, (n, 3)), axis=0) + rng.integers(0, n, 3)
        d = d[((d >= 0) & (d < n)).all(1)]
        line[tuple(d.T)] = True
    pts = np.argwhere(line)
    body = np.zeros_like(line)
    r = radius
    for off in np.argwhere(((np.indices((2 * r + 1,) * 3).transpose(1, 2, 3, 0) - r) ** 2).sum(-1) <= r * r) - r:
        body[tuple(np.clip(pts + off, 0, n - 1).T)] = True
    labels, _ = ndi.label(body, structure=np.ones((3, 3, 3)))
    return labels.astype(np.int32)


def scene(n):
    """labels (1, n, n, n), {key: [edges]} and {level: (t, label, value, value1)}"""
    labels = walks_frame(n)
    rng = np.random.default_rng(11)
    lab = labels[labels > 0]
    V = len(lab)
    n_branch, n_node, n_org = max(V // 40, 1), max(V // 50, 1), int(lab.max())
    counts = rng.integers(0, 7, V)
    edges = {"v_o": [np.column_stack([np.arange(V), lab]).astype(np.int64)],
             "v_b": [np.column_stack([np.arange(V), rng.integers(0, n_branch, V)]).astype(np.int64)],
             "v_n": [np.column_stack([np.repeat(np.arange(V), counts), rng.integers(0, n_node, int(counts.sum()))]).astype(np.int64)]}
    rows = {"voxel": np.arange(V), "node": np.arange(n_node), "branch": np.arange(1, n_branch + 1), "organelle": np.arange(1, n_org + 1)}
    tables = {lv: (np.zeros(len(r), np.int64), r, rng.normal(size=len(r)) * 100.0, rng.normal(size=len(r))) for lv, r in rows.items()}
    return labels[None], edges, tables


def device_side(n, repeat):
    import pandas as pd
    from nellie_amd import build, hipnative
    from nellie_amd.feature_extraction import FeatureOverlay
    import feature_overlay_restatement as fr
    build.build(verbose=False)
    labels, edges, tables = scene(n)
    V = int((labels > 0).sum())
    with tempfile.TemporaryDirectory() as tmp:
        paths = {"im_instance_label": os.path.join(tmp, "labels"), "adjacency_maps": os.path.join(tmp, "adjacency.pkl")}
        open(paths["im_instance_label"], "wb").close()
        with open(paths["adjacency_maps"], "wb") as f:
            pickle.dump(edges, f)
        for lv, (t, lab, a, b) in tables.items():
            paths[TABLES[lv]] = os.path.join(tmp, lv + ".csv")
            pd.DataFrame({"t": t, "label": lab, "value": a, "value1": b}).to_csv(paths[TABLES[lv]], index=False)
        im_info = SimpleNamespace(no_t=False, no_z=False, axes="TZYX", shape=labels.shape, pipeline_paths=paths, get_memmap=lambda p: labels)
        with FeatureOverlay(im_info) as fo:
            out64, out32 = np.empty(labels.shape[1:], np.float64), np.empty(labels.shape[1:], np.float32)
            for lv in LEVELS:
                fo.columns(lv)                                     # the table is read outside the timed calls
                best = dict(values=[], paint_f64=[], paint_f32=[], frame_cold=[], frame_resident=[], frame_resident_f32=[])
                for k in range(repeat + 1):                        # the first round warms up
                    fo._state = None                               # the frame goes up again
                    t0 = time.perf_counter()
                    fo.frame(lv, "value", 0, out=out64)
                    cold = time.perf_counter() - t0
                    t0 = time.perf_counter()
                    fo.frame(lv, "value1", 0, out=out64)
                    warm = time.perf_counter() - t0
                    ms64 = dict(fo.kernel_ms)
                    t0 = time.perf_counter()
                    fo.frame(lv, "value1", 0, out=out32, dtype=np.float32)
                    warm32 = time.perf_counter() - t0
                    ms32 = dict(fo.kernel_ms)
                    if k:
                        for key, v in (("values", ms64["values"]), ("paint_f64", ms64["paint"]), ("paint_f32", ms32["paint"]), ("frame_cold", cold * 1e3),
                                       ("frame_resident", warm * 1e3), ("frame_resident_f32", warm32 * 1e3)):
                            best[key].append(v)
                t_col, lab, _, b = tables[lv]
                res = {key: round(min(v), 4) for key, v in best.items()}
                nvox = labels[0].size
                res.update(side="device", level=lv, frame=n, voxels=nvox, labelled=V, edges=int(len(edges[fr.EDGE_KEYS[lv]][0])) if lv != "voxel" else V,
                           paint_f64_stored_TBps=round(nvox * 8 / (res["paint_f64"] * 1e-3) / 1e12, 3),
                           paint_f32_stored_TBps=round(nvox * 4 / (res["paint_f32"] * 1e-3) / 1e12, 3), device=hipnative.load().device_name(0))
                if lv != "node":                                   # the node level's restatement takes minutes: the host side checks nothing either
                    want = fr.overlay_sparse(labels, lv, t_col, lab, b, edges.get(fr.EDGE_KEYS.get(lv)))[0]
                    res["same_as_restatement"] = bool(fr.same(out64, want)) and bool(fr.same(out32, want.astype(np.float32)))
                print(json.dumps(res), flush=True)


def host_side(n):
    import feature_overlay_restatement as fr
    labels, edges, tables = scene(n)
    V = int((labels > 0).sum())
    for lv in LEVELS:
        t_col, lab, a, _ = tables[lv]
        t0 = time.perf_counter()
        fr.overlay_sparse(labels, lv, t_col, lab, a, edges.get(fr.EDGE_KEYS.get(lv)))
        wall = time.perf_counter() - t0
        groups = len(lab)
        print(json.dumps(dict(side="host", level=lv, frame=n, labelled=V, sparse_restatement_ms=round(wall * 1e3, 1),
                              literal_dense_form_GB=None if lv == "voxel" else round(V * (groups + 1) * 10 / 1e9, 1),
                              note="literal form: a bool and a float64 matrix of (groups + 1) x labelled voxels and nanmean's bool mask, 10 B per entry; not run")),
              flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frame", type=int, default=256)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--timeout", type=float, default=600.0, help="seconds for each side")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--side", choices=("device", "host"), default=None, help="run this side in this process")
    a = ap.parse_args()
    if a.side == "device":
        return device_side(a.frame, a.repeat)
    if a.side == "host":
        return host_side(a.frame)
    for name in ("device",) + (() if a.no_host else ("host",)):
        cmd = [sys.executable, os.path.abspath(__file__), "--side", name, "--frame", str(a.frame), "--repeat", str(a.repeat)]
        done = subprocess.run(cmd, timeout=a.timeout, check=True, capture_output=True, text=True)
        print(done.stdout.strip(), flush=True)


if __name__ == "__main__":
    main()
