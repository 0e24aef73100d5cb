#!/usr/bin/env python3
"""Flow-vector interpolation timing: a 128x512x512 frame, the flow rows of 3 000 markers per frame (a third of them repeated as
column-based candidates), every voxel of a synthetic label mask (2 % of the frame) as a query, forward and backward.
    python tools/bench_flow.py [--out profiles/flow_bench.jsonl] [--reps 5] [Z Y X [markers]]
Appends one JSON line: per direction the kernel time (device events around the interpolation kernels), the call time of
FlowField.interpolate (upload of the queries and download of the vectors included) and the time to load a time point's rows."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

SPACING = (0.2, 0.1, 0.1)
RADIUS = 0.5


def make_input(shape=(128, 512, 512), n_markers=3000, seed=11):
    """(flow_vector_array with rows for t = 0 and t = 1, query coordinates (n, 3) float64)"""
    rng = np.random.default_rng(seed)
    mask = rng.random(shape) < 0.02
    q = np.argwhere(mask).astype(np.float64)
    rows = []
    for t in range(2):
        pos = q[rng.choice(len(q), n_markers, replace=False)]
        vec = rng.integers(-3, 4, (n_markers, 3)).astype(np.float64)
        dup = rng.choice(n_markers, n_markers // 3, replace=False)
        pos = np.concatenate([pos, pos[dup]])
        vec = np.concatenate([vec, rng.integers(-3, 4, (len(dup), 3)).astype(np.float64)])
        cost = rng.random(len(pos)).astype(np.float32).astype(np.float64)
        rows.append(np.column_stack([np.full(len(pos), float(t)), pos, vec, cost]))
    return np.concatenate(rows), q


def check_rows(flow, t, forward):
    rows = flow[flow[:, 0] == (t if forward else t - 1)]
    return (rows[:, 1:4] if forward else rows[:, 1:4] + rows[:, 4:7]), rows[:, 4:7], rows[:, 7]


def bench(shape, n_markers, reps):
    from nellie_amd import hipnative
    flow, q = make_input(shape, n_markers)
    rec = {"shape": list(shape), "markers": n_markers, "queries": len(q), "spacing": list(SPACING), "radius_um": RADIUS,
           "device": hipnative.load().device_name(0)}
    with hipnative.FlowField(3, SPACING, RADIUS) as field:
        for name, forward in (("forward", True), ("backward", False)):
            c, v, k = check_rows(flow, 1, forward)
            load, call, kern = [], [], []
            for rep in range(reps + 1):                      # the first repetition warms up
                t0 = time.perf_counter(); field.load(c, v, k); t1 = time.perf_counter()
                out, found = field.interpolate(q); t2 = time.perf_counter()
                if rep:
                    load.append(t1 - t0); call.append(t2 - t1); kern.append(field.kernel_ms())
            rec[name] = {"rows": len(c), "found": found, "load_ms": round(min(load) * 1e3, 3), "kernel_ms": round(min(kern), 3),
                         "call_ms": round(min(call) * 1e3, 3), "call_ms_median": round(float(np.median(call)) * 1e3, 3)}
    rec["note"] = "kernel_ms: flow_interp_kernel alone; call_ms: FlowField.interpolate, query upload and vector download included"
    return rec


if __name__ == "__main__":
    args = sys.argv[1:]
    out, reps = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "flow_bench.jsonl"), 5
    if "--out" in args:
        k = args.index("--out"); out = args[k + 1]; del args[k:k + 2]
    if "--reps" in args:
        k = args.index("--reps"); reps = int(args[k + 1]); del args[k:k + 2]
    shape = tuple(int(a) for a in args[:3]) if len(args) >= 3 else (128, 512, 512)
    nm = int(args[3]) if len(args) > 3 else 3000
    line = json.dumps(bench(shape, nm, reps))
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "a") as f:
        f.write(line + "\n")
