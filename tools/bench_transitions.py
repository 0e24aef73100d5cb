"""The label transitions of one frame pair: the device path (hipnative.Transitions, which the tool drives directly; it is what
nellie_amd.tracking.match_transitions.transition_counts and MatchTransitions call) against the vectorised numpy restatement on the same host (tests/match_transitions_restatement.py).

    python tools/bench_transitions.py [--frame 512] [--repeat 5] [--save] [--out FILE]

The pair is synthetic: the frame is cut into cells of 16^3 voxels, about one cell in eight holds a cube of 12^3 voxels with a label
of its own (about 5 % of the voxels are labelled); the earlier frame is the later one moved back by (1, 2, 3) voxels under other
labels.  There is one match per labelled voxel of the later frame, in raster order, from the voxel (1, 1, 2) steps back: five rows
in six land on the object they came from, the rim lands on background and is dropped.

Medians of `repeat` after a warm-up, one JSON line (appended to profiles/transitions_bench.jsonl with --save): the device time per
kernel group (clear, count, compact, relabel; transfers excluded), the wall time of count() with both frames resident (coordinate
upload, kernels, download, host sort), of the pair from nothing (two frame uploads more) and of relabel() (table upload, kernel,
frame download), the restatement's wall time, and the atomic adds issued per row (the run heads).  The yardstick is the restatement;
the line says whether the device's table equals it."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def scene(n, cell=16, cube=12, share=0.12, shift=(1, 2, 3), matched=(1, 1, 2), seed=26):
    """-> A, B (n, n, n) int32 and prev, next (rows, 3) uint16"""
    rng = np.random.default_rng(seed)
    cells = n // cell
    on = rng.random((cells,) * 3) < share
    ids = np.where(on, np.arange(1, cells ** 3 + 1).reshape((cells,) * 3), 0).astype(np.int32)
    B = np.zeros((n, n, n), np.int32)
    B.reshape(cells, cell, cells, cell, cells, cell)[:, :cube, :, :cube, :, :cube] = ids[:, None, :, None, :, None]
    perm = np.concatenate([[0], rng.permutation(cells ** 3) + 1]).astype(np.int32)
    A = perm[np.roll(B, tuple(-s for s in shift), axis=(0, 1, 2))]
    nxt = np.column_stack(np.nonzero(B))
    prev = np.clip(nxt - np.asarray(matched), 0, n - 1)
    return A, B, prev.astype(np.uint16), nxt.astype(np.uint16)


def median(v):
    return round(statistics.median(v), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frame", type=int, default=512)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--save", action="store_true", help="append the line to profiles/transitions_bench.jsonl")
    ap.add_argument("--out", default=None, help="append the line to this file instead")
    a = ap.parse_args()
    from nellie_amd import build, hipnative
    from nellie_amd.tracking import match_transitions as mt
    import match_transitions_restatement as mr
    build.build(verbose=False)
    A, B, prev, nxt = scene(a.frame)
    rows = len(prev)
    host = []
    for k in range(a.repeat + 1):                                  # the first round warms up, as on the device side
        t0 = time.perf_counter()
        want = mr.transition_counts(prev, nxt, A, B)
        if k:
            host.append((time.perf_counter() - t0) * 1e3)
    parts = {k: [] for k in hipnative.Transitions.PARTS}
    wall = dict(count_resident=[], pair_cold=[], relabel=[])
    with hipnative.Transitions(A.shape) as tr:
        for k in range(a.repeat + 1):                              # the first round warms up
            t0 = time.perf_counter()
            tr.frame(A)
            tr.frame(B)
            got = tr.count(prev, nxt)
            cold = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            got = tr.count(prev, nxt)
            warm = (time.perf_counter() - t0) * 1e3
            best = mt.best_src(got[0])
            lut = np.zeros(tr.label_max() + 1, np.int32)
            lut[best[:, 0]] = best[:, 1]
            out = np.empty(A.shape, np.int32)
            t0 = time.perf_counter()
            tr.relabel(lut, out=out)
            paint = (time.perf_counter() - t0) * 1e3
            if k:
                for name, v in tr.kernel_ms_parts().items():
                    parts[name].append(v)
                for name, v in (("count_resident", warm), ("pair_cold", cold), ("relabel", paint)):
                    wall[name].append(v)
        heads, slots = tr.n_heads, tr.table_slots
    res = dict(frame=a.frame, voxels=int(A.size), labelled_share=round(float((B > 0).mean()), 4), rows=rows, keys=int(len(got[0])), dropped=int(got[1]),
               coord_dtype=str(prev.dtype), table_slots=slots, heads=heads, atomic_adds_per_row=round(heads / rows, 4),
               kernel_ms={k: median(v) for k, v in parts.items()}, wall_ms={k: median(v) for k, v in wall.items()},
               restatement_ms=median(host), same_as_restatement=bool(np.array_equal(got[0], want[0]) and got[1] == want[1]),
               relabel_same=bool(np.array_equal(out, mr.relabel(B, want[0]))) if a.frame <= 128 else None,
               repeat=a.repeat, device=hipnative.load().device_name(0))
    line = json.dumps(res)
    print(line, flush=True)
    path = a.out or (os.path.join(REPO, "profiles", "transitions_bench.jsonl") if a.save else None)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
