#!/usr/bin/env python3
"""Hu-moment tracking timing per frame pair on synthetic stacks (random textured intensities, Frangi and distance values,
markers at a fixed density): features of one frame (upload included, and device-only) and matching in each mode.
    python tools/bench_tracking.py [Z Y X [markers]]        default: 64x256x256 and 128x512x512, 3 000 markers per frame
One JSON line per shape."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from nellie_amd import hipnative


def stack(shape, n_markers, seed):
    rng = np.random.default_rng(seed)
    out = []
    for t in range(2):
        im = rng.integers(0, 4000, shape, dtype=np.uint16)
        fr = (rng.gamma(1.5, 2.0, shape) * (rng.random(shape) < 0.3)).astype(np.float32)
        dist = np.sqrt(rng.integers(0, 10, shape)).astype(np.float32)
        mk = np.zeros(shape, np.uint8)
        mk.flat[rng.choice(mk.size, n_markers, replace=False)] = 1
        out.append((im, fr, dist, mk))
    return out


def bench(shape, n_markers, reps=5):
    frames = stack(shape, n_markers, 11)
    spacing = (0.2, 0.1, 0.1)
    rec = {"shape": list(shape), "markers": n_markers}
    with hipnative.Tracker(shape, spacing) as trk:
        t_feat = []
        for rep in range(reps):
            for f in frames:
                t0 = time.perf_counter(); trk.frame(*f); t_feat.append(time.perf_counter() - t0)
        match = {}
        for mode in ("dense", "sparse"):
            ts = []
            for rep in range(reps):
                t0 = time.perf_counter(); trk.match(mode, 1.0); ts.append(time.perf_counter() - t0)
            match[mode] = round(min(ts) * 1e3, 3)
    rec.update({"features_ms_with_upload": round(min(t_feat) * 1e3, 3), "match_ms": match,
                "pair_ms_dense": round((min(t_feat) + match["dense"] / 1e3) * 1e3, 3),
                "note": "ms per frame pair = features of the new frame (the previous frame's stay resident) + one match"})
    return rec


if __name__ == "__main__":
    if len(sys.argv) >= 4:
        shapes = [tuple(int(a) for a in sys.argv[1:4])]
        nm = int(sys.argv[4]) if len(sys.argv) > 4 else 3000
    else:
        shapes, nm = [(64, 256, 256), (128, 512, 512)], 3000
    for s in shapes:
        print(json.dumps(bench(s, nm)), flush=True)
