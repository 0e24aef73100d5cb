#!/usr/bin/env python3
"""NELLIE_SCALE_ORDER A/B in one process on one resident volume (the switch is read per frame): blocks of Filter + Label steps under each
order, alternating, then -- outside the timed blocks -- the eigen-queue entries per voxel after every walk, in walk order.

    python tools/ab_scale_order.py Z Y X [--seed S] [--aniso] [--orders sigma auto ...] [--rounds R] [--steps K]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from nellie_amd import pipeline as pl
from nellie_amd.synthetic import ANISO_03, ISO_01, make_volume

ap = argparse.ArgumentParser()
ap.add_argument("shape", type=int, nargs=3)
ap.add_argument("--seed", type=int, default=2345)
ap.add_argument("--aniso", action="store_true")
ap.add_argument("--orders", nargs="+", default=["sigma", "auto"])
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--steps", type=int, default=10)
args = ap.parse_args()

shape = tuple(args.shape)
dr = ANISO_03 if args.aniso else ISO_01
p = pl.FilterParams(dim_res=dr)
min_area = pl.min_area_pixels_of(dr)
pipe = pl.FramePipeline(shape)
pipe.load_input(make_volume(shape, args.seed))


def step():
    pipe.filter(None, p)
    return pipe.label(pipe.frangi_threshold(), min_area)


for order in args.orders:                       # warm-up: every order once
    os.environ["NELLIE_SCALE_ORDER"] = order
    step()
ms = {o: [] for o in args.orders}
for _ in range(args.rounds):
    for order in args.orders:
        os.environ["NELLIE_SCALE_ORDER"] = order
        pipe.ctx.sync()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            n = step()
        pipe.ctx.sync()
        ms[order].append(round((time.perf_counter() - t0) / args.steps * 1e3, 3))

# queue entries per voxel after each walk (a stream wait per walk: not timed)
nvox = float(np.prod(shape))
out = {"shape": shape, "seed": args.seed, "aniso": args.aniso, "steps_per_block": args.steps, "orders": {}}
ctx = pipe.ctx
for order in args.orders:
    os.environ["NELLIE_SCALE_ORDER"] = order
    q = []
    hooked = {}
    for name in ("chain_walk", "chain_scale"):
        real = getattr(ctx, name)
        hooked[name] = real
        setattr(ctx, name, (lambda real: lambda *a, **k: (real(*a, **k), q.append(round(ctx.info("queue_entries") / nvox, 4)))[0])(real))
    try:
        n = step()
    finally:
        for name in hooked:
            delattr(ctx, name)
    tr = pipe.trace
    walk = pipe.last_scale_order
    out["orders"][order] = {"ms_per_step": ms[order], "median_ms": float(np.median(ms[order])),
                            "walk_order": [k + 1 for k in walk] if walk is not None else list(range(1, len(tr.scales) + 1)),
                            "queue_entries_per_voxel_in_walk_order": q, "queue_entries_sum": round(sum(q), 4),
                            "mask_fraction_per_scale": [round(s.mask_count / nvox, 4) for s in tr.scales],
                            "fallbacks": pipe.chain_fallbacks, "labels": int(n), "positives": int(tr.n_positive)}
print(json.dumps(out), flush=True)
pipe.close()
