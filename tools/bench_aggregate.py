"""Device time of one `aggregate()` call (`kernel_ms_parts()["aggregation"]`: every kernel of the call, transfers excluded) on the
two shapes the wide levels of the hierarchy send it, for every threshold `--wide-from` of the block path:

  (a) the image: one group of every index over n float32 values, n = 333 078 (the voxels of the frame below), 1 048 583 and 4 000 000;
  (b) the organelles: the component groups of the voxels of tools/bench_components.py's frame (128 x 512 x 512: 189 groups, the
      largest 8 757).

    python tools/bench_aggregate.py [--wide-from 0 8193 32769] [--repeat 5] [--no-frame]

Per case and threshold: the median of `--repeat` calls after a warm-up, with the smallest and the largest, one JSON line in all.
The outputs of every threshold are compared with those of the first: they must be the same bytes.  A library without
nl_nodefeat_set_wide_from (before section 19) is timed as it is, under the name "as_built".
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
IMAGE_SIZES = (333_078, 1_048_583, 4_000_000)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--wide-from", type=int, nargs="+", default=[0, 8193, 4 * 8192 + 1])
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-frame", action="store_true", help="leave out (b), which builds the 128 x 512 x 512 frame on the host")
    a = ap.parse_args()
    from nellie_amd import build, hipnative
    build.build(verbose=False)
    rng = np.random.default_rng(1)
    cases = {}
    for n in IMAGE_SIZES:
        cases[f"image_{n}"] = (np.array([0, n], np.int64), np.arange(n, dtype=np.int64), n)
    if not a.no_frame:
        from bench_voxels import make_frame
        from nellie_amd.feature_extraction.components import _groups_of
        comp = make_frame((128, 512, 512), 1)[2]
        labels = comp[comp > 0]
        off, idx = _groups_of(np.unique(labels), labels)
        cases["components_frame"] = (off, idx, len(labels))
    out = dict(tool="bench_aggregate", device=hipnative.load().device_name(0), repeat=a.repeat, cases={})
    with hipnative.NodeFeatures() as eng:
        settable = hasattr(eng, "set_wide_from")
        for name, (off, idx, n) in cases.items():
            x = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3, n)).astype(np.float32)
            k = np.diff(off)
            case = dict(values=int(n), groups=int(len(k)), longest=int(k.max()), groups_above_8192=int((k > 8192).sum()), ms={})
            first = None
            for wide_from in (a.wide_from if settable else ["as_built"]):
                if settable:
                    eng.set_wide_from(wide_from)
                ms = []
                for i in range(a.repeat + 1):                     # the first call warms up (allocations, code objects)
                    eng.groups(off, idx)
                    res = eng.aggregate(x)
                    if i:
                        ms.append(eng.kernel_ms_parts()["aggregation"])
                data = b"".join(res[key].tobytes() for key in eng.KEYS)
                first = first or data
                assert data == first, (name, wide_from, "the thresholds disagree")
                case["ms"][str(wide_from)] = dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))
            out["cases"][name] = case
    print(json.dumps(out))


if __name__ == "__main__":
    main()
