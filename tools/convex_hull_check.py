"""Runs the host hull builder (nellie_amd/csrc/convex_hull.h) under AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone
program (tools/convex_hull_check.cpp) on every region of tests/golden/solidity and of `labels` / `relabelled` of
tests/golden/network_steps, on all their voxels and on their row ends, against the facets and counts of the exact restatement
(tests/solidity_restatement.py).

    python tools/convex_hull_check.py [--cxx c++]
"""
import argparse
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
import solidity_restatement as sr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cxx", default="c++")
    a = ap.parse_args()
    frames = [np.load(p)["labels"] for p in sorted(glob.glob(os.path.join(REPO, "tests", "golden", "solidity", "*.npz")))]
    for p in sorted(glob.glob(os.path.join(REPO, "tests", "golden", "network_steps", "*.npz"))):
        z = np.load(p)
        frames += [z["labels"], z["relabelled"]]
    with tempfile.TemporaryDirectory() as tmp:
        data, exe = os.path.join(tmp, "regions.txt"), os.path.join(tmp, "convex_hull_check")
        with open(data, "w") as f:
            for frame in frames:
                for _, c, e in sr.regions_of(frame):
                    facets = sr.exact_facets(c)
                    count = sr.count_facets(facets, [int(v) for v in e])
                    ext = [1] * (3 - len(e)) + [int(v) for v in e]
                    for cand in (c, sr.row_ends(c)):
                        f.write(f"{c.shape[1]} {len(cand)} {len(facets)} {count} {ext[0]} {ext[1]} {ext[2]}\n")
                        f.write("\n".join(" ".join(str(int(v)) for v in row) for row in cand) + "\n")
        subprocess.check_call([a.cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                               os.path.join(REPO, "tools", "convex_hull_check.cpp"), "-o", exe])
        return subprocess.call([exe, data])


if __name__ == "__main__":
    sys.exit(main())
