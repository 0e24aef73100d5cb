"""
Captures tests/golden/image/image_*.npz from the reference's Image class (nellie/feature_extraction/hierarchical.py), driven by a
SimpleNamespace hierarchy:

    python tests/golden/make_golden_image.py /path/to/nellie-reference

Every fixture sits on a component golden and through it on its branch, voxel and node golden (tests/golden/components, branches,
voxels, nodes): the reference's Voxels and Nodes attributes in them are `hierarchy.voxels` and `hierarchy.nodes`.
`hierarchy.branches` is the branch golden's reference attributes with the region columns filled in from
tests/branch_features_restatement.py, and `hierarchy.components` is tests/component_features_restatement.py's Components:
skimage is not installed where this runs, so the reference's own Branches and Components leave their region columns empty, which
Image would index out of range.  `genuine` in every fixture names the statistics whose inputs are reference output; the
aggregation itself is the reference's for every column (layout: tests/image_goldens.py).

The capture checks tests/image_features_restatement.py against everything it stores, bit for bit, and asserts that the set covers
the regimes listed in REGIMES.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402
import branch_goldens as bg  # noqa: E402
import component_goldens as cg  # noqa: E402
import image_features_restatement as ir  # noqa: E402
import image_goldens as ig  # noqa: E402
import node_goldens as ng  # noqa: E402

REGIMES = ("empty frame between full ones", "2-D", "anisotropic 3-D", "skip_nodes", "no_t")


def capture_case(Image, name, seen):
    gc = cg.load("components_" + name)
    base = gc["base"]
    T = base["T"]
    ref, own = Image(ig.hierarchy_double(gc)), ir.Image(ig.hierarchy_double(gc))
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")                           # the mean of an empty frame's one empty group
        ref.run()
        own.run()
    assert list(ref.time) == list(own.time) == list(range(T))
    assert list(ref.image_name) == list(own.image_name) == [base["filename"]] * T
    assert ref.stats_to_aggregate == [] and ref.features_to_save == []
    out = dict(base=np.str_("components_" + name), time=np.array(ref.time, np.int64), image_name=np.array(ref.image_name))
    for level in ig.LEVELS:
        a, b = getattr(ref, f"aggregate_{level}_metrics"), getattr(own, f"aggregate_{level}_metrics")
        if level == "node" and base["skip_nodes"]:
            assert a == [] and b == []
            continue
        stats = ig.stats_of(level, base)
        assert len(a) == len(b) == T
        for t in range(T):
            ng.assert_same_aggregates(b[t], a[t], (name, level, t))
            assert list(a[t]) == stats and all(a[t][s][k].shape == (1, 1) for s in stats for k in ig.KEYS), (name, level, t)
        out[f"agg_{level}"] = np.array([np.concatenate([f[s][k][0] for f in a]) for s in stats for k in ig.KEYS])
    out["genuine"] = np.array(cg.stats_of("vox", base) + list(bg.NODE_STATS) + list(bg.FLOAT32))
    h = ig.hierarchy_double(gc)
    rows = [ir.rows_of(h, t)["voxel"] for t in range(T)]
    for t in range(T):
        if rows[t] == 0:                                          # one group of no values: NaN, and 0 for the sum
            for level in ig.LEVELS:
                for f in getattr(ref, f"aggregate_{level}_metrics")[t:t + 1]:
                    assert all(np.isnan(f[s]["mean"]).all() and (f[s]["sum"] == 0).all() for s in f), (name, level, t)
    if 0 in rows[1:-1] and rows[0] and rows[-1]:
        seen.add("empty frame between full ones")
    seen.add("2-D" if base["D"] == 2 else "anisotropic 3-D" if len(set(base["spacing"])) > 1 else "3-D")
    if base["skip_nodes"]:
        seen.add("skip_nodes")
    if gc["no_t"]:
        seen.add("no_t")
    return out, rows


def main():
    make_golden.REF = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else make_golden.REF
    make_golden._import_reference()
    from nellie.feature_extraction import hierarchical
    os.makedirs(ig.GOLDEN_DIR, exist_ok=True)
    seen = set()
    for cname in cg.names():
        name = cname[len("components_"):]
        out, rows = capture_case(hierarchical.Image, name, seen)
        path = os.path.join(ig.GOLDEN_DIR, "image_" + name + ".npz")
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) < 20_000, (name, os.path.getsize(path))
        print(f"image_{name}: voxels per frame {rows}, {os.path.getsize(path)} B")
    missing = [r for r in REGIMES if r not in seen]
    assert not missing, missing
    print("regimes:", sorted(seen))


if __name__ == "__main__":
    main()
