"""
Captures tests/golden/components/components_*.npz from the reference's Components class (nellie/feature_extraction/hierarchical.py),
driven by a SimpleNamespace hierarchy:

    python tests/golden/make_golden_components.py /path/to/nellie-reference

Every fixture sits on a branch golden and through it on its voxel and node golden (tests/golden/branches, voxels, nodes): the
reference's Voxels and Nodes attributes in them are `hierarchy.voxels` and `hierarchy.nodes`.  `hierarchy.branches` is the branch
golden's reference attributes with the region columns filled in from tests/branch_features_restatement.py: with the stub below the
reference's Branches leaves them empty lists, which Components would index out of range.

skimage is not installed where this runs, so `regionprops` is replaced in this process by a function that returns []:
component_label, time, image_name and the three aggregate dicts are genuine reference output; the region columns are not captured
(`regions_are_reference_output` = False; layout: tests/component_goldens.py).

The capture checks tests/component_features_restatement.py against everything it stores, bit for bit, and asserts that the set
covers the regimes listed in REGIMES.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402
import branch_goldens as bg  # noqa: E402
import component_features_restatement as cr  # noqa: E402
import component_goldens as cg  # noqa: E402
import node_goldens as ng  # noqa: E402

REGIMES = ("component without nodes", "component without a skeleton label", "empty frame between full ones", "2-D", "anisotropic 3-D", "skip_nodes",
           "no_t")
NO_T = ("3d_t_without_flow",)                                      # the cases captured under im_info.no_t = True


def capture_case(Components, name, seen):
    gb = bg.load("branches_" + name)
    base = gb["base"]
    no_t = name in NO_T
    rng = np.random.default_rng([len(name), 17])
    reassigned = rng.integers(0, 3, base["comp"].shape).astype(np.int32)      # never read: no region is visited
    double = lambda: cg.hierarchy_double(gb, voxels=ng.voxels_double(base, fill_empty_vectors=True), reassigned=reassigned, no_t=no_t)   # noqa: E731
    ref = Components(double())
    with np.errstate(all="ignore"):
        ref.run()
    own = cr.Components(double())
    with np.errstate(all="ignore"):
        own.run(regions=False)
    T = base["T"]
    h = double()
    for t in range(T):
        R = len(ref.component_label[t])
        for k in cg.PER_COMPONENT:
            assert cg.same(np.asarray(getattr(ref, k)[t]), np.asarray(getattr(own, k)[t])), (name, k, t)
        assert list(ref.image_name[t]) == list(own.image_name[t]) == [base["filename"]] * R
        for k in cg.REGION:
            assert getattr(ref, k)[t] == [] and getattr(own, k)[t] == [], (name, k, "regionprops returned []")
        for key, attr in cg.AGGREGATES:
            if key == "node" and base["skip_nodes"]:
                continue
            a, b = getattr(ref, attr)[t], getattr(own, attr)[t]
            if R == 0:
                assert a == b == {}
                continue
            ng.assert_same_aggregates(b, a, (name, key, t))
            assert list(a) == cg.stats_of(key, base) and a[list(a)[0]]["sum"].shape == (1, R), (name, key, t)
        if R == 0:
            continue
        labels = ref.component_label[t]
        listed = np.unique(h.voxels.component_labels[t])
        assert np.array_equal(labels, listed[listed != 0]), (name, t, "one row per label everywhere: the table of this frame can be written")
        if not base["skip_nodes"] and any(l not in set(np.asarray(h.nodes.component_label[t]).tolist()) for l in labels):
            seen.add("component without nodes")
        if any(l not in set(np.asarray(h.branches.component_label[t]).tolist()) for l in labels):
            seen.add("component without a skeleton label")
    counts = [len(a) for a in ref.component_label]
    if 0 in counts[1:-1] and counts[0] and counts[-1]:
        seen.add("empty frame between full ones")
    seen.add("2-D" if base["D"] == 2 else "anisotropic 3-D" if len(set(base["spacing"])) > 1 else "3-D")
    if base["skip_nodes"]:
        seen.add("skip_nodes")
        assert ref.aggregate_node_metrics == []
    if no_t:
        seen.add("no_t")
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    out = dict(base=np.str_("branches_" + name), comp_off=off, col_off=off, no_t=np.bool_(no_t), regions_are_reference_output=np.bool_(False))
    for k in cg.PER_COMPONENT:
        out[k] = np.concatenate([np.asarray(a) for a in getattr(ref, k)])
    for key, attr in cg.AGGREGATES:
        frames = getattr(ref, attr)
        if not frames:
            continue
        out[f"agg_{key}"] = np.array([np.concatenate([f[s][k][0] if f else np.zeros(0) for f in frames]) for s in cg.stats_of(key, base) for k in cg.KEYS])
    return out, counts


def main():
    make_golden.REF = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else make_golden.REF
    make_golden._import_reference()
    from nellie.feature_extraction import hierarchical
    hierarchical.regionprops = lambda *a, **k: []                  # skimage is not installed: no region is visited
    os.makedirs(cg.GOLDEN_DIR, exist_ok=True)
    seen = set()
    for bname in bg.names():
        name = bname[len("branches_"):]
        out, counts = capture_case(hierarchical.Components, name, seen)
        path = os.path.join(cg.GOLDEN_DIR, "components_" + name + ".npz")
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) < 40_000, (name, os.path.getsize(path))
        print(f"components_{name}: components {counts}, {os.path.getsize(path)} B")
    missing = [r for r in REGIMES if r not in seen]
    assert not missing, missing
    print("regimes:", sorted(seen))


if __name__ == "__main__":
    main()
