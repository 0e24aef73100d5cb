"""
Captures tests/golden/adjacency/adjacency_*.npz from the reference's Hierarchy._save_adjacency_maps
(nellie/feature_extraction/hierarchical.py), called as a plain function on a SimpleNamespace hierarchy:

    python tests/golden/make_golden_adjacency.py /path/to/nellie-reference

One fixture per image golden (tests/golden/image): the hierarchy double is that golden's (tests/adjacency_goldens.py), with a
temporary pipeline_paths["adjacency_maps"]; the pickle the reference writes there is read back and stored (layout:
tests/adjacency_goldens.py).  Neither skimage nor a GPU is needed.

The capture checks tests/adjacency_restatement.py against everything it stores and asserts that the set covers the regimes listed in
REGIMES.
"""
import os
import pickle
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402
import adjacency_goldens as ag  # noqa: E402
import adjacency_restatement as ar  # noqa: E402
import image_goldens as ig  # noqa: E402

REGIMES = ("empty frame between full ones", "2-D", "anisotropic 3-D", "skip_nodes", "no_t", "a voxel with two or more nodes", "a voxel without a node")


def capture_case(save, gi, tmp, seen):
    base = gi["base"]
    h = ag.double_of_image(gi)
    h.im_info.pipeline_paths = {"adjacency_maps": os.path.join(tmp, gi["name"] + ".pkl")}
    save(h)
    with open(h.im_info.pipeline_paths["adjacency_maps"], "rb") as f:
        ref = pickle.load(f)
    assert ar.same_lists(ar.adjacency_lists(ag.double_of_image(gi)), ref)
    T = base["T"]
    assert len(ref["v_b"]) == len(ref["v_o"]) == len(ref["b_o"]) == T
    assert [len(ref[k]) for k in ("v_n", "n_b", "n_o")] == [0 if base["skip_nodes"] else T] * 3
    rows = [len(c) for c in h.voxels.coords]
    if 0 in rows[1:-1] and rows[0] and rows[-1]:
        seen.add("empty frame between full ones")
    seen.add("2-D" if base["D"] == 2 else "anisotropic 3-D" if len(set(base["spacing"])) > 1 else "3-D")
    if base["skip_nodes"]:
        seen.add("skip_nodes")
    if gi["components"]["no_t"]:
        seen.add("no_t")
    for t, edges in enumerate(ref["v_n"]):
        per_voxel = np.bincount(edges[:, 0], minlength=rows[t])
        if rows[t] and per_voxel.max() >= 2:
            seen.add("a voxel with two or more nodes")
        if rows[t] and per_voxel.min() == 0:
            seen.add("a voxel without a node")
    return ref


def main():
    make_golden.REF = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else make_golden.REF
    make_golden._import_reference()
    from nellie.feature_extraction import hierarchical
    os.makedirs(ag.GOLDEN_DIR, exist_ok=True)
    seen = set()
    with tempfile.TemporaryDirectory() as tmp:
        for iname in ig.names():
            ref = capture_case(hierarchical.Hierarchy._save_adjacency_maps, ig.load(iname), tmp, seen)
            path = os.path.join(ag.GOLDEN_DIR, "adjacency_" + iname[len("image_"):] + ".npz")
            np.savez_compressed(path, base=np.str_(iname), **ag.pack(ref))
            assert os.path.getsize(path) < 20_000, (iname, os.path.getsize(path))
            print(f"adjacency_{iname[len('image_'):]}: edges {({k: [len(a) for a in ref[k]] for k in ar.KEYS})}, {os.path.getsize(path)} B")
    missing = [r for r in REGIMES if r not in seen]
    assert not missing, missing
    print("regimes:", sorted(seen))


if __name__ == "__main__":
    main()
