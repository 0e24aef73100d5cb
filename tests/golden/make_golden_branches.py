"""
Captures tests/golden/branches/branches_*.npz from the reference's Branches class (nellie/feature_extraction/hierarchical.py),
driven by a SimpleNamespace hierarchy:

    python tests/golden/make_golden_branches.py /path/to/nellie-reference

Every fixture sits on a voxel golden and its node golden (tests/golden/voxels, tests/golden/nodes): the reference's Voxels and
Nodes attributes in them are `hierarchy.voxels` and `hierarchy.nodes`.  A skeleton stack is generated here from a stored seed and
kept in the fixture: thin figures inside the branch labels that carry the label of the voxel they lie in, one per label, cycling
through a path (two tips, or a lone voxel where the label has no room), two separate paths (a label in two pieces, four tips), an
L of three voxels (a loop: no tip) and an L with a tail (one tip).  The border is the node golden's; in a frame whose border is a
shell, one lone skeleton voxel (or the first skeleton voxel) gets a border bit: radius 0.

skimage is not installed where this runs, so `regionprops` is replaced in this process by a function that returns []: the four
skeleton statistics, branch_idxs, branch_label, component_label, time, image_name and both aggregate dicts are genuine reference
output; the region columns are not captured (`regions_are_reference_output` = False; layout: tests/branch_goldens.py).

The capture checks tests/branch_features_restatement.py against everything it stores, bit for bit, and asserts that the set covers
the regimes listed in REGIMES.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402
import branch_features_restatement as br  # noqa: E402
import branch_goldens as bg  # noqa: E402
import node_goldens as ng  # noqa: E402
import voxel_goldens as vg  # noqa: E402

REGIMES = ("lone voxel", "one tip", "two tips", "three or more tips", "no tip", "two pieces", "even median count", "odd median count", "swap",
           "radius 0 and aspect NaN", "frame without border", "corner border", "empty frame between full ones", "2-D", "anisotropic 3-D", "skip_nodes")


def neighbours(p, q):
    return max(abs(a - b) for a, b in zip(p, q)) <= 1


def walk(rng, room, taken, longest):
    """a path inside `room` (a set of voxels): every new voxel touches the previous one and no other voxel of the path or of `taken`"""
    free = [p for p in sorted(room) if not any(neighbours(p, q) for q in taken)]
    if not free:
        return []
    path = [free[rng.integers(len(free))]]
    D = len(path[0])
    steps = [d for d in np.ndindex(*(3,) * D) if any(v != 1 for v in d)]
    while len(path) < longest:
        head = path[-1]
        nxt = [tuple(h + d - 1 for h, d in zip(head, step)) for step in steps]
        nxt = [p for p in nxt if p in room and not any(neighbours(p, q) for q in path[:-1]) and not any(neighbours(p, q) for q in taken)]
        if not nxt:
            break
        path.append(nxt[rng.integers(len(nxt))])
    return path


def ell(room, tail):
    """an L of three voxels in the last two axes, with a one-voxel tail straight on from its far end if asked; [] without room"""
    for p in sorted(room):
        a, b, c = p, p[:-1] + (p[-1] + 1,), p[:-2] + (p[-2] + 1, p[-1] + 1)
        d = p[:-2] + (p[-2] + 2, p[-1] + 1)
        if b in room and c in room and (not tail or d in room):
            return [a, b, c] + ([d] if tail else [])
    return []


def make_skeleton(rng, branch):
    skel = np.zeros(branch.shape, np.int32)
    kind = 0
    for t in range(len(branch)):
        for label in np.unique(branch[t][branch[t] > 0]):
            room = set(map(tuple, np.argwhere(branch[t] == label).tolist()))
            figure = []
            if kind % 4 == 1:
                first = walk(rng, room, [], int(rng.integers(2, 5)))
                figure = first + walk(rng, room, first, int(rng.integers(2, 5)))
            elif kind % 4 in (2, 3):
                figure = ell(room, tail=kind % 4 == 3)
            if not figure:
                figure = walk(rng, room, [], int(rng.integers(2, 12)))
            kind += 1
            for p in figure:
                skel[(t,) + p] = label
    return skel


def observe(seen, skel, border, sk, spacing):
    """the regimes one frame shows"""
    if len(sk["branch_idxs"]) == 0:
        return
    lab, deg = sk["labels"], sk["degree"]
    for i, l in enumerate(sk["branch_label"]):
        mine = lab == l
        tips, n = int((deg[mine] == 1).sum()), int(mine.sum())
        seen.add(("one tip", "two tips")[tips - 1] if tips in (1, 2) else "three or more tips" if tips >= 3 else "no tip" if n > 1 else "lone voxel")
        seen.add("even median count" if n % 2 == 0 else "odd median count")
        pts = sk["branch_idxs"][mine]
        linked = {0}
        for _ in range(n):
            linked |= {j for j in range(n) if any(neighbours(pts[j], pts[k]) for k in linked)}
        if len(linked) < n:
            seen.add("two pieces")
        if np.isnan(sk["branch_aspect_ratio"][i]) and sk["branch_thickness"][i] == 0:
            seen.add("radius 0 and aspect NaN")
    med = np.array([np.median(2.0 * sk["radius"][lab == l]) for l in sk["branch_label"]]).astype(np.float32)
    if np.any((med != sk["branch_thickness"]) & ~np.isnan(med)):
        seen.add("swap")
    if not border.any():
        seen.add("frame without border")
    if border.sum() == 1 and border.reshape(-1)[-1]:
        seen.add("corner border")


def capture_case(Branches, name, seen, seed=0):
    g, gn = vg.load("voxels_" + name), ng.load("nodes_" + name)
    rng = np.random.default_rng([seed, len(name), 11])
    skel = make_skeleton(rng, g["branch"])
    border = gn["border"].copy()
    for t in range(g["T"]):
        if border[t].sum() > 1 and skel[t].any():
            idxs = np.argwhere(skel[t] > 0)
            _, degree = br.pair_counts(skel[t], np.unique(skel[t][skel[t] > 0]))
            lone = idxs[degree[tuple(idxs.T)] == 0]
            border[t][tuple((lone[0] if len(lone) else idxs[0]))] = 1
    h = bg.hierarchy_double(g, skel, border, voxels=ng.voxels_double(g, fill_empty_vectors=True), node_ref=gn["ref"])
    ref = Branches(h)
    with np.errstate(all="ignore"):
        ref.run()
    own = br.Branches(bg.hierarchy_double(g, skel, border, node_ref=gn["ref"]))
    own.run(regions=False)
    T = g["T"]
    for t in range(T):
        B = len(ref.branch_label[t])
        assert np.array_equal(ref.branch_idxs[t], own.branch_idxs[t]) and ref.branch_idxs[t].dtype == np.int64
        for k in bg.PER_BRANCH:
            a, b = np.asarray(ref.__dict__[k][t]), np.asarray(own.__dict__[k][t])
            assert (B == 0 and k in bg.FLOAT32 and ref.__dict__[k][t] == own.__dict__[k][t] == []) or bg.same(a, b), (name, k, t, a, b)
        assert list(ref.image_name[t]) == list(own.image_name[t]) == [g["filename"]] * B
        for k in bg.REGION:
            assert ref.__dict__[k][t] == [], (name, k, "regionprops returned []")
        for a, b in ((ref.aggregate_voxel_metrics, own.aggregate_voxel_metrics),) + (() if g["skip_nodes"] else ((ref.aggregate_node_metrics, own.aggregate_node_metrics),)):
            if B == 0:
                assert a[t] == b[t] == {}
            else:
                ng.assert_same_aggregates(b[t], a[t], (name, t))
        # one row per label everywhere: the table of this frame can be written
        regions = np.unique(g["branch"][t][g["branch"][t] > 0])
        assert np.array_equal(regions, ref.branch_label[t]), (name, t, "a branch label without a skeleton voxel")
        if B:
            assert ref.aggregate_voxel_metrics[t]["intensity"]["sum"].shape == (1, B), (name, t)
        observe(seen, skel[t], border[t], br.skeleton_stats(skel[t], border[t], h.spacing), h.spacing)
    counts = [len(a) for a in ref.branch_label]
    if 0 in counts[1:-1] and counts[0] and counts[-1]:
        seen.add("empty frame between full ones")
    seen.add("2-D" if g["D"] == 2 else "anisotropic 3-D" if len(set(g["spacing"])) > 1 else "3-D")
    if g["skip_nodes"]:
        seen.add("skip_nodes")
        assert ref.aggregate_node_metrics == []
    cat = lambda parts, dtype=None: np.concatenate([np.asarray(p, dtype) for p in parts])   # noqa: E731
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    out = dict(base=np.str_("voxels_" + name), nodes=np.str_("nodes_" + name), seed=np.int64(seed), skel=skel, border=border, branch_off=off,
               regions_are_reference_output=np.bool_(False))
    for k in bg.PER_BRANCH:
        out[k] = cat(getattr(ref, k), np.float32 if k in bg.FLOAT32 else None)
    out["branch_idxs"] = np.concatenate([a.reshape(-1, g["D"]) for a in ref.branch_idxs])
    out["idx_off"] = np.concatenate([[0], np.cumsum([len(a) for a in ref.branch_idxs])]).astype(np.int64)
    for key, frames, stats in (("vox", ref.aggregate_voxel_metrics, g["ref"]["stats_to_aggregate"]), ("node", ref.aggregate_node_metrics, bg.NODE_STATS)):
        if not frames:
            continue
        widths = [f[stats[0]]["sum"].shape[1] if f else 0 for f in frames]
        out[f"{key}_off"] = np.concatenate([[0], np.cumsum(widths)]).astype(np.int64)
        out[f"agg_{key}"] = np.array([np.concatenate([f[s][k][0] if f else np.zeros(0) for f in frames]) for s in stats for k in bg.KEYS])
    return out, counts


def main():
    make_golden.REF = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else make_golden.REF
    make_golden._import_reference()
    from nellie.feature_extraction import hierarchical
    hierarchical.regionprops = lambda *a, **k: []                  # skimage is not installed: no region is visited
    os.makedirs(bg.GOLDEN_DIR, exist_ok=True)
    seen = set()
    for vname in vg.names():
        name = vname[len("voxels_"):]
        out, counts = capture_case(hierarchical.Branches, name, seen)
        path = os.path.join(bg.GOLDEN_DIR, "branches_" + name + ".npz")
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) < 400_000, (name, os.path.getsize(path))
        print(f"branches_{name}: branches {counts}, skeleton voxels {np.diff(out['idx_off']).tolist()}, {os.path.getsize(path)} B")
    missing = [r for r in REGIMES if r not in seen]
    assert not missing, missing
    print("regimes:", sorted(seen))


if __name__ == "__main__":
    main()
