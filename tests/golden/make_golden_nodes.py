"""
Captures tests/golden/nodes/nodes_*.npz from the reference's Nodes class and aggregate_stats_for_class
(nellie/feature_extraction/hierarchical.py), driven by a SimpleNamespace hierarchy:

    python tests/golden/make_golden_nodes.py /path/to/nellie-reference

Every fixture sits on a voxel golden (tests/golden/voxels, read through tests/voxel_goldens.py): the reference's Voxels attributes
in it are `hierarchy.voxels`, and a border stack is generated here from a stored seed.  A fixture holds only that border stack and
what the reference's Nodes filled (layout: tests/node_goldens.py), with L, the longest voxel list, per frame.  A frame of vec01 /
vec12 with zero rows (no voxel had a flow neighbour) is handed to the reference as (n, D) NaN: its Nodes raises on the empty array.

Border per frame (BORDERS): "shell" = the background voxels that touch a labelled one plus 0.5 % of all voxels, "empty" = none,
"corner" = the last voxel of the frame alone.

nodes_synthetic.npz: calls of aggregate_stats_for_class alone with the groups handed in, one per L of SYNTHETIC_L, over float32,
uint16 and float64 statistics and a 2-D one (skipped); 10 % of the float values are NaN, one group is empty, one all NaN, one made
of -0.0 only, one as long as L.

nodes_synthetic_wide.npz: the same kind of call for every L of WIDE_L, at and past numpy's reduction buffer of 8192 elements
(`python tests/golden/make_golden_nodes.py /path/to/nellie-reference synthetic_wide` writes it alone): the same special groups,
groups of every k of WIDE_K that fits, and groups of L - 1 and L // 2 + 3; the groups are strided ranges over 1500 values, which
are unsorted and repeat, and keep the file small.

The capture checks tests/node_features_restatement.py against everything it stores, bit for bit, and asserts that the set covers
the three regimes of the summation tree (L < 8, 8 <= L <= 128, L > 128) and that in the anisotropic 3-D fixture some node's
nearest border voxel in um is not its nearest in voxels.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402
import node_features_restatement as nr  # noqa: E402
import node_goldens as ng  # noqa: E402
import voxel_goldens as vg  # noqa: E402

# per frame of the four; a case not listed has a shell in every frame
BORDERS = {
    "3d_sparse_flow": ("shell", "empty", "corner", "shell"),
    "2d_aniso": ("shell", "corner", "shell", "empty"),
    "3d_integer_flow": ("shell", "shell", "corner", "shell"),
    "2d_no_motility": ("corner", "shell", "shell", "shell"),
}
SYNTHETIC_L = (1, 7, 8, 9, 127, 128, 129, 136, 255, 256, 257, 1000)
SYNTHETIC_STATS = ("f32", "u16", "f64", "vec2d")
WIDE_L = (8192, 8193, 16_385, 20_011)
WIDE_K = (1, 7, 129, 8191, 8192, 8193)


def make_border(rng, comp, modes):
    border = np.zeros(comp.shape, np.uint8)
    for t, mode in enumerate(modes):
        if mode == "corner":
            border[t].reshape(-1)[-1] = 1
        elif mode == "shell":
            on = comp[t] > 0
            near = np.zeros_like(on)
            for ax in range(on.ndim):
                for step in (1, -1):
                    moved = np.roll(on, step, axis=ax)
                    edge = [slice(None)] * on.ndim
                    edge[ax] = 0 if step == 1 else -1
                    moved[tuple(edge)] = False
                    near |= moved
            border[t] = ((near & ~on) | (rng.random(on.shape) < 0.005)) * rng.integers(1, 4, on.shape)
    return border


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def same_aggregates(got, want, what):
    assert list(got) == list(want), what
    for stat in want:
        for key in ng.KEYS:
            assert same(got[stat][key], want[stat][key]), (what, stat, key)


def nearest_differs(border, nodes, spacing):
    """does some node have a nearest border voxel in um that is not (one of) its nearest in voxels?"""
    b = np.argwhere(border).astype(np.float64)
    if len(b) == 0 or len(nodes) == 0:
        return False
    d = nodes[:, None, :].astype(np.float64) - b[None, :, :]
    vox, um = (d * d).sum(axis=2), (d * spacing * d * spacing).sum(axis=2)
    at = np.argmin(um, axis=1)
    return bool(np.any(vox[np.arange(len(nodes)), at] > vox.min(axis=1)))


def capture_case(Nodes, name, seed=0):
    g = vg.load("voxels_" + name)
    rng = np.random.default_rng([seed, len(name), 7])
    border = make_border(rng, g["comp"], BORDERS.get(name, ("shell",) * g["T"]))
    h = ng.hierarchy_double(g, border, voxels=ng.voxels_double(g, fill_empty_vectors=True))
    ref = Nodes(h)
    with np.errstate(all="ignore"):
        ref.run()
    own = nr.Nodes(ng.hierarchy_double(g, border))              # the restatement reads the zero-row vectors as they are
    own.run()
    out = dict(base=np.str_("voxels_" + name), seed=np.int64(seed), border=border)
    if g["skip_nodes"]:
        for k in ng.PER_NODE + ("aggregate_voxel_metrics",):
            assert getattr(ref, k) == [] and getattr(own, k) == [], (name, k)
        out["longest"] = np.zeros(0, np.int64)
        return out, []
    longest = [max((len(a) for a in h.voxels.node_voxel_idxs[t]), default=0) for t in range(g["T"])]
    assert longest == own.longest, (name, longest, own.longest)
    for t in range(g["T"]):
        for k in ng.PER_NODE:
            want = np.asarray(getattr(ref, k)[t])
            want = want.astype(np.float64) if k in nr.NODE_STATS and want.size == 0 else want       # an empty Python list
            assert same(getattr(own, k)[t], want), (name, k, t, "the restatement is not bit-equal")
        assert list(ref.image_name[t]) == list(own.image_name[t]) == [g["filename"]] * len(ref.nodes[t])
        same_aggregates(own.aggregate_voxel_metrics[t], ref.aggregate_voxel_metrics[t], (name, t))
    off = np.concatenate([[0], np.cumsum([len(a) for a in ref.nodes])]).astype(np.int64)
    for k in ng.PER_NODE:
        parts = [np.asarray(a, np.float64) if k in nr.NODE_STATS else np.asarray(a) for a in getattr(ref, k)]
        out[k] = np.concatenate(parts) if k != "nodes" else np.concatenate([p.reshape(-1, g["D"]) for p in parts])
    stats = [s for s in h.voxels.stats_to_aggregate]
    out["agg"] = np.array([np.concatenate([ref.aggregate_voxel_metrics[t][s][key][0] for t in range(g["T"])]) for s in stats for key in ng.KEYS])
    assert out["agg"].shape == (55, off[-1]) and out["agg"].dtype == np.float64
    out.update(node_off=off, longest=np.asarray(longest, np.int64))
    if name == "3d_aniso":
        assert any(nearest_differs(border[t], ref.nodes[t], g["spacing"]) for t in range(g["T"])), "no node whose nearest voxel differs in um"
    return out, longest


def capture_synthetic(aggregate, seed=3):
    rng = np.random.default_rng(seed)
    out = dict(stats=np.asarray(SYNTHETIC_STATS), n_calls=np.int64(len(SYNTHETIC_L)))
    n = 400
    for c, L in enumerate(SYNTHETIC_L):
        f64 = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3, n)
        hole = rng.random(n) < 0.1
        hole[:4] = True                                            # the all-NaN group draws from these
        hole[4:8] = False
        f64[hole] = np.nan
        f64[4:8] = -0.0                                            # the -0.0 group from these
        f32 = f64.astype(np.float32)
        u16 = rng.integers(0, 65536, n).astype(np.uint16)
        u16[4:8] = 0
        child = SimpleNamespace(stats_to_aggregate=list(SYNTHETIC_STATS), f32=[f32], u16=[u16], f64=[f64], vec2d=[rng.random((n, 2)).astype(np.float32)])
        lens = [L, 0, min(L, 5), min(L, 9), L] + [int(v) for v in rng.integers(0, L + 1, 6)]
        groups = [rng.integers(0, n, k) for k in lens]             # unsorted, with repeats, overlapping
        groups[2] = rng.integers(0, 4, lens[2])
        groups[3] = rng.integers(4, 8, lens[3])
        groups = [np.array([]) if len(a) == 0 else a.astype(np.int64) for a in groups]
        with np.errstate(all="ignore"):
            want = aggregate(child, 0, groups)
        own = nr.aggregate_stats_for_class(child, 0, groups)
        same_aggregates(own, want, ("synthetic", L))
        assert all(want["vec2d"][key].shape == (0,) for key in ng.KEYS) and want["f64"]["sum"].shape == (1, len(groups))
        assert np.isnan(want["f64"]["mean"][0, 2]) and want["f64"]["sum"][0, 2] == 0.0 and np.isnan(want["f64"]["max"][0, 1])
        off, idx = nr.as_csr(groups)
        out.update({f"c{c}_L": np.int64(L), f"c{c}_off": off, f"c{c}_idx": idx})
        for s in SYNTHETIC_STATS:
            out[f"c{c}_{s}"] = getattr(child, s)[0]
            for key in ng.KEYS:
                out[f"c{c}_{s}_{key}"] = want[s][key]
    return out


def capture_wide(aggregate, seed=5):
    rng = np.random.default_rng(seed)
    out = dict(stats=np.asarray(SYNTHETIC_STATS), n_calls=np.int64(len(WIDE_L)))
    n = 1500
    for c, L in enumerate(WIDE_L):
        f64 = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3, n)
        hole = rng.random(n) < 0.1
        hole[:4] = True                                            # the all-NaN group reads these
        hole[4:8] = False
        f64[hole] = np.nan
        f64[4:8] = -0.0                                            # the -0.0 group these
        f32 = f64.astype(np.float32)
        u16 = rng.integers(0, 65536, n).astype(np.uint16)
        u16[4:8] = 0
        child = SimpleNamespace(stats_to_aggregate=list(SYNTHETIC_STATS), f32=[f32], u16=[u16], f64=[f64], vec2d=[rng.random((n, 2)).astype(np.float32)])
        lens = [L, 0, 5, 9, L] + [k for k in WIDE_K if k <= L] + [L - 1, L // 2 + 3]
        groups = [(3 + 5 * j + (7 + 6 * j) * np.arange(k)) % n for j, k in enumerate(lens)]       # strided: unsorted, with repeats, overlapping
        groups[2] = np.arange(lens[2]) % 4
        groups[3] = 4 + np.arange(lens[3]) % 4
        groups[4] = groups[4][::-1]
        groups = [np.array([]) if len(a) == 0 else a.astype(np.int64) for a in groups]
        with np.errstate(all="ignore"):
            want = aggregate(child, 0, groups)
        own = nr.aggregate_stats_for_class(child, 0, groups)
        same_aggregates(own, want, ("wide", L))
        assert max(len(a) for a in groups) == L and want["f64"]["sum"].shape == (1, len(groups))
        assert np.isnan(want["f64"]["mean"][0, 2]) and want["f64"]["sum"][0, 2] == 0.0 and np.isnan(want["f64"]["max"][0, 1])
        assert np.signbit(want["f64"]["min"][0, 3]) and not np.signbit(want["f64"]["sum"][0, 3])
        off, idx = nr.as_csr(groups)
        out.update({f"c{c}_L": np.int64(L), f"c{c}_off": off, f"c{c}_idx": idx})
        for s in SYNTHETIC_STATS:
            out[f"c{c}_{s}"] = getattr(child, s)[0]
            for key in ng.KEYS:
                out[f"c{c}_{s}_{key}"] = want[s][key]
    return out


def main():
    make_golden.REF = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else make_golden.REF
    make_golden._import_reference()
    from nellie.feature_extraction.hierarchical import Nodes, aggregate_stats_for_class
    os.makedirs(ng.GOLDEN_DIR, exist_ok=True)
    only = sys.argv[2:]
    seen = list(SYNTHETIC_L)
    for vname in vg.names():
        name = vname[len("voxels_"):]
        if only and name not in only:
            continue
        out, longest = capture_case(Nodes, name)
        path = os.path.join(ng.GOLDEN_DIR, "nodes_" + name + ".npz")
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) < 400_000, (name, os.path.getsize(path))
        assert len(out["longest"]) == (0 if vg.load(vname)["skip_nodes"] else vg.load(vname)["T"])
        seen += longest
        print(f"nodes_{name}: nodes {np.diff(out['node_off']).tolist() if 'node_off' in out else []}, L {longest}, {os.path.getsize(path)} B")
    if not only or "synthetic_wide" in only:
        path = os.path.join(ng.GOLDEN_DIR, ng.WIDE + ".npz")
        np.savez_compressed(path, **capture_wide(aggregate_stats_for_class))
        assert os.path.getsize(path) < 400_000, os.path.getsize(path)
        print(f"{ng.WIDE}: L {list(WIDE_L)}, {os.path.getsize(path)} B")
    if not only:
        path = os.path.join(ng.GOLDEN_DIR, ng.SYNTHETIC + ".npz")
        np.savez_compressed(path, **capture_synthetic(aggregate_stats_for_class))
        assert os.path.getsize(path) < 400_000, os.path.getsize(path)
        frames = seen[len(SYNTHETIC_L):]
        assert any(0 < v < 8 for v in seen) and any(8 <= v <= 128 for v in frames) and any(v > 128 for v in frames), seen
        print(f"{ng.SYNTHETIC}: L {list(SYNTHETIC_L)}, {os.path.getsize(path)} B; frames' L: {sorted(set(frames))}")


if __name__ == "__main__":
    main()
