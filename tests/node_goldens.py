"""Reading tests/golden/nodes/*.npz (written by tests/golden/make_golden_nodes.py) back into the reference's lists per frame, and
the hierarchy double that Nodes(hierarchy) reads; test infrastructure only.  A fixture `nodes_<case>.npz` sits on the voxel golden
`voxels_<case>.npz` (tests/voxel_goldens.py), whose reference attributes are the double's `voxels`; it adds the border stack and
the outputs of the reference's Nodes, concatenated over the frames with the offsets `node_off`: `agg` is (55, nodes), the rows in
the order of the voxel statistics times KEYS.  `nodes_synthetic.npz` and `nodes_synthetic_wide.npz` (L from 8192 on) hold calls of
the reference's aggregate_stats_for_class alone."""
import glob
import os
from types import SimpleNamespace

import numpy as np

import voxel_goldens as vg

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(HERE, "golden", "nodes")
KEYS = ("mean", "std_dev", "min", "max", "sum")
PER_NODE = ("time", "nodes", "component_label", "branch_label", "node_thickness", "z", "y", "x", "divergence", "convergence", "vergere")
SYNTHETIC = "nodes_synthetic"
WIDE = "nodes_synthetic_wide"


def names():
    found = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, "nodes_*.npz")))
    return [n for n in found if n not in (SYNTHETIC, WIDE)]


def voxels_double(g, fill_empty_vectors=False):
    """a plain object with the lists the reference's Voxels filled for the voxel golden g.  fill_empty_vectors: a frame of vec01 /
    vec12 with zero rows becomes (n, D) NaN, which is what lets the reference's Nodes run on it."""
    ref = g["ref"]
    v = SimpleNamespace(**{k: list(ref[k]) for k in vg.PER_VOXEL + vg.FLOAT_ATTRS})
    v.stats_to_aggregate, v.features_to_save = list(ref["stats_to_aggregate"]), list(ref["features_to_save"])
    if fill_empty_vectors:
        for name in ("vec01", "vec12"):
            vecs = getattr(v, name)
            for t, a in enumerate(vecs):
                if len(a) == 0 and len(v.coords[t]) > 0:
                    vecs[t] = np.full((len(v.coords[t]), g["D"]), np.nan, np.float32)
    if g["skip_nodes"]:
        v.node_voxel_idxs, v.node_labels, v.node_dim0_lims, v.node_dim1_lims, v.node_dim2_lims = [], [], [], [], []
    else:
        v.node_voxel_idxs = [vg.split_node_lists(*csr) for csr in ref["node_voxel_idxs_csr"]]
        v.node_labels = [vg.split_node_lists(*csr) for csr in ref["node_labels_csr"]]
        v.node_dim0_lims, v.node_dim1_lims, v.node_dim2_lims = (list(ref[f"node_dim{ax}_lims"]) for ax in range(3))
    return v


def hierarchy_double(g, border, voxels=None, **extra):
    """the object Nodes(hierarchy) reads: the voxel golden's double with a border stack, `voxels` and low_memory"""
    extra.setdefault("low_memory", False)
    h = vg.hierarchy_double(g, im_border_mask=border, **extra)
    h.voxels = voxels if voxels is not None else voxels_double(g)
    return h


_CACHE = {}


def load(name):
    """dict: `base` (the voxel golden, loaded), `border`, `longest` (L per frame) and `ref` = {attribute: list per frame};
    `ref["agg"][t]` is {stat: {key: (1, nodes) float64}}.  Read once and shared (do not modify)."""
    if name in _CACHE:
        return _CACHE[name]
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    base = vg.load(str(z["base"]))
    out = dict(name=name, base=base, border=z["border"], longest=[int(v) for v in z["longest"]], seed=int(z["seed"]))
    ref = {}
    if base["skip_nodes"]:
        ref = {k: [] for k in PER_NODE + ("agg",)}
    else:
        off = z["node_off"]
        ref = {k: vg.split(z[k], off) for k in PER_NODE}
        stats = [s for s in base["ref"]["stats_to_aggregate"]]
        rows = [(s, key) for s in stats for key in KEYS]
        ref["agg"] = []
        for a, b in zip(off[:-1], off[1:]):
            frame = {s: {} for s in stats}
            for j, (s, key) in enumerate(rows):
                frame[s][key] = z["agg"][j, a:b][None, :]
            ref["agg"].append(frame)
    out["ref"] = ref
    _CACHE[name] = out
    return out


def _calls(name):
    if name in _CACHE:
        return _CACHE[name]
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    stats = [str(s) for s in z["stats"]]
    calls = []
    for c in range(int(z["n_calls"])):
        child = SimpleNamespace(stats_to_aggregate=list(stats), **{s: [z[f"c{c}_{s}"]] for s in stats})
        want = {s: {key: z[f"c{c}_{s}_{key}"] for key in KEYS} for s in stats}
        calls.append(dict(L=int(z[f"c{c}_L"]), offsets=z[f"c{c}_off"], idx=z[f"c{c}_idx"], child=child, want=want))
    _CACHE[name] = calls
    return calls


def synthetic_calls():
    """[dict(L, offsets, idx, child (stats_to_aggregate and one array per statistic in a list), want {stat: {key: array}})]"""
    return _calls(SYNTHETIC)


def wide_calls():
    """the same for the calls whose L reaches numpy's buffer of 8192 elements and passes it"""
    return _calls(WIDE)


def groups_of(call):
    """the call's groups as the reference takes them: a list of index arrays, an empty group numpy's empty float64 array"""
    return vg.split_node_lists(call["offsets"], call["idx"])


def same(a, b):
    """same shape, dtype and bits; a NaN equals a NaN whatever its sign and payload (the device's and numpy's differ)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return a.tobytes() == b.tobytes()
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes()


def assert_same_aggregates(got, want, what):
    """{stat: {key: array}} equal bit for bit, NaN pattern, shape and dtype included"""
    assert list(got) == list(want), (what, list(got), list(want))
    for stat in want:
        assert tuple(got[stat]) == KEYS, (what, stat)
        for key in KEYS:
            a, b = np.asarray(got[stat][key]), np.asarray(want[stat][key])
            assert a.dtype == np.float64 and same(a, b), (what, stat, key, a, b)


def assert_same_nodes(got, ref, base, frames=None):
    """a Nodes object against reference lists per frame (a golden's `ref`, or another Nodes object): every attribute of every node
    equal, floats bit for bit.  base: the voxel golden or stack behind both."""
    get = (lambda k: ref[k]) if isinstance(ref, dict) else (lambda k: getattr(ref, "aggregate_voxel_metrics" if k == "agg" else k))
    assert got.stats_to_aggregate == ["divergence", "convergence", "vergere", "node_thickness"]
    assert got.features_to_save == got.stats_to_aggregate + ["x", "y", "z"]
    if base["skip_nodes"]:
        for k in PER_NODE + ("aggregate_voxel_metrics", "image_name"):
            assert getattr(got, k) == [], k
        return
    T = base["T"]
    for k in PER_NODE + ("aggregate_voxel_metrics", "image_name"):
        assert len(getattr(got, k)) == T, k
    for t in (range(T) if frames is None else frames):
        m = len(get("nodes")[t])
        for k in PER_NODE:
            a, b = np.asarray(getattr(got, k)[t]), np.asarray(get(k)[t])
            assert same(a, b), (k, t, a, b)
            assert len(a) == m, (k, t)
        assert got.image_name[t].dtype == object and list(got.image_name[t]) == [base["filename"]] * m
        assert_same_aggregates(got.aggregate_voxel_metrics[t], get("agg")[t], t)
