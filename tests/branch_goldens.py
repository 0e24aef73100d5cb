"""Reading tests/golden/branches/*.npz (written by tests/golden/make_golden_branches.py) back into the reference's lists per frame,
and the hierarchy double that Branches(hierarchy) reads; test infrastructure only.  A fixture `branches_<case>.npz` sits on the
voxel golden `voxels_<case>.npz` and the node golden `nodes_<case>.npz`, whose reference attributes are the double's `voxels` and
`nodes`; it adds the skeleton stack `skel`, its own border stack and the outputs of the reference's Branches, concatenated over the
frames with the offsets `branch_off` (per-branch columns), `idx_off` (branch_idxs), `vox_off` and `node_off` (the columns of the
voxel and node aggregates: one per distinct non-zero label of the voxels or the nodes).  `agg_vox` is (55, columns), `agg_node`
(20, columns), the rows in the order of the statistics times KEYS.

The reference ran with `regionprops` returning []: the four skeleton statistics, branch_idxs, branch_label, component_label, time,
image_name and both aggregate dicts are its output; the region columns are NOT in the fixtures (`regions_are_reference_output` is
False in every one)."""
import glob
import os
from types import SimpleNamespace

import numpy as np

import node_goldens as ng
import voxel_goldens as vg

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(HERE, "golden", "branches")
KEYS = ng.KEYS
PER_BRANCH = ("time", "branch_label", "component_label", "branch_length", "branch_thickness", "branch_aspect_ratio", "branch_tortuosity")
FLOAT32 = ("branch_length", "branch_thickness", "branch_aspect_ratio", "branch_tortuosity")
REGION = ("branch_area", "branch_axis_length_maj", "branch_axis_length_min", "branch_extent", "branch_solidity", "reassigned_label", "z", "y", "x")
NODE_STATS = ["divergence", "convergence", "vergere", "node_thickness"]
STATS_TO_AGGREGATE = ["branch_length", "branch_thickness", "branch_aspect_ratio", "branch_tortuosity", "branch_area", "branch_axis_length_maj",
                      "branch_axis_length_min", "branch_extent", "branch_solidity", "reassigned_label"]


def names():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, "branches_*.npz")))


def nodes_double(node_ref, skip_nodes):
    """a plain object with the lists the reference's Nodes filled (a node golden's `ref`)"""
    n = SimpleNamespace(stats_to_aggregate=list(NODE_STATS), features_to_save=NODE_STATS + ["x", "y", "z"])
    for k in ("branch_label", "component_label", "nodes", "x", "y", "z") + tuple(NODE_STATS):
        setattr(n, k, [] if skip_nodes else list(node_ref[k]))
    return n


def hierarchy_double(base, skel, border, voxels=None, nodes=None, node_ref=None, reassigned=None, no_t=False, **extra):
    """the object Branches(hierarchy) reads: the voxel golden's (or a scene's) double with the skeleton and border stacks, `voxels`,
    `nodes`, `im_branch_reassigned`, low_memory and use_gpu"""
    extra.setdefault("low_memory", False)
    h = vg.hierarchy_double(base, im_border_mask=border, im_skel=skel, im_branch_reassigned=reassigned, use_gpu=False, **extra)
    h.im_info.no_t = no_t
    h.voxels = voxels if voxels is not None else ng.voxels_double(base)
    h.nodes = nodes if nodes is not None else nodes_double(node_ref, base["skip_nodes"])
    return h


def _agg_frames(table, off, stats):
    frames = []
    rows = [(s, key) for s in stats for key in KEYS]
    for a, b in zip(off[:-1], off[1:]):
        frame = {s: {} for s in stats}
        for j, (s, key) in enumerate(rows):
            frame[s][key] = table[j, a:b][None, :]
        frames.append(frame)
    return frames


_CACHE = {}


def load(name):
    """dict: `base` (the voxel golden), `nodes` (the node golden), `skel`, `border` and `ref` = {attribute: list per frame};
    `ref["agg_vox"][t]` / `ref["agg_node"][t]` are {stat: {key: (1, columns) float64}}, {} for a frame without branches.  Read once
    and shared (do not modify)."""
    if name in _CACHE:
        return _CACHE[name]
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    base = vg.load(str(z["base"]))
    nodes = ng.load(str(z["nodes"]))
    assert not bool(z["regions_are_reference_output"])
    out = dict(name=name, base=base, nodes=nodes, skel=z["skel"], border=z["border"], seed=int(z["seed"]))
    off = z["branch_off"]
    ref = {k: vg.split(z[k], off) for k in PER_BRANCH}
    ref["branch_idxs"] = vg.split(z["branch_idxs"], z["idx_off"])
    # stored as one int64 array: a frame without branches has the reference's empty int64 array, every other the labels' dtype
    ref["component_label"] = [a.astype(base["comp"].dtype) if len(a) else a for a in ref["component_label"]]
    empty = [a == b for a, b in zip(off[:-1], off[1:])]
    vox = _agg_frames(z["agg_vox"], z["vox_off"], base["ref"]["stats_to_aggregate"])
    ref["agg_vox"] = [{} if e else f for e, f in zip(empty, vox)]
    if base["skip_nodes"]:
        ref["agg_node"] = []
    else:
        node = _agg_frames(z["agg_node"], z["node_off"], NODE_STATS)
        ref["agg_node"] = [{} if e else f for e, f in zip(empty, node)]
    out["ref"] = ref
    _CACHE[name] = out
    return out


def double_of(g, **extra):
    return hierarchy_double(g["base"], g["skel"], g["border"], node_ref=g["nodes"]["ref"], **extra)


same = ng.same


def assert_same_skeleton(got, ref, base, frames=None):
    """a Branches object against reference lists per frame (a golden's `ref`, or another Branches object): every attribute the
    reference computes without regionprops, floats bit for bit"""
    is_dict = isinstance(ref, dict)
    get = (lambda k: ref[k]) if is_dict else (lambda k: getattr(ref, {"agg_vox": "aggregate_voxel_metrics", "agg_node": "aggregate_node_metrics"}.get(k, k)))
    assert got.stats_to_aggregate == STATS_TO_AGGREGATE and got.features_to_save == STATS_TO_AGGREGATE + ["x", "y", "z"]
    T = base["T"]
    for k in PER_BRANCH + ("branch_idxs", "aggregate_voxel_metrics", "image_name"):
        assert len(getattr(got, k)) == T, k
    assert len(got.aggregate_node_metrics) == (0 if base["skip_nodes"] else T)
    for t in (range(T) if frames is None else frames):
        B = len(get("branch_label")[t])
        a, b = np.asarray(got.branch_idxs[t]), np.asarray(get("branch_idxs")[t])
        assert a.dtype == np.int64 and a.shape == b.shape == (len(b), base["D"]) and np.array_equal(a, b), ("branch_idxs", t)
        for k in PER_BRANCH:
            a, b = np.asarray(getattr(got, k)[t]), np.asarray(get(k)[t])
            if B == 0 and k in FLOAT32:
                assert getattr(got, k)[t] == [], (k, t)            # the reference's empty list
                continue
            assert same(a, b), (k, t, a, b)
            assert len(a) == B and (k not in FLOAT32 or a.dtype == np.float32), (k, t)
        assert got.image_name[t].dtype == object and list(got.image_name[t]) == [base["filename"]] * B
        for key in ("agg_vox",) + (() if base["skip_nodes"] else ("agg_node",)):
            mine = getattr(got, {"agg_vox": "aggregate_voxel_metrics", "agg_node": "aggregate_node_metrics"}[key])[t]
            want = get(key)[t]
            if B == 0:
                assert mine == {} and want == {}, (key, t)
            else:
                ng.assert_same_aggregates(mine, want, (key, t))


def assert_same_regions(got, own, frames=None):
    """the region columns and the reassigned label of a Branches object against the restatement's, bit for bit"""
    for t in (range(len(own.branch_label)) if frames is None else frames):
        if len(own.branch_label[t]) == 0:
            assert all(getattr(got, k)[t] == [] for k in REGION), t
            continue
        assert np.array_equal(got.region_label[t], own.region_label[t]), t
        for k in REGION:
            a, b = np.asarray(getattr(got, k)[t]), np.asarray(getattr(own, k)[t])
            assert a.dtype == np.float64 and same(a, b), (k, t, a, b)
        assert np.isnan(got.branch_solidity[t]).all()
