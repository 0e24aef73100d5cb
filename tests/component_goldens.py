"""Reading tests/golden/components/*.npz (written by tests/golden/make_golden_components.py) back into the reference's lists per
frame, and the hierarchy double that Components(hierarchy) reads; test infrastructure only.  A fixture `components_<case>.npz` sits
on the branch golden `branches_<case>.npz` (tests/branch_goldens.py) and through it on the voxel and the node golden, whose reference
attributes are the double's `voxels` and `nodes`; the double's `branches` holds the branch golden's reference attributes with the
region columns filled in from tests/branch_features_restatement.py (the reference ran with `regionprops` returning [], which leaves
them empty).  The fixture adds the outputs of the reference's Components, concatenated over the frames with the offsets `comp_off`
(component_label, time) and `col_off` (the columns of the three aggregates: one per label of np.unique(voxels.component_labels[t])
without 0).  `agg_vox` is (55, columns), `agg_node` (20, columns), `agg_branch` (45, columns), the rows in the order of the
statistics times KEYS.  `no_t` is the value of im_info.no_t the reference ran under.

component_label, time, image_name and the three aggregate dicts are the reference's output; the region columns are NOT in the
fixtures (`regions_are_reference_output` is False in every one)."""
import glob
import os
from types import SimpleNamespace

import numpy as np

import branch_features_restatement as br
import branch_goldens as bg
import node_goldens as ng
import voxel_goldens as vg

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(HERE, "golden", "components")
KEYS = ng.KEYS
PER_COMPONENT = ("time", "component_label")
REGION = ("organelle_area", "organelle_axis_length_maj", "organelle_axis_length_min", "organelle_extent", "organelle_solidity", "reassigned_label",
          "z", "y", "x")
STATS_TO_AGGREGATE = list(REGION[:6])
BRANCH_STATS = [s for s in bg.STATS_TO_AGGREGATE if s != "reassigned_label"]
AGGREGATES = (("vox", "aggregate_voxel_metrics"), ("node", "aggregate_node_metrics"), ("branch", "aggregate_branch_metrics"))
same = ng.same


def names():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, "components_*.npz")))


_BRANCHES = {}


def branches_double(gb):
    """a plain object with the lists the reference's Branches filled for the branch golden gb, and the region columns the
    restatement gives for its branch labels (no reassigned labels: NaN).  Built once per golden and shared (do not modify)."""
    if gb["name"] in _BRANCHES:
        return _BRANCHES[gb["name"]]
    base, ref = gb["base"], gb["ref"]
    b = SimpleNamespace(stats_to_aggregate=list(bg.STATS_TO_AGGREGATE), features_to_save=bg.STATS_TO_AGGREGATE + ["x", "y", "z"])
    for k in bg.PER_BRANCH:
        setattr(b, k, list(ref[k]))
    for k in bg.REGION:
        setattr(b, k, [])
    for t in range(base["T"]):
        cols = br.region_columns(base["branch"][t], base["spacing"]) if len(ref["branch_label"][t]) else {k: [] for k in bg.REGION}
        for k in bg.REGION:
            getattr(b, k).append(cols[k])
    _BRANCHES[gb["name"]] = b
    return b


def hierarchy_double(gb, voxels=None, nodes=None, branches=None, reassigned=None, no_t=False, **extra):
    """the object Components(hierarchy) reads: the branch golden's double with `branches` and `im_obj_reassigned`"""
    h = bg.hierarchy_double(gb["base"], gb["skel"], gb["border"], voxels=voxels, nodes=nodes, node_ref=gb["nodes"]["ref"], no_t=no_t,
                            im_obj_reassigned=reassigned, **extra)
    h.branches = branches if branches is not None else branches_double(gb)
    return h


def stats_of(key, base):
    return {"vox": list(base["ref"]["stats_to_aggregate"]), "node": list(bg.NODE_STATS), "branch": list(BRANCH_STATS)}[key]


_CACHE = {}


def load(name):
    """dict: `branches` (the branch golden), `base` (the voxel golden), `no_t` and `ref` = {attribute: list per frame};
    `ref["agg_vox"][t]`, `ref["agg_node"][t]` and `ref["agg_branch"][t]` are {stat: {key: (1, columns) float64}}, {} for a frame
    without components.  Read once and shared (do not modify)."""
    if name in _CACHE:
        return _CACHE[name]
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    gb = bg.load(str(z["base"]))
    base = gb["base"]
    assert not bool(z["regions_are_reference_output"])
    off = z["comp_off"]
    ref = {k: vg.split(z[k], off) for k in PER_COMPONENT}
    # stored as one int64 array: a frame without components has the reference's empty int64 array, every other the labels' dtype
    ref["component_label"] = [a.astype(base["comp"].dtype) if len(a) else a for a in ref["component_label"]]
    empty = [a == b for a, b in zip(off[:-1], off[1:])]
    for key, _ in AGGREGATES:
        if key == "node" and base["skip_nodes"]:
            ref["agg_node"] = []
            continue
        frames = bg._agg_frames(z[f"agg_{key}"], z["col_off"], stats_of(key, base))
        ref[f"agg_{key}"] = [{} if e else f for e, f in zip(empty, frames)]
    out = dict(name=name, branches=gb, base=base, no_t=bool(z["no_t"]), ref=ref)
    _CACHE[name] = out
    return out


def double_of(g, **extra):
    extra.setdefault("no_t", g["no_t"])
    return hierarchy_double(g["branches"], **extra)


def assert_same_components(got, ref, base, frames=None):
    """a Components object against reference lists per frame (a golden's `ref`, or another Components object): every attribute the
    reference computes without regionprops, floats bit for bit"""
    is_dict = isinstance(ref, dict)
    attr = dict(("agg_" + key, name) for key, name in AGGREGATES)
    get = (lambda k: ref[k]) if is_dict else (lambda k: getattr(ref, attr.get(k, k)))
    assert got.stats_to_aggregate == STATS_TO_AGGREGATE and got.features_to_save == STATS_TO_AGGREGATE + ["x", "y", "z"]
    T = base["T"]
    for k in PER_COMPONENT + REGION + ("aggregate_voxel_metrics", "aggregate_branch_metrics", "image_name"):
        assert len(getattr(got, k)) == T, k
    assert len(got.aggregate_node_metrics) == (0 if base["skip_nodes"] else T)
    for t in (range(T) if frames is None else frames):
        R = len(get("component_label")[t])
        for k in PER_COMPONENT:
            a, b = np.asarray(getattr(got, k)[t]), np.asarray(get(k)[t])
            assert same(a, b) and len(a) == R, (k, t, a, b)
        assert got.image_name[t].dtype == object and list(got.image_name[t]) == [base["filename"]] * R
        for key, name in AGGREGATES:
            if key == "node" and base["skip_nodes"]:
                continue
            mine, want = getattr(got, name)[t], get("agg_" + key)[t]
            if R == 0:
                assert mine == {} and want == {}, (key, t)
            else:
                ng.assert_same_aggregates(mine, want, (key, t))


def assert_same_regions(got, own, frames=None):
    """the region columns and the reassigned label of a Components object against the restatement's, bit for bit"""
    for t in (range(len(own.component_label)) if frames is None else frames):
        if len(own.component_label[t]) == 0:
            assert all(getattr(got, k)[t] == [] for k in REGION), t
            continue
        assert same(np.asarray(got.component_label[t]), np.asarray(own.component_label[t])), t
        for k in REGION:
            a, b = np.asarray(getattr(got, k)[t]), np.asarray(getattr(own, k)[t])
            assert a.dtype == np.float64 and same(a, b), (k, t, a, b)
        assert np.isnan(got.organelle_solidity[t]).all()
