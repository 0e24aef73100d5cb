"""Reading tests/golden/image/*.npz (written by tests/golden/make_golden_image.py) back into the reference's lists per frame, and
the hierarchy double that Image(hierarchy) reads; test infrastructure only.  A fixture `image_<case>.npz` sits on the component
golden `components_<case>.npz` (tests/component_goldens.py) and through it on the branch, the voxel and the node golden.  The
double's `voxels` and `nodes` are those goldens' reference attributes; its `branches` holds the branch golden's reference attributes
with the region columns of tests/branch_features_restatement.py; its `components` is tests/component_features_restatement.py's
Components on the component golden's double (the reference ran with `regionprops` returning [], which leaves the region columns
empty, and Image would index them out of range).

The fixture holds the outputs of the reference's Image, one column per frame: `agg_voxel` (55, T), `agg_node` (20, T, absent under
skip_nodes), `agg_branch` (45, T) and `agg_component` (25, T), the rows in the order of the statistics times KEYS, and `time`.
`genuine` names the statistics whose inputs are the reference's own output (the voxel and node statistics and the four skeleton
statistics of the branches); the others are the reference's aggregation of restated region columns."""
import glob
import os

import numpy as np

import branch_goldens as bg
import component_features_restatement as cr
import component_goldens as cg
import node_goldens as ng

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(HERE, "golden", "image")
KEYS = ng.KEYS
LEVELS = ("voxel", "node", "branch", "component")
COMPONENT_STATS = [s for s in cg.STATS_TO_AGGREGATE if s != "reassigned_label"]
same = ng.same


def names():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, "image_*.npz")))


_COMPONENTS = {}


def components_double(gc):
    """the restatement's Components of the component golden gc, region columns included (no reassigned labels: NaN).  Built once
    per golden and shared (do not modify)."""
    if gc["name"] not in _COMPONENTS:
        own = cr.Components(cg.double_of(gc, voxels=ng.voxels_double(gc["base"], fill_empty_vectors=True)))
        with np.errstate(all="ignore"):
            own.run()
        own.hierarchy = None
        _COMPONENTS[gc["name"]] = own
    return _COMPONENTS[gc["name"]]


def hierarchy_double(gc, components=None, **extra):
    """the object Image(hierarchy) reads: the component golden's double with `components`"""
    extra.setdefault("voxels", ng.voxels_double(gc["base"], fill_empty_vectors=True))
    h = cg.double_of(gc, **extra)
    h.components = components if components is not None else components_double(gc)
    return h


def stats_of(level, base):
    return cg.stats_of("vox", base) if level == "voxel" else COMPONENT_STATS if level == "component" else cg.stats_of(level, base)


_CACHE = {}


def load(name):
    """dict: `components` (the component golden), `base` (the voxel golden), `genuine` and `ref` = {attribute: list per frame};
    `ref["agg_<level>"][t]` is {stat: {key: (1, 1) float64}}, `ref["agg_node"]` [] under skip_nodes.  Read once and shared."""
    if name in _CACHE:
        return _CACHE[name]
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    gc = cg.load(str(z["base"]))
    base = gc["base"]
    T = base["T"]
    ref = dict(time=[int(t) for t in z["time"]], image_name=[str(s) for s in z["image_name"]])
    off = np.arange(T + 1)
    for level in LEVELS:
        if level == "node" and base["skip_nodes"]:
            ref["agg_node"] = []
            continue
        ref[f"agg_{level}"] = bg._agg_frames(z[f"agg_{level}"], off, stats_of(level, base))
    out = dict(name=name, components=gc, base=base, genuine=[str(s) for s in z["genuine"]], ref=ref)
    _CACHE[name] = out
    return out


def double_of(g, **extra):
    return hierarchy_double(g["components"], **extra)


def assert_same_image(got, ref, base):
    """an Image object against reference lists per frame (a golden's `ref`, or another Image object): every attribute, floats bit
    for bit, shapes and dtypes included"""
    get = (lambda k: ref[k]) if isinstance(ref, dict) else (lambda k: getattr(ref, f"aggregate_{k[4:]}_metrics" if k.startswith("agg_") else k))
    T = base["T"]
    assert got.stats_to_aggregate == [] and got.features_to_save == []
    assert list(got.time) == list(get("time")) == list(range(T))
    assert list(got.image_name) == list(get("image_name")) == [base["filename"]] * T
    for level in LEVELS:
        mine, want = getattr(got, f"aggregate_{level}_metrics"), get(f"agg_{level}")
        if level == "node" and base["skip_nodes"]:
            assert mine == [] and list(want) == []
            continue
        assert len(mine) == len(want) == T, level
        for t in range(T):
            ng.assert_same_aggregates(mine[t], want[t], (level, t))
            assert all(mine[t][s][key].shape == (1, 1) for s in mine[t] for key in KEYS), (level, t)
