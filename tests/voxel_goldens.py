"""Reading tests/golden/voxels/*.npz (written by tests/golden/make_golden_voxels.py) back into the reference's lists per frame;
test infrastructure only.  Per-voxel attributes are stored concatenated over the frames with their own offsets `<name>_off`
(a frame of `vec01` / `vec12` in which no voxel had a flow neighbour has zero rows in the reference); the node lists as CSR per
frame (`node_labels_<t>_off / _val`, `node_voxel_idxs_<t>_off / _val`)."""
import glob
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(HERE, "golden", "voxels")
PER_VOXEL = ("time", "coords", "x", "y", "z", "intensity", "structure", "branch_labels", "component_labels")
FLOAT_ATTRS = ("vec01", "vec12", "linear_vel_vector", "linear_vel", "angular_vel_vector", "angular_vel", "linear_acc", "angular_acc",
               "rel_linear_vel", "rel_angular_vel", "rel_linear_acc", "rel_angular_acc", "rel_directionality")
INPUTS = ("comp", "branch", "raw", "struct", "pixel_class", "distance")


def names():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, "*.npz")))


def split(values, offsets):
    return [values[a:b] for a, b in zip(offsets[:-1], offsets[1:])]


def split_node_lists(offsets, values):
    """CSR -> list of arrays as the reference builds them: np.array(list of indices), so an empty list is an empty float64
    array and every other one int64"""
    return [np.array([]) if a == b else np.asarray(values[a:b], np.int64) for a, b in zip(offsets[:-1], offsets[1:])]


_CACHE = {}


def load(name):
    """dict: the inputs, spacing, dt, flags, and `ref` = {attribute: list per frame}; read once and shared (do not modify)"""
    if name in _CACHE:
        return _CACHE[name]
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    g = {k: z[k] for k in INPUTS + ("flow", "spacing")}
    g.update(name=name, dt=float(z["dt"]), skip_nodes=bool(z["skip_nodes"]), enable_motility=bool(z["enable_motility"]),
             T=len(z["comp"]), D=z["comp"].ndim - 1, filename=str(z["filename"]), margin=float(z["margin"]), gap=float(z["gap"]))
    ref = {k: split(z[k], z[k + "_off"]) for k in PER_VOXEL + FLOAT_ATTRS}
    ref["stats_to_aggregate"] = [str(s) for s in z["stats_to_aggregate"]]
    ref["features_to_save"] = [str(s) for s in z["features_to_save"]]
    if not g["skip_nodes"]:
        for ax in range(3):
            ref[f"node_dim{ax}_lims"] = [z[f"node_dim{ax}_lims_{t}"] if f"node_dim{ax}_lims_{t}" in z else None for t in range(g["T"])]
        ref["node_labels_csr"] = [(z[f"node_labels_{t}_off"], z[f"node_labels_{t}_val"]) for t in range(g["T"])]
        ref["node_voxel_idxs_csr"] = [(z[f"node_voxel_idxs_{t}_off"], z[f"node_voxel_idxs_{t}_val"]) for t in range(g["T"])]
    # the reference's own float64 interpolation results in voxels, (0, D) where it found nothing
    g["ref_flow_px"] = {(t, key): z[f"flow_px_{t}_{key}"] for t in range(g["T"]) for key in ("bw", "fw") if f"flow_px_{t}_{key}" in z}
    g["ref"] = ref
    _CACHE[name] = g
    return g


def hierarchy_double(g, **extra):
    """the object Voxels(hierarchy) reads, built from a golden's inputs"""
    from types import SimpleNamespace
    D = g["D"]
    axes = "TYX" if D == 2 else "TZYX"
    dim_res = dict(zip(axes[1:], (float(s) for s in g["spacing"])))
    dim_res["T"] = g["dt"]
    im_info = SimpleNamespace(no_t=False, no_z=D == 2, shape=g["comp"].shape, axes=axes, dim_res=dim_res,
                              file_info=SimpleNamespace(filename_no_ext=g["filename"]))
    h = SimpleNamespace(im_info=im_info, num_t=g["T"], spacing=tuple(float(s) for s in g["spacing"]), viewer=None,
                        label_components=g["comp"], label_branches=g["branch"], im_raw=g["raw"], im_struct=g["struct"],
                        im_pixel_class=g["pixel_class"], im_distance=g["distance"], skip_nodes=g["skip_nodes"],
                        enable_motility=g["enable_motility"], flow_interpolator_fw=None, flow_interpolator_bw=None)
    for k, v in extra.items():
        setattr(h, k, v)
    return h


def expected_csv(ref):
    """header and rows of the voxel table from attributes as lists per frame: the rule of the reference's feature saving -- per
    frame the columns t, label (the row number within the frame) and <feature>_raw for every feature of features_to_save, stacked
    into one float64 array and written by pandas' to_csv (header once)"""
    import io
    import pandas as pd
    buf = io.StringIO()
    header = ["t", "label"] + [f + "_raw" for f in ref["features_to_save"]]
    for t in range(len(ref["x"])):
        n = len(ref["x"][t])
        cols = [np.full(n, t, dtype=np.int64), np.arange(n, dtype=np.int64)] + [np.array([np.array(ref[f][t])])[0] for f in ref["features_to_save"]]
        pd.DataFrame(np.array(cols).T, columns=header).to_csv(buf, index=False, mode="a", header=t == 0)
    return buf.getvalue()
