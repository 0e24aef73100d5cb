"""Reading tests/golden/overlay/*.npz (written by tests/golden/make_golden_overlay.py) and making the inputs they were captured from;
test infrastructure only.  A fixture `overlay_<case>.npz` sits on the adjacency golden `adjacency_<case>.npz`
(tests/adjacency_goldens.py): the label stack is that golden's component labels and the pickle its edge lists.  Per level the fixture
holds the table (`<level>_t`, `<level>_label`, `<level>_value`), the frames the reference's overlay painted (`<level>_frames`,
float64, NaN off the painted voxels) and its contrast limits (`<level>_clim`)."""
import glob
import os

import numpy as np

import adjacency_goldens as ag
from feature_overlay_restatement import LEVELS

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_DIR = os.path.join(HERE, "golden", "overlay")


def names():
    return sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLDEN_DIR, "overlay_*.npz")))


def _column(obj, attr, rows, t, rng):
    """the attribute's frame-t column where it has one value per row, else random values"""
    col = getattr(obj, attr, None)
    if col is not None and len(col) > t and np.shape(col[t]) == (rows,):
        return np.asarray(col[t], np.float64)
    return rng.normal(size=rows)


def inputs_of(g, special=False):
    """(label stack (T, ...), {level: (t, label, value) columns}) of an adjacency golden: the tables as the hierarchy's writer lays
    them out (voxels and nodes are labelled by their row number, branches and organelles by their label).  special: the values are
    replaced by a pattern of NaN, +inf, -inf, -0.0 and small integers."""
    h = ag.double_of(g)
    base = g["image"]["base"]
    labels = np.asarray(base["comp"])
    rng = np.random.default_rng(len(g["name"]))
    tables = {}
    for level in LEVELS:
        t_col, label_col, val_col = [], [], []
        for t in range(labels.shape[0]):
            if level == "voxel":
                lab = np.arange(len(h.voxels.coords[t]))
                val = _column(h.voxels, "structure", len(lab), t, rng)
            elif level == "node":
                if base["skip_nodes"]:
                    continue
                lab = np.arange(len(h.nodes.nodes[t]))
                val = _column(h.nodes, "node_thickness", len(lab), t, rng)
            elif level == "branch":
                lab = np.asarray(h.branches.branch_label[t])
                val = _column(h.branches, "branch_length", len(lab), t, rng)
            else:
                lab = np.asarray(h.components.component_label[t])
                val = _column(h.components, "organelle_area", len(lab), t, rng)
            if special:
                pattern = np.array([np.nan, np.inf, -np.inf, -0.0, 1.0, -0.0, 2.0, 3.0, np.nan, -0.0, 5.0])
                val = pattern[(np.arange(len(lab)) * 7 + t) % len(pattern)]
            t_col.append(np.full(len(lab), t, np.int64))
            label_col.append(np.asarray(lab, np.int64))
            val_col.append(np.asarray(val, np.float64))
        cat = [np.concatenate(c) if c else np.zeros(0) for c in (t_col, label_col, val_col)]
        tables[level] = (cat[0].astype(np.int64), cat[1].astype(np.int64), cat[2].astype(np.float64))
    return labels, tables


_CACHE = {}


def load(name):
    """dict: `adjacency` (the adjacency golden), `labels` (the stack), `edges` ({key: frames}), and per level `tables[level]` =
    (t, label, value), `frames[level]`, `clim[level]`.  Read once and shared (do not modify)."""
    if name in _CACHE:
        return _CACHE[name]
    z = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    g = ag.load(str(z["base"]))
    out = dict(name=name, adjacency=g, labels=np.asarray(g["image"]["base"]["comp"]), edges=g["ref"],
               tables={lv: (z[f"{lv}_t"], z[f"{lv}_label"], z[f"{lv}_value"]) for lv in LEVELS},
               frames={lv: z[f"{lv}_frames"] for lv in LEVELS}, clim={lv: [float(v) for v in z[f"{lv}_clim"]] for lv in LEVELS})
    _CACHE[name] = out
    return out
