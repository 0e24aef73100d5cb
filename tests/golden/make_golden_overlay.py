"""
Captures tests/golden/overlay/overlay_*.npz from the reference's own NellieAnalysis.overlay (nellie_napari/nellie_analysis.py):

    python tests/golden/make_golden_overlay.py /path/to/nellie-reference

The panel's module imports Qt, napari and matplotlib's Qt canvas, none of which the capture needs: stand-in modules of a few lines go
into sys.modules, the module file is loaded on its own (not through its package, whose __init__ pulls in the whole plug-in), and
`overlay` is called unbound on a plain object that carries what the method reads -- `nellie.im_info`, `df`, `selected_level`,
`selected_attr`, `all_attr_data`, `time_col`, `scale` and a `viewer` whose add_image / add_labels record the array and the contrast
limits.

One fixture per adjacency golden (tests/golden/adjacency, which sits on the image goldens): the label stack is that golden's
component labels, the pickle its edge lists, and per level a table (t, label, one column) made from the golden's hierarchy double --
the voxels' structure values, the nodes' thickness, the branches' length and the organelles' area.  `overlay_3d_aniso_special`
repeats one golden with columns that hold NaN, +inf, -inf and -0.0.  A fixture holds arrays only: per level `<level>_t`,
`<level>_label`, `<level>_value`, the captured `<level>_frames` (T, ...) float64 and `<level>_clim`.

Nothing is written unless tests/feature_overlay_restatement.py's literal form equals the captured frames (equal values, NaN in the
same places, zeros of the same sign) and its contrast limits equal the captured ones.
"""
import importlib.util
import os
import pickle
import sys
import tempfile
import types
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402
import adjacency_goldens as ag  # noqa: E402
import feature_overlay_restatement as fr  # noqa: E402
import overlay_goldens as og  # noqa: E402


def stand_ins():
    """modules that satisfy the panel's imports: every name it asks of Qt is an empty class"""
    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m
    widgets = ("QComboBox", "QCheckBox", "QPushButton", "QLabel", "QTableWidget", "QTableWidgetItem", "QSpinBox", "QDoubleSpinBox", "QWidget",
               "QVBoxLayout", "QGroupBox", "QHBoxLayout")
    module("qtpy")
    module("qtpy.QtWidgets", **{w: type(w, (), {}) for w in widgets})
    module("qtpy.QtCore", Qt=type("Qt", (), {}))
    module("napari")
    module("napari.utils")
    module("napari.utils.notifications", show_info=lambda *a, **k: None)
    for name in ("matplotlib", "matplotlib.backends"):
        if importlib.util.find_spec(name) is None:
            module(name)
    module("matplotlib.backends.backend_qtagg", FigureCanvasQTAgg=type("FigureCanvasQTAgg", (), {}))


def load_panel(ref):
    stand_ins()
    spec = importlib.util.spec_from_file_location("reference_nellie_analysis", os.path.join(ref, "nellie_napari", "nellie_analysis.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.NellieAnalysis


class Viewer:
    def __init__(self):
        self.shown = None

    def _record(self, data, **kw):
        self.shown = (np.array(data), kw.get("contrast_limits"))
        return SimpleNamespace(mouse_drag_callbacks=[])

    add_image = add_labels = _record

    def reset_view(self):
        pass


def capture(panel, labels, pkl_path, level, t_col, label_col, val_col, column="value"):
    import pandas as pd
    df = pd.DataFrame({"t": t_col, "label": label_col, column: val_col})
    im_info = SimpleNamespace(shape=labels.shape, no_z=labels.ndim == 3, pipeline_paths={"im_instance_label": "labels", "adjacency_maps": pkl_path},
                              get_memmap=lambda p: labels)
    viewer = Viewer()
    this = SimpleNamespace(selected_attr=column, df=df, label_mask=None, label_coords=None, adjacency_maps=None, nellie=SimpleNamespace(im_info=im_info),
                           all_attr_data=df[column], time_col=df["t"], selected_level=level, viewer=viewer, scale=None, label_mask_layer=None,
                           get_index=None)
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            panel.overlay(this)
    frames, clim = viewer.shown
    return np.asarray(frames, np.float64), np.asarray(clim, np.float64)


def main():
    make_golden.REF = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else make_golden.REF
    panel = load_panel(make_golden.REF)
    os.makedirs(og.GOLDEN_DIR, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        for aname in ag.names():
            g = ag.load(aname)
            case = aname[len("adjacency_"):]
            for special in ((False, True) if case == "3d_aniso" else (False,)):
                labels, tables = og.inputs_of(g, special)
                pkl = os.path.join(tmp, aname + ".pkl")
                with open(pkl, "wb") as f:
                    pickle.dump(g["ref"], f)
                out = {}
                for level in fr.LEVELS:
                    t_col, label_col, val_col = tables[level]
                    frames, clim = capture(panel, labels, pkl, level, t_col, label_col, val_col)
                    own = fr.overlay_literal(labels, level, t_col, label_col, val_col, g["ref"].get(fr.EDGE_KEYS.get(level)))
                    assert fr.same(own, frames), (aname, level, "the literal restatement differs from the reference")
                    assert fr.contrast_limits(val_col) == list(clim), (aname, level, fr.contrast_limits(val_col), clim)
                    out.update({f"{level}_t": np.asarray(t_col, np.int64), f"{level}_label": np.asarray(label_col, np.int64),
                                f"{level}_value": np.asarray(val_col, np.float64), f"{level}_frames": frames, f"{level}_clim": clim})
                name = "overlay_" + case + ("_special" if special else "")
                path = os.path.join(og.GOLDEN_DIR, name + ".npz")
                np.savez_compressed(path, base=np.str_(aname), special=np.bool_(special), **out)
                assert os.path.getsize(path) < 200_000, (name, os.path.getsize(path))
                painted = {level: int(np.isfinite(out[f"{level}_frames"]).sum()) for level in fr.LEVELS}
                print(f"{name}: finite voxels {painted}, {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
