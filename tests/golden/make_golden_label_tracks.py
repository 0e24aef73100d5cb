"""
Captures tests/golden/label_tracks/label_tracks_*.npz from the reference's LabelTracks.run (cKDTree on the CPU):

    python tests/golden/make_golden_label_tracks.py /path/to/nellie-reference

Each fixture holds a label stack of four time points with a few blobs per frame, a flow_vector_array from make_golden_flow's
generator, spacing, dt, max_distance_um, the keywords of the run, and the reference's tracks and frame_num.  A seed is replaced
by the next one until (asserted): the reference loses no coordinate (its loop over the good rows drops tail rows after a loss in
mid-array, DESIGN.md section 11.2: such a capture records the defect, not the intent); no (query, row) pair has a squared
distance within 1e-9 relative of r*r; no track coordinate is within 1e-9 of a half-integer; some query has more than one
neighbour (section 11.1); the final filter keeps at least a tenth and drops at least a tenth of the rows.
"""
import os
import sys
import tempfile
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402
from make_golden_flow import ANISO2, ANISO_2D, T, make_flow  # noqa: E402
import label_tracks_restatement as lrs  # noqa: E402

SHAPES = {"3d": ((10, 28, 28), ANISO2, 260), "2d": ((48, 52), ANISO_2D, 220)}
MAXD, DT, VMAX = 1.0, 1.0, 3
# name: keywords of run()
RUNS = {
    "forward_only": dict(start_frame=0),
    "backward_only": dict(start_frame=T - 1),
    "both_directions": dict(start_frame=1),
    "label_num": dict(start_frame=2, label_num=2),
    "skip_3": dict(start_frame=1, skip_coords=3),
    "min_track_num_7": dict(start_frame=2, min_track_num=7),
}


def make_labels(rng, shape, blobs=4):
    """T frames of a few balls (label = the ball's number) whose centres wander by a voxel or two from frame to frame"""
    D = len(shape)
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1).astype(float)
    centres = np.column_stack([rng.uniform(0.2 * s, 0.8 * s, blobs) for s in shape])
    radii = rng.uniform(2.0, 3.2, blobs)
    stack = np.zeros((T,) + tuple(shape), np.int32)
    for t in range(T):
        for b in range(blobs):
            d2 = ((grid - centres[b]) ** 2).sum(axis=-1)
            stack[t][d2 <= radii[b] ** 2] = b + 1
        centres = centres + rng.uniform(-1.5, 1.5, (blobs, D))
    return stack


def reference_im(flow, labels, spacing, dt):
    D = labels.ndim - 1
    path = os.path.join(tempfile.mkdtemp(), "flow.npy")
    np.save(path, flow)
    axes = "TYX" if D == 2 else "TZYX"
    dim_res = dict(zip(axes[1:], spacing))
    dim_res["T"] = dt
    stack = np.zeros(labels.shape, np.uint8)
    return SimpleNamespace(no_t=False, no_z=D == 2, shape=labels.shape, axes=axes, dim_res=dim_res, im_path="im",
                           pipeline_paths={"flow_vector_array": path, "im_instance_label": "labels"},
                           get_memmap=lambda p: labels if p == "labels" else stack)


def main():
    make_golden.REF = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else make_golden.REF
    make_golden._import_reference()
    from nellie.tracking.all_tracks_for_label import LabelTracks
    os.makedirs(os.path.join(HERE, "label_tracks"), exist_ok=True)
    r = max(MAXD * DT, 0.5)
    for dim, (shape, spacing, n_rows) in SHAPES.items():
        for run, kw in RUNS.items():
            name = f"label_tracks_{dim}_{run}"
            seed = 0
            while True:
                rng = np.random.default_rng([seed, len(name), len(shape)])
                flow = make_flow(rng, shape, n_rows, vmax=VMAX)
                labels = make_labels(rng, shape)
                rows, frame_num, info = lrs.label_tracks(labels, flow, spacing, r, **kw)
                n_seeds = len(lrs.seeds(labels, kw["start_frame"], kw.get("label_num"), kw.get("skip_coords", 1)))
                start = kw["start_frame"]
                full = n_seeds * ((T - start if start < T - 1 else 0) + (start + 1 if start > 0 else 0))
                ok = (n_seeds > 0 and len(info["raw"]) == full and info["radius_margin"] > 1e-9 and info["half_margin"] > 1e-9
                      and info["kmax"] > 1 and 0.1 * full <= len(rows) <= 0.9 * full)
                if ok:
                    break
                seed += 1
            lt = LabelTracks(reference_im(flow, labels, spacing, DT))
            lt.initialize()
            tracks, props = lt.run(max_distance_um=MAXD, **kw)
            tracks = np.asarray(tracks, float)
            assert len(info["raw"]) == full, name                          # no coordinate is lost
            assert info["radius_margin"] > 1e-9 and info["half_margin"] > 1e-9 and info["kmax"] > 1, name
            assert 0.1 * full <= len(tracks) <= 0.9 * full and len(tracks) == len(rows), name
            assert list(props) == ["frame_num"], name
            path = os.path.join(HERE, "label_tracks", name + ".npz")
            np.savez_compressed(path, flow=flow, labels=labels, spacing=np.asarray(spacing, float), dt=np.float64(DT),
                                max_distance_um=np.float64(MAXD), seed=np.int64(seed), tracks=tracks,
                                frame_num=np.asarray(props["frame_num"], np.int64), radius_margin=np.float64(info["radius_margin"]),
                                half_margin=np.float64(info["half_margin"]), kmax=np.int64(info["kmax"]),
                                **{"kw_" + k: np.int64(v) for k, v in kw.items()})
            print(f"{name}: skipped {seed} seeds, {n_seeds} seed voxels, {full} rows tracked, {len(tracks)} kept, max k {info['kmax']}, "
                  f"radius margin {info['radius_margin']:.3g}, half margin {info['half_margin']:.3g}, {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
