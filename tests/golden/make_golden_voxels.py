"""
Captures tests/golden/voxels/voxels_*.npz from the reference's Voxels class (nellie/feature_extraction/hierarchical.py), driven by
a SimpleNamespace hierarchy and the reference's FlowInterpolator (cKDTree on the CPU):

    python tests/golden/make_golden_voxels.py /path/to/nellie-reference

Each fixture holds the inputs (component, branch, raw, structure, pixel-class and distance stacks, flow_vector_array, spacing, dt,
the two flags) and every attribute the reference filled (layout: tests/voxel_goldens.py), plus what the reference's
interpolate_coord returned for every call (`flow_px_<t>_<bw|fw>`, float64 in voxels).  T = 4: frame 0 has no backward direction,
the last frame no forward one.  Scenes come from tests/reassign_scenes.py; single-voxel branches, node classes and radii are added
here.  A seed is replaced by the next one until (asserted, stored as `margin`, `gap`, `min_max_k`):
  - no (voxel, flow row) pair has a squared distance within 1e-9 relative of r*r;
  - for every branch label and direction the smallest |vec| is either shared bit for bit (lowest index decides) or separated
    from the next larger one by a relative gap above 1e-6;
  - every interpolation call that finds a neighbour has a voxel with two or more.
The capture itself checks tests/voxel_features_restatement.py against the reference: everything but the interpolated vectors
exactly (the motility recomputed from the reference's own vectors, bit for bit), the vectors within the bound of section 11.
"""
import os
import sys
import tempfile
import time
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402
import reassign_scenes as scenes  # noqa: E402
import flow_interpolation_restatement as fr  # noqa: E402
import voxel_features_restatement as vr  # noqa: E402
import voxel_goldens as vg  # noqa: E402

ISO, ANISO, ANISO2, ISO_2D, ANISO_2D = (0.107,) * 3, (0.29, 0.0973, 0.0973), (0.211, 0.083, 0.083), (0.0973, 0.0973), (0.107, 0.083)
T = 4

# raw: dtype of the intensity stack; radius: (low, high) of the node radii in voxels; far_nodes: nodes whose radius reaches past
# every face; zero_radius: share of nodes with radius 0; singles: single-voxel branches per frame; sparse: flow rows only in the
# low-x third of the frame
CASES = {
    "voxels_3d_aniso": dict(shape=(10, 32, 32), spacing=ANISO, raw=np.uint16, scene=dict(n_obj=5), singles=3),
    "voxels_3d_x70": dict(shape=(12, 24, 70), spacing=ANISO, raw=np.uint8, scene=dict(n_obj=6, drift_um=0.08), singles=2, zero_radius=0.3),
    "voxels_2d": dict(shape=(48, 52), spacing=ISO_2D, raw=np.float32, scene=dict(n_obj=6, size_um=(0.4, 0.7)), singles=3, far_nodes=2),
    "voxels_2d_aniso": dict(shape=(44, 50), spacing=ANISO_2D, raw=np.uint16, dt=1.7, scene=dict(n_obj=5, size_um=(0.4, 0.7)), zero_radius=0.3),
    "voxels_3d_empty_frame": dict(shape=(10, 28, 28), spacing=ANISO, raw=np.uint8, scene=dict(n_obj=4, empty_t=2, drift_um=0.08), singles=1),
    "voxels_3d_t_without_flow": dict(shape=(8, 28, 30), spacing=ANISO2, raw=np.uint16, scene=dict(n_obj=4, no_flow_t=1)),
    "voxels_3d_sparse_flow": dict(shape=(8, 24, 66), spacing=ANISO2, raw=np.float32, scene=dict(n_obj=7, rows_per_obj=6, drift_um=0.08), sparse=True,
                                  singles=2),
    "voxels_3d_integer_flow": dict(shape=(16, 32, 32), spacing=ISO, raw=np.uint16, dt=0.5,
                                   scene=dict(n_obj=5, integer_flow=True, drift_um=0.06, size_um=(0.2, 0.3)), far_nodes=2),
    "voxels_2d_integer_flow": dict(shape=(48, 48), spacing=ISO_2D, raw=np.uint8, scene=dict(n_obj=6, size_um=(0.4, 0.7), integer_flow=True), singles=2),
    "voxels_3d_skip_nodes": dict(shape=(8, 24, 24), spacing=ANISO, raw=np.uint16, scene=dict(n_obj=3, drift_um=0.08), skip_nodes=True),
    "voxels_3d_no_motility": dict(shape=(8, 24, 24), spacing=ANISO2, raw=np.uint8, scene=dict(n_obj=3, drift_um=0.08), enable_motility=False, far_nodes=1),
    "voxels_2d_no_motility": dict(shape=(30, 34), spacing=ISO_2D, raw=np.float32, scene=dict(n_obj=3, size_um=(0.4, 0.7)), enable_motility=False),
}


def make_inputs(rng, case):
    shape, spacing = case["shape"], case["spacing"]
    D = len(shape)
    branch, comp, flow = scenes.make_scene(rng, shape, T, spacing, **case.get("scene", {}))
    if case.get("sparse"):                                    # rows in the low-x third only, each twice (another vector and cost)
        flow = flow[flow[:, D] < shape[-1] / 3]
        again = flow.copy()
        again[:, 1 + D:1 + 2 * D] += rng.uniform(-0.3, 0.3, (len(flow), D))
        again[:, -1] = rng.random(len(flow)).astype(np.float32)
        flow = np.concatenate([flow, again])
        flow = flow[np.argsort(flow[:, 0], kind="stable")]
    top_c, top_b = int(comp.max()), int(branch.max())
    for t in range(T):                                        # single-voxel branches next to objects, within reach of their flow rows
        if not comp[t].any():
            continue
        body = np.argwhere(comp[t] > 0)
        for _ in range(case.get("singles", 0)):
            p = body[rng.integers(len(body))] + rng.integers(-3, 4, D)
            if np.all(p >= 0) and np.all(p < shape) and comp[t][tuple(p)] == 0:
                top_c, top_b = top_c + 1, top_b + 1
                comp[t][tuple(p)], branch[t][tuple(p)] = top_c, top_b
    # intensity and structure values at the labelled voxels and at a fiftieth of the background (a gather from a wrong voxel
    # shows; a stack of zeros elsewhere keeps the fixture small)
    lit = (comp > 0) | (rng.random(comp.shape) < 0.02)
    raw = rng.gamma(2.0, 40.0, comp.shape) * lit
    raw = raw.astype(case["raw"]) if np.issubdtype(case["raw"], np.floating) else np.clip(raw, 0, np.iinfo(case["raw"]).max).astype(case["raw"])
    struct = (rng.random(comp.shape) * lit).astype(np.float64 if case["raw"] == np.float32 else np.float32)
    pixel_class = np.zeros(comp.shape, np.uint8)
    distance = np.zeros(comp.shape, np.float32)
    lo, hi = case.get("radius", (0.5, 3.2))
    for t in range(T):
        core = np.argwhere(branch[t] > 0)
        if len(core) == 0:
            continue
        pick = core[rng.choice(len(core), max(1, len(core) // 5), replace=False)]
        pixel_class[t][tuple(pick.T)] = rng.integers(1, 5, len(pick))
        rad = rng.uniform(lo, hi, len(pick)).astype(np.float32)
        rad[rng.random(len(pick)) < case.get("zero_radius", 0.0)] = 0.0
        distance[t][tuple(pick.T)] = rad
        far = pick[:case.get("far_nodes", 0)]
        distance[t][tuple(far.T)] = np.float32(1.5 * max(shape) + 0.25)
    return comp, branch, raw, struct, pixel_class, distance, flow


class Recorder:
    """the reference's interpolator, keeping what every interpolate_coord call returned"""

    def __init__(self, inner, key, seen):
        self.inner, self.key, self.seen = inner, key, seen

    def interpolate_coord(self, coords, t):
        res = self.inner.interpolate_coord(coords, t)
        self.seen[(t, self.key)] = np.asarray(res, np.float64).reshape(-1, coords.shape[1]).copy()
        return res


def run_reference(Voxels, FlowInterpolator, g, seen):
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "flow.npy")
    np.save(path, g["flow"])
    h = vg.hierarchy_double(g)
    h.im_info.im_path = "im"
    h.im_info.pipeline_paths = {"flow_vector_array": path}
    h.im_info.get_memmap = lambda p: g["raw"]
    h._resolve_node_chunk_size = lambda num_nodes, num_voxels: int(max(1, min(97, num_voxels)))    # several chunks per frame
    h.flow_interpolator_fw = Recorder(FlowInterpolator(h.im_info), "fw", seen)
    h.flow_interpolator_bw = Recorder(FlowInterpolator(h.im_info, forward=False), "bw", seen)
    v = Voxels(h)
    t0 = time.perf_counter()
    with np.errstate(all="ignore"):
        v.run()
    return v, time.perf_counter() - t0


def cat(arrays):
    off = np.concatenate([[0], np.cumsum([len(a) for a in arrays])]).astype(np.int64)
    return np.concatenate([np.asarray(a) for a in arrays]), off


def csr(lists):
    """list of index arrays -> (offsets, int64 values); every non-empty entry is int64, every empty one numpy's empty float64"""
    for a in lists:
        assert isinstance(a, np.ndarray) and a.dtype == (np.int64 if len(a) else np.float64) and a.ndim == 1
    off = np.concatenate([[0], np.cumsum([len(a) for a in lists])]).astype(np.int64)
    val = np.concatenate([a for a in lists if len(a)]).astype(np.int64) if off[-1] else np.zeros(0, np.int64)
    return off, val


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def check_restatement(name, g, v, seen):
    """restatement vs reference; returns (margin, gap, min_max_k) of the restatement's own run"""
    kw = dict(skip_nodes=g["skip_nodes"], enable_motility=g["enable_motility"])
    args = [g[k] for k in vg.INPUTS] + [g["flow"], g["spacing"], g["dt"]]
    own = vr.voxels(*args, **kw)
    fed = vr.voxels(*args, vectors=seen, **kw)
    for t in range(T):
        n = len(v.coords[t])
        for k in vg.PER_VOXEL:
            assert same(own[k][t], getattr(v, k)[t]), (name, k, t)
        for k in vg.FLOAT_ATTRS:
            want = getattr(v, k)[t]
            if k in ("vec01", "vec12") and len(want) == 0 and n > 0:      # the reference found no neighbour: (0, D) there, NaN here
                assert np.isnan(fed[k][t]).all() and np.isnan(own[k][t]).all(), (name, k, t)
                continue
            assert same(fed[k][t], want), (name, k, t, "motility from the reference's vectors is not bit-equal")
            assert np.array_equal(np.isnan(own[k][t]), np.isnan(want)), (name, k, t)
        for key in ("bw", "fw"):
            if (t, key) in seen and len(seen[(t, key)]) == n and n > 0:
                fr.assert_close(own["flow_px"][(t, key)], seen[(t, key)], own["flow_k"][(t, key)], own["flow_vmax"][(t, key)], f"{name} t{t} {key}")
            elif (t, key) in seen:
                assert np.isnan(own["flow_px"][(t, key)]).all(), (name, t, key)
        if not g["skip_nodes"]:
            lims = own["node_lims"][t]
            for ax, attr in enumerate((v.node_dim0_lims, v.node_dim1_lims, v.node_dim2_lims)):
                if ax < g["D"]:
                    assert same(lims[ax], attr[t]), (name, "lims", ax, t)
                else:
                    assert attr[t] is None
            (noff, nval), (voff, vval) = own["node_voxels"][t], own["voxel_nodes"][t]
            roff, rval = csr(v.node_voxel_idxs[t])
            assert np.array_equal(noff, roff) and np.array_equal(nval, rval), (name, "node_voxel_idxs", t)
            if n == 0:
                assert v.node_labels[t] == []
            else:
                roff, rval = csr(v.node_labels[t])
                assert np.array_equal(voff, roff) and np.array_equal(vval, rval), (name, "node_labels", t)
    return own["margin"], own["gap"], own["min_max_k"]


def main():
    make_golden.REF = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else make_golden.REF
    make_golden._import_reference()
    from nellie.feature_extraction.hierarchical import Voxels
    from nellie.tracking.flow_interpolation import FlowInterpolator
    os.makedirs(vg.GOLDEN_DIR, exist_ok=True)
    only = sys.argv[2:]
    for name, case in CASES.items():
        if only and name not in only:
            continue
        seed = 0
        while True:
            rng = np.random.default_rng([seed, len(name)])
            comp, branch, raw, struct, pixel_class, distance, flow = make_inputs(rng, case)
            g = dict(comp=comp, branch=branch, raw=raw, struct=struct, pixel_class=pixel_class, distance=distance, flow=flow,
                     spacing=np.asarray(case["spacing"], float), dt=float(case.get("dt", 1.0)), skip_nodes=case.get("skip_nodes", False),
                     enable_motility=case.get("enable_motility", True), T=T, D=len(case["shape"]), filename="golden_" + name)
            pre = vr.voxels(*[g[k] for k in vg.INPUTS], flow, g["spacing"], g["dt"], skip_nodes=True, enable_motility=g["enable_motility"])
            if pre["margin"] > 1e-9 and pre["gap"] > 1e-6 and (pre["min_max_k"] >= 2 or not g["enable_motility"]):
                break
            seed += 1
        seen = {}
        v, seconds = run_reference(Voxels, FlowInterpolator, g, seen)
        margin, gap, min_max_k = check_restatement(name, g, v, seen)
        assert margin > 1e-9 and gap > 1e-6, (name, margin, gap)
        assert min_max_k >= 2 or not g["enable_motility"], (name, min_max_k)
        out = {k: g[k] for k in vg.INPUTS + ("flow", "spacing")}
        out.update(dt=np.float64(g["dt"]), skip_nodes=np.bool_(g["skip_nodes"]), enable_motility=np.bool_(g["enable_motility"]),
                   filename=np.str_(g["filename"]), seed=np.int64(seed), margin=np.float64(margin), gap=np.float64(gap),
                   min_max_k=np.int64(min(min_max_k, 2 ** 31)), stats_to_aggregate=np.asarray(v.stats_to_aggregate),
                   features_to_save=np.asarray(v.features_to_save))
        for k in vg.PER_VOXEL + vg.FLOAT_ATTRS:
            out[k], out[k + "_off"] = cat(getattr(v, k))
        for t in range(T):
            assert list(v.image_name[t]) == [g["filename"]] * len(v.coords[t]) and v.image_name[t].dtype == object
            for key in ("bw", "fw"):
                if (t, key) in seen:
                    out[f"flow_px_{t}_{key}"] = seen[(t, key)]
            if g["skip_nodes"]:
                continue
            for ax, attr in enumerate((v.node_dim0_lims, v.node_dim1_lims, v.node_dim2_lims)):
                if attr[t] is not None:
                    out[f"node_dim{ax}_lims_{t}"] = attr[t]
            out[f"node_voxel_idxs_{t}_off"], out[f"node_voxel_idxs_{t}_val"] = csr(v.node_voxel_idxs[t])
            out[f"node_labels_{t}_off"], out[f"node_labels_{t}_val"] = csr(v.node_labels[t]) if len(v.coords[t]) else csr([])
        if g["skip_nodes"]:
            assert v.node_labels == [] and v.node_voxel_idxs == [] and v.node_dim0_lims == []
        path = os.path.join(vg.GOLDEN_DIR, name + ".npz")
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) < 400_000, (name, os.path.getsize(path))
        nvox = [len(c) for c in v.coords]
        assert all(n > 0 or t == case.get("scene", {}).get("empty_t") for t, n in enumerate(nvox)), (name, nvox)
        nodes = [len(a) for a in v.node_voxel_idxs]
        nan12 = [int(np.isnan(a).any(axis=-1).sum()) if a.ndim == 2 else 0 for a in v.vec12]
        print(f"{name}: seed {seed}, voxels {nvox}, nodes {nodes}, {len(flow)} flow rows, NaN vec12 rows {nan12}, margin {margin:.3g}, "
              f"pivot gap {gap:.3g}, min max k {min_max_k}, reference {seconds:.2f} s, {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
