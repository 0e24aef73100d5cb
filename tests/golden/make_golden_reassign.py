"""
Captures tests/golden/reassign/reassign_*.npz from the reference's VoxelReassigner (device="cpu": cKDTree):

    python tests/golden/make_golden_reassign.py /path/to/nellie-reference

Each fixture holds the branch and object label stacks (int32), the flow_vector_array, spacing, dt, max_distance_um, the keywords,
and what the reference wrote: the two reassigned stacks, running_matches (match_<t>_prev / match_<t>_next, `n_matches` pairs, the
shape of the saved object array) and the seed.  Scenes come from tests/reassign_scenes.py.  A seed is replaced by the next one
until no decision of the fixture rests on cKDTree's pruning order, a float32 rounding or a summation order (asserted):
margin (a) > 1e-9, margins (b), (c), (d) > 1e-6 (tests/voxel_reassignment_restatement.py), and every interpolation call that
finds a neighbour has a query with two or more (below that the reference's interpolator loses rows).

reassign_3d_integer_flow is realistic rather than tie-free: T = 2, whole-voxel flow vectors as HuMomentTracking writes them, so
predicted centroids fall on lattice points and ties of the nearest-voxel step occur.  Its `tainted` targets are the voxels whose
candidates rest on such a tie; the mismatch between drift and flow is halved, or the seed replaced, until at most 5 % of the
labelled target voxels are tainted.
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
import voxel_reassignment_restatement as rs  # noqa: E402

ISO, ANISO, ANISO2, ISO_2D, ANISO_2D = (0.107,) * 3, (0.29, 0.0973, 0.0973), (0.211, 0.083, 0.083), (0.0973, 0.0973), (0.107, 0.083)

CASES = {
    "reassign_3d_iso": dict(shape=(16, 64, 64), spacing=ISO, T=4, scene=dict(n_obj=12)),
    "reassign_3d_aniso": dict(shape=(10, 72, 72), spacing=ANISO, T=3, scene=dict(n_obj=14)),
    "reassign_2d": dict(shape=(128, 120), spacing=ANISO_2D, T=4, scene=dict(n_obj=16, size_um=(0.4, 0.7))),
    "reassign_3d_appearing": dict(shape=(14, 56, 100), spacing=ISO, T=3, scene=dict(appear=True, x_share=0.5, n_obj=8)),
    "reassign_3d_vanishing": dict(shape=(14, 64, 64), spacing=ANISO2, T=4, scene=dict(vanish=True, n_obj=10)),
    "reassign_3d_converging": dict(shape=(14, 64, 64), spacing=ISO, T=4, scene=dict(converge=True, n_obj=10)),
    "reassign_3d_empty_frame": dict(shape=(12, 56, 56), spacing=ISO, T=4, scene=dict(empty_t=2, n_obj=10)),
    "reassign_2d_pair_without_flow": dict(shape=(120, 120), spacing=ISO_2D, T=4, scene=dict(no_flow_t=1, n_obj=14, size_um=(0.4, 0.7))),
    "reassign_3d_no_running_matches": dict(shape=(12, 56, 60), spacing=ISO, T=3, store=False, scene=dict(n_obj=10)),
    "reassign_3d_wide_radius": dict(shape=(12, 64, 64), spacing=ANISO, T=3, dt=1.7, scene=dict(drift_um=0.3, noise=0.6, n_obj=12)),
    "reassign_3d_integer_flow": dict(shape=(14, 64, 64), spacing=ISO, T=2, scene=dict(integer_flow=True, n_obj=12), tainted=True),
}


def reference_im(tmp, branch, obj, flow, spacing, dt):
    D = branch.ndim - 1
    axes = "TYX" if D == 2 else "TZYX"
    dim_res = dict(zip(axes[1:], spacing))
    dim_res["T"] = dt
    paths = {k: os.path.join(tmp, k + ".npy") for k in ("flow_vector_array", "voxel_matches")}
    paths.update({k: k for k in ("im_skel_relabelled", "im_instance_label", "im_branch_label_reassigned", "im_obj_label_reassigned")})
    np.save(paths["flow_vector_array"], flow)
    store = {"im": np.zeros(branch.shape, np.uint8), "im_skel_relabelled": branch, "im_instance_label": obj}

    def allocate_memory(path, dtype="float", data=None, description="", return_memmap=False, read_mode="r+"):
        store[path] = np.zeros(branch.shape, dtype)
        return store[path]
    return SimpleNamespace(no_t=False, no_z=D == 2, shape=branch.shape, axes=axes, dim_res=dim_res, im_path="im", pipeline_paths=paths,
                           get_memmap=lambda p, read_mode="r+": store[p], allocate_memory=allocate_memory), store


def run_reference(ref, branch, obj, flow, spacing, dt, maxd, store, iters):
    with tempfile.TemporaryDirectory() as tmp:
        im, out = reference_im(tmp, branch, obj, flow, spacing, dt)
        vr = ref.VoxelReassigner(im, store_running_matches=store, max_refine_iterations=iters, device="cpu")
        t0 = time.perf_counter()
        vr.run()
        seconds = time.perf_counter() - t0
        saved = np.load(im.pipeline_paths["voxel_matches"], allow_pickle=True) if store else None
        assert store or not os.path.exists(im.pipeline_paths["voxel_matches"])
        assert vr.flow_interpolator_fw.max_distance_um == max(maxd * dt, 0.5)
        return out["im_branch_label_reassigned"], out["im_obj_label_reassigned"], vr.running_matches, saved, seconds


def labelled_targets(branch, obj):
    return (branch[1:] > 0) | (obj[1:] > 0)


def main():
    make_golden.REF = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else make_golden.REF
    make_golden._import_reference()
    from nellie.tracking import voxel_reassignment as ref
    os.makedirs(os.path.join(HERE, "reassign"), exist_ok=True)
    for name, case in CASES.items():
        shape, spacing, T = case["shape"], case["spacing"], case["T"]
        dt, maxd, store, iters = case.get("dt", 1.0), case.get("maxd", 0.5), case.get("store", True), case.get("iters", 3)
        r = max(maxd * dt, 0.5)
        seed, mismatch = 0, 0.5
        while True:
            rng = np.random.default_rng([seed, len(name)])
            kw = dict(case.get("scene", {}))
            if case.get("tainted"):
                kw["mismatch"] = mismatch
            branch, obj, flow = scenes.make_scene(rng, shape, T, spacing, **kw)
            mine = rs.reassign(branch, obj, flow, spacing, r, store_running_matches=True, max_refine_iterations=iters)
            good = mine["min_max_k"] == 0 or mine["min_max_k"] >= 2
            if case.get("tainted"):
                taint = np.stack(mine["tainted"])
                share = float(taint.sum()) / max(1, int(labelled_targets(branch, obj).sum()))
                good = good and share <= 0.05 and mine["margin_b"] > 1e-6
                if not good:
                    if mismatch > 0.05:
                        mismatch /= 2
                    else:
                        seed, mismatch = seed + 1, 0.5
                    continue
                break
            good = good and mine["margin_a"] > 1e-9 and min(mine["margin_b"], mine["margin_c"], mine["margin_d"]) > 1e-6
            if good:
                break
            seed += 1
        ref_b, ref_o, matches, saved, seconds = run_reference(ref, branch, obj, flow, spacing, dt, maxd, store, iters)
        out = dict(branch=branch, obj=obj, flow=flow, spacing=np.asarray(spacing, float), dt=np.float64(dt), max_distance_um=np.float64(maxd),
                   kw_store_running_matches=np.bool_(store), kw_max_refine_iterations=np.int64(iters), seed=np.int64(seed),
                   ref_branch=ref_b.astype(np.int32), ref_obj=ref_o.astype(np.int32), n_matches=np.int64(len(matches)),
                   saved_shape=np.asarray(saved.shape if saved is not None else (), np.int64),
                   margin_a=np.float64(mine["margin_a"]), margin_b=np.float64(mine["margin_b"]), margin_c=np.float64(mine["margin_c"]),
                   margin_d=np.float64(mine["margin_d"]), min_max_k=np.int64(mine["min_max_k"]))
        for t, (p, n) in enumerate(matches):
            out[f"match_{t}_prev"], out[f"match_{t}_next"] = p, n
        if case.get("tainted"):
            out["tainted"] = taint
            out["mismatch"] = np.float64(mismatch)
            keep = ~taint
            assert share <= 0.05
            assert np.array_equal(mine["reassigned_branch"][1:][keep], ref_b[1:][keep]), name
            assert np.array_equal(mine["reassigned_obj"][1:][keep], ref_o[1:][keep]), name
            diff = int((mine["reassigned_obj"] != ref_o).sum() + (mine["reassigned_branch"] != ref_b).sum())
            info = f"tainted share {share:.4f}, mismatch {mismatch}, {diff} voxels differ from the reference (all tainted)"
        else:                                            # the capture itself checks the restatement against the reference
            assert np.array_equal(mine["reassigned_branch"], ref_b) and np.array_equal(mine["reassigned_obj"], ref_o), name
            assert len(matches) == (len(mine["running_matches"]) if store else 0), name
            for (p, n), (p2, n2) in zip(matches, mine["running_matches"]):
                assert p.dtype == p2.dtype and np.array_equal(p, p2) and np.array_equal(n, n2), name
            info = f"margins a {mine['margin_a']:.3g} b {mine['margin_b']:.3g} c {mine['margin_c']:.3g} d {mine['margin_d']:.3g}"
        assert ref_o[0].any() and np.array_equal(ref_o[0], obj[0])
        path = os.path.join(HERE, "reassign", name + ".npz")
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) < 200_000, (name, os.path.getsize(path))
        nvox = [int(((branch[t] > 0) | (obj[t] > 0)).sum()) for t in range(T)]
        print(f"{name}: seed {seed}, voxels per frame {nvox}, {len(flow)} flow rows, {mine['pairs']} pairs ran, min max k "
              f"{mine['min_max_k']}, {info}, reference {seconds:.2f} s, {os.path.getsize(path)} B")


if __name__ == "__main__":
    main()
