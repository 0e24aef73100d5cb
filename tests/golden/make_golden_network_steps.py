"""
Captures tests/golden/network_steps/*.npz from the reference's Network (device="cpu": numpy / scipy):

    python tests/golden/make_golden_network_steps.py /path/to/nellie-reference

skimage is stubbed like the other missing imports (make_golden._import_reference), so the thinning has a stand-in: `_skeletonize` is
replaced on the instance by a function that returns labels * a stored mask (scenes: tests/network_scenes.py).  Each fixture holds the
inputs (labels int32, skel_mask bool, frangi float32, spacing) and what the reference's own methods returned, step by step:

  skel            labels * skel_mask                                  (networking.py:408)
  skel_clean      `_remove_connected_label_pixels(force_cpu=True)`
  skel_seeded     `_add_missing_skeleton_labels`
  pixel_class     `_get_pixel_class(force_cpu=True)` on (skel_seeded > 0) * labels
  branch          `_get_branch_skel_labels(force_cpu=True)`
  relabelled      `_relabel_objects`
  frame_*         the three products of `_run_frame_backend(0)`

Every label's Frangi maximum is unique (asserted): the reference's pick among equal maxima follows no rule.  The capture itself checks
tests/network_steps_restatement.py against every array.  Only arrays and scalars travel.
"""
import os
import sys
from types import SimpleNamespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden  # noqa: E402
import network_scenes as scenes  # noqa: E402
import network_steps_restatement as rs  # noqa: E402

CASES = {
    "net_3d_iso": dict(shape=(12, 36, 40), spacing=(1.0, 1.0, 1.0), scene=dict(n_obj=6)),
    "net_3d_aniso_03": dict(shape=(10, 40, 36), spacing=(0.3, 0.1, 0.1), scene=dict(n_obj=6)),
    "net_3d_aniso_029": dict(shape=(11, 33, 45), spacing=(0.29, 0.11, 0.11), scene=dict(n_obj=7, radius=2)),
    "net_2d": dict(shape=(70, 90), spacing=(0.107, 0.083), scene=dict(n_obj=8, steps=40)),
    "net_3d_empty": dict(shape=(6, 20, 24), spacing=(0.29, 0.11, 0.11), empty=True),
    "net_3d_seedless": dict(shape=(12, 36, 40), spacing=(0.3, 0.1, 0.1), scene=dict(n_obj=4, blocks=3)),
    "net_2d_seedless": dict(shape=(60, 64), spacing=(1.0, 1.0), scene=dict(n_obj=4, blocks=3)),
    "net_3d_seeding": dict(shape=(12, 36, 40), spacing=(1.0, 1.0, 1.0), scene=dict(n_obj=6, drop=3)),
    "net_3d_touching": dict(shape=(12, 36, 40), spacing=(0.29, 0.11, 0.11), scene=dict(n_obj=5, touching=True)),
    "net_2d_touching": dict(shape=(64, 80), spacing=(0.11, 0.11), scene=dict(n_obj=5, touching=True, steps=40)),
}


def reference_network(ref, shape, spacing, labels, frangi):
    ndim = len(shape)
    axes = "TYX" if ndim == 2 else "TZYX"
    im = SimpleNamespace(no_t=False, no_z=ndim == 2, shape=(1,) + tuple(shape), axes=axes, dim_res=dict(zip(axes[1:], spacing), T=1.0))
    net = ref.Network(im, device="cpu")
    net.label_memmap = labels[None]
    net.im_frangi_memmap = frangi[None]
    return net


def main():
    make_golden.REF = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else make_golden.REF
    make_golden._import_reference()
    from nellie.segmentation import networking as ref
    out_dir = os.path.join(HERE, "network_steps")
    os.makedirs(out_dir, exist_ok=True)
    for k, (name, case) in enumerate(CASES.items()):
        shape, spacing = case["shape"], case["spacing"]
        rng = np.random.default_rng([k, 2024])
        if case.get("empty"):
            labels, mask, frangi = np.zeros(shape, np.int32), np.zeros(shape, bool), scenes.unique_frangi(rng, shape)
        else:
            labels, mask, frangi = scenes.walks_scene(rng, shape, **case["scene"])
        assert rs.unique_maxima(labels, frangi), name
        net = reference_network(ref, shape, spacing, labels, frangi)
        assert tuple(net.scaling) == tuple(spacing)
        net._skeletonize = lambda label_frame: np.asarray(label_frame) * mask
        skel = net._skeletonize(labels)
        skel_clean = np.asarray(net._remove_connected_label_pixels(skel, force_cpu=True))
        skel_seeded = np.asarray(net._add_missing_skeleton_labels(skel_clean.copy(), labels, frangi))
        skel_pre = (skel_seeded > 0) * labels
        pc = np.asarray(net._get_pixel_class(skel_pre, force_cpu=True))
        branch = np.asarray(net._get_branch_skel_labels(pc, force_cpu=True))
        relabelled = np.asarray(net._relabel_objects(branch, labels))
        f_branch, f_pc, f_rel = (np.asarray(a) for a in net._run_frame_backend(0))
        assert np.array_equal(f_branch, branch) and np.array_equal(f_pc, pc) and np.array_equal(f_rel, relabelled), name
        mine = rs.frame(labels, mask, frangi, spacing)
        for key, got in (("skel", skel), ("skel_clean", skel_clean), ("skel_seeded", skel_seeded), ("pixel_class", pc), ("branch", branch),
                         ("relabelled", relabelled)):
            assert np.array_equal(mine[key], got), (name, key)
        n_removed = int(((skel > 0) & (skel_clean == 0)).sum())
        seedless = int(np.setdiff1d(np.unique(labels), np.unique(labels[branch > 0])).size) - int(0 in labels)
        out = dict(labels=labels, skel_mask=mask, frangi=frangi, spacing=np.asarray(spacing, np.float64), skel=skel.astype(np.int32),
                   skel_clean=skel_clean.astype(np.int32), skel_seeded=skel_seeded.astype(np.int32), pixel_class=pc.astype(np.uint8),
                   branch=branch.astype(np.int32), relabelled=relabelled.astype(np.uint32), frame_branch=f_branch.astype(np.int32),
                   frame_pixel_class=f_pc.astype(np.uint8), frame_relabelled=f_rel.astype(np.uint32), n_removed=np.int64(n_removed),
                   n_seeded=np.int64(mine["n_seeded"]), n_seedless=np.int64(seedless))
        assert relabelled.dtype == np.uint32 and pc.dtype == np.uint8, (relabelled.dtype, pc.dtype)
        path = os.path.join(out_dir, name + ".npz")
        np.savez_compressed(path, **out)
        assert os.path.getsize(path) < 200_000, (name, os.path.getsize(path))
        print(f"{name}: {int(labels.max())} labels, {int(mask.sum())} mask voxels, clean removed {n_removed}, seeded {mine['n_seeded']}, "
              f"{int(branch.max())} branches, {seedless} seedless objects, {int((relabelled > 0).sum())} relabelled voxels, "
              f"{os.path.getsize(path)} B")
        if "seedless" in name:
            assert seedless > 0, name
        if "seeding" in name:
            assert mine["n_seeded"] > 0, name
        if "touching" in name:
            assert n_removed > 0, name


if __name__ == "__main__":
    main()
