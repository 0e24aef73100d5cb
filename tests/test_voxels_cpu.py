"""CPU tests of the voxel level of the hierarchy: tests/voxel_features_restatement.py against every golden the reference's Voxels
class produced (tests/golden/voxels, tests/golden/make_golden_voxels.py).

Which comparison applies to which attribute:
  exact (values and dtype): time, coords, x, y, z, intensity, structure, branch_labels, component_labels, the three node limit
      arrays and both node lists (CSR), stats_to_aggregate, features_to_save, and the NaN pattern of every float attribute.
  bit for bit: all 13 float attributes (vec01 .. rel_directionality) when the restatement's motility is fed the reference's own
      float64 interpolation results (stored with the golden): from there on the restatement uses numpy's own operations in the
      reference's order.
  bounded: the interpolated vectors themselves, where the restatement sums the neighbours in another order than the reference:
      within the bound of DESIGN.md section 11 (flow_interpolation_restatement.tolerance) per row, in voxels.  The motility from the
      restatement's own vectors is that error propagated; it is checked at its source, the vectors, and its NaN pattern exactly.
"""
import numpy as np
import pytest

import flow_interpolation_restatement as fr
import voxel_features_restatement as vr
import voxel_goldens as vg

NAMES = vg.names()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def test_goldens_cover_the_cases():
    assert len(NAMES) >= 12
    gs = [vg.load(n) for n in NAMES]
    assert {g["D"] for g in gs} == {2, 3} and all(g["T"] == 4 for g in gs)
    assert {g["raw"].dtype for g in gs} >= {np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.float32)}
    assert any(g["skip_nodes"] for g in gs) and any(not g["enable_motility"] for g in gs)
    assert any(g["comp"].shape[-1] == 70 for g in gs)
    assert all(g["margin"] > 1e-9 and g["gap"] > 1e-6 for g in gs)
    assert any(len(c) == 0 for g in gs for c in g["ref"]["coords"])                                  # an all-background frame
    assert any(((g["branch"] == 0) & (g["comp"] > 0)).any() for g in gs)                             # branch label 0 inside objects
    nodes = [g for g in gs if not g["skip_nodes"]]
    assert any((g["distance"][g["pixel_class"] > 0] == 0).any() for g in nodes)                      # radii of 0
    assert any((g["distance"] > max(g["comp"].shape[1:])).any() for g in nodes)                      # radii past every face


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_golden(name):
    g = vg.load(name)
    ref = g["ref"]
    args = [g[k] for k in vg.INPUTS] + [g["flow"], g["spacing"], g["dt"]]
    kw = dict(skip_nodes=g["skip_nodes"], enable_motility=g["enable_motility"])
    own = vr.voxels(*args, **kw)
    fed = vr.voxels(*args, vectors=g["ref_flow_px"], **kw)
    assert own["margin"] > 1e-9 and own["gap"] > 1e-6
    for t in range(g["T"]):
        n = len(ref["coords"][t])
        for k in vg.PER_VOXEL:
            assert same(own[k][t], ref[k][t]), (k, t)
        for k in vg.FLOAT_ATTRS:
            want = ref[k][t]
            if k in ("vec01", "vec12") and len(want) == 0 and n > 0:         # no voxel had a flow neighbour: (0, D) there, NaN here
                assert own[k][t].shape == (n, g["D"]) and np.isnan(own[k][t]).all() and np.isnan(fed[k][t]).all()
                continue
            assert same(fed[k][t], want), (k, t)
            assert np.array_equal(np.isnan(own[k][t]), np.isnan(want)), (k, t)
        for key in ("bw", "fw"):
            seen = g["ref_flow_px"].get((t, key))
            if seen is None:
                assert np.isnan(own["flow_px"][(t, key)]).all()
            elif len(seen) == n and n > 0:
                fr.assert_close(own["flow_px"][(t, key)], seen, own["flow_k"][(t, key)], own["flow_vmax"][(t, key)], f"{name} t{t} {key}")
            else:
                assert np.isnan(own["flow_px"][(t, key)]).all()
        if g["skip_nodes"]:
            continue
        for ax in range(3):
            want = ref[f"node_dim{ax}_lims"][t]
            assert (want is None and ax >= g["D"]) or same(own["node_lims"][t][ax], want), (ax, t)
        for mine, theirs in ((own["node_voxels"][t], ref["node_voxel_idxs_csr"][t]), (own["voxel_nodes"][t], ref["node_labels_csr"][t])):
            if n == 0 and len(theirs[0]) == 1 and mine is own["voxel_nodes"][t]:
                assert len(mine[1]) == 0
                continue
            assert same(mine[0], theirs[0]) and same(mine[1], theirs[1]), t


def test_node_boxes_clamp_and_include_both_ends():
    pc = np.zeros((6, 7), np.uint8)
    dist = np.zeros((6, 7), np.float32)
    pc[2, 3], dist[2, 3] = 1, 1.5                    # trunc(0.5) = 0 .. trunc(3.5) + 1 = 4; 1 .. 5
    pc[0, 0], dist[0, 0] = 2, 0.0                    # 0 .. 1
    pc[5, 6], dist[5, 6] = 1, 40.0                   # clamped to 0 .. shape
    nodes, lims = vr.node_boxes(pc, dist)
    assert nodes.tolist() == [[0, 0], [2, 3], [5, 6]]
    assert lims[0].tolist() == [[0, 1], [0, 4], [0, 6]] and lims[1].tolist() == [[0, 1], [1, 5], [0, 7]]
    coords = np.argwhere(np.ones((6, 7), bool))
    (noff, nval), (voff, vval) = vr.node_assignment(lims, coords)
    assert np.diff(noff).tolist() == [4, 25, 42]
    assert vval[voff[0]:voff[1]].tolist() == [0, 2] and vval[voff[-2]:voff[-1]].tolist() == [2]


def test_pivot_is_the_lowest_index_of_the_smallest_norm():
    vec = np.array([[3.0, 4.0], [0.0, 5.0], [np.nan, 1.0], [1.0, 0.0], [5.0, 0.0]])
    pivot, gap = vr.pivots(vec, np.array([2, 2, 0, 3, 2]))
    assert pivot.tolist() == [-1, -1, 0, 3] and gap == np.inf


def test_voxel_features_opens_the_files_and_writes_the_reference_table(tmp_path):
    """without a GPU: VoxelFeatures reads back the stacks an ImInfo of this package wrote, its saving rule on the golden's
    attributes gives the reference's table byte for byte, and device="cpu" raises"""
    from types import SimpleNamespace
    from nellie_amd.feature_extraction import VoxelFeatures
    from nellie_amd.im_info.verifier import ImInfo
    g = vg.load("voxels_3d_aniso")
    dim_res = dict(zip("ZYX", (float(s) for s in g["spacing"])), T=g["dt"])
    im_info = ImInfo(g["raw"], dim_res=dim_res, output_dir=str(tmp_path), name="voxels")
    paths = im_info.pipeline_paths
    stacks = dict(im_preprocessed=g["struct"], im_distance=g["distance"], im_skel=(g["pixel_class"] > 0).astype(np.uint8), im_instance_label=g["comp"],
                  im_skel_relabelled=g["branch"], im_border=np.zeros(g["comp"].shape, np.uint8), im_pixel_class=g["pixel_class"])
    for key, data in stacks.items():
        im_info.allocate_memory(paths[key], dtype=str(data.dtype), data=data, description=key)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        VoxelFeatures(im_info, device="cpu")
    vf = VoxelFeatures(im_info)
    assert vf.num_t == 4 and vf.spacing == tuple(float(s) for s in g["spacing"]) and vf.skip_nodes is False and vf.enable_motility is True
    vf._allocate_memory()
    for attr, key in (("im_raw", "raw"), ("im_struct", "struct"), ("im_distance", "distance"), ("label_components", "comp"),
                      ("label_branches", "branch"), ("im_pixel_class", "pixel_class")):
        assert same(np.asarray(getattr(vf, attr)), g[key]), attr
    vf.voxels = SimpleNamespace(features_to_save=g["ref"]["features_to_save"], **{k: g["ref"][k] for k in g["ref"]["features_to_save"]})
    from nellie_amd.feature_extraction.hierarchy import write_table
    write_table(vf.voxels, paths["features_voxels"])
    assert open(paths["features_voxels"]).read() == vg.expected_csv(g["ref"])
