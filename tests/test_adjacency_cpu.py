"""CPU tests of the adjacency maps and of Hierarchy's surface: the numpy restatement (tests/adjacency_restatement.py) against the
reference's goldens (tests/golden/adjacency), its three primitives on the cases that decide them, Hierarchy's signature and
device rules, and the files run(reassign=True) and run(features=True) ask for before any stage runs."""
import inspect
import os

import numpy as np
import pytest

import adjacency_goldens as ag
import adjacency_restatement as ar

NAMES = ag.names()
SIGNATURE = [("im_info", inspect.Parameter.empty), ("skip_nodes", True), ("viewer", None), ("use_gpu", True), ("low_memory", False),
             ("enable_motility", True), ("enable_adjacency", True), ("device", None), ("node_chunk_size", None), ("max_node_mask_elems", int(5e7)),
             ("device_index", 0)]


def test_there_is_a_fixture_per_image_golden():
    import image_goldens as ig
    assert NAMES and [n[len("adjacency_"):] for n in NAMES] == [n[len("image_"):] for n in ig.names()]


@pytest.mark.parametrize("name", NAMES)
def test_restatement_equals_the_reference(name):
    g = ag.load(name)
    assert ar.same_lists(ar.adjacency_lists(ag.double_of(g)), g["ref"])
    base = g["image"]["base"]
    assert len(g["ref"]["v_b"]) == base["T"] and (g["ref"]["v_n"] == []) == base["skip_nodes"]


def test_goldens_cover_the_regimes():
    most, least, empty_frames, skipped = 0, 10 ** 9, 0, 0
    for name in NAMES:
        g = ag.load(name)
        h = ag.double_of(g)
        skipped += g["ref"]["v_n"] == []
        for t, edges in enumerate(g["ref"]["v_n"]):
            rows = len(h.voxels.coords[t])
            empty_frames += rows == 0
            if rows:
                per_voxel = np.bincount(edges[:, 0], minlength=rows)
                most, least = max(most, per_voxel.max()), min(least, per_voxel.min())
    assert most >= 2 and least == 0 and empty_frames and skipped


def test_primitives_on_the_deciding_cases():
    assert ar.pairs([0, 3, 0, 1], 1).tolist() == [[1, 2], [3, 0]] and ar.pairs(np.zeros(5, np.int32)).shape == (0, 2)
    assert ar.pairs([], 0).shape == (0, 2) and ar.pairs([-2, 2]).tolist() == [[1, 2]]
    off = [0, 0, 0, 2, 2, 3, 3]                                     # empty rows at the start, in the middle and at the end
    assert ar.expand(off, [7, 5, 9]).tolist() == [[2, 7], [2, 5], [4, 9]] and ar.expand([0], []).shape == (0, 2)
    assert ar.lookup([5, 0, 2, 9, 3], [9, 5, 3, 5]).tolist() == [[0, 3], [3, 0], [4, 2]]      # 5 twice: the last position wins
    assert ar.lookup([1, 2], []).shape == (0, 2) and ar.lookup([], [4]).shape == (0, 2)
    with pytest.raises(IndexError):
        ar.lookup([3, 10], [9, 5])
    for a in (ar.pairs([1]), ar.expand([0, 1], [4]), ar.lookup([4], [4])):
        assert a.dtype == np.int64 and a.flags.c_contiguous


def test_restated_lookup_is_the_table_construction():
    """the reference's label_to_idx table, written out, against the sort-based restatement on random labels with repeats"""
    rng = np.random.default_rng(3)
    for _ in range(20):
        parent = rng.integers(0, 40, rng.integers(1, 60))
        child = rng.integers(0, int(parent.max()) + 1, rng.integers(0, 80))
        table = np.full(int(parent.max()) + 1, -1, np.int64)
        for j, lab in enumerate(parent):
            table[lab] = j
        idx = table[child]
        want = np.stack([np.flatnonzero(idx >= 0), idx[idx >= 0]], axis=1)
        assert np.array_equal(ar.lookup(child, parent), want)


def test_hierarchy_has_the_reference_signature():
    from nellie_amd.feature_extraction import Hierarchy, adjacency_maps
    params = inspect.signature(Hierarchy.__init__).parameters
    assert [(k, p.default) for k, p in params.items() if k != "self"] == SIGNATURE
    assert list(inspect.signature(adjacency_maps).parameters)[:2] == ["hierarchy", "device_index"]


def test_hierarchy_module_imports_no_level_module():
    """the level modules import hierarchy.py, so its imports at module level name none of them"""
    import ast
    from nellie_amd.feature_extraction import hierarchy
    tree = ast.parse(open(hierarchy.__file__).read())
    named = [a.name for node in tree.body if isinstance(node, ast.Import) for a in node.names]
    named += [node.module for node in tree.body if isinstance(node, ast.ImportFrom)]
    assert named and not [m for m in named if m.startswith("nellie_amd.feature_extraction")]
    assert hasattr(hierarchy, "Hierarchy") and hasattr(hierarchy, "adjacency_maps")


def _im_info(tmp_path, T=3):
    from nellie_amd.im_info.verifier import ImInfo
    data = np.zeros((T, 4, 8, 8) if T else (4, 8, 8), np.uint16)
    return ImInfo(data, dim_res={"X": .1, "Y": .1, "Z": .1, "T": 1.0}, output_dir=str(tmp_path), name="adj")


def test_hierarchy_device_rules(tmp_path):
    from nellie_amd.feature_extraction import Hierarchy
    from nellie_amd.feature_extraction.image import ImageFeatures
    im_info = _im_info(tmp_path)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Hierarchy(im_info, device="cpu")
    with pytest.raises(ValueError):
        Hierarchy(im_info, device="tpu")
    h = Hierarchy(im_info, low_memory=True, node_chunk_size=7, max_node_mask_elems=11, device="gpu")
    assert h.levels == ImageFeatures.levels and len(h.levels) == 5 and h.skip_nodes and h.enable_adjacency and h.enable_motility
    assert h.num_t == 3 and h.device_index == 0 and h.viewer is None


def _outputs(im_info):
    return sorted(k for k, p in im_info.pipeline_paths.items() if os.path.exists(p))


@pytest.mark.parametrize("keyword, files", [("features", ["im_skel", "im_pixel_class", "im_skel_relabelled", "im_distance", "im_border"]),
                                            ("reassign", ["flow_vector_array", "im_skel_relabelled"])])
def test_run_names_the_missing_files_before_any_stage(tmp_path, keyword, files):
    from nellie_amd.run import run
    im_info = _im_info(tmp_path)
    before = _outputs(im_info)
    with pytest.raises(FileNotFoundError) as exc:
        run(im_info, **{keyword: True})
    assert all(f"'{k}'" in str(exc.value) for k in files) and f"run({keyword}=True)" in str(exc.value)
    assert _outputs(im_info) == before == []


def test_run_counts_the_stages_that_were_asked_for(tmp_path):
    """a file that a requested stage writes is not asked for; one that none writes still is"""
    from nellie_amd.run import run
    im_info = _im_info(tmp_path)
    with pytest.raises(FileNotFoundError) as exc:
        run(im_info, features=True, markers=True)
    assert "im_distance" not in str(exc.value) and "im_border" not in str(exc.value) and "'im_skel'" in str(exc.value)
    with pytest.raises(FileNotFoundError) as exc:
        run(im_info, reassign=True, tracking=True, markers=True)
    assert "flow_vector_array" not in str(exc.value) and "im_skel_relabelled" in str(exc.value)
    assert _outputs(im_info) == []
