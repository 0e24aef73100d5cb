"""CPU tests of the one writer of the five feature tables (feature_extraction/hierarchy.py, write_table): for every level the
restatement's text from the same object, character for character, and the edge cases of the header rule -- no frame with rows, an
empty first frame, a clash of statistic names -- each against text written out here."""
import warnings
from types import SimpleNamespace

import numpy as np
import pytest

import branch_features_restatement as br
import branch_goldens as bg
import component_features_restatement as cr
import component_goldens as cg
import image_features_restatement as ir
import image_goldens as ig
import node_features_restatement as nr
import node_goldens as ng
import voxel_goldens as vg

KEYS = ["mean", "std_dev", "min", "max", "sum"]
VOXEL_STATS = ["linear_vel", "angular_vel", "linear_acc", "angular_acc", "rel_linear_vel", "rel_angular_vel", "rel_linear_acc", "rel_angular_acc",
               "rel_directionality", "structure", "intensity"]
NODE_RAW = ["divergence", "convergence", "vergere", "node_thickness", "x", "y", "z"]
BRANCH_RAW = ["branch_length", "branch_thickness", "branch_aspect_ratio", "branch_tortuosity", "branch_area", "branch_axis_length_maj",
              "branch_axis_length_min", "branch_extent", "branch_solidity", "reassigned_label", "x", "y", "z"]
ORGANELLE_RAW = ["organelle_area", "organelle_axis_length_maj", "organelle_axis_length_min", "organelle_extent", "organelle_solidity",
                 "reassigned_label", "x", "y", "z"]


def written(level, tmp_path, labels=None):
    from nellie_amd.feature_extraction.hierarchy import write_table
    path = str(tmp_path / "table.csv")
    write_table(level, path, labels)
    return open(path).read()


def quiet(run):
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        run()


# ---- the five tables from the goldens ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["voxels_3d_aniso", "voxels_2d"])
def test_the_voxel_table(name, tmp_path):
    ref = vg.load(name)["ref"]
    level = SimpleNamespace(features_to_save=ref["features_to_save"], **{k: ref[k] for k in ref["features_to_save"]})
    assert written(level, tmp_path) == vg.expected_csv(ref)


@pytest.mark.parametrize("name", ["nodes_3d_aniso", "nodes_2d"])
def test_the_node_table(name, tmp_path):
    g = ng.load(name)
    own = nr.Nodes(ng.hierarchy_double(g["base"], g["border"]))
    own.run()
    assert written(own, tmp_path) == nr.feature_table(own)[1]


@pytest.mark.parametrize("name, skip_nodes", [("branches_3d_integer_flow", False), ("branches_3d_empty_frame", True), ("branches_2d", True)])
def test_the_branch_table(name, skip_nodes, tmp_path):
    g = bg.load(name)                                             # with nodes only where every frame has as many node labels as branches
    own = br.Branches(bg.double_of(g, skip_nodes=True) if skip_nodes else bg.double_of(g))
    own.run()
    assert written(own, tmp_path, own.branch_label) == br.feature_table(own)[1]


@pytest.mark.parametrize("name", ["components_3d_empty_frame", "components_2d", "components_3d_skip_nodes"])
def test_the_organelle_table(name, tmp_path):
    own = cr.Components(cg.double_of(cg.load(name)))
    own.run()
    assert written(own, tmp_path, own.component_label) == cr.feature_table(own)[1]


@pytest.mark.parametrize("name", ["image_3d_empty_frame", "image_3d_skip_nodes", "image_2d"])
def test_the_image_table(name, tmp_path):
    own = ir.Image(ig.double_of(ig.load(name)))
    quiet(own.run)
    assert written(own, tmp_path, [np.zeros(1, np.int64)] * len(own.time)) == ir.feature_table(own)[1]


# ---- the header rule ----------------------------------------------------------------------------------------------------------------
def level_of(raw, frames, **aggregates):
    """a level of `frames` frames without rows: every feature of `raw` an empty column, the aggregates as given"""
    return SimpleNamespace(features_to_save=list(raw), **{k: [np.zeros(0)] * frames for k in raw}, **aggregates)


def empty_nodes():
    """two frames without nodes: the voxel aggregates over no groups are named all the same, (1, 0) each"""
    frame = {stat: {key: np.zeros((1, 0)) for key in KEYS} for stat in VOXEL_STATS}
    return level_of(NODE_RAW, 2, aggregate_voxel_metrics=[frame, dict(frame)])


EMPTY_NODES = ",".join(["t", "label"] + [f"{stat}_{key}" for stat in VOXEL_STATS for key in KEYS] + [f"{k}_raw" for k in NODE_RAW]) + "\n"


def empty_branches():
    level = level_of(BRANCH_RAW, 2, aggregate_node_metrics=[{}, {}], aggregate_voxel_metrics=[{}, {}])
    level.branch_label = [np.array([], dtype=int)] * 2
    return level


EMPTY_BRANCHES = ("t,label,branch_length_raw,branch_thickness_raw,branch_aspect_ratio_raw,branch_tortuosity_raw,branch_area_raw,"
                  "branch_axis_length_maj_raw,branch_axis_length_min_raw,branch_extent_raw,branch_solidity_raw,reassigned_label_raw,x_raw,y_raw,z_raw\n")


def empty_organelles():
    level = level_of(ORGANELLE_RAW, 2, aggregate_node_metrics=[{}, {}], aggregate_voxel_metrics=[{}, {}], aggregate_branch_metrics=[{}, {}])
    level.component_label = [np.array([], dtype=int)] * 2
    return level


EMPTY_ORGANELLES = ("t,label,organelle_area_raw,organelle_axis_length_maj_raw,organelle_axis_length_min_raw,organelle_extent_raw,"
                    "organelle_solidity_raw,reassigned_label_raw,x_raw,y_raw,z_raw\n")


def late_voxels():
    """no voxel in frame 0, two in frame 1"""
    return SimpleNamespace(features_to_save=["intensity", "x", "z"], intensity=[np.zeros(0, np.uint16), np.array([7, 9], np.uint16)],
                           x=[np.zeros(0, np.int64), np.array([3, 4])], z=[np.zeros(0), np.full(2, np.nan)])


LATE_VOXELS = "t,label,intensity_raw,x_raw,z_raw\n1.0,0.0,7.0,3.0,\n1.0,1.0,9.0,4.0,\n"


def late_nodes():
    """no node in frame 0, two in frame 1"""
    keys0 = {key: np.zeros((1, 0)) for key in KEYS}
    keys1 = dict(mean=np.array([[1.5, np.nan]]), std_dev=np.array([[0.5, np.nan]]), min=np.array([[1.0, np.nan]]), max=np.array([[2.0, np.nan]]),
                 sum=np.array([[3.0, 0.0]]))
    return SimpleNamespace(features_to_save=["node_thickness", "x"], aggregate_voxel_metrics=[{"intensity": keys0}, {"intensity": keys1}],
                           node_thickness=[np.zeros(0), np.array([0.25, np.nan])], x=[np.zeros(0), np.array([5.0, 6.0])])


LATE_NODES = ("t,label,intensity_mean,intensity_std_dev,intensity_min,intensity_max,intensity_sum,node_thickness_raw,x_raw\n"
              "1.0,0.0,1.5,0.5,1.0,2.0,3.0,0.25,5.0\n1.0,1.0,,,,,0.0,,6.0\n")


def test_no_node_in_any_frame_keeps_the_aggregate_columns(tmp_path):
    text = written(empty_nodes(), tmp_path)
    assert text == EMPTY_NODES and len(text.strip().split(",")) == 2 + 11 * 5 + 7


def test_no_branch_and_no_organelle_in_any_frame_leaves_the_raw_columns(tmp_path):
    level = empty_branches()
    assert written(level, tmp_path, level.branch_label) == EMPTY_BRANCHES
    level = empty_organelles()
    assert written(level, tmp_path, level.component_label) == EMPTY_ORGANELLES


def test_no_frame_at_all_leaves_the_raw_columns(tmp_path):
    assert written(level_of(BRANCH_RAW, 0, aggregate_node_metrics=[], aggregate_voxel_metrics=[]), tmp_path, []) == EMPTY_BRANCHES
    assert written(level_of(NODE_RAW, 0, aggregate_voxel_metrics=[]), tmp_path) == "t,label," + ",".join(f"{k}_raw" for k in NODE_RAW) + "\n"


def test_an_empty_first_frame_writes_one_header_and_the_rows_of_the_second(tmp_path):
    assert written(late_voxels(), tmp_path) == LATE_VOXELS
    assert written(late_nodes(), tmp_path) == LATE_NODES


def test_a_statistic_aggregated_from_two_levels_is_refused(tmp_path):
    g = bg.load("branches_3d_integer_flow")
    own = br.Branches(bg.double_of(g))
    own.run()
    own.aggregate_node_metrics[0] = dict(own.aggregate_node_metrics[0], intensity=own.aggregate_voxel_metrics[0]["intensity"])
    with pytest.raises(AssertionError, match="intensity"):
        written(own, tmp_path, own.branch_label)
    own = cr.Components(cg.double_of(cg.load("components_2d")))
    own.run()
    own.aggregate_branch_metrics[0] = dict(own.aggregate_branch_metrics[0], structure=own.aggregate_voxel_metrics[0]["structure"])
    with pytest.raises(AssertionError, match="structure"):
        written(own, tmp_path, own.component_label)
    own = ir.Image(ig.double_of(ig.load("image_2d")))
    quiet(own.run)
    own.aggregate_component_metrics[1] = dict(own.aggregate_component_metrics[1], branch_length=own.aggregate_branch_metrics[1]["branch_length"])
    with pytest.raises(AssertionError, match="branch_length"):
        written(own, tmp_path, [np.zeros(1, np.int64)] * len(own.time))
