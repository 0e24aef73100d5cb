"""Feature extraction: the hierarchy's levels on the HIP engine (voxels, nodes, branches, organelles, image), `Hierarchy`, which
runs them all and writes the adjacency maps, and `FeatureOverlay`, which paints a column of their tables onto the label mask."""
from nellie_amd.feature_extraction.branches import BranchFeatures, Branches, convex_counts
from nellie_amd.feature_extraction.components import ComponentFeatures, Components
from nellie_amd.feature_extraction.hierarchy import Hierarchy, adjacency_maps
from nellie_amd.feature_extraction.image import Image, ImageFeatures
from nellie_amd.feature_extraction.nodes import NodeFeatures, Nodes, aggregate_stats_for_class
from nellie_amd.feature_extraction.overlay import FeatureOverlay, overlay_frame, overlay_values
from nellie_amd.feature_extraction.voxels import VoxelFeatures, Voxels

__all__ = ["Voxels", "VoxelFeatures", "Nodes", "NodeFeatures", "aggregate_stats_for_class", "Branches", "BranchFeatures", "Components",
           "ComponentFeatures", "Image", "ImageFeatures", "Hierarchy", "adjacency_maps", "FeatureOverlay",
           "overlay_values", "overlay_frame", "convex_counts"]
