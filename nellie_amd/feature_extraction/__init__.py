"""Feature extraction: the hierarchy's levels on the HIP engine (voxels, nodes, branches, organelles, image), and `Hierarchy`, which
runs them all and writes the adjacency maps."""
from nellie_amd.feature_extraction.branches import BranchFeatures, Branches
from nellie_amd.feature_extraction.components import ComponentFeatures, Components
from nellie_amd.feature_extraction.hierarchy import Hierarchy, adjacency_maps
from nellie_amd.feature_extraction.image import Image, ImageFeatures
from nellie_amd.feature_extraction.nodes import NodeFeatures, Nodes, aggregate_stats_for_class
from nellie_amd.feature_extraction.voxels import VoxelFeatures, Voxels

__all__ = ["Voxels", "VoxelFeatures", "Nodes", "NodeFeatures", "aggregate_stats_for_class", "Branches", "BranchFeatures", "Components",
           "ComponentFeatures", "Image", "ImageFeatures", "Hierarchy", "adjacency_maps"]
