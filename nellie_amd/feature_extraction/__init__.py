"""Feature extraction: the hierarchy's levels on the HIP engine (voxels, nodes)."""
from nellie_amd.feature_extraction.nodes import NodeFeatures, Nodes, aggregate_stats_for_class
from nellie_amd.feature_extraction.voxels import VoxelFeatures, Voxels

__all__ = ["Voxels", "VoxelFeatures", "Nodes", "NodeFeatures", "aggregate_stats_for_class"]
