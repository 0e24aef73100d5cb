"""Feature extraction on the MI355X HIP engine: the voxel level of the reference's Hierarchy."""
from nellie_amd.feature_extraction.voxels import VoxelFeatures, Voxels

__all__ = ["Voxels", "VoxelFeatures"]
