"""The segmentation stages.  `Network` is exported here as the reference exports its own, `skeletonize` is the 3-D thinning on the device
(resolved on first use: importing the package loads no stage)."""
__all__ = ["Network", "skeletonize"]


def __getattr__(name):
    if name == "Network":
        from nellie_amd.segmentation.networking import Network
        return Network
    if name == "skeletonize":
        from nellie_amd.segmentation.thinning import skeletonize
        return skeletonize
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
