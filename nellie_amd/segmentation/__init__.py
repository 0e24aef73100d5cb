"""The segmentation stages.  `Network` is exported here as the reference exports its own (resolved on first use: importing the
package loads no stage)."""
__all__ = ["Network"]


def __getattr__(name):
    if name == "Network":
        from nellie_amd.segmentation.networking import Network
        return Network
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
