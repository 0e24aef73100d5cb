"""
What the stage classes (Filter, Label, Markers, HipNetworkKernels, HuMomentTracking, FlowInterpolator, VoxelReassigner,
VoxelFeatures / Voxels) and run.py share: which device, how many frames, the spacing, which rank of which job, one device object
per frame shape, who creates the output files.  Each stage keeps what carries its own name or a line of the reference.
"""
from __future__ import annotations

import os

from nellie_amd.utils import adaptive_run
from nellie_amd.utils.base_logger import logger


def resolve_device(device, prefer_gpu=True):
    """The reference's per-stage `_resolve_backend` (filtering.py:117-159, labelling.py:115-154) with HIP in the role of CuPy:
    "hip" for every device string that can mean this engine, an error for the others.  Whether a GPU is there is `require_gpu`'s
    question, which each stage asks when the reference's would first touch the device."""
    dev = str(device or "auto").lower()
    if dev not in ("auto", "cpu", "gpu", "cuda", "hip"):          # "hip": what INTEGRATION.md's dispatch forwards; same engine as "gpu"
        raise ValueError(f"Unsupported device '{dev}'. Use 'auto', 'cpu', or 'gpu'.")
    if dev == "cpu" or (dev == "auto" and not prefer_gpu):
        raise RuntimeError("nellie_amd provides the MI355X HIP backend only: device='cpu' is not available "
                           "(no CPU fallback exists in this package; use the reference implementation on CPU)")
    return "hip"


def require_gpu():
    """adaptive_run.is_gpu_unavailable_error recognises this message by its text: it is written here only."""
    if not adaptive_run.gpu_available():
        raise RuntimeError("GPU backend requested but no HIP device / libnellie_hip.so is available.")


def frame_count(im_info, num_t=None):
    """`num_t` when the caller gave one, else the length of the T axis (1 without one)."""
    if num_t is not None:
        return num_t
    return 1 if im_info.no_t else im_info.shape[im_info.axes.index("T")]


def spacing_of(im_info):
    """(Z, Y, X) or (Y, X) voxel size in um."""
    return tuple(im_info.dim_res[a] for a in ("YX" if im_info.no_z else "ZYX"))


def scaled_max_distance(im_info, max_distance_um):
    """The reach of one frame step in um: `max_distance_um` is per second, and never less than 0.5 um
    (hu_tracking.py:150-156, flow_interpolation.py:80-86)."""
    dt = im_info.dim_res.get("T") or 1.0
    if im_info.dim_res.get("T") is None:
        logger.warning("Time resolution missing; assuming 1.0s for max_distance_um scaling.")
    return max(max_distance_um * dt, 0.5)


def env_shard():
    """NELLIE_SHARD: the `shard` of a process that was given none."""
    return os.environ.get("NELLIE_SHARD") or None


def resolve_shard(shard, rendezvous_dir=None, use_env=True):
    """A stage's `shard` argument -> engine.ShardSpec or None (a single process): "env" reads WORLD_SIZE / RANK / LOCAL_RANK,
    a ShardSpec passes through."""
    from nellie_amd.engine import ShardSpec
    if shard is None and use_env:
        shard = env_shard()
    if isinstance(shard, str):
        if shard != "env":
            raise ValueError("shard must be 'env' or an engine.ShardSpec")
        shard = ShardSpec.from_env(rendezvous_dir=rendezvous_dir)
    return shard


class Held:
    """One device object (a pipeline, an engine, a context) for the frame shape in use: asked for another key it closes the one
    it has before it builds the next, so that two never hold HBM at once."""

    def __init__(self):
        self.key = self.obj = None

    def get(self, key, factory):
        if self.obj is None or self.key != key:
            self.close()
            self.obj = factory()
            self.key = key
        return self.obj

    def close(self):
        obj, self.obj, self.key = self.obj, None, None
        if obj is not None:
            obj.close()


def shape_key(shape):
    return tuple(int(s) for s in shape)


def open_outputs(im_info, outputs, creator, announce=None, wait=None):
    """The memmaps of `outputs`, a list of (path, dtype, description).  The creator (a single process, or rank 0) creates every
    file and then announces them; every other rank waits for that and maps them."""
    if creator:
        maps = [im_info.allocate_memory(path, dtype=dtype, description=description, return_memmap=True)
                for path, dtype, description in outputs]
        if announce is not None:
            announce()
        return maps
    if wait is not None:
        wait()
    return [im_info.get_memmap(path) for path, _, _ in outputs]


def flush(*memmaps):
    for mm in memmaps:
        if hasattr(mm, "flush"):
            mm.flush()


class FrameCounted:
    """Mixin of the stages with the reference's `_get_t`."""

    def _get_t(self):
        self.num_t = frame_count(self.im_info, self.num_t)
