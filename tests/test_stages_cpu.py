"""The scaffolding the stage classes share (nellie_amd/stage.py), without a GPU: device strings, when each class asks for the GPU,
shard resolution, one device object per frame shape, who creates the output files, frame count / spacing / reach.  Wherever a
class shows the behaviour, the case goes through the class, so that the same case holds whatever the class is built from."""
import logging
import os
from types import SimpleNamespace

import numpy as np
import pytest

from nellie_amd.engine import ShardSpec

PATHS = ("im_preprocessed", "im_instance_label", "im_marker", "im_distance", "im_border", "im_skel", "im_skel_relabelled",
         "im_pixel_class", "flow_vector_array", "voxel_matches", "im_branch_label_reassigned", "im_obj_label_reassigned",
         "features_voxels")


def _im_info(tmp_path, no_t=False, no_z=False, dt=1.0):
    """(3, 4, 8, 8) TZYX, (5, 8, 8) TYX, or the same without T; a log of every file it is asked to create or map"""
    def boom(*a, **kw):
        raise AssertionError("must not touch files")
    dim_res = {"X": .107, "Y": .107, "Z": None if no_z else .29}
    if dt is not None:
        dim_res["T"] = dt
    shape, axes = ((5, 8, 8), "TYX") if no_z else ((3, 4, 8, 8), "TZYX")
    return SimpleNamespace(no_t=no_t, no_z=no_z, shape=shape[no_t:], axes=axes[no_t:], dim_res=dim_res, im_path=str(tmp_path / "im.npy"),
                           pipeline_paths={k: str(tmp_path / f"{k}.npy") for k in PATHS}, get_memmap=boom, allocate_memory=boom)


def _stage(name):
    from nellie_amd.feature_extraction.voxels import VoxelFeatures
    from nellie_amd.segmentation.filtering import Filter
    from nellie_amd.segmentation.labelling import Label
    from nellie_amd.segmentation.mocap_marking import Markers
    from nellie_amd.segmentation.networking import HipNetworkKernels
    from nellie_amd.tracking.flow_interpolation import FlowInterpolator
    from nellie_amd.tracking.hu_tracking import HuMomentTracking
    from nellie_amd.tracking.voxel_reassignment import VoxelReassigner
    return {c.__name__: c for c in (Filter, Label, Markers, HipNetworkKernels, HuMomentTracking, FlowInterpolator, VoxelReassigner,
                                    VoxelFeatures)}[name]


@pytest.fixture
def gpu(monkeypatch):
    """adaptive_run.gpu_available() answers what the test sets: gpu(True) / gpu(False)"""
    from nellie_amd.utils import adaptive_run
    return lambda there: monkeypatch.setattr(adaptive_run, "gpu_available", lambda: there)


WITH_DEVICE = ["Filter", "Label", "Markers", "HuMomentTracking", "VoxelReassigner", "VoxelFeatures"]


# ---------------------------------------------------------------------------------------------------------------- 1. device strings
@pytest.mark.parametrize("name", WITH_DEVICE)
def test_device_strings(name, tmp_path, gpu):
    gpu(True)
    cls, im = _stage(name), _im_info(tmp_path)
    with pytest.raises(ValueError, match="Unsupported device"):
        cls(im, device="tpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        cls(im, device="cpu")
    for device in (None, "auto", "gpu", "GPU", "cuda", "hip"):
        assert cls(im, device=device).im_info is im


def test_markers_auto_without_prefer_gpu_is_the_cpu_request(tmp_path, gpu):
    gpu(True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _stage("Markers")(_im_info(tmp_path), device="auto", prefer_gpu=False)
    assert _stage("Markers")(_im_info(tmp_path), device="gpu", prefer_gpu=False).device_type == "hip"


# ---------------------------------------------------------------------------------------------------------------- 2. when the GPU is asked for
NO_GPU = "GPU backend requested but no HIP device / libnellie_hip.so is available."


@pytest.mark.parametrize("name", ["Filter", "Label", "Markers", "HuMomentTracking", "FlowInterpolator"])
def test_no_gpu_raises_at_construction(name, tmp_path, gpu):
    gpu(False)
    with pytest.raises(RuntimeError, match="GPU backend requested") as err:
        _stage(name)(_im_info(tmp_path))
    assert str(err.value) == NO_GPU
    from nellie_amd.utils import adaptive_run
    assert adaptive_run.is_gpu_unavailable_error(err.value)


@pytest.mark.parametrize("name", ["VoxelReassigner", "VoxelFeatures"])
def test_no_gpu_raises_in_run(name, tmp_path, gpu):
    gpu(False)
    stage = _stage(name)(_im_info(tmp_path))                   # constructs
    with pytest.raises(RuntimeError, match="GPU backend requested") as err:
        stage.run()
    assert str(err.value) == NO_GPU and not os.listdir(tmp_path)


def test_no_gpu_raises_in_voxels_run(gpu):
    from nellie_amd.feature_extraction.voxels import Voxels
    gpu(False)
    voxels = Voxels(SimpleNamespace(num_t=None))
    with pytest.raises(RuntimeError, match="GPU backend requested"):
        voxels.run()


def test_no_gpu_raises_at_the_first_network_context(gpu):
    gpu(False)
    kernels = _stage("HipNetworkKernels")()
    with pytest.raises(RuntimeError, match="GPU backend requested") as err:
        kernels._get_pixel_class(np.zeros((4, 4), np.int32))
    assert str(err.value) == NO_GPU
    kernels.close()


@pytest.mark.parametrize("name", ["HuMomentTracking", "VoxelReassigner", "FlowInterpolator"])
def test_no_gpu_is_never_asked_for_without_t(name, tmp_path, gpu):
    gpu(False)
    stage = _stage(name)(_im_info(tmp_path, no_t=True))
    if name != "FlowInterpolator":
        assert stage.run() is None
    assert not os.listdir(tmp_path)


# ---------------------------------------------------------------------------------------------------------------- 3. shard
def _resolved(name, im, shard):
    """what the class makes of its `shard` argument and the environment; the directory its ranks are to meet in"""
    stage = _stage(name)(im, shard=shard)
    if name == "Markers":
        return stage._slab_plan(im.shape[1:])[1], None
    return stage._shard_spec(), os.path.dirname(im.pipeline_paths["im_preprocessed"])


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("env", [None, "env"])
@pytest.mark.parametrize("arg", [None, "env", "spec", "nonsense"])
@pytest.mark.parametrize("name", ["Filter", "Label", "Markers"])
def test_shard_resolution(name, arg, env, world, tmp_path, gpu, monkeypatch):
    gpu(True)
    monkeypatch.delenv("NELLIE_SHARD", raising=False)
    if env is not None:
        monkeypatch.setenv("NELLIE_SHARD", env)
    for key, value in (("WORLD_SIZE", world), ("RANK", 1), ("LOCAL_RANK", 1), ("MASTER_PORT", 29999)):
        monkeypatch.setenv(key, str(value))
    im = _im_info(tmp_path)
    if arg == "nonsense":
        with pytest.raises(ValueError, match="shard must be 'env' or an engine.ShardSpec"):
            _resolved(name, im, arg)
        return
    given = ShardSpec(rank=1, world=2, device=3)
    spec, meet_in = _resolved(name, im, given if arg == "spec" else arg)
    if arg == "spec":
        assert spec is given
    elif world == 2 and (arg == "env" or env == "env"):
        assert spec == ShardSpec(rank=1, world=2, device=1, rendezvous_dir=meet_in, tag="29999")
    else:
        assert spec is None


# ---------------------------------------------------------------------------------------------------------------- 4. one object per shape
def _recording(log):
    class Device:
        """stands for a FramePipeline, an engine or a Context"""
        def __init__(self, *a, **kw):
            self.shape = tuple(a[0]) if a else None                 # a FramePipeline's
            log.append(("build", self))

        def close(self):
            log.append(("close", self))
    return Device


HOLDERS = {  # class, the method, what it builds (module, name), two keys
    "filter-pipeline": ("Filter", "_get_pipeline", ("nellie_amd.segmentation.filtering", "FramePipeline"), ((8, 16, 16), (8, 16, 24))),
    "filter-engine": ("Filter", "_get_engine", ("nellie_amd.engine", "make_engine"), ((8, 16, 16), (8, 16, 24))),
    "label-pipeline": ("Label", "_get_pipeline", ("nellie_amd.segmentation.labelling", "FramePipeline"), ((8, 16, 16), (8, 16, 24))),
    "label-engine": ("Label", "_get_engine", ("nellie_amd.engine", "make_engine"), ((8, 16, 16), (8, 16, 24))),
    "markers-pipeline": ("Markers", "_get_pipeline", ("nellie_amd.segmentation.mocap_marking", "FramePipeline"), ((8, 16, 16), (16, 24))),
    "network-context": ("HipNetworkKernels", "_hip_context", ("nellie_amd.hipnative", "Context"), ((16, 16), (4, 16, 16))),
}


@pytest.mark.parametrize("case", list(HOLDERS))
def test_one_device_object_per_shape(case, tmp_path, gpu, monkeypatch):
    import importlib
    gpu(True)
    monkeypatch.delenv("NELLIE_SHARD", raising=False)
    name, method, (module, built), (k1, k2) = HOLDERS[case]
    log = []
    monkeypatch.setattr(importlib.import_module(module), built, _recording(log))
    stage = _stage(name)() if name == "HipNetworkKernels" else _stage(name)(_im_info(tmp_path))
    get = getattr(stage, method)
    a = get(k1)
    assert get(k1) is a and get(list(k1)) is a and log == [("build", a)]            # same key: same object, built once
    b = get(k2)
    assert b is not a and log == [("build", a), ("close", a), ("build", b)]         # new key: the old one closed once, and first
    assert get(k2) is b
    stage.close()
    stage.close()                                                                   # twice is harmless
    assert log[3:] == [("close", b)]
    c = get(k2)
    assert c is not b and log[4:] == [("build", c)]
    stage.close()


def test_holder_with_a_factory_that_raises():
    from nellie_amd.stage import Held
    log = []
    device = _recording(log)
    held = Held()
    a = held.get("a", device)
    assert held.get("a", device) is a

    def fails():
        raise MemoryError("no room")
    with pytest.raises(MemoryError):
        held.get("b", fails)
    assert log == [("build", a), ("close", a)] and held.obj is None and held.key is None
    b = held.get("a", device)                                                       # no stale key: the closed object is not handed out
    assert b is not a and log[2:] == [("build", b)]
    held.close()
    held.close()
    assert log[3:] == [("close", b)]


# ---------------------------------------------------------------------------------------------------------------- 5. output files
def _logging_files(im, log, shape):
    im.get_memmap = lambda path: (log.append(("map", os.path.basename(path))), np.zeros(shape, np.int32))[1]
    im.allocate_memory = lambda path, dtype=None, description="", return_memmap=False: (
        log.append(("create", os.path.basename(path), dtype)), np.zeros(shape, dtype))[1]


OUTPUTS = {"Filter": [("im_preprocessed.npy", "float32")], "Label": [("im_instance_label.npy", "int32")],
           "Markers": [("im_marker.npy", "uint8"), ("im_distance.npy", "float32"), ("im_border.npy", "uint8")]}


@pytest.mark.parametrize("rank", [None, 0, 1])
@pytest.mark.parametrize("name", ["Filter", "Label", "Markers"])
def test_who_creates_the_output_files(name, rank, tmp_path, gpu, monkeypatch):
    """rank 0 (or a single process) creates every file and then tells the others; another rank waits and then maps them"""
    gpu(True)
    monkeypatch.delenv("NELLIE_SHARD", raising=False)
    im, log = _im_info(tmp_path), []
    _logging_files(im, log, im.shape)
    if name == "Markers":
        from nellie_amd import rendezvous
        meet = SimpleNamespace(rank=rank, publish=lambda what: log.append(("publish", what)), wait=lambda what: log.append(("wait", what)))
        monkeypatch.setattr(rendezvous, "rendezvous_for", lambda spec, directory: meet)
        stage = _stage(name)(im, shard=None if rank is None else ShardSpec(rank=rank, world=2))
        stage.sigmas = [1.0]
        stage._allocate_memory()
        told, waited = ("publish", "markers_files_ready"), ("wait", "markers_files_ready")
    else:
        stage = _stage(name)(im)
        engine = None if rank is None else SimpleNamespace(kind="rank-slab", spec=SimpleNamespace(rank=rank), barrier=lambda: log.append("barrier"))
        stage._allocate_memory(engine)
        told = waited = "barrier"
    outputs = [base for base, _ in OUTPUTS[name]]
    log = [e for e in log if not (e[0] == "map" and e[1] not in outputs)]           # the inputs every rank maps
    create = [("create", base, dtype) for base, dtype in OUTPUTS[name]]
    if rank is None:
        assert log == create
    elif rank == 0:
        assert log == create + [told]
    else:
        assert log == [waited] + [("map", base) for base in outputs]


def test_open_outputs_order():
    from nellie_amd.stage import open_outputs
    log = []
    im = SimpleNamespace()
    _logging_files(im, log, (2, 2))
    outputs = [("d/a.npy", "uint8", "first"), ("d/b.npy", "float32", "second")]
    announce, wait = (lambda: log.append("announce")), (lambda: log.append("wait"))
    a, b = open_outputs(im, outputs, True, announce, wait)
    assert (a.dtype, b.dtype) == (np.uint8, np.float32) and log == [("create", "a.npy", "uint8"), ("create", "b.npy", "float32"), "announce"]
    del log[:]
    assert len(open_outputs(im, outputs, False, announce, wait)) == 2 and log == ["wait", ("map", "a.npy"), ("map", "b.npy")]
    del log[:]
    open_outputs(im, outputs, True)
    assert log == [("create", "a.npy", "uint8"), ("create", "b.npy", "float32")]


# ---------------------------------------------------------------------------------------------------------------- 6. frames, spacing, reach
REACH = [  # dt, max_distance_um -> reach, warns
    (2.0, 0.4, 0.8, False), (1.0, 0.3, 0.5, False), (0.5, 2.0, 1.0, False), (None, 0.7, 0.7, True), (None, 0.2, 0.5, True)]


@pytest.mark.parametrize("no_z", [False, True])
@pytest.mark.parametrize("dt,um,reach,warns", REACH)
def test_frames_spacing_and_reach_of_the_classes(dt, um, reach, warns, no_z, tmp_path, gpu, caplog):
    gpu(True)
    im = _im_info(tmp_path, no_z=no_z, dt=dt)
    spacing, frames = ((.107, .107), 5) if no_z else ((.29, .107, .107), 3)
    with caplog.at_level(logging.WARNING):
        hu = _stage("HuMomentTracking")(im, max_distance_um=um)
    assert (hu.scaling, hu.num_t, hu.max_distance_um) == (spacing, frames, reach)
    assert ["Time resolution missing" in r.getMessage() for r in caplog.records] == [True] * warns
    assert _stage("HuMomentTracking")(im, num_t=2).num_t == 2
    np.save(im.im_path, np.zeros(im.shape, np.uint8))
    np.save(im.pipeline_paths["flow_vector_array"], np.zeros((0, 2 + 2 * len(spacing))))
    im.get_memmap = np.load
    flow = _stage("FlowInterpolator")(im, max_distance_um=um)
    assert (flow.scaling, flow.num_t, flow.max_distance_um) == (spacing, frames, reach) and type(flow.max_distance_um) is np.float64
    voxels = _stage("VoxelFeatures")(im)
    assert (voxels.spacing, voxels.num_t) == (spacing, frames)


@pytest.mark.parametrize("name", ["Filter", "Label", "Markers", "VoxelReassigner"])
def test_frame_count_of_the_classes(name, tmp_path, gpu):
    gpu(True)
    cls = _stage(name)
    assert cls(_im_info(tmp_path)).num_t == 3 and cls(_im_info(tmp_path), num_t=2).num_t == 2
    assert cls(_im_info(tmp_path, no_z=True)).num_t == 5
    single = cls(_im_info(tmp_path, no_t=True))
    assert single.num_t == (None if name in ("Filter", "Label") else 1)             # the reference's Filter and Label count in run()
    single._get_t()
    assert single.num_t == 1
    late = cls(_im_info(tmp_path))
    late.num_t = None
    late._get_t()
    assert late.num_t == 3


def test_frame_count_spacing_and_reach(tmp_path, caplog):
    from nellie_amd.stage import frame_count, scaled_max_distance, spacing_of
    for no_z, spacing, frames in ((False, (.29, .107, .107), 3), (True, (.107, .107), 5)):
        im = _im_info(tmp_path, no_z=no_z)
        assert frame_count(im) == frames and frame_count(im, 2) == 2 and spacing_of(im) == spacing
        single = _im_info(tmp_path, no_t=True, no_z=no_z)
        assert frame_count(single) == 1 and frame_count(single, 4) == 4 and spacing_of(single) == spacing
    for dt, um, reach, warns in REACH:
        caplog.clear()
        with caplog.at_level(logging.WARNING):
            assert scaled_max_distance(_im_info(tmp_path, dt=dt), um) == reach
        assert ["Time resolution missing" in r.getMessage() for r in caplog.records] == [True] * warns
