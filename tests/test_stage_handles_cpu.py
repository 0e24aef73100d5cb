"""CPU tests of what the four stage handles share (csrc/nl_stage.h, hipnative._Handle): the create calls reject bad arguments
before they look at the device and fail loudly without one, and the binding's lifecycle works the same for every class."""
import ctypes as C
import os
import shutil
from types import SimpleNamespace

import numpy as np
import pytest

from nellie_amd import hipnative
from nellie_amd.hipnative import NL_ESTATE, NellieHipError


@pytest.fixture(scope="module")
def lib():
    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        if not os.path.exists(hipnative.LIB_PATH):
            pytest.skip("no hipcc and no prebuilt libnellie_hip.so")
    else:
        from nellie_amd import build
        build.build(verbose=False)
    return hipnative.load()


_SP = np.array([0.3, 0.1, 0.1])
_ZERO_SP = np.array([0.3, 0.0, 0.1])


def _create(lib, name, device=0, ndim=3, shape=(4, 8, 8), spacing=_SP, extra=0.5):
    """calls nl_<name>_create with these arguments; a handle that comes back is destroyed"""
    h = C.c_void_p()
    sp = None if spacing is None else hipnative._ptr(spacing)
    args = [C.byref(h), device, ndim]
    if name != "flow":
        args += list(shape)
    args.append(sp)
    if name != "track":
        args.append(float(extra))              # radius (flow, reassign) or time step (voxfeat)
    try:
        lib.call(f"nl_{name}_create", *args)
    finally:
        if h:
            getattr(lib.cdll, f"nl_{name}_destroy")(h)


NAMES = ("track", "flow", "reassign", "voxfeat")


@pytest.mark.parametrize("name", NAMES)
def test_create_rejects_bad_arguments_before_the_device(lib, name):
    # device 10**6 exists nowhere: an argument error reported for these calls was found before the device was looked at
    for bad in (dict(ndim=4), dict(spacing=None), dict(spacing=_ZERO_SP)):
        with pytest.raises(ValueError):
            _create(lib, name, device=10**6, **bad)
    if name != "flow":
        with pytest.raises(ValueError):
            _create(lib, name, device=10**6, shape=(4, 0, 8))
    if name != "track":
        with pytest.raises(ValueError):
            _create(lib, name, device=10**6, extra=0.0)


@pytest.mark.parametrize("name", NAMES)
def test_create_without_gpu_raises(lib, name):
    if lib.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError, match="GPU backend requested"):
        _create(lib, name)


@pytest.mark.parametrize("name", NAMES)
def test_create_on_missing_device_raises(lib, name):
    if lib.device_count() == 0:
        pytest.skip("no GPU")
    with pytest.raises(RuntimeError, match="GPU backend requested"):
        _create(lib, name, device=10**6)


# ---- the Python base, on a fake library ------------------------------------------------------------------------------------------
class FakeLib:
    """stands in for hipnative._Lib: hands out handle 1 and records the calls"""

    def __init__(self):
        self.calls, self.destroyed = [], []
        self.cdll = SimpleNamespace(**{s: (lambda h, s=s: self.destroyed.append(s)) for s in hipnative._PLAIN if s.endswith("_destroy")})

    def call(self, name, *args):
        self.calls.append(name)
        if name.endswith("_create"):
            args[0]._obj.value = 1


CASES = {
    "context": (lambda: hipnative.Context((4, 8, 8)), "nl_ctx_destroy", lambda o: o.sync()),
    "tracker": (lambda: hipnative.Tracker((4, 8, 8), _SP), "nl_track_destroy", lambda o: o.features()),
    "flow field": (lambda: hipnative.FlowField(3, _SP, 0.5), "nl_flow_destroy", lambda o: o.kernel_ms()),
    "reassigner": (lambda: hipnative.Reassigner((4, 8, 8), _SP, 0.5), "nl_reassign_destroy", lambda o: o.kernel_ms()),
    "voxel-feature object": (lambda: hipnative.VoxelFeatures((4, 8, 8), _SP, 1.0), "nl_voxfeat_destroy", lambda o: o.kernel_ms()),
}


@pytest.fixture
def fake(monkeypatch):
    f = FakeLib()
    monkeypatch.setattr(hipnative, "load", lambda: f)
    return f


@pytest.mark.parametrize("noun", list(CASES))
def test_handle_lifecycle(fake, noun):
    make, destroy, use = CASES[noun]
    obj = make()
    use(obj)
    obj.close()
    obj.close()                                            # harmless
    assert fake.destroyed == [destroy]
    n_calls = len(fake.calls)
    with pytest.raises(NellieHipError, match=f"{noun} is closed") as e:
        use(obj)
    assert e.value.code == NL_ESTATE and len(fake.calls) == n_calls
    with make() as obj:
        assert obj._h
    assert not obj._h and fake.destroyed == [destroy, destroy]


@pytest.mark.parametrize("noun", ["tracker", "reassigner", "voxel-feature object"])
def test_wrong_frame_shape_is_rejected_before_the_library(fake, noun):
    obj = CASES[noun][0]()
    n_calls = len(fake.calls)
    good, bad = np.zeros((4, 8, 8), np.int32), np.zeros((4, 8, 9), np.int32)
    frames = {"tracker": (good, good, good, bad), "reassigner": (good, bad), "voxel-feature object": (good, good, bad, good)}[noun]
    with pytest.raises(ValueError, match="does not match"):
        obj.frame(*frames)
    assert len(fake.calls) == n_calls
    obj.close()
