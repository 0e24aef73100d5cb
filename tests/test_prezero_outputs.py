"""
GPU tests (-m gpu) of the pre-zeroed label volume (NELLIE_PREZERO, csrc/nl_host.h: NL_ENTER_KEEP_PZ).

The frame's last fused cascade step zeroes its dead third ping-pong volume in passing, every entry point up to nl_label_run keeps
that volume clean, and Label then stores only the voxels inside the runs.  Everything here is bit for bit: the dense kernels
(NELLIE_PREZERO=0) are the reference, computed once per (shape, seed) on a fresh context and never modified.

"prezero_used" is 2 on such a frame (bit 1: the labels).  Bit 0, a sparse write of the Frangi frame, is never set: the one volume a
cascade step can zero serves Label, where the dense paint costs more, and a fill of a second volume beside the last scale's walk or
inside its resolve kernel cost what it saved (profiles/prezero_1024cube.txt).

Shapes: (40, 70, 130) -- nx no multiple of 4 or 64, ny no multiple of the cascade step's 48- or 32-row tile, every tile an edge
tile; (33, 96, 128) -- interior tiles and the aligned 16-byte store paths.  NELLIE_GAUSS_FUSED=1 makes the fused step run on them.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [(40, 70, 130), (33, 96, 128)]
SEED_A, SEED_B = 31, 47

_REF = {}
_VOL = {}


def _volume(shape, seed):
    from nellie_amd.synthetic import make_volume
    if (shape, seed) not in _VOL:
        _VOL[(shape, seed)] = make_volume(shape, seed)
    return _VOL[(shape, seed)]


def _used(pipe):
    return int(pipe.ctx.info("prezero_used"))


def _frame(pipe, vol):
    """filter + label as bench.py's step runs them -> (frangi, labels, n_labels, prezero_used)"""
    from nellie_amd import pipeline as pl
    from nellie_amd.synthetic import ISO_01
    pipe.filter(vol, pl.FilterParams(dim_res=ISO_01))
    fr = pipe.download_frangi()
    n = pipe.label(pipe.frangi_threshold(), pl.min_area_pixels_of(ISO_01))
    return fr, pipe.download_labels(), int(n), _used(pipe)


def _reference(shape, seed, monkeypatch):
    """The dense writers on a fresh context: computed once, shared, read-only."""
    from nellie_amd import pipeline as pl
    if (shape, seed) not in _REF:
        monkeypatch.setenv("NELLIE_GAUSS_FUSED", "1")
        monkeypatch.setenv("NELLIE_PREZERO", "0")
        pipe = pl.FramePipeline(shape)
        try:
            fr, lab, n, used = _frame(pipe, _volume(shape, seed))
            assert pipe.chain_fallbacks == 0
        finally:
            pipe.close()
        assert used == 0, "NELLIE_PREZERO=0 must keep the dense writers"
        assert (fr > 0).any() and n > 0 and int(lab.max()) == n
        fr.setflags(write=False)
        lab.setflags(write=False)
        _REF[(shape, seed)] = (fr, lab, n)
        monkeypatch.delenv("NELLIE_PREZERO")
    return _REF[(shape, seed)]


def _same(got, ref, what):
    fr, lab, n = got[:3]
    assert n == ref[2], f"{what}: {n} labels, dense {ref[2]}"
    assert fr.dtype == np.float32 and np.array_equal(fr.view(np.uint32), ref[0].view(np.uint32)), f"{what}: the Frangi frame differs"
    assert lab.dtype == ref[1].dtype and np.array_equal(lab, ref[1]), f"{what}: the labels differ"


@pytest.mark.parametrize("ahead", [None, "0", "1"])
@pytest.mark.parametrize("shape", SHAPES)
def test_sparse_writers_equal_the_dense_ones(hip, shape, ahead, monkeypatch):
    """On versus off, with the last cascade step in order and running ahead on the side stream; None = the pipeline's own choice.
    Two frames: the second starts from what the first left in the volumes."""
    from nellie_amd import pipeline as pl
    ref = _reference(shape, SEED_A, monkeypatch)
    monkeypatch.setenv("NELLIE_GAUSS_FUSED", "1")
    monkeypatch.delenv("NELLIE_PREZERO", raising=False)
    pipe = pl.FramePipeline(shape)
    try:
        if ahead is not None:
            pipe._chain_ahead_env = ahead
        for k in range(2):
            got = _frame(pipe, _volume(shape, SEED_A))
            assert pipe.chain_fallbacks == 0
            assert got[3] == 2, f"frame {k}: prezero_used = {got[3]}"
            _same(got, ref, f"frame {k}")
        monkeypatch.setenv("NELLIE_PREZERO", "0")              # read per frame: the same context, the dense way
        got = _frame(pipe, _volume(shape, SEED_A))
        assert got[3] == 0
        _same(got, ref, "switched off")
    finally:
        pipe.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_nothing_of_the_previous_frame_survives(hip, shape, monkeypatch):
    """Seed A, seed B, seed A on one context: each equals the dense result of a fresh context.  A voxel, a label or a union-find
    word left in a "pre-zeroed" volume by the frame before would show."""
    from nellie_amd import pipeline as pl
    refs = {s: _reference(shape, s, monkeypatch) for s in (SEED_A, SEED_B)}
    assert not np.array_equal(refs[SEED_A][1] > 0, refs[SEED_B][1] > 0)
    monkeypatch.setenv("NELLIE_GAUSS_FUSED", "1")
    monkeypatch.delenv("NELLIE_PREZERO", raising=False)
    pipe = pl.FramePipeline(shape)
    try:
        for k, seed in enumerate((SEED_A, SEED_B, SEED_A)):
            got = _frame(pipe, _volume(shape, seed))
            assert got[3] == 2
            _same(got, refs[seed], f"frame {k} (seed {seed})")
    finally:
        pipe.close()


def test_a_second_label_on_the_same_frame_is_dense(hip, monkeypatch):
    from nellie_amd import pipeline as pl
    from nellie_amd.synthetic import ISO_01
    shape = SHAPES[0]
    ref = _reference(shape, SEED_A, monkeypatch)
    monkeypatch.setenv("NELLIE_GAUSS_FUSED", "1")
    monkeypatch.delenv("NELLIE_PREZERO", raising=False)
    pipe = pl.FramePipeline(shape)
    try:
        got = _frame(pipe, _volume(shape, SEED_A))
        assert got[3] == 2
        thr = pipe.frangi_threshold()
        n = pipe.label(thr, pl.min_area_pixels_of(ISO_01))
        assert _used(pipe) & 2 == 0, "the label volume was not zeroed again: the second paint must be dense"
        _same((pipe.download_frangi(), pipe.download_labels(), int(n)), ref, "second label()")
        n = pipe.label(thr, pl.min_area_pixels_of(ISO_01), fill_holes=False)         # ... and a third, another way
        assert _used(pipe) & 2 == 0 and int(pipe.download_labels().max()) == int(n)
    finally:
        pipe.close()


def test_an_uploaded_frangi_frame_is_labelled_densely(hip, monkeypatch):
    from nellie_amd import pipeline as pl
    from nellie_amd.synthetic import ISO_01
    shape = SHAPES[0]
    ref_a, ref_b = _reference(shape, SEED_A, monkeypatch), _reference(shape, SEED_B, monkeypatch)
    monkeypatch.setenv("NELLIE_GAUSS_FUSED", "1")
    monkeypatch.delenv("NELLIE_PREZERO", raising=False)
    pipe = pl.FramePipeline(shape)
    try:
        # the filtered frame leaves a flagged, pre-zeroed volume behind: the upload must drop it
        pipe.filter(_volume(shape, SEED_A), pl.FilterParams(dim_res=ISO_01))
        assert _used(pipe) == 0
        pipe.upload_frangi(ref_b[0].copy())
        n = pipe.label(pipe.frangi_threshold(), pl.min_area_pixels_of(ISO_01))
        assert _used(pipe) == 0
        _same((pipe.download_frangi(), pipe.download_labels(), int(n)), ref_b, "uploaded frame")
        # ... and after a complete sparse frame
        assert _frame(pipe, _volume(shape, SEED_A))[3] == 2
        pipe.upload_frangi(ref_b[0].copy())
        n = pipe.label(pipe.frangi_threshold(), pl.min_area_pixels_of(ISO_01))
        assert _used(pipe) == 0
        _same((pipe.download_frangi(), pipe.download_labels(), int(n)), ref_b, "uploaded frame after a sparse one")
        _same(_frame(pipe, _volume(shape, SEED_A)), ref_a, "the frame after")
    finally:
        pipe.close()


def test_the_synchronous_path_keeps_the_dense_writers(hip, monkeypatch):
    """The frame redone without the device chain (what a chain flag leads to) pre-zeroes nothing; the chain frames around it do."""
    from nellie_amd import pipeline as pl
    shape = SHAPES[1]
    ref = _reference(shape, SEED_A, monkeypatch)
    monkeypatch.setenv("NELLIE_GAUSS_FUSED", "1")
    monkeypatch.delenv("NELLIE_PREZERO", raising=False)
    pipe = pl.FramePipeline(shape)
    try:
        for k, chain in enumerate((True, False, True, False)):
            pipe._device_chain = chain
            got = _frame(pipe, _volume(shape, SEED_A))
            assert got[3] == (2 if chain else 0), f"frame {k}: prezero_used = {got[3]}"
            _same(got, ref, f"frame {k} (device chain {chain})")
    finally:
        pipe.close()
