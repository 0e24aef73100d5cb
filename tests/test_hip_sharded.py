"""
GPU test of the Z-slab Filter on the real HIP engine: `world` contexts on ONE device, one Python thread per
rank, ghost planes exchanged through nl_planes_get / nl_planes_put ("fake multi-GPU").
Filter AND Label: the concatenated slabs must equal the single-context result BIT FOR BIT (every cross-slab quantity is an
integer sum, a min or a max, or is recomputed from identical inputs).  The RCCL path differs only in how the
same planes and scalars travel.
"""
import threading

import numpy as np
import pytest

from comms import ThreadComm, ThreadGroup

pytestmark = pytest.mark.gpu



def _need_torch():
    """Skips without torch -- WITHOUT importing it here: the workers run in their own processes, and a torch imported into the pytest
    process brings its bundled librccl / HIP runtime along, which the library's own dlopen("librccl.so.1") then gets handed
    (ncclCommInitRank: "unhandled cuda error", 150 tests later -- round 5)."""
    import importlib.util
    if importlib.util.find_spec("torch") is None:
        pytest.skip("torch (torch.distributed.run + gloo for the worker processes) is not installed")


def _comm_factory(transport, world, group):
    """rank -> comm_factory(ctx).  "host": planes and scalars travel through numpy arrays (nl_planes_get / _put); "loopback":
    the production RcclComm over the library's loopback transport -- the nccl* call sites, their plane offsets and counts,
    both communicators, the side stream and its events run exactly as over RCCL (include/nellie_amd.h: nl_comm_loopback_id)."""
    if transport == "host":
        return lambda rank: (lambda ctx: ThreadComm(group, rank))
    from nellie_amd import hipnative
    from nellie_amd.sharded import RcclComm
    uid, uid2 = hipnative.comm_unique_id(loopback=True), hipnative.comm_unique_id(loopback=True)
    assert uid[:8] == b"NLLOOPBK" and uid != uid2
    return lambda rank: (lambda ctx: RcclComm(ctx, world, rank, uid, uid2=uid2))


def _run_sharded(gshape, dr, seed, world, halo_mode="steps", raw_ghosts=False, transport="host"):
    from nellie_amd.pipeline import FilterParams, min_area_pixels_of
    from nellie_amd.sharded import ShardedFramePipeline, slab_range
    from nellie_amd.synthetic import make_volume
    group = ThreadGroup(world)
    factory = _comm_factory(transport, world, group)
    out, errs = [None] * world, []

    def worker(rank):
        try:
            p = FilterParams(dim_res=dr)
            o0, o1 = slab_range(gshape[0], world, rank)
            pipe = ShardedFramePipeline(gshape, rank, world, factory(rank), p, halo_mode=halo_mode)
            g_lo, g_hi = pipe.raw_ghost_needed() if raw_ghosts else (0, 0)      # raw ghost planes handed over with the frame
            own = make_volume((o1 - o0 + g_lo + g_hi,) + tuple(gshape[1:]), seed, z_offset=o0 - g_lo, global_nz=gshape[0])
            pipe.filter(own, p)
            thr = pipe.frangi_threshold()
            n = pipe.label(thr, min_area_pixels_of(dr))
            out[rank] = (pipe.download_frangi(), thr, [s.mask_count for s in pipe.trace.scales],
                         pipe.download_labels(), n)
            pipe.close()
        except Exception as exc:  # noqa: BLE001
            errs.append(exc)
            group.barrier.abort()

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errs:
        raise errs[0]
    return out


@pytest.mark.parametrize("halo_mode", ["steps", "fat", "steps+raw", "fat+raw"])
@pytest.mark.parametrize("gshape,aniso,world", [((96, 64, 80), False, 2), ((100, 48, 70), False, 3),
                                               ((60, 64, 64), True, 4), ((90, 40, 70), False, 6)])
def test_zslab_filter_equals_single_gpu(hip, gshape, aniso, world, halo_mode):
    raw_ghosts = halo_mode.endswith("+raw")       # the raw ghost planes come with the frame: no exchange of raw planes
    halo_mode = halo_mode.split("+")[0]
    from nellie_amd import pipeline as pl
    from nellie_amd.synthetic import ANISO_03, ISO_01, make_volume
    dr = ANISO_03 if aniso else ISO_01
    vol = make_volume(gshape, 91)
    single = pl.FramePipeline(gshape)
    p = pl.FilterParams(dim_res=dr)
    single.filter(vol, p)
    ref = single.download_frangi()
    ref_thr = single.frangi_threshold()
    ref_counts = [s.mask_count for s in single.trace.scales]
    ref_n = single.label(ref_thr, pl.min_area_pixels_of(dr))
    ref_lab = single.download_labels()
    single.close()
    if halo_mode == "fat" and world == 6:
        pytest.skip("15-plane slabs are thinner than the 24-plane fat halo")
    parts = _run_sharded(gshape, dr, 91, world, halo_mode, raw_ghosts)
    got = np.concatenate([p_[0] for p_ in parts])
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} voxels differ"
    for _, thr, counts, _, n in parts:
        assert thr == ref_thr and counts == ref_counts and n == ref_n
    assert (ref > 0).any()
    lab = np.concatenate([p_[3] for p_ in parts])
    assert np.array_equal(lab, ref_lab), f"{int((lab != ref_lab).sum())} label voxels differ"
    assert ref_n >= 1


@pytest.mark.parametrize("gshape,aniso,world,halo_mode", [((96, 64, 80), False, 2, "steps"), ((100, 48, 70), False, 3, "steps+raw"),
                                                         ((60, 64, 64), True, 4, "fat"), ((75, 50, 133), True, 3, "steps")])
def test_zslab_filter_with_the_fused_cascade_kernel(hip, gshape, aniso, world, halo_mode, monkeypatch):
    """The fused Z+Y+X cascade kernel (gauss_zyx.inc; by default only on volumes of 2^26 voxels and more) on Z slabs: ghost planes, plane
    ranges that start inside the slab, reflection at true faces only (gz0 / gnz), partial tiles, rows of a length that is no
    multiple of four -- slabs with the fused kernel forced == one context with the two-kernel form, bit for bit."""
    raw_ghosts = halo_mode.endswith("+raw")
    halo_mode = halo_mode.split("+")[0]
    from nellie_amd import pipeline as pl
    from nellie_amd.synthetic import ANISO_03, ISO_01, make_volume
    dr = ANISO_03 if aniso else ISO_01
    vol = make_volume(gshape, 93)
    monkeypatch.setenv("NELLIE_GAUSS_FUSED", "0")
    single = pl.FramePipeline(gshape)
    p = pl.FilterParams(dim_res=dr)
    single.filter(vol, p)
    ref = single.download_frangi()
    ref_thr = single.frangi_threshold()
    single.close()
    monkeypatch.setenv("NELLIE_GAUSS_FUSED", "1")
    parts = _run_sharded(gshape, dr, 93, world, halo_mode, raw_ghosts)
    got = np.concatenate([p_[0] for p_ in parts])
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} voxels differ"
    assert all(p_[1] == ref_thr for p_ in parts) and (ref > 0).any()


def test_stage_api_two_processes_share_one_gpu(hip, tmp_path):
    """The multi-process path with the REAL library on a one-GPU box: two processes (torch.distributed.run, gloo), each with its own HIP
    context on device 0, run `Filter(im_info, shard=...).run()` and `Label(im_info, shard=...).run()` on their Z slabs of both
    frames -- rank 0 creates the files, both write their planes (nellie_amd/engine.py: RankSlab; the exchanges are host-staged over
    gloo, tests/comms.py: RCCL refuses two ranks on one device).  The files equal what ONE context writes, byte for byte; the second
    Label run masks with the original image (labelling.py:513-520)."""
    import os
    import subprocess
    import sys
    _need_torch()
    from fakes import ArrayImInfo
    from nellie_amd.im_info import ome_tiff
    from nellie_amd.im_info.verifier import ImInfo
    from nellie_amd.segmentation.filtering import Filter
    from nellie_amd.segmentation.labelling import Label
    from nellie_amd.synthetic import ISO_01, make_volume
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    vols = np.stack([make_volume((72, 50, 66), 170 + t) for t in range(2)])
    src = str(tmp_path / "stack.ome.tif")
    ome_tiff.create(src, vols.shape, np.float32, ISO_01, "raw", data=vols)
    out_dir = str(tmp_path / "out")
    im_info = ImInfo(src, output_dir=out_dir)
    port = 29700 + (os.getpid() % 90)
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(repo, "tests", "dist_stage_worker.py"), src, out_dir, "101.5", "--hip"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    fr = np.asarray(im_info.get_memmap(im_info.pipeline_paths["im_preprocessed"], read_mode="r"))
    lab = np.load(os.path.join(out_dir, "labels_plain.npy"))
    lab_thr = np.asarray(im_info.get_memmap(im_info.pipeline_paths["im_instance_label"], read_mode="r"))
    one = ArrayImInfo(vols, ISO_01)
    Filter(one).run()
    Label(one).run()
    assert np.array_equal(fr, np.asarray(one.store["frangi"])), f"{int((fr != np.asarray(one.store['frangi'])).sum())} voxels differ"
    assert np.array_equal(lab, np.asarray(one.store["labels"])) and lab.max() >= 1
    Label(one, threshold=101.5).run()
    assert np.array_equal(lab_thr, np.asarray(one.store["labels"])) and not np.array_equal(lab_thr, lab)
    assert np.array_equal(np.asarray(im_info.get_memmap(im_info.im_path, read_mode="r")), vols), "input file was modified"


def _single_reference(gshape, dr, seed):
    from nellie_amd import pipeline as pl
    from nellie_amd.synthetic import make_volume
    single = pl.FramePipeline(gshape)
    p = pl.FilterParams(dim_res=dr)
    single.filter(make_volume(gshape, seed), p)
    ref = single.download_frangi()
    thr = single.frangi_threshold()
    counts = [s.mask_count for s in single.trace.scales]
    n = single.label(thr, pl.min_area_pixels_of(dr))
    lab = single.download_labels()
    single.close()
    return ref, thr, counts, n, lab


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("halo_mode", ["steps", "fat", "steps+raw"])
@pytest.mark.parametrize("gshape,aniso,world", [((96, 64, 80), False, 2), ((100, 48, 70), False, 3),
                                               ((60, 64, 64), True, 4), ((90, 40, 70), False, 6)])
def test_zslab_over_the_loopback_transport(hip, gshape, aniso, world, halo_mode, fused, monkeypatch):
    """The N >= 2 exchange code itself -- ncclSend / ncclRecv of float and bit planes (halo_exchange_impl,
    nl_slab_bits_exchange), the fused all-reduces between the sampling kernels, nl_allgather_var with several blocks, the
    second communicator with its stream and events, the cascade step running ahead (NELLIE_GAUSS_AHEAD, default on slabs)
    -- on world contexts of one GPU: Filter and Label equal the single-context result bit for bit."""
    from nellie_amd.synthetic import ANISO_03, ISO_01
    monkeypatch.setenv("NELLIE_FUSE_REDUCE", "1" if fused else "0")
    monkeypatch.setenv("NELLIE_DEVICE_CHAIN_SLABS", "1")      # fused: the scale loop's thresholds decided on the device, on slabs too
    raw_ghosts = halo_mode.endswith("+raw")
    halo_mode = halo_mode.split("+")[0]
    if halo_mode == "fat" and world == 6:
        pytest.skip("15-plane slabs are thinner than the 24-plane fat halo")
    dr = ANISO_03 if aniso else ISO_01
    ref, ref_thr, ref_counts, ref_n, ref_lab = _single_reference(gshape, dr, 91)
    parts = _run_sharded(gshape, dr, 91, world, halo_mode, raw_ghosts, transport="loopback")
    got = np.concatenate([p_[0] for p_ in parts])
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} voxels differ"
    for _, thr, counts, _, n in parts:
        assert thr == ref_thr and counts == ref_counts and n == ref_n
    lab = np.concatenate([p_[3] for p_ in parts])
    assert (ref > 0).any() and ref_n >= 1
    assert np.array_equal(lab, ref_lab), f"{int((lab != ref_lab).sum())} label voxels differ"


@pytest.mark.parametrize("delay_us,seed", [(200, 7), (1500, 8)])
@pytest.mark.parametrize("world", [2, 4])
def test_zslab_loopback_with_randomised_transfer_delays(hip, world, delay_us, seed, monkeypatch):
    """Every transfer of the loopback transport is held back by a random spin on its stream (NELLIE_LOOPBACK_DELAY_US): the
    asynchronous ghost-plane exchange then finishes long after the host has moved on, and any consumer that is not ordered
    behind it by an event reads stale planes.  Results must not move."""
    from nellie_amd.synthetic import ISO_01
    monkeypatch.setenv("NELLIE_LOOPBACK_DELAY_US", str(delay_us))
    monkeypatch.setenv("NELLIE_GAUSS_AHEAD", "1")
    monkeypatch.setenv("NELLIE_DEVICE_CHAIN_SLABS", "1" if seed == 8 else "0")    # once with the device chain, once with the cascade step running ahead
    gshape = (32 * world, 56, 72)
    ref, ref_thr, ref_counts, ref_n, ref_lab = _single_reference(gshape, ISO_01, seed)
    for _ in range(2):
        parts = _run_sharded(gshape, ISO_01, seed, world, "steps", False, transport="loopback")
        assert np.array_equal(np.concatenate([p_[0] for p_ in parts]), ref)
        assert np.array_equal(np.concatenate([p_[3] for p_ in parts]), ref_lab)
        assert all(p_[1] == ref_thr and p_[2] == ref_counts and p_[4] == ref_n for p_ in parts)


GROW_SIZES = (16, 70000, 16)


def _payload(rank, size):
    return ((np.arange(size) * (rank + 3) + rank) % 251).astype(np.uint8)


def test_loopback_collectives_known_answers(hip):
    """The transport itself against numpy: all-reduce (sum / min / max, int64 and float32), variable all-gather with empty
    and unequal blocks, on 3 ranks."""
    from nellie_amd import hipnative
    world = 3
    uid = hipnative.comm_unique_id(loopback=True)
    out, errs = [None] * world, []

    def worker(rank):
        try:
            ctx = hipnative.Context((8, 16, 16), gz0=0, gnz=8, own=(0, 8))
            ctx.comm_init(world, rank, uid)
            res = {}
            res["sum"] = ctx.allreduce(np.array([rank + 1, 10 * rank], np.int64), "sum")
            res["min"] = ctx.allreduce(np.array([rank + 1, -rank], np.int64), "min")
            res["maxf"] = ctx.allreduce(np.array([0.5 * rank, -1.0 - rank], np.float32), "max")
            res["gather"] = ctx.allgather_var(np.arange(rank * 1000, dtype=np.int32) + rank, world)
            res["gather_bytes"] = ctx.allgather_var(np.frombuffer(bytes([rank] * (rank + 1)), np.uint8).copy(), world)
            # the staging buffers of both all-gathers grow, then serve a smaller payload again
            res["grow"] = [(ctx.allgather_bytes(_payload(rank, size).tobytes(), size, world), ctx.allgather_var(_payload(rank, size), world))
                           for size in GROW_SIZES]
            out[rank] = res
            ctx.close()
        except Exception as exc:  # noqa: BLE001
            errs.append(exc)

    ts = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    if errs:
        raise errs[0]
    for rank in range(world):
        r = out[rank]
        assert np.array_equal(r["sum"], [6, 30]) and np.array_equal(r["min"], [1, -2])
        assert np.array_equal(r["maxf"], np.array([1.0, -1.0], np.float32))
        for q in range(world):
            assert np.array_equal(r["gather"][q], np.arange(q * 1000, dtype=np.int32) + q)
            assert bytes(r["gather_bytes"][q]) == bytes([q] * (q + 1))
            for size, (fixed, var) in zip(GROW_SIZES, r["grow"]):
                assert fixed[q] == _payload(q, size).tobytes() and np.array_equal(var[q], _payload(q, size))


@pytest.mark.parametrize("fused", [True, False])
def test_rccl_communicator_world1(hip, fused, monkeypatch):
    """RCCL plumbing on a single device: unique ids, both communicators, all-reduce, variable all-gather, and a 1-rank sharded
    run of Filter + Label -- with the reductions fused into the sampling / statistics entry points (nl_comm_fuse: the production
    setting) and as host-level all-reduces; outputs, thresholds and h_mask counts equal the single-GPU run's."""
    from nellie_amd import hipnative
    from nellie_amd import pipeline as pl
    from nellie_amd.sharded import RcclComm, ShardedFramePipeline
    from nellie_amd.synthetic import ISO_01, make_volume
    monkeypatch.setenv("NELLIE_FUSE_REDUCE", "1" if fused else "0")
    gshape = (40, 48, 56)
    vol = make_volume(gshape, 5)
    p = pl.FilterParams(dim_res=ISO_01)
    ma = pl.min_area_pixels_of(ISO_01)
    uid, uid2 = hipnative.comm_unique_id(), hipnative.comm_unique_id()
    assert len(uid) == 128 and uid != uid2
    pipe = ShardedFramePipeline(gshape, 0, 1, lambda ctx: RcclComm(ctx, 1, 0, uid, uid2=uid2), p)
    assert pipe.comm.fused == fused and pipe._chain_hist == fused
    assert np.array_equal(pipe.comm.allreduce(np.array([3, 4], np.int64), "sum"), [3, 4])
    assert np.array_equal(pipe.comm.allreduce(np.array([1.5], np.float32), "max"), np.array([1.5], np.float32))
    for arr in (np.arange(7, dtype=np.int32), np.zeros(0, np.int32), np.arange(5000, dtype=np.int64)):
        got = pipe.comm.allgather_list(arr)
        assert len(got) == 1 and got[0].dtype == arr.dtype and np.array_equal(got[0], arr)
    pipe.filter(vol, p)
    got = pipe.download_frangi()
    thr = pipe.frangi_threshold()
    n = pipe.label(thr, ma)
    lab = pipe.download_labels()
    tr = pipe.trace
    pipe.close()
    single = pl.FramePipeline(gshape)
    single.filter(vol, p)
    assert np.array_equal(got, single.download_frangi())
    assert thr == single.frangi_threshold()
    assert n == single.label(thr, ma) and np.array_equal(lab, single.download_labels())
    for a, b in zip(tr.scales, single.trace.scales):
        assert (a.gamma, a.max_abs, a.frob_thr, a.mask_count, a.one_pass) == (b.gamma, b.max_abs, b.frob_thr, b.mask_count, b.one_pass)
    assert tr.n_positive == single.trace.n_positive
    single.close()


@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_zslab_label_golden_on_hip_slabs(hip, world):
    """Label without replication on HIP contexts (nl_slab_*): the reference's labels of the label-only golden volumes
    (cavities, face contacts, 65/66/67-voxel objects), numbering included; the replicated variant agrees."""
    from conftest import load_golden
    from nellie_amd.pipeline import FilterParams
    from nellie_amd.sharded import ShardedFramePipeline, slab_range
    for name in ("labelonly_24x48x48", "labelonly_aniso_24x48x48"):
        g = load_golden(name)
        fr, thr, ma = g["frangi"], float(g["label_thr"]), int(g["min_area_pixels"])
        for replicated in (False, True):
            group = ThreadGroup(world)
            out, errs = [None] * world, []

            def worker(rank):
                try:
                    o0, o1 = slab_range(fr.shape[0], world, rank)
                    pipe = ShardedFramePipeline(fr.shape, rank, world, lambda ctx: ThreadComm(group, rank), FilterParams(dim_res=g["dim_res_dict"]), halo=1)
                    pipe.upload_frangi(fr[o0:o1])
                    n = (pipe.label_replicated if replicated else pipe.label)(thr, ma)
                    out[rank] = (pipe.download_labels(), n)
                    pipe.close()
                except Exception as exc:  # noqa: BLE001
                    errs.append(exc)
                    group.barrier.abort()

            ts = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
            for t in ts:
                t.start()
            for t in ts:
                t.join()
            if errs:
                raise errs[0]
            lab = np.concatenate([o[0] for o in out])
            assert np.array_equal(lab, g["labels"]), f"{name} world {world} replicated={replicated}: {int((lab != g['labels']).sum())} voxels differ"
            assert [o[1] for o in out] == [int(g["labels"].max())] * world


def _label_as_slabs_vs_one_context(shape, world, seed, n_shells=40):
    from nellie_amd import pipeline as pl
    from nellie_amd.pipeline import FilterParams
    from nellie_amd.sharded import ShardedFramePipeline, slab_range
    dr = {"X": 0.1, "Y": 0.1, "Z": 0.1, "T": 1.0}
    rng = np.random.default_rng(seed)
    zz, yy, xx = np.meshgrid(*[np.arange(s, dtype=np.float32) for s in shape], indexing="ij")
    fr = np.zeros(shape, np.float32)
    for _ in range(n_shells):
        c = [rng.uniform(0, s) for s in shape]
        r = rng.uniform(2.0, 9.0)
        d = np.sqrt((zz - c[0]) ** 2 + (yy - c[1]) ** 2 + (xx - c[2]) ** 2)
        fr[(d < r) & (d > r - rng.uniform(1.2, 3.0))] = 1.0
    for _ in range(30):
        y0, x0 = rng.integers(0, shape[1]), rng.integers(0, shape[2])
        z0, z1 = sorted(rng.integers(0, shape[0], 2))
        fr[z0:z1 + 1, y0:y0 + 2, x0:x0 + 2] = 1.0
    fr[rng.random(shape) < 0.02] = 1.0
    single = pl.FramePipeline(shape)
    single.upload_frangi(fr)
    ref_n = single.label(0.5, 12)
    ref = single.download_labels()
    single.close()
    group = ThreadGroup(world)
    out, errs = [None] * world, []

    def worker(rank):
        try:
            o0, o1 = slab_range(shape[0], world, rank)
            pipe = ShardedFramePipeline(shape, rank, world, lambda ctx: ThreadComm(group, rank), FilterParams(dim_res=dr), halo=2)
            pipe.upload_frangi(fr[o0:o1])
            n = pipe.label(0.5, 12)
            out[rank] = (pipe.download_labels(), n)
            pipe.close()
        except Exception as exc:  # noqa: BLE001
            errs.append(exc)
            group.barrier.abort()

    ts = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    if errs:
        raise errs[0]
    lab = np.concatenate([o[0] for o in out])
    assert np.array_equal(lab, ref), f"world {world}: {int((lab != ref).sum())} voxels differ"
    assert [o[1] for o in out] == [ref_n] * world and ref_n > 5


def test_zslab_label_random_on_hip_slabs(hip):
    """Shells, tubes and specks across up to 6 interfaces: slabs == one context, bit for bit."""
    for world, seed in ((2, 0), (5, 1), (7, 2)):
        _label_as_slabs_vs_one_context((9 * world + 2, 70, 130), world, seed)


@pytest.mark.parametrize("shape,world", [((291, 256, 72), 2), ((293, 256, 40), 3), ((131, 520, 64), 2)])
def test_zslab_label_uneven_slabs_cut_shared_planes_alike(hip, shape, world):
    """the tables the ranks exchange hold one entry per SEGMENT component of a shared plane, so both ranks have to
    cut the plane into the same row bands.  Round 4 derived the bands from the rank's own plane count: 291 planes on 2 ranks are 147 +
    146 (+ ghosts), which gave bands of 64 rows on one side and 32 on the other -- "slab tables disagree".  The bands of a slab are a
    function of ny alone now."""
    _label_as_slabs_vs_one_context(shape, world, seed=3, n_shells=60)


def test_zslab_remove_edges_equals_single_gpu(hip):
    """Filter(remove_edges=True) on slabs: the ghost planes lose their edge rows too (they feed the opening of the
    boundary planes), so the sharded frame equals the single-context frame bit for bit."""
    from nellie_amd import pipeline as pl
    from nellie_amd.pipeline import FilterParams
    from nellie_amd.sharded import ShardedFramePipeline, slab_range
    from nellie_amd.synthetic import ISO_01, make_volume
    gshape, world = (96, 64, 80), 2
    vol = make_volume(gshape, 17)
    p = FilterParams(dim_res=ISO_01)
    single = pl.FramePipeline(gshape)
    single.filter(vol, p, remove_edges=True)
    ref = single.download_frangi()
    single.close()
    group = ThreadGroup(world)
    out, errs = [None] * world, []

    def worker(rank):
        try:
            o0, o1 = slab_range(gshape[0], world, rank)
            pipe = ShardedFramePipeline(gshape, rank, world, lambda ctx: ThreadComm(group, rank), p)
            pipe.filter(vol[o0:o1], p, remove_edges=True)
            out[rank] = pipe.download_frangi()
            pipe.close()
        except Exception as exc:  # noqa: BLE001
            errs.append(exc)
            group.barrier.abort()

    ts = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    if errs:
        raise errs[0]
    got = np.concatenate(out)
    assert (ref > 0).any() and np.array_equal(got, ref), f"{int((got != ref).sum())} voxels differ"


@pytest.mark.parametrize("how", ["force3", "devices00"])
def test_stage_api_runs_a_frame_as_local_slabs(hip, how, tmp_path, monkeypatch):
    """Filter(...).run() / Label(...).run() / run(file_info) with the frame cut into Z slabs inside the process
    (nellie_amd/engine.py: LocalSlabs over the loopback transport) -- forced on a small frame the way a frame beyond 2^31
    voxels gets it, and through devices=[...] -- write the files the single-context run writes (2 frames, uint16 input)."""
    import os
    from nellie_amd.im_info import ome_tiff
    from nellie_amd.im_info.verifier import FileInfo, ImInfo
    from nellie_amd.run import run
    from nellie_amd.synthetic import ISO_01, make_volume
    vols = np.stack([make_volume((72, 48, 60), 30 + t, dtype=np.uint16) for t in range(2)])
    src = str(tmp_path / "stack.ome.tif")
    ome_tiff.create(src, vols.shape, np.uint16, ISO_01, "raw", data=vols)
    single = run(FileInfo(src, output_dir=str(tmp_path / "single")), device="gpu")
    kw = {}
    if how == "force3":
        monkeypatch.setenv("NELLIE_FORCE_SLABS", "3")
    else:
        kw["devices"] = [0, 0]
    sharded = run(FileInfo(src, output_dir=str(tmp_path / how)), device="gpu", **kw)
    for key in ("im_preprocessed", "im_instance_label"):
        a = np.asarray(single.get_memmap(single.pipeline_paths[key], read_mode="r"))
        b = np.asarray(sharded.get_memmap(sharded.pipeline_paths[key], read_mode="r"))
        assert a.dtype == b.dtype and np.array_equal(a, b), f"{key}: {int((a != b).sum())} voxels differ"
    lab = np.asarray(sharded.get_memmap(sharded.pipeline_paths["im_instance_label"], read_mode="r"))
    assert lab.max() >= 1 and np.array_equal(np.asarray(sharded.get_memmap(sharded.im_path, read_mode="r")), vols)


def test_stage_api_remove_edges_on_local_slabs(hip, monkeypatch):
    """Filter(remove_edges=True) through the slab engine == the single-context stage (in-memory ImInfo)."""
    from fakes import ArrayImInfo
    from nellie_amd.segmentation.filtering import Filter
    from nellie_amd.synthetic import ISO_01, make_volume
    vols = make_volume((80, 64, 72), 19)[None]
    a, b = ArrayImInfo(vols, ISO_01), ArrayImInfo(vols, ISO_01)
    Filter(a, remove_edges=True, device="gpu").run()
    monkeypatch.setenv("NELLIE_FORCE_SLABS", "2")
    Filter(b, remove_edges=True, device="gpu").run()
    assert (a.store["frangi"] > 0).any() and np.array_equal(a.store["frangi"], b.store["frangi"])


@pytest.mark.parametrize("kw", [dict(threshold=101.5), dict(otsu_thresh_intensity=True)])
def test_stage_api_label_intensity_thresholds_on_local_slabs(hip, monkeypatch, kw):
    """Label(threshold=...) / Label(otsu_thresh_intensity=True) through the slab engine (every slab masks the planes it owns with
    the original image, labelling.py:513-520, 550-552) == the single-context stage; uint16 input."""
    from fakes import ArrayImInfo
    from nellie_amd.segmentation.filtering import Filter
    from nellie_amd.segmentation.labelling import Label
    from nellie_amd.synthetic import ISO_01, make_volume
    vols = make_volume((80, 64, 72), 23, dtype=np.uint16)[None]
    a, b, plain = ArrayImInfo(vols, ISO_01), ArrayImInfo(vols, ISO_01), ArrayImInfo(vols, ISO_01)
    Filter(a, device="gpu").run(); Label(a, device="gpu", **kw).run()
    Filter(plain, device="gpu").run(); Label(plain, device="gpu").run()
    monkeypatch.setenv("NELLIE_FORCE_SLABS", "3")
    Filter(b, device="gpu").run(); Label(b, device="gpu", **kw).run()
    assert np.array_equal(a.store["frangi"], b.store["frangi"])
    assert a.store["labels"].max() >= 1 and np.array_equal(a.store["labels"], b.store["labels"])
    assert not np.array_equal(a.store["labels"], plain.store["labels"])          # the threshold did something


def test_stage_api_rank_slabs_over_loopback_threads(hip, tmp_path):
    """The multi-process layout of the stage API (engine.RankSlab: one rank per process, rank 0 creates the files, every rank
    writes its own planes) with the real HIP engine -- the ranks are three threads here, their communicators the library's
    loopback transport: Filter(...).run() and Label(...).run() per rank == the single-context files."""
    from nellie_amd import hipnative
    from nellie_amd.engine import ShardSpec
    from nellie_amd.im_info import ome_tiff
    from nellie_amd.im_info.verifier import FileInfo, ImInfo
    from nellie_amd.run import run
    from nellie_amd.segmentation.filtering import Filter
    from nellie_amd.segmentation.labelling import Label
    from nellie_amd.sharded import RcclComm
    from nellie_amd.synthetic import ISO_01, make_volume
    world = 3
    vols = np.stack([make_volume((78, 40, 56), 60 + t) for t in range(2)])
    src = str(tmp_path / "stack.ome.tif")
    ome_tiff.create(src, vols.shape, np.float32, ISO_01, "raw", data=vols)
    single = run(FileInfo(src, output_dir=str(tmp_path / "single")), device="gpu")
    out_dir = str(tmp_path / "ranks")
    ImInfo(src, output_dir=out_dir)                                  # the canonical copy the ranks reuse
    ids = {stage: (hipnative.comm_unique_id(loopback=True), hipnative.comm_unique_id(loopback=True)) for stage in ("filter", "label")}
    gate = threading.Barrier(world)
    infos, errs = [None] * world, []

    def worker(rank):
        try:
            im = ImInfo(src, output_dir=out_dir)
            infos[rank] = im
            for stage, cls in (("filter", Filter), ("label", Label)):
                u1, u2 = ids[stage]
                spec = ShardSpec(rank=rank, world=world, device=0, comm_factory=lambda ctx, a=u1, b=u2: RcclComm(ctx, world, rank, a, uid2=b))
                cls(im, device="gpu", shard=spec).run()
                gate.wait()
        except BaseException as exc:  # noqa: BLE001
            errs.append(exc)
            gate.abort()

    ts = [threading.Thread(target=worker, args=(r,)) for r in range(world)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    if errs:
        raise errs[0]
    for key in ("im_preprocessed", "im_instance_label"):
        a = np.asarray(single.get_memmap(single.pipeline_paths[key], read_mode="r"))
        b = np.asarray(infos[0].get_memmap(infos[0].pipeline_paths[key], read_mode="r"))
        assert a.dtype == b.dtype and np.array_equal(a, b), f"{key}: {int((a != b).sum())} voxels differ"
    assert np.asarray(infos[0].get_memmap(infos[0].pipeline_paths["im_instance_label"], read_mode="r")).max() >= 1


@pytest.mark.parametrize("transport", ["host", "loopback"])
def test_slab_tables_beyond_one_block_are_fetched_again(hip, transport, monkeypatch):
    """nl_slab_phase ships a rank's tables in fixed blocks (64 KiB by default; all-gathered without a size negotiation over RCCL).
    Tables that do not fit report their size, and the caller fetches them again in larger blocks without recomputing anything:
    forced here with 24-int blocks (header 8 + room for 8 entries), through the host gather and through the gathered device path."""
    from nellie_amd import hipnative
    from nellie_amd.synthetic import ISO_01
    monkeypatch.setattr(hipnative.Context, "SLAB_BLOCK_INTS", 24)
    calls = []
    orig = hipnative.Context._call

    def spy(self, name, *a):
        if name == "nl_slab_phase":
            calls.append(int(a[0]))
        return orig(self, name, *a)
    monkeypatch.setattr(hipnative.Context, "_call", spy)
    gshape, world = (96, 64, 80), 3
    ref, ref_thr, ref_counts, ref_n, ref_lab = _single_reference(gshape, ISO_01, 91)
    parts = _run_sharded(gshape, ISO_01, 91, world, "steps", False, transport=transport)
    assert -1 in calls, "no phase needed a second fetch: the test volume has too few boundary components"
    lab = np.concatenate([p_[3] for p_ in parts])
    assert np.array_equal(lab, ref_lab) and all(p_[4] == ref_n for p_ in parts) and ref_n >= 1
    assert np.array_equal(np.concatenate([p_[0] for p_ in parts]), ref)


def test_plan_with_occupied_hbm(hip):
    """Round 6 (VERDICT r05 "next 5"): the engine plan looks at the FREE HBM.  Dummy contexts take the device's memory until less than a
    1024^3 frame's worth is left: the plan of that frame -- which the index range alone would run as one context -- now raises
    MemoryError with the figures ("out of memory", what adaptive_run.is_oom_error and the reference's ladder look for,
    nellie/utils/adaptive_run.py:88-127), also when the same GPU is named twice (two slabs on one GPU need MORE memory, and the message
    says so); a frame that still fits plans, runs and gives the bits it gave on the empty device."""
    from nellie_amd import engine
    from nellie_amd import pipeline as pl
    from nellie_amd.synthetic import ISO_01, make_volume
    from nellie_amd.utils import adaptive_run
    p = pl.FilterParams(dim_res=ISO_01)
    big, small = (1024, 1024, 1024), (64, 160, 192)
    need_big = engine.context_bytes(big)
    free0, total = hip.device_mem_info(0)
    if free0 < need_big * 2:
        pytest.skip("needs a mostly empty device")
    assert engine.plan_engine(big, p) == ("single", 1) and adaptive_run.frame_fits_on_device(big, 0)
    vol = make_volume(small, 77)
    ref = pl.FramePipeline(small)
    ref.filter(vol, p)
    fr_ref = ref.download_frangi()
    n_ref = ref.label(ref.frangi_threshold(), pl.min_area_pixels_of(ISO_01))
    lab_ref = ref.download_labels()
    ref.close()
    dummies = []
    try:
        while hip.device_mem_info(0)[0] * engine.HBM_HEADROOM >= need_big and len(dummies) < 8:
            dummies.append(pl.FramePipeline((1000, 1024, 1024)))           # ~41 GB each
        free1 = hip.device_mem_info(0)[0]
        assert free1 * engine.HBM_HEADROOM < need_big, (free1, need_big)
        assert not adaptive_run.frame_fits_on_device(big, 0)
        with pytest.raises(MemoryError) as exc:
            engine.plan_engine(big, p)
        assert adaptive_run.is_oom_error(exc.value) and "GiB free" in str(exc.value)
        with pytest.raises(MemoryError) as exc2:
            engine.plan_engine(big, p, devices=[0, 0])
        assert "more memory, not less" in str(exc2.value)
        with pytest.raises(MemoryError):
            engine.make_engine(big, p)
        eng = engine.make_engine(small, p)                                    # what still fits runs, unchanged
        assert eng.kind == "single"
        eng.filter(vol, p)
        assert np.array_equal(eng.download_frangi(), fr_ref)
        assert eng.label(eng.frangi_threshold(), pl.min_area_pixels_of(ISO_01)) == n_ref and np.array_equal(eng.download_labels(), lab_ref)
        eng.close()
    finally:
        for d in dummies:
            d.close()
    assert engine.plan_engine(big, p) == ("single", 1)                        # ... and the memory came back
