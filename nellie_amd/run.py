"""
`run()`: the hot-path half of nellie.run.run (reference nellie/run.py:18-130) -- Filter then Label on the
MI355X engine, same keyword names, same `timeit` prints.  The later stages are opt-in: `network=True` runs this
package's Network (reference run.py:85-86) behind Label and writes im_skel / im_pixel_class / im_skel_relabelled
(its thinning is the one host call: skimage's, or the `skeletonize` callable -- or none with skeletonize="hip"); `markers=True` runs this package's
Markers stage (reference run.py:88-89; it does not depend on Network) and writes im_marker / im_distance /
im_border; `tracking=True` then runs this package's HuMomentTracking on them (run.py:91-92) and writes
flow_vector_array; `reassign=True` runs this package's VoxelReassigner behind tracking (run.py:94-95) and writes
im_obj_label_reassigned / im_branch_label_reassigned; `features=True` runs this package's Hierarchy last (run.py:97-98) and writes the
five feature tables and the adjacency maps.  `full=True` turns all five on: the reference's whole run().  `transitions=True` runs
this package's MatchTransitions behind VoxelReassigner and writes the label_transitions pickle; `full` leaves it off.  Without these keywords the
later stages are left to the caller, who finds the two files Filter and Label wrote.
"""
from __future__ import annotations

import os
import time

from nellie_amd.segmentation.filtering import Filter
from nellie_amd.segmentation.labelling import Label
from nellie_amd.stage import env_shard, flush, open_outputs, resolve_shard


def _wait_for(path, timeout_s=600.0):
    t0 = time.time()
    while not os.path.exists(path):
        if time.time() - t0 > timeout_s:
            raise TimeoutError(f"no {path} after {timeout_s} s")
        time.sleep(0.02)


def _build_im_info(file_info, shard):
    """ImInfo(file_info) as run.py:49 -- in a multi-process launch (shard="env") rank 0 first, so that the canonical copy of the
    input (verifier.py:620-695) is written once; the other ranks then find it complete (ome_tiff.create moves files into place
    atomically) and reuse it instead of re-creating it under readers."""
    from nellie_amd.im_info.verifier import ImInfo
    # only "env" makes the ranks take turns here; whatever else `shard` or NELLIE_SHARD holds is for the stages to judge
    spec = resolve_shard("env") if (env_shard() if shard is None else shard) == "env" else None
    if spec is None or spec.world <= 1:
        return ImInfo(file_info)
    import tempfile
    from nellie_amd.rendezvous import rendezvous_for
    src = getattr(file_info, "filepath", None) or (file_info if isinstance(file_info, (str, os.PathLike)) else None)
    d = getattr(file_info, "output_dir", None) or (os.path.dirname(os.path.abspath(os.fspath(src))) if src else tempfile.gettempdir())
    rdv = rendezvous_for(spec, d)
    if spec.rank == 0:
        im_info = ImInfo(file_info)
        rdv.publish("im_info_ready")
    else:
        rdv.wait("im_info_ready")
        im_info = ImInfo(file_info)
    rdv.barrier("im_info_built")
    if spec.rank == 0:
        rdv.remove("im_info_ready")
    return im_info


def run_streamed(im_info, viewer=None, device_index=0, devices=None, shard=None):
    """
    Filter + Label of every frame with the three legs overlapped (nellie_amd/streaming.py): same two files as
    `run()`, default parameters only (no remove_edges / intensity thresholds), 3-D frames.

    Frames of a T stack are independent ("for C5 prefer frame-parallel"):
      devices=[...]  one streamer per GPU in this process (one host thread each), GPU k takes frames k, k + N, ...;
      shard="env"    this process is one rank of a multi-process job (WORLD_SIZE / RANK / LOCAL_RANK): it takes frames
                     RANK, RANK + WORLD_SIZE, ... on GPU LOCAL_RANK; rank 0 creates the two files, the others map them.
    No data crosses between the GPUs; the files are the ones a single GPU writes.
    """
    from nellie_amd.pipeline import FilterParams
    from nellie_amd.streaming import StreamedSegmenter
    if im_info.no_z:
        raise NotImplementedError("streaming covers 3-D frames")
    spec = resolve_shard(shard, use_env=False)               # (NELLIE_SHARD is for the Z-slab stages: frames are dealt out on request only)
    rank, world = (spec.rank, spec.world) if spec is not None else (0, 1)
    fr_path, lab_path = im_info.pipeline_paths["im_preprocessed"], im_info.pipeline_paths["im_instance_label"]
    # a multi-process run meets through files that carry this launch's nonce (nellie_amd/rendezvous.py): the markers of a launch
    # that died on the same MASTER_PORT are never mistaken for this one's
    rdv = None
    if spec is not None and world > 1:
        from nellie_amd.rendezvous import rendezvous_for
        rdv = rendezvous_for(spec, os.path.dirname(lab_path))
    im = im_info.get_memmap(im_info.im_path)
    fr, lab = open_outputs(
        im_info, [(fr_path, "float32", "frangi filtered im"), (lab_path, "int32", "instance segmentation")], creator=rank == 0,
        announce=rdv and (lambda: rdv.publish("streamed_files_ready")), wait=rdv and (lambda: rdv.wait("streamed_files_ready")))
    devs = [spec.device] if spec is not None else ([int(d) for d in devices] if devices else [int(device_index)])
    params = FilterParams(dim_res=im_info.dim_res)
    num_t = im.shape[0]

    def lane(k, n_lanes, first, device):
        """frames first + k, first + k + n_lanes, ... on one GPU"""
        sl = slice(first + k, None, n_lanes)
        if len(range(num_t)[sl]) == 0:
            return
        seg = StreamedSegmenter(im.shape[1:], im.dtype, params, device=device)
        try:
            def status(t, n):
                if viewer is not None and k == 0:
                    viewer.status = f"Preprocessing + extracting organelles. Frame: {t * n_lanes + 1} of {num_t}."
            seg.run(im[sl], fr[sl], lab[sl], status=status, outputs_zeroed=True)   # both files were created (zero-filled) above
        finally:
            seg.close()

    if len(devs) == 1:
        lane(0, world, rank, devs[0])
    else:
        import threading
        errs = []

        def work(k):
            try:
                lane(k, len(devs), 0, devs[k])
            except BaseException as exc:  # noqa: BLE001
                errs.append(exc)
        ts = [threading.Thread(target=work, args=(k,)) for k in range(len(devs))]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        if errs:
            raise errs[0]
    flush(fr, lab)
    if rdv:                                                    # EVERY rank returns only when every rank has flushed its frames
        rdv.barrier("streamed_done")
        if rank == 0:
            rdv.remove("streamed_files_ready")
    return im_info


def _require_inputs(im_info, keyword, asked, written, with_keywords, stages):
    """run(<keyword>=True): every file of `written` ({key of pipeline_paths: a requested stage will write it}) that no stage of
    this call writes must exist already"""
    if not asked:
        return
    missing = [k for k, comes in written.items() if not comes and not os.path.exists(im_info.pipeline_paths[k])]
    if missing:
        raise FileNotFoundError(f"run({keyword}=True) needs the files {missing}: run with {with_keywords}, or run {stages} first")


def run(file_info, remove_edges=False, otsu_thresh_intensity=False, threshold=None, timeit=False, device="auto",
        low_memory=False, markers=False, devices=None, shard=None, tracking=False, network=False, skeletonize=None, reassign=False,
        features=False, full=False, solidity=False, transitions=False):
    """nellie.run.run's signature (run.py:18-26): `file_info` is a FileInfo (this package's or any object with the same
    fields) from which the ImInfo is built as run.py:49 does; an ImInfo (anything with `pipeline_paths`) or a path / array
    is accepted too.  Returns the ImInfo.
    devices=[...]: every 3-D frame runs as Z slabs over these GPUs; shard="env": this process is one rank (WORLD_SIZE / RANK /
    LOCAL_RANK) of a multi-process Z-slab job over RCCL -- see nellie_amd/engine.py.  Frames beyond one context's size are
    cut into slabs without being asked.
    tracking=True: Hu-moment tracking after Markers; without markers=True it needs Markers' files (im_marker, im_distance)
    and raises before anything runs if they do not exist.
    network=True: Network after Label and before Markers; skeletonize: its thinning, a callable(bool ndarray) -> bool ndarray
    (None: skimage.morphology.skeletonize, whose absence raises ImportError before anything runs), or "hip": the 3-D thinning on the
    device (NotImplementedError for a 2-D image, before any stage runs).
    reassign=True: VoxelReassigner after tracking (skipped, as tracking is, for a stack without T); features=True: Hierarchy
    (skip_nodes=False) last.  Either needs the files of the stages before it: those that no requested stage will write must exist, or
    FileNotFoundError names them before anything runs.
    full=True: network, markers, tracking, reassign and features, the reference's whole run().
    solidity=True (with features or full): Hierarchy fills `branch_solidity` and `organelle_solidity` from exact convex-hull voxel
    counts; by default they stay NaN.
    transitions=True (or "organelle"), or "branch": MatchTransitions of that level after VoxelReassigner (skipped for a stack
    without T); it writes the label_transitions pickle.  It needs voxel_matches, which reassign=True writes;
    `full` does not turn it on."""
    level = "organelle" if transitions is True else transitions
    if transitions and level not in ("organelle", "branch"):
        raise ValueError(f"transitions must be True, 'organelle' or 'branch', got {transitions!r}")
    if full:
        network = markers = tracking = reassign = features = True
    if network and skeletonize is None:
        from nellie_amd.segmentation.networking import _import_skeletonize
        _import_skeletonize()
    elif network:
        from nellie_amd.segmentation.networking import _check_thinning
        _check_thinning(skeletonize, file_info)         # an unknown name, or "hip" where `file_info` already says 2-D: before anything runs
    if hasattr(file_info, "pipeline_paths"):
        im_info = file_info
    else:
        im_info = _build_im_info(file_info, shard)
        if network:
            _check_thinning(skeletonize, im_info)      # a path or an array: known only now, still before any stage
    if tracking and not markers:
        missing = [k for k in ("im_marker", "im_distance") if not os.path.exists(im_info.pipeline_paths[k])]
        if missing:
            raise FileNotFoundError(f"run(tracking=True) needs Markers' outputs {missing}: run with markers=True, or run Markers first")
    _require_inputs(im_info, "reassign", reassign and not im_info.no_t, dict(flow_vector_array=tracking, im_skel_relabelled=network, im_instance_label=True),
                    "tracking=True and network=True", "HuMomentTracking and Network")
    _require_inputs(im_info, "features", features, dict(im_skel=network, im_pixel_class=network, im_skel_relabelled=network, im_distance=markers,
                                                        im_border=markers), "network=True and markers=True", "Network and Markers")
    needed = dict(voxel_matches=reassign, im_instance_label=True)     # Label always writes the organelle labels
    if level == "branch":
        needed["im_skel_relabelled"] = network                         # read by the branch level only
    _require_inputs(im_info, "transitions", bool(transitions) and not im_info.no_t, needed,
                    "reassign=True" + (" and network=True" if level == "branch" else ""), "VoxelReassigner")
    t0 = time.perf_counter() if timeit else None
    preprocessing = Filter(im_info, remove_edges=remove_edges, device=device, low_memory=low_memory, devices=devices, shard=shard)
    preprocessing.run()
    if timeit:
        t1 = time.perf_counter()
        print(f"[timeit] Filter: {t1 - t0:.3f}s")
    segmenting = Label(im_info, otsu_thresh_intensity=otsu_thresh_intensity, threshold=threshold, device=device,
                       low_memory=low_memory, devices=devices, shard=shard)
    segmenting.run()
    if timeit:
        t2 = time.perf_counter()
        print(f"[timeit] Label: {t2 - t1:.3f}s")
    if network:
        from nellie_amd.segmentation.networking import Network
        Network(im_info, device=device, low_memory=low_memory, skeletonize=skeletonize).run()
        if timeit:
            t_net = time.perf_counter()
            print(f"[timeit] Network: {t_net - t2:.3f}s")
            t2 = t_net
    if markers:
        from nellie_amd.segmentation.mocap_marking import Markers
        Markers(im_info, device=device, low_memory=low_memory, devices=devices, shard=shard).run()
        if timeit:
            print(f"[timeit] Markers: {time.perf_counter() - t2:.3f}s")
    if tracking and not im_info.no_t:
        from nellie_amd.tracking.hu_tracking import HuMomentTracking
        t3 = time.perf_counter()
        HuMomentTracking(im_info, device=device, low_memory=low_memory).run()
        if timeit:
            print(f"[timeit] Tracking: {time.perf_counter() - t3:.3f}s")
    if reassign and not im_info.no_t:
        from nellie_amd.tracking.voxel_reassignment import VoxelReassigner
        t4 = time.perf_counter()
        VoxelReassigner(im_info, device=device, low_memory=low_memory).run()
        if timeit:
            print(f"[timeit] VoxelReassigner: {time.perf_counter() - t4:.3f}s")
    if transitions and not im_info.no_t:
        from nellie_amd.tracking.match_transitions import MatchTransitions
        t_tr = time.perf_counter()
        MatchTransitions(im_info, level=level, device=device).run()
        if timeit:
            print(f"[timeit] MatchTransitions: {time.perf_counter() - t_tr:.3f}s")
    if features:
        from nellie_amd.feature_extraction.hierarchy import Hierarchy
        t5 = time.perf_counter()
        Hierarchy(im_info, skip_nodes=False, device=device, low_memory=low_memory, solidity=solidity).run()
        if timeit:
            print(f"[timeit] Hierarchy: {time.perf_counter() - t5:.3f}s")
    if timeit:
        print(f"[timeit] Total: {time.perf_counter() - t0:.3f}s")
    return im_info
