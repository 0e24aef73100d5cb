"""
ctypes binding of libnellie_hip.so (C-ABI: include/nellie_amd.h).

There is no CPU fallback: if the library is missing or no MI355X is present, every
entry point raises.  Status codes map to the exception classes the reference's retry
ladder recognises (nellie/utils/adaptive_run.py:116-141):
    NL_ENODEV -> RuntimeError("GPU backend requested but ...")
    NL_ENOMEM -> MemoryError("... out of memory ...")
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NELLIE_HIP_LIB") or os.path.join(_HERE, "libnellie_hip.so")   # the override is for A/B builds (tools/build_variant.sh)

NL_OK, NL_EINVAL, NL_ENODEV, NL_ENOMEM, NL_EHIP, NL_ESTATE, NL_ECOMM = range(7)
FIELD_GAUSS, FIELD_FROB, FIELD_FRANGI, FIELD_VESSELNESS = 0, 1, 2, 3

DTYPE_CODES = {
    np.dtype(np.uint8): 0, np.dtype(np.int8): 1, np.dtype(np.uint16): 2, np.dtype(np.int16): 3,
    np.dtype(np.uint32): 4, np.dtype(np.int32): 5, np.dtype(np.float32): 6, np.dtype(np.float64): 7,
    np.dtype(np.uint64): 8, np.dtype(np.int64): 9,
}

_ERRLEN = 512
_i64, _int, _f32, _f64 = C.c_int64, C.c_int, C.c_float, C.c_double
_p = C.c_void_p
_ERR = (C.c_char_p, C.c_size_t)

# name -> argtypes WITHOUT the trailing (err, errlen) pair; every listed function returns int
_PROTOS = {
    "nl_device_count": [C.POINTER(_int)],
    "nl_device_mem_info": [_int, C.POINTER(_i64), C.POINTER(_i64)],
    "nl_device_name": [_int, C.c_char_p, C.c_size_t],
    "nl_ctx_create": [C.POINTER(_p), _int, _i64, _i64, _i64, _i64, _i64, _i64, _i64],
    "nl_sync": [_p],
    "nl_filter_load": [_p, _p, _int, _i64, _i64],
    "nl_input_load": [_p, _p, _int, _i64, _i64],
    "nl_filter_begin": [_p],
    "nl_gauss_step": [_p, _p, _int, _p, _int, _p, _int, _i64, _i64],
    "nl_gauss_step_ahead": [_p, _p, _int, _p, _int, _p, _int, _i64, _i64],
    "nl_gauss_commit": [_p],
    "nl_sample_gather": [_p, _int, _i64, _i64, _i64, _p, _i64, C.POINTER(_i64)],
    "nl_sample_gather_positive": [_p, _int, _i64, _i64, _i64, _p, _i64, C.POINTER(_i64)],
    "nl_sample_gather_positive_begin": [_p, _int, _i64, _i64, _i64, C.POINTER(_i64)],
    "nl_sample_gather_positive_end": [_p, _p, _i64, C.POINTER(_i64)],
    "nl_sample_minmax": [_p, _int, _i64, _i64, _i64, C.POINTER(_f32), C.POINTER(_f32), C.POINTER(_i64)],
    "nl_sample_hist": [_p, _int, _i64, _i64, _i64, _p, _int, _p],
    "nl_sample_range_hist": [_p, _int, _i64, _i64, _i64, _int, C.POINTER(_f32), C.POINTER(_f32), C.POINTER(_i64), _p, _p, C.POINTER(_int)],
    "nl_sample_range_hist2": [_p, _int, _int, _i64, _i64, _i64, _int, _p, _p, _p, _p, _p, _p],
    "nl_hist_thresholds": [_p, _p, _int, C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_int)],
    "nl_hist_thresholds_ex": [_p, _p, _int, _int, C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_int)],
    "nl_host_hist_thresholds_f32": [_p, _i64, _int, C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_int), _p, _p],
    "nl_tail_enqueue": [_p, _i64, _i64, _i64, _f64],
    "nl_tail_finish": [_p, _int, C.POINTER(_i64), C.POINTER(_f32), C.POINTER(_f32), C.POINTER(_f32), C.POINTER(_f32), C.POINTER(_i64)],
    "nl_mask_volume_dev": [_p, _i64, _i64, _i64, _f64, C.POINTER(_i64), C.POINTER(_f32), C.POINTER(_f32), C.POINTER(_f32), C.POINTER(_f32)],
    "nl_debug_percentile": [_p, _p, _i64, _f64, C.POINTER(_f32), C.POINTER(_f32), C.POINTER(_f32)],
    "nl_positive_samples_world": [_p, _int, _int, _i64, _i64, _i64, _i64, _p, _i64, _p],
    "nl_host_slab_join": [_int, _p, _i64, _i64, C.POINTER(_i64), C.POINTER(_i64), _p, _p, _p, _p],
    "nl_host_walk_plan": [_int, _i64, _i64, _i64, _i64, _i64, _i64, _i64, _int, _int, _p, _p],
    "nl_outputs_pack": [_p, _int, _p],
    "nl_outputs_pack_with_label": [_p, _int],
    "nl_outputs_fetch_packed_async": [_p, _p, _i64],
    "nl_outputs_unpack": [_p, _i64, _p, _p, _i64, _int, _int],
    "nl_host_zero": [_p, _i64, _int],
    "nl_hessian_stats": [_p, C.POINTER(_f64), C.POINTER(_f32), C.POINTER(_f32), C.POINTER(_int)],
    "nl_set_frob_norm": [_p, _f32, _f32],
    "nl_vesselness_step": [_p, _f32, _f32, _f32, _int, _f32, _i64, _i64, C.POINTER(_i64)],
    "nl_set_spacing": [_p, C.POINTER(_f64)],
    "nl_vesselness_spec": [_p, C.POINTER(_f64), _f32, _f32, _i64, _i64, C.POINTER(_f32), C.POINTER(_f32),
                           C.POINTER(_int), C.POINTER(_int)],
    "nl_vesselness_resolve": [_p, _f32, _f32, _f32, _int, _f32, C.POINTER(_int), C.POINTER(_i64)],
    "nl_vesselness_count": [_p, C.POINTER(_i64)],
    "nl_set_ndim": [_p, _int],
    "nl_markers_begin": [_p, _p, _p, _int],
    "nl_markers_distance": [_p, _f32, C.POINTER(_i64)],
    "nl_markers_log_step": [_p, C.POINTER(_f64), C.POINTER(_f64), _int, C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_f64),
                            C.POINTER(_f64), _int, _f32],
    "nl_markers_finish": [_p, _int, C.POINTER(_i64)],
    "nl_markers_use_image": [_p, _p],
    "nl_markers_store": [_p, _p, _p, _p],
    "nl_skel_pixel_class": [_p, _p, _p, C.POINTER(_i64)],
    "nl_skel_branch_labels": [_p, _p, _p, C.POINTER(_i64)],
    "nl_network_load": [_p, _p, _p, _p, _int, C.POINTER(_i64)],
    "nl_network_clean_seed": [_p, C.POINTER(_i64), C.POINTER(_i64)],
    "nl_network_classes": [_p, C.POINTER(_i64), C.POINTER(_i64)],
    "nl_network_relabel_load": [_p, _p, _p, _int, C.POINTER(_i64)],
    "nl_network_relabel": [_p, C.POINTER(_f64), _i64, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)],
    "nl_network_fetch": [_p, _p, _p, _p],
    "nl_network_kernel_ms": [_p, C.POINTER(_f32)],
    "nl_thin": [_p, _p, _p, _int, _int, C.POINTER(_i64)],
    "nl_network_load_thin": [_p, _p, _p, _int, _int, C.POINTER(_i64), C.POINTER(_i64)],
    "nl_network_fetch_mask": [_p, _p],
    "nl_thin_info": [_p, C.POINTER(_i64), C.POINTER(_f32)],
    "nl_mask_volume_fused": [_p, _f32, C.POINTER(_i64)],
    "nl_log2d_step": [_p, C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_f64), C.POINTER(_f64), _int, _f32, _int, _int],
    "nl_log2d_finish": [_p, C.POINTER(_i64)],
    "nl_filter_finish": [_p, _i64, _i64, C.POINTER(_i64)],
    "nl_remove_edges": [_p, _int, C.POINTER(_i64)],
    "nl_planes_get": [_p, _int, _i64, _i64, _p],
    "nl_planes_put": [_p, _int, _i64, _i64, _p],
    "nl_comm_unique_id": [C.c_char_p],
    "nl_comm_loopback_id": [C.c_char_p],
    "nl_comm_init": [_p, _int, _int, C.c_char_p],
    "nl_halo_exchange": [_p, _int, _i64],
    "nl_halo_exchange_at": [_p, _int, _i64, _i64, _int],
    "nl_comm_init2": [_p, _int, _int, C.c_char_p],
    "nl_allreduce": [_p, _p, _i64, _int, _int],
    "nl_mask_volume": [_p, _f32],
    "nl_filter_store": [_p, _p, _i64, _i64],
    "nl_gauss_store": [_p, _p, _i64, _i64],
    "nl_label_load_frangi": [_p, _p, _i64, _i64],
    "nl_label_intensity_mask": [_p, _p, _int, _f64],
    "nl_label_intensity_mask_planes": [_p, _p, _int, _f64, _i64, _i64],
    "nl_label_intensity_mask_int": [_p, _p, _int, _i64, _i64, _i64],
    "nl_flat_sample_gather": [_p, _int, _i64, _i64, _p, _i64, C.POINTER(_i64)],
    "nl_flat_sample_gather_positive": [_p, _int, _i64, _i64, _p, _i64, C.POINTER(_i64)],
    "nl_label_run": [_p, _int, _f32, _i64, _int, C.POINTER(_i64)],
    "nl_label_store": [_p, _p, _i64, _i64],
    "nl_label_pack": [_p, _int, _f32],
    "nl_label_bits_get": [_p, _i64, _i64, _p],
    "nl_label_bits_put": [_p, _i64, _i64, _p],
    "nl_label_bits_allgather": [_p, _p],
    "nl_label_run_global": [_p, _i64, _int, C.POINTER(_i64)],
    "nl_slab_label_pack": [_p, _int, _f32],
    "nl_slab_bits_get": [_p, _int, _i64, _p],
    "nl_slab_bits_put": [_p, _int, _i64, _p],
    "nl_slab_bits_exchange": [_p, _int],
    "nl_slab_phase": [_p, _int, _int, _i64, _p, C.POINTER(_i64), C.POINTER(_i64)],
    "nl_slab_patch": [_p, _i64, _p, _p],
    "nl_slab_apply": [_p, _i64],
    "nl_slab_majority": [_p],
    "nl_slab_number": [_p, _i64, _p, _i64, _p, C.POINTER(_i64), _p],
    "nl_slab_paint": [_p, _i64, _i64, _p, _p],
    "nl_allgather_bytes": [_p, _p, _i64, _p, _i64, _p],
    "nl_allgather_var": [_p, _p, _i64, _p, _p, _p],
    "nl_comm_fuse": [_p, _int],
    "nl_chain_begin": [_p, _int],
    "nl_chain_scale": [_p, _p, _i64, _i64, _i64, _f64, _f64, _f64, _f64, _f64, _i64, _i64],
    "nl_chain_flush": [_p],
    "nl_chain_finish": [_p, _p, _p, _p, _p, _p],
    "nl_chain_log": [_p, _int, _int, _p, _p, _p, _p],
    "nl_gauss_step_fused": [_p, _p, _int, _p, _int, _p, _int, C.POINTER(_int)],
    "nl_chain_begin_unordered": [_p, _int],
    "nl_chain_sample": [_p, _int, _p, _i64, _i64, _i64, _f64, _f64, _f64],
    "nl_chain_estimates": [_p, _p, _int],
    "nl_chain_walk": [_p, _int, _p, _i64, _i64, _i64, _f64, _f64, _f64, _i64, _i64],
    "nl_pinned_alloc": [C.POINTER(_p), _i64],
    "nl_host_register": [_p, _i64],
    "nl_input_load_async": [_p, _int, _p, _int],
    "nl_input_select": [_p, _int],
    "nl_input_wait": [_p, _int],
    "nl_outputs_stage": [_p, _int],
    "nl_outputs_fetch_async": [_p, _p, _p],
    "nl_outputs_wait": [_p],
    "nl_debug_eig_frangi": [_p, _p, _i64, _int, _f32, _f32, _f32, _p],
    "nl_timer_begin": [_p],
    "nl_timer_end_ms": [_p, C.POINTER(_f32)],
    "nl_track_create": [C.POINTER(_p), _int, _int, _i64, _i64, _i64, _p],
    "nl_track_frame": [_p, _p, _int, _p, _p, _p, C.POINTER(_i64)],
    "nl_track_features": [_p, _int, _p, _p, _p],
    "nl_track_match": [_p, _int, _f64, _p, _p, _p, _p, _p],
    "nl_flow_create": [C.POINTER(_p), _int, _int, _p, _f64],
    "nl_flow_load": [_p, _p, _p, _p, _i64],
    "nl_flow_interpolate": [_p, _p, _i64, _p, C.POINTER(_i64)],
    "nl_flow_interpolate_dev": [_p, _p, _i64, _p, C.POINTER(_i64)],
    "nl_flow_kernel_ms": [_p, C.POINTER(_f32)],
    "nl_flow_grid_info": [_p, _p, C.POINTER(_i64), _p, C.POINTER(_i64), C.POINTER(_i64)],
    "nl_reassign_create": [C.POINTER(_p), _int, _int, _i64, _i64, _i64, _p, _f64],
    "nl_reassign_frame": [_p, _p, _p, _int, C.POINTER(_i64)],
    "nl_reassign_pair": [_p, _p, _p, C.POINTER(_i64)],
    "nl_reassign_fetch": [_p, _int, _p, _p, _p, _p],
    "nl_reassign_kernel_ms": [_p, C.POINTER(_f32)],
    "nl_tracks_create": [C.POINTER(_p), _int, _int, _i64, _i64, _i64, _int],
    "nl_tracks_mask": [_p, _int, _p],
    "nl_tracks_seed": [_p, _int, _p, _int, C.c_int32, _int, C.POINTER(_i64)],
    "nl_tracks_begin": [_p, _i64, _i64, _i64],
    "nl_tracks_step": [_p, _p, _int, _int, _i64, _i64, C.POINTER(_i64)],
    "nl_tracks_filter": [_p, _i64, _int],
    "nl_tracks_finish": [_p, C.POINTER(_i64)],
    "nl_tracks_fetch": [_p, _p],
    "nl_tracks_kernel_ms": [_p, _p],
    "nl_overlay_create": [C.POINTER(_p), _int, _int, _i64, _i64, _i64],
    "nl_overlay_load": [_p, _p, C.POINTER(_i64)],
    "nl_overlay_groups": [_p, _p, _p, _p, _i64],
    "nl_overlay_values": [_p, _p, _i64, _int, _int],
    "nl_overlay_paint": [_p, _int],
    "nl_overlay_fetch_values": [_p, _p],
    "nl_overlay_fetch_frame": [_p, _p],
    "nl_overlay_kernel_ms": [_p, _p],
    "nl_trans_create": [C.POINTER(_p), _int, _int, _i64, _i64, _i64],
    "nl_trans_frame": [_p, _p, _int],
    "nl_trans_begin": [_p, _i64],
    "nl_trans_count": [_p, _p, _p, _int, _i64, _i64, C.POINTER(_int)],
    "nl_trans_finish": [_p, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_int)],
    "nl_trans_fetch": [_p, _p],
    "nl_trans_label_max": [_p, C.POINTER(_i64)],
    "nl_trans_relabel": [_p, _p, _i64],
    "nl_trans_fetch_frame": [_p, _p],
    "nl_trans_kernel_ms": [_p, _p],
    "nl_voxfeat_create": [C.POINTER(_p), _int, _int, _i64, _i64, _i64, _p, _f64],
    "nl_voxfeat_frame": [_p, _p, _p, _p, _int, _p, _int, C.POINTER(_i64)],
    "nl_voxfeat_fetch_voxels": [_p, _p, _p, _p, _p, _p],
    "nl_voxfeat_motility": [_p, _p, _p, C.POINTER(_i64), C.POINTER(_i64)],
    "nl_voxfeat_fetch_motility": [_p, C.POINTER(_p)],
    "nl_voxfeat_nodes": [_p, _p, _int, _p, _int, C.POINTER(_i64), C.POINTER(_i64)],
    "nl_voxfeat_fetch_nodes": [_p, _p, _p, _p, _p, _p, _p, _p],
    "nl_voxfeat_kernel_ms": [_p, _p],
    "nl_nodefeat_create": [C.POINTER(_p), _int, _int, _i64, _i64, _i64, _p],
    "nl_nodefeat_frame": [_p, _p, _int, _p, _int, _p, _int, _p, _int, C.POINTER(_i64)],
    "nl_nodefeat_fetch": [_p, _p, _p, _p, _p],
    "nl_nodefeat_groups": [_p, _p, _p, _i64, C.POINTER(_i64)],
    "nl_nodefeat_set_wide_from": [_p, _i64],
    "nl_nodefeat_aggregate": [_p, _p, _int, _i64, _p],
    "nl_nodefeat_node_stats": [_p, _p, _p, _p, _i64, _p],
    "nl_nodefeat_kernel_ms": [_p, _p],
    "nl_branchfeat_create": [C.POINTER(_p), _int, _int, _i64, _i64, _i64, _p],
    "nl_branchfeat_frame": [_p, _p, _int, _p, _int, _p, _int, C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i64)],
    "nl_branchfeat_fetch": [_p] * 12,
    "nl_branchfeat_regions": [_p, _p, _int, _p, _int, C.POINTER(_i64)],
    "nl_branchfeat_regions_rows": [_p, _p, _int, _p, _int, C.POINTER(_i64)],
    "nl_branchfeat_fetch_regions": [_p, _p, _p, _p],
    "nl_branchfeat_kernel_ms": [_p, _p],
    "nl_branchfeat_convex": [_p],
    "nl_branchfeat_fetch_convex": [_p, _p, _p, _p],
    "nl_branchfeat_convex_ms": [_p, _p],
    "nl_branchfeat_convex_limits": [_p],
    "nl_host_convex_facets": [_p, _i64, _int, _p, _i64, C.POINTER(_i64)],
    "nl_adjacency_create": [C.POINTER(_p), _int],
    "nl_adjacency_pairs": [_p, _p, _int, _i64, _i64, C.POINTER(_i64)],
    "nl_adjacency_expand": [_p, _p, _p, _i64, C.POINTER(_i64)],
    "nl_adjacency_lookup": [_p, _p, _i64, _p, _i64, C.POINTER(_i64)],
    "nl_adjacency_fetch": [_p, _p],
    "nl_adjacency_kernel_ms": [_p, _p],
    "nl_host_half_round": [_p, _p, _i64],
    "nl_host_half_nansum": [_p, _i64, _int, _p],
    "nl_host_np_sum_f32": [_p, _i64, _p],
}
# functions without the (err, errlen) tail
_PLAIN = {
    "nl_version": (C.c_char_p, []),
    "nl_ctx_destroy": (_int, [_p]),
    "nl_ctx_bytes": (_i64, [_i64, _i64, _i64]),
    "nl_prof_enable": (_int, [_p, _int]),
    "nl_prof_get": (_int, [_p, C.c_char_p, C.POINTER(_f64), C.POINTER(_i64)]),
    "nl_prof_reset": (_int, [_p]),
    "nl_pinned_free": (_int, [_p]),
    "nl_host_unregister": (_int, [_p]),
    "nl_ctx_info": (_int, [_p, C.c_char_p, C.POINTER(_f64)]),
    "nl_track_destroy": (_int, [_p]),
    "nl_flow_destroy": (_int, [_p]),
    "nl_reassign_destroy": (_int, [_p]),
    "nl_tracks_destroy": (_int, [_p]),
    "nl_overlay_destroy": (_int, [_p]),
    "nl_trans_destroy": (_int, [_p]),
    "nl_voxfeat_destroy": (_int, [_p]),
    "nl_nodefeat_destroy": (_int, [_p]),
    "nl_branchfeat_destroy": (_int, [_p]),
    "nl_adjacency_destroy": (_int, [_p]),
    "nl_thin_decide_host": (_int, [_p, _i64, _p]),
}
ALL_SYMBOLS = sorted(list(_PROTOS) + list(_PLAIN))


class NellieHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


class LibraryUnavailable(RuntimeError):
    """libnellie_hip.so is not built or cannot be loaded (as opposed to an error the loaded library reports)."""


def _raise(code: int, msg: str):
    if code == NL_ENODEV:
        if "GPU backend requested" not in msg:
            msg = "GPU backend requested but " + msg
        raise RuntimeError(msg)
    if code == NL_ENOMEM:
        raise MemoryError(f"HIP out of memory: {msg}")
    if code == NL_EINVAL:
        raise ValueError(msg)
    raise NellieHipError(code, f"libnellie_hip error {code}: {msg}")


class _Lib:
    def __init__(self, path: str):
        self.path = path
        self.cdll = C.CDLL(path)
        for name, argtypes in _PROTOS.items():
            fn = getattr(self.cdll, name)
            fn.restype = _int
            fn.argtypes = list(argtypes) + list(_ERR)
        for name, (res, argtypes) in _PLAIN.items():
            fn = getattr(self.cdll, name)
            fn.restype = res
            fn.argtypes = argtypes

    def call(self, name: str, *args):
        buf = C.create_string_buffer(_ERRLEN)
        rc = getattr(self.cdll, name)(*args, buf, _ERRLEN)
        if rc != NL_OK:
            _raise(rc, buf.value.decode("utf-8", "replace"))

    def version(self) -> str:
        return self.cdll.nl_version().decode()

    def device_count(self) -> int:
        n = _int(0)
        buf = C.create_string_buffer(_ERRLEN)
        rc = self.cdll.nl_device_count(C.byref(n), buf, _ERRLEN)
        return int(n.value) if rc == NL_OK else 0

    def device_mem_info(self, device=0):
        f, t = _i64(0), _i64(0)
        self.call("nl_device_mem_info", device, C.byref(f), C.byref(t))
        return int(f.value), int(t.value)

    def device_name(self, device=0) -> str:
        b = C.create_string_buffer(256)
        self.call("nl_device_name", device, b, 256)
        return b.value.decode()


_LIB = None


def load() -> _Lib:
    """Load libnellie_hip.so or raise.  Never falls back to a CPU implementation."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise LibraryUnavailable(
                f"GPU backend requested but {LIB_PATH} is not built "
                "(run `python -m nellie_amd.build`); nellie_amd has no CPU fallback")
        try:
            _LIB = _Lib(LIB_PATH)
        except OSError as e:
            raise LibraryUnavailable(f"GPU backend requested but {LIB_PATH} cannot be loaded: {e}") from e
    return _LIB


def hist_thresholds(counts, edges, with_variance=False):
    """(triangle, otsu) bin-centre thresholds of a finished histogram (nl_hist_thresholds_ex; gpu_functions.py:36-50, 64-94),
    in the dtype of the edges: float32 edges (float32 data) give float32 centres, anything else is numpy's float64 path
    (integer / float64 data).  with_variance: (triangle, otsu, between-class variance at otsu).
    Raises numpy's ValueError where the reference's triangle construction does (one non-empty bin)."""
    counts = np.ascontiguousarray(counts, dtype=np.int64)
    edges = np.asarray(edges)
    f64 = edges.dtype != np.float32
    edges = np.ascontiguousarray(edges, dtype=np.float64 if f64 else np.float32)
    nbins = int(counts.size)
    assert edges.size == nbins + 1
    tri, otsu, var, status = _f64(0.0), _f64(0.0), _f64(0.0), _int(0)
    load().call("nl_hist_thresholds_ex", _ptr(counts), _ptr(edges), 1 if f64 else 0, nbins, C.byref(tri), C.byref(otsu), C.byref(var),
                C.byref(status))
    if status.value == 1:
        raise ValueError("attempt to get argmax of an empty sequence")
    out_t = np.float64 if f64 else np.float32
    if with_variance:
        return out_t(tri.value), out_t(otsu.value), np.float64(var.value)
    return out_t(tri.value), out_t(otsu.value)


def thin_decide_host(words):
    """The thinning kernels' decision functions on the host (nl_thin_decide_host): uint8 flags per 27-bit neighbourhood word, bit 0
    endpoint, bit 1 Euler-invariant, bit 2 simple.  Needs the library, no device."""
    w = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1)
    flags = np.zeros(w.size, np.uint8)
    rc = load().cdll.nl_thin_decide_host(_ptr(w), int(w.size), _ptr(flags))
    if rc != NL_OK:
        raise ValueError("nl_thin_decide_host refused its arguments")
    return flags


def host_hist_thresholds(values, nbins=256, with_histogram=False):
    """(triangle, otsu) of np.histogram(values, bins=nbins) for float32 host data, computed by the library in one call
    (nl_host_hist_thresholds_f32); with_histogram: (triangle, otsu, counts, edges).  Raises ValueError where numpy would."""
    v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
    tri, otsu, status = _f64(0.0), _f64(0.0), _int(0)
    counts = np.zeros(nbins, np.int64) if with_histogram else None
    edges = np.zeros(nbins + 1, np.float32) if with_histogram else None
    load().call("nl_host_hist_thresholds_f32", _ptr(v), int(v.size), int(nbins), C.byref(tri), C.byref(otsu), C.byref(status),
                None if counts is None else _ptr(counts), None if edges is None else _ptr(edges))
    if status.value == 2:
        raise ValueError("autodetected range of [%s, %s] is not finite" % (v.min(), v.max()))
    if status.value == 1:
        raise ValueError("attempt to get argmax of an empty sequence")
    out = (np.float32(tri.value), np.float32(otsu.value))
    return out + (counts, edges) if with_histogram else out


def host_slab_join(blobs):
    """The joined view of the slab tables of all ranks (nl_host_slab_join; host code, no device): blobs = one int32 array per
    rank as Context.slab_phase returns them.  -> (rank, root, val, comp, ncomp): one node per (rank, tree)."""
    world = len(blobs)
    block = max(8, max(int(b.size) for b in blobs))
    flat = np.zeros(world * block, np.int32)
    for r, b in enumerate(blobs):
        flat[r * block:r * block + b.size] = b
    cap = max(1, sum(int(b[:4].sum()) for b in blobs))            # nodes <= entries
    n, nc = _i64(0), _i64(0)
    rank, root, val, comp = np.empty(cap, np.int64), np.empty(cap, np.int32), np.empty(cap, np.int64), np.empty(cap, np.int64)
    load().call("nl_host_slab_join", world, _ptr(flat), block, cap, C.byref(n), C.byref(nc), _ptr(rank), _ptr(root), _ptr(val), _ptr(comp))
    k = int(n.value)
    if k > cap:          # (the library reports this as an error: the arrays above are sized from the entry counts, which bound the nodes)
        raise NellieHipError(NL_EINVAL, f"nl_host_slab_join: {k} nodes for arrays of {cap}")
    return rank[:k], root[:k], val[:k], comp[:k], int(nc.value)


WALK_PLAN_FIELDS = ("family", "tile_rows", "rs", "np", "division", "zchunk", "ntx", "nty", "nzc", "grid", "regions", "qcap", "launch_planes")
WALK_SWITCH_DEFAULTS = {"NELLIE_HV_RS": 8, "NELLIE_HV_NP": 1, "NELLIE_HV_DPP": 0, "NELLIE_HM_TY": 8, "NELLIE_HV_ZCHUNK": 0, "NELLIE_VQ_CAP": 0,
                        "NELLIE_SPEC_MAX_GB": 64}


def host_walk_plan(mode, shape, own=None, planes=None, fast_div=1, fast_div2=1, **switches):
    """The launch plan of the Hessian walk (nl_host_walk_plan; host code, no device) for a slab of `shape` with the owned planes `own` walked
    over `planes` (both default to the whole slab) -> dict of WALK_PLAN_FIELDS.  switches: NELLIE_* = the value the variable would hold."""
    nzl, ny, nx = (int(v) for v in shape)
    own_lo, own_hi = own or (0, nzl)
    z0, z1 = planes or (own_lo, own_hi)
    assert set(switches) <= set(WALK_SWITCH_DEFAULTS), sorted(set(switches) - set(WALK_SWITCH_DEFAULTS))
    sw = np.array([switches.get(k, d) for k, d in WALK_SWITCH_DEFAULTS.items()], np.int64)
    plan = np.zeros(len(WALK_PLAN_FIELDS), np.int64)
    load().call("nl_host_walk_plan", int(mode), nzl, ny, nx, int(own_lo), int(own_hi), int(z0), int(z1), int(fast_div), int(fast_div2), _ptr(sw), _ptr(plan))
    return dict(zip(WALK_PLAN_FIELDS, (int(v) for v in plan)))


def outputs_unpack(blob, nbytes, frangi, labels=None, zero_fill=True, threads=8):
    """Expand a packed-output blob (Context.outputs_pack) into dense C-contiguous arrays; host code, `threads` host threads."""
    assert frangi.dtype == np.float32 and frangi.flags.c_contiguous and frangi.flags.writeable
    if labels is not None:
        assert labels.dtype == np.int32 and labels.flags.c_contiguous and labels.shape == frangi.shape
    src = blob._p if hasattr(blob, "_p") else _ptr(blob)
    load().call("nl_outputs_unpack", src, int(nbytes), _ptr(frangi), None if labels is None else _ptr(labels),
                int(frangi.size), 1 if zero_fill else 0, int(threads))


def host_zero(array, threads=8):
    """Zero a C-contiguous host array with `threads` host threads (nl_host_zero; the call releases the GIL, so it can run on a
    Python thread beside the GPU calls of the frame whose outputs the array will receive)."""
    assert array.flags.c_contiguous and array.flags.writeable
    load().call("nl_host_zero", _ptr(array), int(array.nbytes), int(threads))


def host_half_round(x):
    """numpy's float64 -> float16 cast as the dense tracking matcher does it (include/nellie_amd.h nl_host_half_round)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty(x.shape, np.float16)
    load().call("nl_host_half_round", _ptr(x), _ptr(out), x.size)
    return out


def host_half_nansum(h):
    """np.nansum(h, axis=-1) of float16 rows (row length <= 23) as the dense tracking matcher does it"""
    h = np.ascontiguousarray(h, dtype=np.float16)
    out = np.empty(h.shape[:-1], np.float16)
    load().call("nl_host_half_nansum", _ptr(h), int(np.prod(h.shape[:-1])), int(h.shape[-1]), _ptr(out))
    return out


def host_np_sum_f32(a):
    """np.sum of a flat float32 array in numpy's order, as the tracking feature kernel sums the float stats"""
    a = np.ascontiguousarray(a, dtype=np.float32).ravel()
    out = np.zeros(1, np.float32)
    load().call("nl_host_np_sum_f32", _ptr(a), a.size, _ptr(out))
    return out[0]


def comm_unique_id(loopback: bool = False) -> bytes:
    """128-byte communicator id (rank 0 creates it and hands it to the other ranks out of band).  loopback=True: an id of
    the in-process loopback transport (nl_comm_loopback_id) -- the ranks are then contexts of this process, one host thread
    each, and every exchange runs through the same library code as over RCCL."""
    buf = C.create_string_buffer(128)
    load().call("nl_comm_loopback_id" if loopback else "nl_comm_unique_id", buf)
    return buf.raw


class PinnedArray:
    """A numpy array over page-locked host memory (hipHostMalloc): asynchronous copies need it."""

    def __init__(self, shape, dtype):
        self.lib = load()
        self.dtype = np.dtype(dtype)
        self.shape = tuple(int(s) for s in shape)
        nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = _p()
        self.lib.call("nl_pinned_alloc", C.byref(p), nbytes)
        self._p = p
        buf = (C.c_char * nbytes).from_address(p.value)
        self.array = np.frombuffer(buf, dtype=self.dtype).reshape(self.shape)

    def free(self):
        if getattr(self, "_p", None):
            self.array = None
            self.lib.cdll.nl_pinned_free(self._p)
            self._p = None

    __del__ = free


class RegisteredArray:
    """Page-locks an existing C-contiguous numpy array for the lifetime of this object (hipHostRegister).
    `ok` is False when the runtime refuses (e.g. some file-backed maps): callers then stage through PinnedArray."""

    def __init__(self, array: np.ndarray):
        self.array = array
        self.ok = False
        self._ptr = None
        if isinstance(array, np.ndarray) and array.flags.c_contiguous and array.flags.writeable and array.nbytes > 0:
            try:
                load().call("nl_host_register", _ptr(array), array.nbytes)
                self.ok = True
                self._ptr = _ptr(array)
            except Exception:
                self.ok = False

    def release(self):
        if self._ptr is not None:
            load().cdll.nl_host_unregister(self._ptr)
            self._ptr = None
            self.ok = False

    __del__ = release


def gpu_available() -> bool:
    """adaptive_run.gpu_available (nellie/utils/adaptive_run.py:23-31) for the HIP backend."""
    try:
        return load().device_count() > 0
    except Exception:
        return False


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(_p)


def _opt(a):
    return None if a is None else _ptr(a)


class _Handle:
    """An opaque handle of the library: created by `nl_*_create`, passed first to every call, destroyed once."""

    _destroy = None      # the destroy symbol (no error buffer)
    _noun = None         # what the error messages call the object
    _h = None

    def _create(self, name, *args):
        self.lib = load()
        h = _p()
        self.lib.call(name, C.byref(h), *args)
        self._h = h

    def close(self):
        if self._h:
            getattr(self.lib.cdll, self._destroy)(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _call(self, name, *args):
        if not self._h:
            raise NellieHipError(NL_ESTATE, f"{self._noun} is closed")
        self.lib.call(name, self._h, *args)


class _TimedParts:
    """The kernel times of a handle whose library call `_ms_symbol` fills one float per name of `PARTS`."""

    PARTS = _ms_symbol = None

    def kernel_ms_parts(self) -> dict:
        ms = (_f32 * len(self.PARTS))()
        self._call(self._ms_symbol, ms)
        return dict(zip(self.PARTS, (float(v) for v in ms)))

    def kernel_ms(self) -> float:
        """device time of the kernels since the last frame(), transfers excluded"""
        return sum(self.kernel_ms_parts().values())


def _frame_geometry(what, spacing, shape=None, ndim=None):
    """The constructor checks of the stage handles -> (ndim, shape, (nz, ny, nx), spacing as float64); a handle without a frame
    shape gives its ndim instead and gets None for both shapes."""
    got = f"ndim {ndim}" if shape is None else f"shape {tuple(shape)}"
    ndim = int(ndim) if shape is None else len(shape)
    if ndim not in (2, 3):
        raise ValueError(f"{what} are 2-D or 3-D, got {got}")
    if shape is not None:
        shape = tuple(int(s) for s in shape)
    sp = np.ascontiguousarray(spacing, dtype=np.float64)
    if sp.size != ndim:
        raise ValueError(f"spacing needs {ndim} values")
    return ndim, shape, (None if shape is None else (1,) * (3 - ndim) + shape), sp


def _frame_array(a, shape, what, owner, dtype=None, dtype_error=TypeError):
    """A frame a stage handle uploads: of the handle's shape, C-contiguous, in `dtype` or (None) in its own dtype, which the
    library must know."""
    a = np.asarray(a)
    if a.shape != shape:
        raise ValueError(f"{what} shape {a.shape} does not match the {owner}'s {shape}")
    if dtype is None and a.dtype not in DTYPE_CODES:
        raise dtype_error(f"unsupported {what} dtype {a.dtype}")
    if dtype is not None and a.dtype != dtype and np.dtype(dtype).kind in "iu":
        _refuse_lossy_cast(a, np.dtype(dtype), what)
    return np.ascontiguousarray(a, dtype=dtype)


def _refuse_lossy_cast(a, dtype, what):
    """ValueError where a.astype(dtype), an integer dtype, would change a value: a label that wrapped or lost its fraction would
    be another object's label, or none.  Checked before the cast, against the extremes and in exact arithmetic."""
    if a.size == 0 or a.dtype.kind == "b":
        return
    if a.dtype.kind not in "iuf":
        raise TypeError(f"{what} of dtype {a.dtype} cannot be converted to {dtype}")
    if a.dtype.kind == "f":
        bad = ~np.isfinite(a)
        if not bad.any():
            bad = a != np.trunc(a)
        if bad.any():
            raise ValueError(f"{what} holds {a[bad].flat[0].item()!r}, which {dtype} cannot hold: refusing a cast that changes values")
    info = np.iinfo(dtype)
    for v in (a.min(), a.max()):
        if not info.min <= int(v) <= info.max:
            raise ValueError(f"{what} holds {int(v)}, outside {dtype}'s range [{info.min}, {info.max}]: refusing a cast that changes values")


def _kernel_ms(handle, name) -> float:
    ms = _f32(0)
    handle._call(name, C.byref(ms))
    return float(ms.value)


class Context(_Handle):
    """One device context = one (device, local slab shape) pair (include/nellie_amd.h nl_ctx)."""

    _destroy, _noun = "nl_ctx_destroy", "context"

    def __init__(self, shape, device=0, gz0=0, gnz=None, own=None):
        nz, ny, nx = (int(s) for s in shape)
        self.shape = (nz, ny, nx)
        self.gz0 = int(gz0)
        self.gnz = int(gnz) if gnz is not None else nz
        self.own = (0, nz) if own is None else (int(own[0]), int(own[1]))
        self.device = int(device)
        self._create("nl_ctx_create", self.device, nz, ny, nx, self.gz0, self.gnz, self.own[0], self.own[1])

    def sync(self):
        self._call("nl_sync")

    # ---------------------------------------------------------------- Filter
    def filter_load(self, frame: np.ndarray, z0=0, z1=None):
        z1 = self.shape[0] if z1 is None else z1
        a = np.ascontiguousarray(frame)
        if a.dtype not in DTYPE_CODES:
            a = a.astype(np.float32)
        assert a.shape == (z1 - z0, self.shape[1], self.shape[2]), (a.shape, self.shape, z0, z1)
        self._call("nl_filter_load", _ptr(a), DTYPE_CODES[a.dtype], z0, z1)

    def input_load(self, frame: np.ndarray, z0=0, z1=None):
        z1 = self.shape[0] if z1 is None else z1
        a = np.ascontiguousarray(frame)
        if a.dtype not in DTYPE_CODES:
            a = a.astype(np.float32)
        assert a.shape == (z1 - z0, self.shape[1], self.shape[2]), (a.shape, self.shape, z0, z1)
        self._call("nl_input_load", _ptr(a), DTYPE_CODES[a.dtype], z0, z1)

    def filter_begin(self):
        self._call("nl_filter_begin")

    def gauss_commit(self):
        self._call("nl_gauss_commit")

    @staticmethod
    def _weight_args(ws):
        args, keep = [], []
        for w in ws:
            if w is None:
                args += [None, 0]
            else:
                w = np.ascontiguousarray(w, dtype=np.float64)
                keep.append(w)
                args += [_ptr(w), (len(w) - 1) // 2]
        return args, keep

    def gauss_step(self, wz, wy, wx, z0=0, z1=None, ahead=False):
        """ahead=True: enqueue the step on the side stream; it becomes current at gauss_commit()."""
        z1 = self.shape[0] if z1 is None else z1
        args, keep = self._weight_args((wz, wy, wx))
        self._call("nl_gauss_step_ahead" if ahead else "nl_gauss_step", *args, z0, z1)

    def gauss_step_fused(self, wz, wy, wx) -> bool:
        """Would gauss_step take this step in one kernel (one volume read, one written)?"""
        args, keep = self._weight_args((wz, wy, wx))
        fused = _int(0)
        self._call("nl_gauss_step_fused", *args, C.byref(fused))
        return bool(fused.value)

    def sample_gather(self, field, strides):
        sz, sy, sx = (int(s) for s in strides)
        n = _i64(0)
        self._call("nl_sample_gather", field, sz, sy, sx, None, 0, C.byref(n))
        out = np.empty(int(n.value), dtype=np.float32)
        if out.size:
            self._call("nl_sample_gather", field, sz, sy, sx, _ptr(out), out.size, C.byref(n))
        return out

    def sample_gather_positive(self, field, strides):
        """The positive lattice samples (device-side compaction, unspecified order)."""
        sz, sy, sx = (int(s) for s in strides)
        n = _i64(0)
        self._call("nl_sample_gather", field, sz, sy, sx, None, 0, C.byref(n))        # lattice size
        out = np.empty(int(n.value), dtype=np.float32)
        if out.size:
            self._call("nl_sample_gather_positive", field, sz, sy, sx, _ptr(out), out.size, C.byref(n))
        return out[:int(n.value)]

    def sample_gather_positive_begin(self, field, strides):
        """Enqueue the compaction; sample_gather_positive_end() fetches.  Only chain_finish / chain_log in between."""
        sz, sy, sx = (int(s) for s in strides)
        n = _i64(0)
        self._call("nl_sample_gather_positive_begin", field, sz, sy, sx, C.byref(n))
        self._gp_cap = int(n.value)

    def sample_gather_positive_end(self):
        out = np.empty(self._gp_cap, dtype=np.float32)
        n = _i64(0)
        self._call("nl_sample_gather_positive_end", _ptr(out), out.size, C.byref(n))
        return out[:int(n.value)]

    def sample_minmax(self, field, strides):
        sz, sy, sx = (int(s) for s in strides)
        mn, mx, n = _f32(0), _f32(0), _i64(0)
        self._call("nl_sample_minmax", field, sz, sy, sx, C.byref(mn), C.byref(mx), C.byref(n))
        return np.float32(mn.value), np.float32(mx.value), int(n.value)

    def sample_hist(self, field, strides, edges: np.ndarray):
        sz, sy, sx = (int(s) for s in strides)
        e = np.ascontiguousarray(edges, dtype=np.float32)
        counts = np.zeros(e.size - 1, dtype=np.int64)
        self._call("nl_sample_hist", field, sz, sy, sx, _ptr(e), e.size - 1, _ptr(counts))
        return counts

    def sample_range_hist(self, field, strides, nbins=256):
        """sample_minmax + sample_hist in one call (the device forms numpy's float32 bin edges itself).
        Returns (min, max, n_positive, counts, edges, valid): valid 0 = no positive sample, 1 = ok, 2 = range not finite."""
        mn, mx, n, valid = _f32(0), _f32(0), _i64(0), _int(0)
        counts = np.zeros(nbins, np.int64)
        edges = np.zeros(nbins + 1, np.float32)
        sz, sy, sx = (int(s) for s in strides)
        self._call("nl_sample_range_hist", int(field), sz, sy, sx, int(nbins), C.byref(mn), C.byref(mx), C.byref(n),
                   _ptr(counts), _ptr(edges), C.byref(valid))
        return np.float32(mn.value), np.float32(mx.value), int(n.value), counts, edges, int(valid.value)

    def sample_range_hist2(self, field_a, field_b, strides, nbins=256):
        """sample_range_hist of two independent fields in one device round trip: two (min, max, n_positive, counts, edges, valid)."""
        mn, mx, n, valid = np.zeros(2, np.float32), np.zeros(2, np.float32), np.zeros(2, np.int64), np.zeros(2, np.int32)
        counts = np.zeros((2, nbins), np.int64)
        edges = np.zeros((2, nbins + 1), np.float32)
        sz, sy, sx = (int(s) for s in strides)
        self._call("nl_sample_range_hist2", int(field_a), int(field_b), sz, sy, sx, int(nbins), _ptr(mn), _ptr(mx), _ptr(n),
                   _ptr(counts), _ptr(edges), _ptr(valid))
        return tuple((np.float32(mn[k]), np.float32(mx[k]), int(n[k]), counts[k], edges[k], int(valid[k])) for k in range(2))

    def hessian_stats(self, spacing):
        sp = (_f64 * 3)(*[float(s) for s in spacing])
        ma, mf, inf = _f32(0), _f32(0), _int(0)
        self._call("nl_hessian_stats", sp, C.byref(ma), C.byref(mf), C.byref(inf))
        return np.float32(ma.value), np.float32(mf.value), bool(inf.value)

    def set_frob_norm(self, max_abs, max_finite):
        self._call("nl_set_frob_norm", float(max_abs), float(max_finite))

    def vesselness_step(self, gamma_sq, alpha_sq, beta_sq, thr, want_count=True, z0=-1, z1=-1):
        n = _i64(0)
        use = 0 if thr is None else 1
        self._call("nl_vesselness_step", float(np.float32(gamma_sq)), float(np.float32(alpha_sq)),
                   float(np.float32(beta_sq)), use, float(np.float32(0.0 if thr is None else thr)),
                   int(z0), int(z1), C.byref(n) if want_count else None)
        return int(n.value)

    def mask_volume_fused(self, thr) -> int:
        n = _i64(0)
        self._call("nl_mask_volume_fused", float(np.float32(thr)), C.byref(n))
        return int(n.value)

    # ---------------------------------------------------------------- Markers stage
    def tail_enqueue(self, strides, q=1.0):
        """The frame's epilogue (percentile threshold selected on the device, mask, opening, product), enqueued without a wait."""
        self._call("nl_tail_enqueue", int(strides[0]), int(strides[1]), int(strides[2]), float(q))

    def tail_finish(self, commit=True):
        """-> dict(n_samples, a, b, gamma, thr, n_positive) of the epilogue nl_tail_enqueue started; commit: it becomes the frame."""
        n, npos = _i64(0), _i64(0)
        a, b, g, t = _f32(0), _f32(0), _f32(0), _f32(0)
        self._call("nl_tail_finish", 1 if commit else 0, C.byref(n), C.byref(a), C.byref(b), C.byref(g), C.byref(t), C.byref(npos))
        return dict(n_samples=int(n.value), a=np.float32(a.value), b=np.float32(b.value), gamma=np.float32(g.value),
                    thr=np.float32(t.value), n_positive=int(npos.value))

    def mask_volume_dev(self, strides, q=1.0):
        """_mask_volume with the percentile selected on the device -> dict(n_samples, a, b, gamma, thr); n_samples = 0: frame unchanged."""
        n = _i64(0)
        a, b, g, t = _f32(0), _f32(0), _f32(0), _f32(0)
        self._call("nl_mask_volume_dev", int(strides[0]), int(strides[1]), int(strides[2]), float(q), C.byref(n), C.byref(a), C.byref(b),
                   C.byref(g), C.byref(t))
        return dict(n_samples=int(n.value), a=np.float32(a.value), b=np.float32(b.value), gamma=np.float32(g.value), thr=np.float32(t.value))

    def debug_percentile(self, values, q=1.0):
        v = np.ascontiguousarray(values, dtype=np.float32).reshape(-1)
        a, b, t = _f32(0), _f32(0), _f32(0)
        self._call("nl_debug_percentile", _ptr(v), v.size, float(q), C.byref(t), C.byref(a), C.byref(b))
        return np.float32(t.value), np.float32(a.value), np.float32(b.value)

    def markers_begin(self, labels=None, intensity=None):
        """labels: int32 (Z, Y, X) host array or None (device labels of label_run); intensity: host array of any
        supported dtype or None (the resident input)."""
        lab_p, int_p, code = None, None, 0
        keep = []
        if labels is not None:
            a = np.ascontiguousarray(labels, dtype=np.int32)
            assert a.shape == self.shape
            keep.append(a); lab_p = _ptr(a)
        if intensity is not None:
            b = np.ascontiguousarray(intensity)
            if b.dtype not in DTYPE_CODES:          # float16, bool, big-endian maps ...: as filter_load / input_load do
                b = b.astype(np.float32)
            assert b.shape == self.shape
            keep.append(b); int_p = _ptr(b); code = DTYPE_CODES[b.dtype]
        self._call("nl_markers_begin", lab_p, int_p, code)

    def markers_distance(self, clamp) -> int:
        n = _i64(0)
        self._call("nl_markers_distance", float(np.float32(clamp)), C.byref(n))
        return int(n.value)

    def markers_log_step(self, wz2, wz0, wy2, wy0, wx2, wx0, s2):
        """One sigma of mocap_marking.py:488-508.  wz2 = wz0 = None: 2-D image (no Z terms)."""
        flat = wz2 is None and wz0 is None
        arrs = [np.ascontiguousarray(w, dtype=np.float64) for w in (wy2, wy0, wx2, wx0)]
        ryx = (arrs[0].size - 1) // 2
        assert all(a.size == arrs[0].size for a in arrs)
        ptr = [a.ctypes.data_as(C.POINTER(_f64)) for a in arrs]
        if flat:
            self._call("nl_markers_log_step", None, None, 0, ptr[0], ptr[1], ptr[2], ptr[3], ryx, float(np.float32(s2)))
            return
        z2, z0 = np.ascontiguousarray(wz2, dtype=np.float64), np.ascontiguousarray(wz0, dtype=np.float64)
        assert z2.size == z0.size
        self._call("nl_markers_log_step", z2.ctypes.data_as(C.POINTER(_f64)), z0.ctypes.data_as(C.POINTER(_f64)), (z2.size - 1) // 2,
                   ptr[0], ptr[1], ptr[2], ptr[3], ryx, float(np.float32(s2)))

    def markers_use_image(self, image=None):
        """use_im='frangi' (mocap_marking.py:675-679): the float32 image the LoG runs on; None = the distance image."""
        if image is None:
            self._call("nl_markers_use_image", None)
            return
        im = np.ascontiguousarray(image, dtype=np.float32)
        if im.size != int(np.prod(self.shape)):
            raise ValueError(f"image shape {im.shape} does not match the context shape {tuple(self.shape)}")
        self._call("nl_markers_use_image", _ptr(im))

    def markers_finish(self, peak_min_distance) -> int:
        n = _i64(0)
        self._call("nl_markers_finish", int(peak_min_distance), C.byref(n))
        return int(n.value)

    def markers_store(self, marker=True, distance=True, border=True):
        m = np.empty(self.shape, np.uint8) if marker else None
        d = np.empty(self.shape, np.float32) if distance else None
        b = np.empty(self.shape, np.uint8) if border else None
        self._call("nl_markers_store", None if m is None else _ptr(m), None if d is None else _ptr(d), None if b is None else _ptr(b))
        return m, d, b

    def skel_pixel_class(self, skel, download=True):
        """networking.py:672-683.  Returns (uint8 pixel classes or None, number of skeleton voxels)."""
        skel = np.ascontiguousarray(skel, dtype=np.int32)
        if skel.size != int(np.prod(self.shape)):
            raise ValueError(f"skeleton shape {skel.shape} does not match the context shape {tuple(self.shape)}")
        out = np.empty(skel.shape, np.uint8) if download else None
        n = _i64(0)
        self._call("nl_skel_pixel_class", _ptr(skel), None if out is None else _ptr(out), C.byref(n))
        return out, int(n.value)

    def skel_branch_labels(self, pixel_class=None):
        """networking.py:758-800.  pixel_class=None: the classes of the previous skel_pixel_class on this context.
        Returns (int32 branch labels, number of branches)."""
        pc = None
        if pixel_class is not None:
            pc = np.ascontiguousarray(pixel_class, dtype=np.uint8)
            if pc.size != int(np.prod(self.shape)):
                raise ValueError(f"pixel_class shape {pc.shape} does not match the context shape {tuple(self.shape)}")
        out = np.empty(self.shape if pc is None else pc.shape, np.int32)
        n = _i64(0)
        self._call("nl_skel_branch_labels", None if pc is None else _ptr(pc), _ptr(out), C.byref(n))
        return out, int(n.value)

    # ---- Network behind the thinning (networking.py:828-851): one frame resident from network_load to network_fetch
    def _network_frame(self, a, what, dtype, like=None):
        """A frame of the context's shape ((1, ny, nx) contexts take (ny, nx) frames too) and of the shape `like` of the frame's
        labels, C-contiguous in `dtype`; integer targets refuse a cast that would change a value."""
        a = np.asarray(a)
        full = tuple(int(s) for s in self.shape)
        if like is not None and a.shape != tuple(like):
            raise ValueError(f"{what} shape {a.shape} does not match the labels' {tuple(like)}")
        if a.shape != full and not (full[0] == 1 and a.shape == full[1:]):
            raise ValueError(f"{what} shape {a.shape} does not match the context shape {full}")
        if a.dtype != dtype and np.dtype(dtype).kind in "iu":
            _refuse_lossy_cast(a, np.dtype(dtype), what)
        return np.ascontiguousarray(a, dtype=dtype)

    def network_load(self, labels, skel_mask, frangi):
        """labels (any integer dtype whose values fit int32), the thinning's mask (bool) and the Frangi frame go up; skel = labels * mask.
        Returns the largest label."""
        labels = self._network_frame(labels, "labels", np.int32)
        mask = np.asarray(skel_mask)
        if mask.dtype != np.bool_:
            mask = mask != 0
        mask = self._network_frame(mask, "skeleton mask", np.bool_, labels.shape).view(np.uint8)
        frangi = self._network_frame(frangi, "frangi frame", np.float32, labels.shape)
        self._network_shape = labels.shape
        n = _i64(0)
        self._call("nl_network_load", _ptr(labels), _ptr(mask), _ptr(frangi), labels.ndim, C.byref(n))
        return int(n.value)

    THIN_COUNTS = ("n_in", "n_out", "outer", "subiters", "rounds", "candidates", "removed")

    def network_load_thin(self, labels, frangi, rounds_per_sync=None):
        """network_load with the mask thinned on the device from labels > 0 (3-D frames).  Returns the largest label."""
        labels = self._network_frame(labels, "labels", np.int32)
        if labels.ndim != 3:
            raise NotImplementedError("the thinning on the device is the 3-D one")
        frangi = self._network_frame(frangi, "frangi frame", np.float32, labels.shape)
        self._network_shape = labels.shape
        n, k = _i64(0), _i64(0)
        self._call("nl_network_load_thin", _ptr(labels), _ptr(frangi), labels.ndim, int(rounds_per_sync or 0), C.byref(n), C.byref(k))
        return int(n.value)

    def thin(self, mask, rounds_per_sync=None):
        """The 3-D thinning of a bool volume of the context's shape -> bool skeleton (skimage.morphology.skeletonize(mask) > 0)."""
        mask = self._network_frame(mask, "mask", np.bool_)
        if mask.ndim != 3:
            raise NotImplementedError("the thinning on the device is the 3-D one")
        out = np.empty(mask.shape, np.bool_)
        self._call("nl_thin", _ptr(mask.view(np.uint8)), _ptr(out.view(np.uint8)), 3, int(rounds_per_sync or 0), None)
        return out

    def network_fetch_mask(self, shape=None):
        """The mask the last thinning on this context left (bool)."""
        out = np.empty(tuple(int(s) for s in self.shape) if shape is None else shape, np.bool_)
        self._call("nl_network_fetch_mask", _ptr(out.view(np.uint8)))
        return out

    def thin_info(self):
        """(dict of the last thinning's seven counts, its stream time in ms)."""
        counts, ms = (_i64 * 7)(), (_f32 * 1)()
        self._call("nl_thin_info", counts, ms)
        return dict(zip(self.THIN_COUNTS, (int(v) for v in counts))), float(ms[0])

    def network_clean_seed(self):
        """networking.py:261-296 and :342-387 -> (voxels zeroed, labels seeded)."""
        a, b = _i64(0), _i64(0)
        self._call("nl_network_clean_seed", C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def network_classes(self):
        """networking.py:839-847 on the resident skeleton -> (skeleton voxels, branches)."""
        a, b = _i64(0), _i64(0)
        self._call("nl_network_classes", C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def network_relabel_load(self, labels, branch):
        """Step 5 alone: labels and branch labels go up.  Returns the largest label."""
        labels = self._network_frame(labels, "labels", np.int32)
        branch = self._network_frame(branch, "branch labels", np.int32, labels.shape)
        self._network_shape = labels.shape
        n = _i64(0)
        self._call("nl_network_relabel_load", _ptr(labels), _ptr(branch), labels.ndim, C.byref(n))
        return int(n.value)

    def network_relabel(self, spacing, scratch_voxels=None):
        """networking.py:485-577 -> (objects with a seed, sum of their box volumes, batches)."""
        sp = np.ascontiguousarray(spacing, dtype=np.float64)
        if sp.size != len(self._network_shape):
            raise ValueError(f"spacing needs {len(self._network_shape)} values")
        a, b, k = _i64(0), _i64(0), _i64(0)
        self._call("nl_network_relabel", sp.ctypes.data_as(C.POINTER(_f64)), int(scratch_voxels or 0), C.byref(a), C.byref(b), C.byref(k))
        return int(a.value), int(b.value), int(k.value)

    def network_fetch(self, branch=True, pixel_class=True, relabelled=True):
        """(branch skeleton labels int32, pixel classes uint8, relabelled uint32), None where not asked for."""
        shape = self._network_shape
        s = np.empty(shape, np.int32) if branch else None
        p = np.empty(shape, np.uint8) if pixel_class else None
        r = np.empty(shape, np.uint32) if relabelled else None
        self._call("nl_network_fetch", _opt(s), _opt(p), _opt(r))
        return s, p, r

    def network_kernel_ms(self):
        ms = (_f32 * 4)()
        self._call("nl_network_kernel_ms", ms)
        return dict(zip(("clean", "seed", "classes", "relabel"), (float(v) for v in ms)))

    def set_ndim(self, ndim: int):
        self._call("nl_set_ndim", int(ndim))

    def log2d_step(self, wy2, wy0, wx2, wx0, s2, first, use_mask=True):
        arrs = [np.ascontiguousarray(w, dtype=np.float64) for w in (wy2, wy0, wx2, wx0)]
        r = (arrs[0].size - 1) // 2
        assert all(a.size == 2 * r + 1 for a in arrs)
        self._call("nl_log2d_step", *[a.ctypes.data_as(C.POINTER(_f64)) for a in arrs], r, float(np.float32(s2)),
                   1 if first else 0, 1 if use_mask else 0)

    def log2d_finish(self) -> int:
        n = _i64(0)
        self._call("nl_log2d_finish", C.byref(n))
        return int(n.value)

    def one_pass_available(self) -> bool:
        return bool(self.info("vesselness_one_pass"))

    def chain_available(self) -> bool:
        """nl_chain_begin's precondition: 3-D, the one-pass walk, and the pair kernel (off for planes of >= 2^30 voxels and with
        NELLIE_HV_RS=0: the synchronous path then runs the one-voxel walk)."""
        return bool(self.info("chain_available"))

    def set_spacing(self, spacing):
        sp = (_f64 * 3)(*[float(s) for s in spacing])
        self._call("nl_set_spacing", sp)

    def vesselness_spec(self, spacing, fsq_lo, fsq_hi, z0=-1, z1=-1):
        """One walk over the Hessian: statistics + vesselness candidates for fsq_min in [fsq_lo, fsq_hi].
        Returns (max_abs, max_frob_sq, any_inf, overflow)."""
        sp = (_f64 * 3)(*[float(s) for s in spacing])
        ma, mf, inf, ovf = _f32(0), _f32(0), _int(0), _int(0)
        self._call("nl_vesselness_spec", sp, float(np.float32(fsq_lo)), float(np.float32(fsq_hi)), int(z0), int(z1),
                   C.byref(ma), C.byref(mf), C.byref(inf), C.byref(ovf))
        return np.float32(ma.value), np.float32(mf.value), bool(inf.value), bool(ovf.value)

    # ---- device-resident threshold chain (include/nellie_amd.h: nl_chain_*)
    def chain_begin(self, n_scales):
        self._call("nl_chain_begin", int(n_scales))
        self._chain_n = int(n_scales)

    def chain_scale(self, spacing, strides, alpha_sq, beta_sq, division, margin, test_scale=1.0, z0=-1, z1=-1):
        sp = (_f64 * 3)(*[float(s) for s in spacing])
        sz, sy, sx = (int(s) for s in strides)
        self._call("nl_chain_scale", sp, sz, sy, sx, float(alpha_sq), float(beta_sq), float(division), float(margin), float(test_scale),
                   int(z0), int(z1))

    # ... with the scales walked out of sigma order (include/nellie_amd.h: nl_chain_begin_unordered)
    def chain_begin_unordered(self, n_scales):
        self._call("nl_chain_begin_unordered", int(n_scales))
        self._chain_n = int(n_scales)

    def chain_sample(self, k, spacing, strides, division, margin, test_scale=1.0):
        sp = (_f64 * 3)(*[float(s) for s in spacing])
        sz, sy, sx = (int(s) for s in strides)
        self._call("nl_chain_sample", int(k), sp, sz, sy, sx, float(division), float(margin), float(test_scale))

    def chain_estimates(self):
        """The forecast h_mask fraction of every scale sampled so far, < 0 where there is none; one short wait."""
        frac = np.full(self._chain_n, -1.0, np.float32)
        self._call("nl_chain_estimates", _ptr(frac), int(frac.size))
        return frac

    def chain_walk(self, k, spacing, strides, alpha_sq, beta_sq, division, z0=-1, z1=-1):
        sp = (_f64 * 3)(*[float(s) for s in spacing])
        sz, sy, sx = (int(s) for s in strides)
        self._call("nl_chain_walk", int(k), sp, sz, sy, sx, float(alpha_sq), float(beta_sq), float(division), int(z0), int(z1))

    def chain_flush(self):
        self._call("nl_chain_flush")

    def chain_finish(self):
        """-> (flags, gamma, max_abs, thr, mask_count) arrays over the scales; flags all zero: the chain's result stands."""
        n = self._chain_n
        flags = np.zeros(n, np.int32)
        gamma, max_abs, thr = np.zeros(n), np.zeros(n), np.zeros(n)
        counts = np.zeros(n, np.int64)
        self._call("nl_chain_finish", _ptr(flags), _ptr(gamma), _ptr(max_abs), _ptr(thr), _ptr(counts))
        return flags, gamma, max_abs, thr, counts

    def chain_log(self, k, which):
        counts, edges = np.zeros(256, np.int64), np.zeros(257, np.float32)
        rng, sc = np.zeros(2, np.float32), np.zeros(8)
        self._call("nl_chain_log", int(k), int(which), _ptr(counts), _ptr(edges), _ptr(rng), _ptr(sc))
        return counts, edges, rng, dict(zip(("fsq_lo", "fsq_hi", "gamma_sq", "fsq_min", "thr_cmp", "max_frob", "tri", "otsu"), sc))

    def vesselness_resolve(self, gamma_sq, alpha_sq, beta_sq, thr) -> bool:
        """hit: False means the bracket missed and vesselness_step must run.  Asynchronous on a hit: the kernel runs
        on the context's side stream, vesselness_count() waits for it and returns the h_mask count."""
        hit = _int(0)
        use = 0 if thr is None else 1
        self._call("nl_vesselness_resolve", float(np.float32(gamma_sq)), float(np.float32(alpha_sq)),
                   float(np.float32(beta_sq)), use, float(np.float32(0.0 if thr is None else thr)),
                   C.byref(hit), None)
        return bool(hit.value)

    def vesselness_count(self) -> int:
        n = _i64(0)
        self._call("nl_vesselness_count", C.byref(n))
        return int(n.value)

    def filter_finish(self, z0=-1, z1=-1) -> int:
        n = _i64(0)
        self._call("nl_filter_finish", int(z0), int(z1), C.byref(n))
        return int(n.value)

    # ---------------------------------------------------------------- Z-slabs
    def remove_edges(self, margin=15) -> int:
        """filtering.py:969-1000 on the resident frame; returns the number of values > 0 left."""
        n = _i64(0)
        self._call("nl_remove_edges", int(margin), C.byref(n))
        return int(n.value)

    def planes_get(self, field, z0, z1):
        out = np.empty((z1 - z0, self.shape[1], self.shape[2]), dtype=np.float32)
        self._call("nl_planes_get", int(field), int(z0), int(z1), _ptr(out))
        return out

    def planes_put(self, field, z0, z1, planes):
        a = np.ascontiguousarray(planes, dtype=np.float32)
        assert a.shape == (z1 - z0, self.shape[1], self.shape[2])
        self._call("nl_planes_put", int(field), int(z0), int(z1), _ptr(a))

    def comm_init(self, world, rank, uid: bytes):
        assert len(uid) == 128
        self._call("nl_comm_init", int(world), int(rank), uid)

    def halo_exchange(self, field, depth):
        self._call("nl_halo_exchange", int(field), int(depth))

    def halo_exchange_at(self, field, offset, depth, run_async=False):
        self._call("nl_halo_exchange_at", int(field), int(offset), int(depth), 1 if run_async else 0)

    def comm_init2(self, world, rank, uid: bytes):
        self._call("nl_comm_init2", int(world), int(rank), uid)

    def allreduce(self, arr: np.ndarray, op: str):
        a = np.ascontiguousarray(arr)
        assert a.dtype in (np.int64, np.float32)
        self._call("nl_allreduce", _ptr(a), a.size, 0 if a.dtype == np.int64 else 1, {"sum": 0, "min": 1, "max": 2}[op])
        return a

    def mask_volume(self, thr):
        self._call("nl_mask_volume", float(np.float32(thr)))

    def filter_store(self, z0=0, z1=None, out=None):
        z1 = self.shape[0] if z1 is None else z1
        if out is None:
            out = np.empty((z1 - z0, self.shape[1], self.shape[2]), dtype=np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous
        self._call("nl_filter_store", _ptr(out), z0, z1)
        return out

    def gauss_store(self, z0=0, z1=None):
        z1 = self.shape[0] if z1 is None else z1
        out = np.empty((z1 - z0, self.shape[1], self.shape[2]), dtype=np.float32)
        self._call("nl_gauss_store", _ptr(out), z0, z1)
        return out

    # ---------------------------------------------------------------- frame streaming
    def input_load_async(self, slot, pinned):
        """`pinned`: a PinnedArray, or a numpy view into registered (page-locked) memory."""
        if isinstance(pinned, np.ndarray):
            self._call("nl_input_load_async", int(slot), _ptr(pinned), DTYPE_CODES[pinned.dtype])
        else:
            self._call("nl_input_load_async", int(slot), pinned._p, DTYPE_CODES[pinned.dtype])

    def input_select(self, slot):
        self._call("nl_input_select", int(slot))

    def input_wait(self, slot):
        """Block until the upload into that slot has arrived (copy-thread call)."""
        self._call("nl_input_wait", int(slot))

    def outputs_stage(self, with_labels=True):
        self._call("nl_outputs_stage", 1 if with_labels else 0)

    def outputs_fetch_async(self, frangi, labels=None):
        def ptr(a):
            if a is None:
                return None
            return _ptr(a) if isinstance(a, np.ndarray) else a._p
        self._call("nl_outputs_fetch_async", ptr(frangi), ptr(labels))

    def outputs_wait(self):
        self._call("nl_outputs_wait")

    def outputs_pack(self, with_labels=True) -> int:
        """Pack the frame's products on the device (see include/nellie_amd.h); bytes of the blob, 0 if it does not pack."""
        n = _i64(0)
        self._call("nl_outputs_pack", 1 if with_labels else 0, C.byref(n))
        return int(n.value)

    def outputs_pack_with_label(self, on=True):
        """label_run() then enqueues the frame's outputs_pack(True) under its own wait; the outputs_pack(True) that follows returns at once."""
        self._call("nl_outputs_pack_with_label", 1 if on else 0)

    def outputs_fetch_packed_async(self, pinned, nbytes):
        self._call("nl_outputs_fetch_packed_async", pinned._p if hasattr(pinned, "_p") else _ptr(pinned), int(nbytes))

    # ---------------------------------------------------------------- Label
    def label_load_frangi(self, frangi: np.ndarray, z0=0, z1=None):
        z1 = self.shape[0] if z1 is None else z1
        a = np.ascontiguousarray(frangi, dtype=np.float32)
        assert a.shape == (z1 - z0, self.shape[1], self.shape[2])
        self._call("nl_label_load_frangi", _ptr(a), z0, z1)

    def label_intensity_mask(self, original: np.ndarray, thresh, z0=None, z1=None):
        """frangi *= (original > thresh); z0, z1: only those planes, `original` holding exactly them.  A float `thresh` is
        compared in float64; an int one (Label._effective_threshold: a 64-bit integer image) as integers of the image's type."""
        a = np.ascontiguousarray(original)
        if a.dtype not in DTYPE_CODES:
            a = a.astype(np.float64)
        if isinstance(thresh, int) and not isinstance(thresh, bool):
            if a.dtype not in (np.uint64, np.int64) or not np.iinfo(a.dtype).min <= thresh <= np.iinfo(a.dtype).max:
                raise ValueError(f"an integer threshold must be of the image's own 64-bit integer type, got {thresh} for {a.dtype}")
            z0 = 0 if z0 is None else int(z0)
            z1 = self.shape[0] if z1 is None else int(z1)
            assert a.shape == (z1 - z0,) + tuple(self.shape[1:])
            self._call("nl_label_intensity_mask_int", _ptr(a), DTYPE_CODES[a.dtype], thresh - (1 << 64) if thresh >= 1 << 63 else thresh, z0, z1)
            return
        if z0 is None and z1 is None:
            assert a.shape == self.shape
            self._call("nl_label_intensity_mask", _ptr(a), DTYPE_CODES[a.dtype], float(thresh))
            return
        z0 = 0 if z0 is None else int(z0)
        z1 = self.shape[0] if z1 is None else int(z1)
        assert a.shape == (z1 - z0,) + tuple(self.shape[1:])
        self._call("nl_label_intensity_mask_planes", _ptr(a), DTYPE_CODES[a.dtype], float(thresh), z0, z1)

    def flat_sample_gather(self, field, offset, step):
        n = _i64(0)
        self._call("nl_flat_sample_gather", field, int(offset), int(step), None, 0, C.byref(n))
        out = np.empty(int(n.value), dtype=np.float32)
        if out.size:
            self._call("nl_flat_sample_gather", field, int(offset), int(step), _ptr(out), out.size, C.byref(n))
        return out

    def flat_sample_gather_positive(self, field, offset, step):
        n = _i64(0)
        self._call("nl_flat_sample_gather", field, int(offset), int(step), None, 0, C.byref(n))
        out = np.empty(int(n.value), dtype=np.float32)
        if out.size:
            self._call("nl_flat_sample_gather_positive", field, int(offset), int(step), _ptr(out), out.size, C.byref(n))
        return out[:int(n.value)]

    def label_run(self, thr, min_area, fill_holes=True) -> int:
        n = _i64(0)
        has = 0 if thr is None else 1
        self._call("nl_label_run", has, float(np.float32(0.0 if thr is None else thr)), int(min_area),
                   1 if fill_holes else 0, C.byref(n))
        return int(n.value)

    def label_pack(self, thr):
        has = 0 if thr is None else 1
        self._call("nl_label_pack", has, float(np.float32(0.0 if thr is None else thr)))

    def label_bits_get(self, row0, nrows):
        out = np.empty((nrows, (self.shape[2] + 63) // 64), dtype=np.uint64)
        self._call("nl_label_bits_get", int(row0), int(nrows), _ptr(out))
        return out

    def label_bits_put(self, row0, words):
        a = np.ascontiguousarray(words, dtype=np.uint64)
        self._call("nl_label_bits_put", int(row0), a.shape[0], _ptr(a))

    def label_bits_allgather(self, slab_plane0):
        a = np.ascontiguousarray(slab_plane0, dtype=np.int64)
        self._call("nl_label_bits_allgather", _ptr(a))

    def label_run_global(self, min_area, fill_holes=True) -> int:
        n = _i64(0)
        self._call("nl_label_run_global", int(min_area), 1 if fill_holes else 0, C.byref(n))
        return int(n.value)

    # ---- Z-slab Label without replication (include/nellie_amd.h "Label on Z-slabs WITHOUT replication") ----
    def slab_label_pack(self, thr):
        has = thr is not None
        self._call("nl_slab_label_pack", 1 if has else 0, float(np.float32(thr)) if has else 0.0)

    def slab_bits_get(self, which, plane):
        words = self.shape[1] * ((self.shape[2] + 63) // 64)
        out = np.empty(words, np.uint64)
        self._call("nl_slab_bits_get", int(which), int(plane), _ptr(out))
        return out

    def slab_bits_put(self, which, plane, words):
        a = np.ascontiguousarray(words, dtype=np.uint64)
        self._call("nl_slab_bits_put", int(which), int(plane), _ptr(a))

    def slab_bits_exchange(self, which):
        self._call("nl_slab_bits_exchange", int(which))

    SLAB_BLOCK_INTS = 16384

    def slab_phase(self, phase, gather_world=0):
        """One phase of the slab protocol up to its tables (nl_slab_phase): -> list of int32 blobs, this rank's only
        (gather_world = 0) or every rank's, all-gathered on the device (gather_world = the communicator's size)."""
        nb = int(gather_world) if gather_world else 1
        block = self.SLAB_BLOCK_INTS
        need, nruns = _i64(0), _i64(0)
        out = np.empty(nb * block, np.int32)
        self._call("nl_slab_phase", int(phase), 1 if gather_world else 0, block, _ptr(out), C.byref(need), C.byref(nruns))
        if need.value > block:                       # rare: tables beyond 64 KiB -- fetch again in larger blocks, nothing is recomputed
            block = int(need.value) + 1024
            out = np.empty(nb * block, np.int32)
            self._call("nl_slab_phase", -1, 1 if gather_world else 0, block, _ptr(out), C.byref(need), C.byref(nruns))
        self.slab_nruns = int(nruns.value)
        return [out[r * block:r * block + int(out[r * block + 4])] for r in range(nb)]

    def slab_patch(self, roots, values):
        r = np.ascontiguousarray(roots, dtype=np.int32)
        v = np.ascontiguousarray(values, dtype=np.int32)
        assert r.size == v.size
        if r.size:
            self._call("nl_slab_patch", r.size, _ptr(r), _ptr(v))

    def slab_apply(self, min_area=0):
        self._call("nl_slab_apply", int(min_area))

    def slab_majority(self):
        self._call("nl_slab_majority")

    def slab_number(self, clear, select):
        """-> (trees this rank numbers, 1-based local rank of every tree of `select`)"""
        c = np.ascontiguousarray(clear, dtype=np.int32)
        s_ = np.ascontiguousarray(select, dtype=np.int32)
        n = _i64(0)
        ids = np.empty(s_.size, np.int32)
        self._call("nl_slab_number", c.size, _ptr(c) if c.size else None, s_.size, _ptr(s_) if s_.size else None, C.byref(n),
                   _ptr(ids) if s_.size else None)
        return int(n.value), ids

    def slab_paint(self, base, roots, labels):
        r = np.ascontiguousarray(roots, dtype=np.int32)
        v = np.ascontiguousarray(labels, dtype=np.int32)
        assert r.size == v.size
        self._call("nl_slab_paint", int(base), r.size, _ptr(r) if r.size else None, _ptr(v) if v.size else None)

    def allgather_bytes(self, data: bytes, max_bytes: int, world: int):
        """Variable-size all-gather over RCCL: the list of every rank's bytes."""
        send = np.frombuffer(data, dtype=np.uint8) if len(data) else np.zeros(0, np.uint8)
        recv = np.empty(int(max_bytes) * int(world), np.uint8)
        sizes = np.zeros(int(world), np.int64)
        self._call("nl_allgather_bytes", _ptr(send) if send.size else None, send.size, _ptr(recv), int(max_bytes), _ptr(sizes))
        return [recv[r * max_bytes:r * max_bytes + int(sizes[r])].tobytes() for r in range(int(world))]

    def positive_samples_world(self, field, mode, a, b, c, block_items, world):
        """Every rank's positive samples (mode 0: lattice strides a, b, c; mode 1: flat offset a, step b), gathered on the device."""
        cap = int(block_items) * int(world)
        out = np.empty(max(cap, 1), np.float32)
        counts = np.zeros(int(world), np.int64)
        self._call("nl_positive_samples_world", int(field), int(mode), int(a), int(b), int(c), int(block_items), _ptr(out), cap, _ptr(counts))
        return out[:int(counts.sum())]

    def allgather_var(self, arr: np.ndarray, world: int):
        """Variable-size all-gather over RCCL of one array per rank (same dtype everywhere): the list of every rank's array."""
        a = np.ascontiguousarray(arr)
        recv, stride = C.c_void_p(), C.c_int64(0)
        sizes = np.zeros(int(world), np.int64)
        self._call("nl_allgather_var", _ptr(a) if a.size else None, a.nbytes, C.byref(recv), C.byref(stride), _ptr(sizes))
        blob = np.ctypeslib.as_array(C.cast(recv, C.POINTER(C.c_uint8)), shape=(int(stride.value) * int(world),))
        st = int(stride.value)
        return [blob[r * st:r * st + int(sizes[r])].view(a.dtype).copy() for r in range(int(world))]

    def comm_fuse(self, on=True):
        self._call("nl_comm_fuse", 1 if on else 0)

    def label_store(self, z0=0, z1=None, out=None):
        z1 = self.shape[0] if z1 is None else z1
        if out is None:
            out = np.empty((z1 - z0, self.shape[1], self.shape[2]), dtype=np.int32)
        assert out.dtype == np.int32 and out.flags.c_contiguous
        self._call("nl_label_store", _ptr(out), z0, z1)
        return out

    def debug_eig_frangi(self, h6, alpha_sq=0.5, beta_sq=0.5, gamma_sq=1.0, impl=0):
        h = np.ascontiguousarray(h6, dtype=np.float32)
        out = np.empty((h.shape[0], 4), dtype=np.float32)
        self._call("nl_debug_eig_frangi", _ptr(h), h.shape[0], int(impl), float(np.float32(alpha_sq)),
                   float(np.float32(beta_sq)), float(np.float32(gamma_sq)), _ptr(out))
        return out

    # ---------------------------------------------------------------- timing
    def timer_begin(self):
        self._call("nl_timer_begin")

    def timer_end_ms(self) -> float:
        ms = _f32(0)
        self._call("nl_timer_end_ms", C.byref(ms))
        return float(ms.value)

    def info(self, key: str) -> float:
        v = _f64(0)
        if self.lib.cdll.nl_ctx_info(self._h, key.encode(), C.byref(v)) != NL_OK:
            raise KeyError(key)
        return float(v.value)

    def prof_enable(self, on=True):
        self.lib.cdll.nl_prof_enable(self._h, 1 if on else 0)

    def prof_reset(self):
        self.lib.cdll.nl_prof_reset(self._h)

    def prof_get(self, name: str):
        ms, k = _f64(0), _i64(0)
        self.lib.cdll.nl_prof_get(self._h, name.encode(), C.byref(ms), C.byref(k))
        return float(ms.value), int(k.value)


class Tracker(_Handle):
    """Device state of Hu-moment tracking for one T stack (include/nellie_amd.h nl_track_*): the features of the last two
    frames stay on the device, so matching a frame against the one before uploads nothing."""

    _destroy, _noun = "nl_track_destroy", "tracker"

    def __init__(self, shape, spacing, device=0):
        self.ndim, self.shape, (nz, ny, nx), sp = _frame_geometry("tracking frames", spacing, shape=shape)
        self.nh = 6 if self.ndim == 2 else 18
        self._create("nl_track_create", int(device), self.ndim, nz, ny, nx, _ptr(sp))
        self.n = [0, 0]                                   # markers of the last frame, of the one before

    def frame(self, intensity, frangi, distance, marker) -> int:
        marker = np.asarray(marker)
        if marker.dtype != np.uint8:
            marker = marker > 0
        i, f, d, m = (_frame_array(a, self.shape, "frame", "tracker", dt, ValueError)
                      for a, dt in ((intensity, None), (frangi, np.float32), (distance, np.float32), (marker, np.uint8)))
        n = _i64(0)
        self._call("nl_track_frame", _ptr(i), DTYPE_CODES[i.dtype], _ptr(f), _ptr(d), _ptr(m), C.byref(n))
        self.n = [int(n.value), self.n[0]]
        return self.n[0]

    def features(self, which=0):
        n = self.n[which]
        coords = np.zeros((n, self.ndim), np.int64)
        stats = np.zeros((n, 4), np.float32)
        hu = np.zeros((n, self.nh), np.float64)
        self._call("nl_track_features", int(which), _ptr(coords), _ptr(stats), _ptr(hu))
        return coords, stats, hu

    def match(self, mode, max_distance, full=False):
        """(row_idx, row_cost, col_idx, col_cost[, float16 cost matrix]) of the last frame against the one before"""
        n_post, n_pre = self.n
        ri, rc = np.full(n_post, -1, np.int32), np.full(n_post, np.inf, np.float32)
        ci, cc = np.full(n_pre, -1, np.int32), np.full(n_pre, np.inf, np.float32)
        m = np.full((n_post, n_pre), np.inf, np.float16) if full else None
        self._call("nl_track_match", 0 if mode == "dense" else 1, float(max_distance), _ptr(ri), _ptr(rc), _ptr(ci), _ptr(cc), _opt(m))
        return (ri, rc, ci, cc, m) if full else (ri, rc, ci, cc)


class FlowField(_Handle):
    """Device state of flow-vector interpolation (include/nellie_amd.h nl_flow_*): the flow rows of one time point and direction,
    binned into a grid of cells of edge r, stay on the device until the next load()."""

    _destroy, _noun = "nl_flow_destroy", "flow field"

    def __init__(self, ndim, spacing, r, device=0):
        self.ndim, _, _, sp = _frame_geometry("flow fields", spacing, ndim=ndim)
        self._create("nl_flow_create", int(device), self.ndim, _ptr(sp), float(r))
        self.n_rows = 0

    def load(self, coords, vectors, costs):
        """check coordinates (n, ndim), vectors (n, ndim) and costs (n) of one time point and direction"""
        c = np.ascontiguousarray(coords, dtype=np.float64).reshape(-1, self.ndim)
        v = np.ascontiguousarray(vectors, dtype=np.float64).reshape(-1, self.ndim)
        k = np.ascontiguousarray(costs, dtype=np.float64).reshape(-1)
        if not (len(c) == len(v) == len(k)):
            raise ValueError(f"coords, vectors and costs disagree in length: {len(c)}, {len(v)}, {len(k)}")
        self._call("nl_flow_load", _ptr(c), _ptr(v), _ptr(k), len(c))
        self.n_rows = len(c)

    def interpolate(self, queries):
        """(vectors (n, ndim) float64 with NaN rows where no flow row is within r, number of rows that found one)"""
        q = np.ascontiguousarray(queries, dtype=np.float64).reshape(-1, self.ndim)
        out = np.empty((len(q), self.ndim), np.float64)
        found = _i64(0)
        self._call("nl_flow_interpolate", _ptr(q), len(q), _ptr(out), C.byref(found))
        return out, int(found.value)

    def kernel_ms(self) -> float:
        return _kernel_ms(self, "nl_flow_kernel_ms")

    def grid(self) -> dict:
        """the plan of the loaded rows as the device holds it: dims (3,), ncell, cell_edge (3,) in um (0 where the plan resolves
        nothing), max_cells (the budget the plan was given) and fullest (rows in the fullest cell); all 0 with no rows loaded"""
        dims, edge = np.zeros(3, np.int32), np.zeros(3, np.float64)
        ncell, max_cells, fullest = _i64(0), _i64(0), _i64(0)
        self._call("nl_flow_grid_info", _ptr(dims), C.byref(ncell), _ptr(edge), C.byref(max_cells), C.byref(fullest))
        return dict(dims=tuple(int(d) for d in dims), ncell=int(ncell.value), cell_edge=tuple(float(e) for e in edge),
                    max_cells=int(max_cells.value), fullest=int(fullest.value))


class Reassigner(_Handle):
    """Device state of voxel reassignment for one label stack (include/nellie_amd.h nl_reassign_*): the last two frames stay on
    the device -- mask, labelled voxels, labels and reassigned labels -- so a frame is uploaded once and only the reassigned
    labels of the labelled voxels (and the best pairs, when asked for) come back."""

    _destroy, _noun = "nl_reassign_destroy", "reassigner"

    def __init__(self, shape, spacing, r, device=0):
        self.ndim, self.shape, (nz, ny, nx), sp = _frame_geometry("label frames", spacing, shape=shape)
        self._create("nl_reassign_create", int(device), self.ndim, nz, ny, nx, _ptr(sp), float(r))
        self.n = [0, 0]                                   # labelled voxels of the last frame, of the one before

    def frame(self, branch, obj, seed=False) -> int:
        """uploads the next frame's labels; returns its number of labelled voxels (branch > 0 | obj > 0)"""
        b, o = (_frame_array(a, self.shape, "frame", "reassigner", np.int32) for a in (branch, obj))
        n = _i64(0)
        self._call("nl_reassign_frame", _ptr(b), _ptr(o), 1 if seed else 0, C.byref(n))
        self.n = [int(n.value), self.n[0]]
        return self.n[0]

    def pair(self, flow_fw=None, flow_bw=None) -> int:
        """matches the last two frames with the rows loaded in the two FlowFields (None: no candidates of that direction);
        returns the number of candidates"""
        n = _i64(0)
        self._call("nl_reassign_pair", flow_fw._h if flow_fw is not None else None, flow_bw._h if flow_bw is not None else None,
                   C.byref(n))
        return int(n.value)

    def fetch(self, which=0, voxels=True, labels=True, best=False):
        """(linear voxel indices, reassigned branch labels, reassigned object labels, best-pair source ranks) of a frame, None
        for what was not asked for"""
        n = self.n[which]
        vox = np.empty(n, np.int64) if voxels else None
        rb = np.empty(n, np.int32) if labels else None
        ro = np.empty(n, np.int32) if labels else None
        bs = np.empty(n, np.int32) if best else None
        self._call("nl_reassign_fetch", int(which), _opt(vox), _opt(rb), _opt(ro), _opt(bs))
        return vox, rb, ro, bs

    def kernel_ms(self) -> float:
        return _kernel_ms(self, "nl_reassign_kernel_ms")


class LabelTrackSet(_TimedParts, _Handle):
    """Device state of the voxel tracks of a label stack (include/nellie_amd.h nl_tracks_*): `mask_slots` frame masks which the
    caller keeps resident, the seeds, the coordinates of a run and its rows.  A run is seed(), begin(), the backward step()s, the
    forward step()s, filter() for every frame with rows, finish(), fetch()."""

    _destroy, _noun = "nl_tracks_destroy", "track set"
    PARTS, _ms_symbol = ("mask", "seed", "flow", "step", "filter", "compact"), "nl_tracks_kernel_ms"

    def __init__(self, shape, mask_slots=1, device=0):
        self.ndim, self.shape, (nz, ny, nx), _ = _frame_geometry("label frames", (1.0,) * len(shape), shape=shape)
        self.mask_slots = int(mask_slots)
        self._create("nl_tracks_create", int(device), self.ndim, nz, ny, nx, self.mask_slots)
        self.n_seeds = self.n_rows = 0

    def _labels(self, labels):
        return _frame_array(labels, self.shape, "label frame", "track set", np.int32)

    def mask(self, slot, labels):
        """the labels > 0 mask of a frame into a slot"""
        self._call("nl_tracks_mask", int(slot), _ptr(self._labels(labels)))

    def seed(self, slot, labels=None, label=None, skip=1) -> int:
        """every skip-th voxel, in raster order, of the slot's mask or (label given, with the start frame in `labels`) of
        labels == label; a frame given in `labels` also becomes the slot's mask.  Returns the number of seeds."""
        lab = None if labels is None else self._labels(labels)
        n = _i64(0)
        self._call("nl_tracks_seed", int(slot), _opt(lab), 0 if label is None else 1, 0 if label is None else int(label), int(skip), C.byref(n))
        self.n_seeds = int(n.value)
        return self.n_seeds

    def begin(self, fw_steps, bw_steps, id0=0):
        self._call("nl_tracks_begin", int(fw_steps), int(bw_steps), int(id0))

    def step(self, flow, backward, first, frame_from, frame_to) -> int:
        """one frame of a direction with the rows loaded in the FlowField `flow` (None: the frame has none); returns the number of
        rows it emitted"""
        n = _i64(0)
        self._call("nl_tracks_step", flow._h if flow is not None else None, 1 if backward else 0, 1 if first else 0, int(frame_from),
                   int(frame_to), C.byref(n))
        return int(n.value)

    def filter(self, frame, slot):
        """the final filter for the rows of one frame against the mask in `slot` (None: the frame is outside the stack)"""
        self._call("nl_tracks_filter", int(frame), -1 if slot is None else int(slot))

    def finish(self) -> int:
        n = _i64(0)
        self._call("nl_tracks_finish", C.byref(n))
        self.n_rows = int(n.value)
        return self.n_rows

    def fetch(self) -> np.ndarray:
        """the surviving rows [id, frame, (z,) y, x], (n_rows, 2 + ndim) float64"""
        rows = np.empty((self.n_rows, 2 + self.ndim), np.float64)
        self._call("nl_tracks_fetch", _ptr(rows))
        return rows


class Overlay(_TimedParts, _Handle):
    """Device state of the analysis overlay for one frame shape (include/nellie_amd.h nl_overlay_*): the mask and rows of the
    loaded label frame, the rows' groups, their values and the painted frame.  load(), groups() or groups_csr(), values() or
    values_direct(), paint(), fetch_values() / fetch_frame(); what an earlier call left stays until load() replaces the frame."""

    _destroy, _noun = "nl_overlay_destroy", "overlay"
    PARTS, _ms_symbol = ("load", "values", "paint"), "nl_overlay_kernel_ms"
    KINDS = {np.dtype(np.float64): 0, np.dtype(np.float32): 1, np.dtype(np.uint64): 2}

    def __init__(self, shape, device=0):
        self.ndim, self.shape, (nz, ny, nx), _ = _frame_geometry("label frames", (1.0,) * len(shape), shape=shape)
        self._create("nl_overlay_create", int(device), self.ndim, nz, ny, nx)
        self.n_rows = None
        self.painted = None

    def load(self, labels) -> int:
        """the label frame; returns V, the number of voxels with label > 0: the rows, in raster order"""
        lab = _frame_array(labels, self.shape, "label frame", "overlay", np.int32)
        self.n_rows = self.painted = None
        n = _i64(0)
        self._call("nl_overlay_load", _ptr(lab), C.byref(n))
        self.n_rows = int(n.value)
        return self.n_rows

    def _rows(self):
        if self.n_rows is None:
            raise NellieHipError(NL_ESTATE, "the overlay holds no frame")
        return self.n_rows

    def groups(self, group):
        """one group index per row, -1 for none"""
        g = np.asarray(group)
        if g.shape != (self._rows(),):
            raise ValueError(f"{g.shape} groups for {self.n_rows} rows")
        if g.dtype != np.int32:
            _refuse_lossy_cast(g, np.dtype(np.int32), "groups")
        self._call("nl_overlay_groups", _ptr(np.ascontiguousarray(g, dtype=np.int32)), None, None, 0)

    def groups_csr(self, offsets, idx):
        """row r has the groups idx[offsets[r] : offsets[r + 1]], in any order, repeats allowed"""
        off, val = np.asarray(offsets), np.asarray(idx)
        if off.shape != (self._rows() + 1,) or val.ndim != 1:
            raise ValueError(f"{off.shape} offsets for {self.n_rows} rows")
        for a, dtype, what in ((off, np.int64, "offsets"), (val, np.int32, "group indices")):
            if a.dtype != dtype:
                _refuse_lossy_cast(a, np.dtype(dtype), what)
        self._call("nl_overlay_groups", None, _ptr(np.ascontiguousarray(off, dtype=np.int64)), _ptr(np.ascontiguousarray(val, dtype=np.int32)), val.size)

    def values(self, attr, pairwise=False):
        """the column by group index (float64, more entries than the largest group index): every row gets the mean over its groups;
        `pairwise`: the sum follows np.sum over a contiguous column instead of one add per entry"""
        a = np.ascontiguousarray(attr, dtype=np.float64)
        if a.ndim != 1:
            raise ValueError("the column must be 1-D")
        self._call("nl_overlay_values", _ptr(a), a.size, 0, 1 if pairwise else 0)

    def values_direct(self, values):
        """the rows' values themselves (float64, one per row)"""
        a = np.ascontiguousarray(values, dtype=np.float64)
        if a.shape != (self._rows(),):
            raise ValueError(f"{a.shape} values for {self.n_rows} rows")
        self._call("nl_overlay_values", _ptr(a), a.size, 1, 0)

    def paint(self, dtype=np.float64):
        """the dense frame on the device: float64 or float32 (NaN off the labelled voxels) or uint64 labels (0 there)"""
        dtype = np.dtype(dtype)
        if dtype not in self.KINDS:
            raise TypeError(f"an overlay is painted as float64, float32 or uint64, not {dtype}")
        self.painted = None
        self._call("nl_overlay_paint", self.KINDS[dtype])
        self.painted = dtype

    def fetch_values(self) -> np.ndarray:
        out = np.empty(self._rows(), np.float64)
        self._call("nl_overlay_fetch_values", _ptr(out))
        return out

    def fetch_frame(self, out=None) -> np.ndarray:
        """the painted frame; `out`: a C-contiguous writeable array of the frame's shape and the painted dtype that receives it"""
        if self.painted is None:
            raise NellieHipError(NL_ESTATE, "the overlay holds no painted frame")
        if out is None:
            out = np.empty(self.shape, self.painted)
        if not (isinstance(out, np.ndarray) and out.shape == self.shape and out.dtype == self.painted and out.flags.c_contiguous and out.flags.writeable):
            raise ValueError(f"out must be a C-contiguous writeable {self.painted} array of shape {self.shape}")
        self._call("nl_overlay_fetch_frame", _ptr(out))
        return out


class Transitions(_TimedParts, _Handle):
    """Device state of the label transition counts for one frame shape (include/nellie_amd.h nl_trans_*): two label frames -- frame()
    makes the resident "next" frame "prev" and uploads a new "next" --, the counting table of a pair and the relabelled frame.
    frame(), frame(), count(), then relabel() for the pair's later frame; count() again after each further frame()."""

    _destroy, _noun = "nl_trans_destroy", "transitions object"
    PARTS, _ms_symbol = ("clear", "count", "compact", "relabel"), "nl_trans_kernel_ms"
    ROWS_PER_LAUNCH = 1 << 24             # rows of one upload and launch: at most 768 MB of coordinates are resident
    SLOT_BYTES = 17                       # of device memory per slot: key, count, and the mask and scan words of the compaction
    COORD_DTYPES = (np.dtype(np.uint16), np.dtype(np.uint32), np.dtype(np.uint64))

    def __init__(self, shape, device=0):
        self.ndim, self.shape, (nz, ny, nx), _ = _frame_geometry("label frames", (1.0,) * len(shape), shape=shape)
        self.device = int(device)
        self._create("nl_trans_create", self.device, self.ndim, nz, ny, nx)
        self.frames = 0                   # frames uploaded so far
        self.resident = 0                 # frames the device holds: 0, 1 ("next") or 2
        self.regrown = self.table_slots = self.n_heads = self.n_rows = 0      # of the last count()

    def frame(self, labels):
        """the next label frame: int32 and int64 go up as they are, other integer types as int32 or (when a value needs it) int64"""
        a = np.asarray(labels)
        if a.dtype not in (np.int32, np.int64):
            wide = a.dtype.kind in "iu" and a.size > 0 and not (-2 ** 31 <= int(a.min()) and int(a.max()) < 2 ** 31)
            a = _frame_array(a, self.shape, "label frame", "transitions object", np.int64 if wide else np.int32)
        a = _frame_array(a, self.shape, "label frame", "transitions object")
        try:
            self._call("nl_trans_frame", _ptr(a), DTYPE_CODES[a.dtype])
        except BaseException:
            self.resident = min(self.resident, 1)        # a failed upload costs the "prev" slot it was written into; "next" stays
            raise
        self.frames += 1
        self.resident = min(self.resident + 1, 2)

    def _coords(self, prev, next):
        """both ends as (n, ndim) rows of one of COORD_DTYPES; other integer types become uint64, a negative coordinate is outside the frame"""
        ends = [np.asarray(a) for a in (prev, next)]
        for a in ends:
            if a.ndim != 2 or a.shape[1] != self.ndim or a.shape != ends[0].shape:
                raise ValueError(f"match coordinates must be two (n, {self.ndim}) arrays, got {ends[0].shape} and {ends[1].shape}")
            if a.dtype.kind not in "iu":
                raise TypeError(f"match coordinates of dtype {a.dtype}")
        dtype = ends[0].dtype if ends[0].dtype == ends[1].dtype and ends[0].dtype in self.COORD_DTYPES else np.dtype(np.uint64)
        if any(a.dtype.kind == "i" for a in ends):
            neg = np.nonzero((ends[0] < 0).any(axis=1) | (ends[1] < 0).any(axis=1))[0]
            if len(neg):
                raise ValueError(f"row {int(neg[0])} holds a coordinate outside the frame {self.shape}")
        return [a if a.dtype == dtype else a.astype(dtype) for a in ends], dtype

    def default_slots(self, n_rows) -> int:
        """a power of two of at least twice the rows (no more of them can be kept), as far as half the free device memory holds it"""
        slots = 64
        while slots < 2 * n_rows:
            slots *= 2
        free, _ = self.lib.device_mem_info(self.device)
        while slots > 64 and slots * self.SLOT_BYTES > free // 2:
            slots //= 2
        return slots

    def count(self, prev, next, table_slots=None, rows_per_launch=None):
        """the matches (prev: coordinates in the "prev" frame, next: in the "next" frame) -> ((E, 3) int64 rows (src, dst, count) in
        lexicographic order, n_dropped).  table_slots: the slots of the counting table to begin with (a power of two; None:
        default_slots); a table that turns out too small is doubled and the pair repeated, `regrown` times.  rows_per_launch: rows
        per upload and launch (None: ROWS_PER_LAUNCH); every chunk counts into the same table."""
        (p, q), dtype = self._coords(prev, next)
        n = len(p)
        step = self.ROWS_PER_LAUNCH if rows_per_launch is None else int(rows_per_launch)
        if step < 1:
            raise ValueError("rows_per_launch must be at least 1")
        self.regrown = self.n_heads = 0
        self.n_rows = n
        self.table_slots = 0
        if n == 0:
            return np.zeros((0, 3), np.int64), 0
        if self.resident < 2:
            raise NellieHipError(NL_ESTATE, "the transitions object holds fewer than two label frames")
        slots = self.default_slots(n) if table_slots is None else int(table_slots)
        over, m, dropped, heads = _int(0), _i64(0), _i64(0), _i64(0)
        while True:
            self._call("nl_trans_begin", slots)
            over.value = 0
            for r0 in range(0, n, step):
                a, b = np.ascontiguousarray(p[r0:r0 + step]), np.ascontiguousarray(q[r0:r0 + step])
                self._call("nl_trans_count", _ptr(a), _ptr(b), DTYPE_CODES[dtype], len(a), r0, C.byref(over))
                if over.value:
                    break
            if not over.value:
                self._call("nl_trans_finish", C.byref(m), C.byref(dropped), C.byref(heads), C.byref(over))
            if not over.value:
                break
            slots *= 2
            self.regrown += 1
        self.table_slots, self.n_heads = slots, int(heads.value)
        ent = np.empty((int(m.value), 2), np.uint64)
        self._call("nl_trans_fetch", _ptr(ent))
        ent = ent[np.argsort(ent[:, 0], kind="stable")]          # slot order depends on arrival; uint64 key order is (src, dst) order
        table = np.stack([ent[:, 0] >> np.uint64(32), ent[:, 0] & np.uint64(0xFFFFFFFF), ent[:, 1]], axis=1).astype(np.int64)
        return table, int(dropped.value)

    def label_max(self) -> int:
        """the largest label of the "next" frame"""
        top = _i64(0)
        self._call("nl_trans_label_max", C.byref(top))
        return int(top.value)

    def relabel(self, lut, out=None) -> np.ndarray:
        """the "next" frame with every label b in (0, len(lut)) replaced by lut[b] and everything else 0, int32; `out`: a C-contiguous
        writeable int32 array of the frame's shape (a memmap, say) that receives it"""
        lut = np.asarray(lut)
        if lut.ndim != 1:
            raise ValueError("the label table must be 1-D")
        if lut.dtype != np.int32:
            _refuse_lossy_cast(lut, np.dtype(np.int32), "label table")
        lut = np.ascontiguousarray(lut, dtype=np.int32)
        if out is None:
            out = np.empty(self.shape, np.int32)
        if not (isinstance(out, np.ndarray) and out.shape == self.shape and out.dtype == np.int32 and out.flags.c_contiguous and out.flags.writeable):
            raise ValueError(f"out must be a C-contiguous writeable int32 array of shape {self.shape}")
        self._call("nl_trans_relabel", _ptr(lut), lut.size)
        self._call("nl_trans_fetch_frame", _ptr(out))
        return out


class VoxelFeatures(_TimedParts, _Handle):
    """Device state of the voxel level of the hierarchy for one stack (include/nellie_amd.h nl_voxfeat_*): one frame stays on
    the device -- mask, labelled voxels and their values -- while its flow vectors, pivots, motility features and node lists are
    computed; only per-voxel results, the two CSR lists and the node limits come back."""

    PARTS = ("load", "flow", "pivot", "motility", "nodes")
    MOTILITY = ("vec01", "vec12", "linear_vel_vector", "linear_vel", "angular_vel_vector", "angular_vel", "linear_acc", "angular_acc",
                "rel_linear_vel", "rel_angular_vel", "rel_linear_acc", "rel_angular_acc", "rel_directionality")

    _destroy, _noun, _ms_symbol = "nl_voxfeat_destroy", "voxel-feature object", "nl_voxfeat_kernel_ms"

    def __init__(self, shape, spacing, dt, device=0):
        self.ndim, self.shape, (nz, ny, nx), sp = _frame_geometry("frames", spacing, shape=shape)
        self._create("nl_voxfeat_create", int(device), self.ndim, nz, ny, nx, _ptr(sp), float(dt))
        self.n = 0                                        # labelled voxels of the loaded frame
        self.n_nodes = self.n_pairs = 0
        self._dtypes = (np.dtype(np.uint8), np.dtype(np.uint8))

    def _frame_array(self, a, what, dtype=None):
        return _frame_array(a, self.shape, what, "object", dtype)

    def frame(self, comp, branch, raw, structure) -> int:
        """uploads a frame; returns the number of voxels with component label > 0"""
        c, b = self._frame_array(comp, "component label", np.int32), self._frame_array(branch, "branch label", np.int32)
        r, s = self._frame_array(raw, "intensity"), self._frame_array(structure, "structure")
        n = _i64(0)
        self._call("nl_voxfeat_frame", _ptr(c), _ptr(b), _ptr(r), DTYPE_CODES[r.dtype], _ptr(s), DTYPE_CODES[s.dtype], C.byref(n))
        self.n, self._dtypes = int(n.value), (r.dtype, s.dtype)
        self.n_nodes = self.n_pairs = 0
        return self.n

    def fetch_voxels(self):
        """(linear voxel indices, component labels, branch labels (int32), intensity, structure) of the loaded frame"""
        vox, c, b = np.empty(self.n, np.int64), np.empty(self.n, np.int32), np.empty(self.n, np.int32)
        r, s = np.empty(self.n, self._dtypes[0]), np.empty(self.n, self._dtypes[1])
        self._call("nl_voxfeat_fetch_voxels", _ptr(vox), _ptr(c), _ptr(b), _ptr(r), _ptr(s))
        return vox, c, b, r, s

    def motility(self, flow_bw=None, flow_fw=None):
        """the motility features of the loaded frame from the rows loaded in the two FlowFields (None: the direction does not
        exist); returns (voxels with a backward neighbour, with a forward neighbour)"""
        a, b = _i64(0), _i64(0)
        self._call("nl_voxfeat_motility", flow_bw._h if flow_bw is not None else None, flow_fw._h if flow_fw is not None else None,
                   C.byref(a), C.byref(b))
        return int(a.value), int(b.value)

    def fetch_motility(self):
        """{name: float32 array} for every name of MOTILITY"""
        D, A = self.ndim, (3 if self.ndim == 3 else 1)
        widths = (D, D, D, 1, A, 1, 1, 1, 1, 1, 1, 1, 1)
        out = {k: np.empty((self.n, w) if w > 1 else self.n, np.float32) for k, w in zip(self.MOTILITY, widths)}
        ptrs = (_p * len(widths))(*[_ptr(out[k]) for k in self.MOTILITY])
        self._call("nl_voxfeat_fetch_motility", ptrs)
        return out

    def nodes(self, pixel_class, distance):
        """assigns the loaded frame's voxels to the nodes (pixel class > 0) whose radius box holds them; returns (nodes, pairs)"""
        pc = self._frame_array(pixel_class, "pixel class")
        d = np.asarray(distance)
        d = self._frame_array(d, "distance", None if d.dtype in (np.float32, np.float64) else (np.float32 if d.dtype == np.float16 else np.float64))
        m, p = _i64(0), _i64(0)
        self._call("nl_voxfeat_nodes", _ptr(pc), DTYPE_CODES[pc.dtype], _ptr(d), DTYPE_CODES[d.dtype], C.byref(m), C.byref(p))
        self.n_nodes, self.n_pairs = int(m.value), int(p.value)
        return self.n_nodes, self.n_pairs

    def fetch_nodes(self):
        """(limits per axis [(n_nodes, 2) int64] * ndim, (node offsets (n_nodes + 1), voxel ranks), (voxel offsets (n + 1), node
        ranks)): both lists as CSR, ascending within a list"""
        m, p = self.n_nodes, self.n_pairs
        lims = [np.zeros((m, 2), np.int64) for _ in range(self.ndim)]
        nstart, vstart = np.zeros(m + 1, np.int32), np.zeros(self.n + 1, np.int32)
        nval, vval = np.zeros(p, np.int32), np.zeros(p, np.int32)
        self._call("nl_voxfeat_fetch_nodes", _ptr(lims[0]), _ptr(lims[1]), _ptr(lims[2]) if self.ndim == 3 else None, _ptr(nstart), _ptr(nval),
                   _ptr(vstart), _ptr(vval))
        nstart[m] = vstart[self.n] = p
        return lims, (nstart.astype(np.int64), nval.astype(np.int64)), (vstart.astype(np.int64), vval.astype(np.int64))


class NodeFeatures(_TimedParts, _Handle):
    """Device state of the node level of the hierarchy (include/nellie_amd.h nl_nodefeat_*): one frame's node list and border
    mask, and one set of groups (CSR lists of indices) over which value arrays are aggregated with numpy's padded pairwise sums.
    An object used for `groups` / `aggregate` alone needs no frame and may have any shape."""

    PARTS = ("node_list", "thickness", "node_stats", "aggregation")
    KEYS = ("mean", "std_dev", "min", "max", "sum")
    STATS = ("z", "y", "x", "divergence", "convergence", "vergere")
    # what the device converts exactly to float64; anything else is converted on the host, as numpy would
    VALUE_DTYPES = tuple(np.dtype(t) for t in (np.uint8, np.int8, np.uint16, np.int16, np.uint32, np.int32, np.float32, np.float64))

    _destroy, _noun, _ms_symbol = "nl_nodefeat_destroy", "node-feature object", "nl_nodefeat_kernel_ms"

    def __init__(self, shape=(1, 1), spacing=(1.0, 1.0), device=0):
        self.ndim, self.shape, (nz, ny, nx), sp = _frame_geometry("frames", spacing, shape=shape)
        self._create("nl_nodefeat_create", int(device), self.ndim, nz, ny, nx, _ptr(sp))
        self.n_nodes = self.n_groups = self.longest = 0
        self._dtypes = (np.dtype(np.uint8), np.dtype(np.uint8))

    def frame(self, pixel_class, comp, branch, border) -> int:
        """uploads a frame, lists its nodes (pixel class > 0) and computes their thickness; returns the number of nodes"""
        pc, c = _frame_array(pixel_class, self.shape, "pixel class", "object"), _frame_array(comp, self.shape, "component label", "object")
        b, o = _frame_array(branch, self.shape, "branch label", "object"), _frame_array(border, self.shape, "border mask", "object")
        m = _i64(0)
        self._call("nl_nodefeat_frame", _ptr(pc), DTYPE_CODES[pc.dtype], _ptr(c), DTYPE_CODES[c.dtype], _ptr(b), DTYPE_CODES[b.dtype], _ptr(o),
                   DTYPE_CODES[o.dtype], C.byref(m))
        self.n_nodes, self._dtypes = int(m.value), (c.dtype, b.dtype)
        return self.n_nodes

    def fetch(self):
        """(coordinates (n_nodes, D) int64, component labels, branch labels (the frames' dtypes), thickness float64)"""
        m = self.n_nodes
        coords, thick = np.empty((m, self.ndim), np.int64), np.empty(m, np.float64)
        c, b = np.empty(m, self._dtypes[0]), np.empty(m, self._dtypes[1])
        self._call("nl_nodefeat_fetch", _ptr(coords), _ptr(c), _ptr(b), _ptr(thick))
        return coords, c, b, thick

    def groups(self, offsets, idx) -> int:
        """loads the groups idx[offsets[j]:offsets[j + 1]]; returns L, the longest"""
        off, idx = np.ascontiguousarray(offsets, dtype=np.int64), np.ascontiguousarray(idx, dtype=np.int64)
        if off.ndim != 1 or off.size < 1 or idx.ndim != 1 or int(off[-1]) != idx.size:
            raise ValueError("offsets must be 1-D, start the first group and end at len(idx)")
        longest = _i64(0)
        self._call("nl_nodefeat_groups", _ptr(off), _ptr(idx), off.size - 1, C.byref(longest))
        self.n_groups, self.longest = off.size - 1, int(longest.value)
        return self.longest

    def set_wide_from(self, n) -> None:
        """from the next groups() on, groups of at least n values are summed a buffer block per wave; 0: never.  Same bits either way."""
        self._call("nl_nodefeat_set_wide_from", int(n))

    def aggregate(self, values) -> dict:
        """{key: (n_groups,) float64} for the keys mean, std_dev, min, max, sum of one 1-D value array over the loaded groups"""
        v = np.asarray(values)
        if v.ndim != 1:
            raise ValueError("values must be 1-D")
        v = np.ascontiguousarray(v, dtype=None if v.dtype in self.VALUE_DTYPES else np.float64)
        out = np.empty((len(self.KEYS), self.n_groups), np.float64)
        self._call("nl_nodefeat_aggregate", _ptr(v), DTYPE_CODES[v.dtype], v.size, _ptr(out))
        return dict(zip(self.KEYS, out))

    def node_stats(self, coords, vec01=None, vec12=None) -> dict:
        """{name: (n_nodes,) float64} for z, y, x, divergence, convergence, vergere; the loaded groups are the nodes' voxel lists,
        indices into coords (n_vox, D) and the two vector arrays (None: all NaN)"""
        xyz = np.ascontiguousarray(coords, dtype=np.int64).reshape(-1, self.ndim)
        vecs = [None if v is None else np.ascontiguousarray(v, dtype=np.float32) for v in (vec01, vec12)]
        for v in vecs:
            if v is not None and v.shape != xyz.shape:
                raise ValueError(f"vectors of shape {v.shape} for coordinates of shape {xyz.shape}")
        out = np.empty((len(self.STATS), self.n_nodes), np.float64)
        self._call("nl_nodefeat_node_stats", _ptr(xyz), _opt(vecs[0]), _opt(vecs[1]), len(xyz), _ptr(out))
        return dict(zip(self.STATS, out))


class BranchFeatures(_TimedParts, _Handle):
    """Device state of the branch level of the hierarchy (include/nellie_amd.h nl_branchfeat_*): one frame's skeleton list with
    degree, radius and tips per voxel and edge counts, voxel counts and medians per label, and one frame's regions (the labels of
    the full branch-label volume) with their exact integer sums and the most frequent reassigned label."""

    PARTS = ("skeleton", "degree", "radii", "lists", "regions")

    _destroy, _noun, _ms_symbol = "nl_branchfeat_destroy", "branch-feature object", "nl_branchfeat_kernel_ms"

    def __init__(self, shape, spacing, device=0):
        self.ndim, self.shape, (nz, ny, nx), sp = _frame_geometry("frames", spacing, shape=shape)
        self._create("nl_branchfeat_create", int(device), self.ndim, nz, ny, nx, _ptr(sp))
        self.n_voxels = self.n_labels = self.n_tips = self.n_lone = self.n_regions = 0
        self.n_offsets = 13 if self.ndim == 3 else 4
        self._comp_dtype = np.dtype(np.uint8)

    @staticmethod
    def _labels(a, shape, what):
        a = _frame_array(a, shape, what, "object")
        if a.dtype.kind not in "iu":
            raise TypeError(f"{what} must have an integer dtype, got {a.dtype}")
        return a

    def frame(self, skel, comp, border):
        """uploads a frame and lists its skeleton (label > 0); returns (skeleton voxels, distinct labels, tips, lone tips)"""
        s, c = self._labels(skel, self.shape, "skeleton label"), _frame_array(comp, self.shape, "component label", "object")
        o = _frame_array(border, self.shape, "border mask", "object")
        counts = [_i64(0) for _ in range(4)]
        self._call("nl_branchfeat_frame", _ptr(s), DTYPE_CODES[s.dtype], _ptr(c), DTYPE_CODES[c.dtype], _ptr(o), DTYPE_CODES[o.dtype],
                   *[C.byref(v) for v in counts])
        self.n_voxels, self.n_labels, self.n_tips, self.n_lone = (int(v.value) for v in counts)
        self._comp_dtype = c.dtype
        return self.n_voxels, self.n_labels, self.n_tips, self.n_lone

    def fetch(self) -> dict:
        """per skeleton voxel `coords` (n, D) int64, `labels` int64, `degree` uint8, `radius` float64, the positions `tips` and
        `lone` in the list; per label `branch_label` int64, `comp`, `edges` (B, offsets) uint32, `count` int32, `median` float64"""
        n, B = self.n_voxels, self.n_labels
        out = dict(coords=np.empty((n, self.ndim), np.int64), labels=np.empty(n, np.int64), degree=np.empty(n, np.uint8), radius=np.empty(n, np.float64),
                   tips=np.empty(self.n_tips, np.int64), lone=np.empty(self.n_lone, np.int64), branch_label=np.empty(B, np.int64),
                   comp=np.empty(B, self._comp_dtype), edges=np.empty((B, self.n_offsets), np.uint32), count=np.empty(B, np.int32),
                   median=np.empty(B, np.float64))
        self._call("nl_branchfeat_fetch", *[_ptr(a) for a in out.values()])
        return out

    def regions(self, labels, reassigned=None, rows=False) -> int:
        """the regions of a label volume, with the most frequent reassigned label of each when `reassigned` is given; `rows` takes
        the sums per run of equal labels along X instead of per voxel: the same values"""
        a = self._labels(labels, self.shape, "branch label")
        r = None if reassigned is None else self._labels(reassigned, self.shape, "reassigned label")
        count = _i64(0)
        self._call("nl_branchfeat_regions_rows" if rows else "nl_branchfeat_regions", _ptr(a), DTYPE_CODES[a.dtype], _opt(r),
                   DTYPE_CODES[r.dtype] if r is not None else 0, C.byref(count))
        self.n_regions = int(count.value)
        return self.n_regions

    def fetch_regions(self):
        """(labels (R) int64, sums (F, R) int64: n, min per axis, max per axis, S_a, Q_ab for a <= b; mode (R) int64, -1 without)"""
        R, D = self.n_regions, self.ndim
        labels, sums, mode = np.empty(R, np.int64), np.empty((1 + 3 * D + D * (D + 1) // 2, R), np.int64), np.empty(R, np.int64)
        self._call("nl_branchfeat_fetch_regions", _ptr(labels), _ptr(sums), _ptr(mode))
        return labels, sums, mode

    CONVEX_PARTS = ("extremes", "planes", "count", "hull")

    def convex(self):
        """takes the convex counts of the regions of the last regions() call, whose label frame is still on the device"""
        self._call("nl_branchfeat_convex")

    def fetch_convex(self, sizes=False):
        """count (R) int64: the lattice points in the closed hull of every region's voxel diamonds, 0 for a flat 3-D region; with
        `sizes` also the facets of every region's hull and the rows of its bounding box, (R) int64 each"""
        R = self.n_regions
        count, facets, rows = np.empty(R, np.int64), np.empty(R, np.int64), np.empty(R, np.int64)
        self._call("nl_branchfeat_fetch_convex", _ptr(count), _ptr(facets), _ptr(rows))
        return (count, facets, rows) if sizes else count

    def convex_ms_parts(self) -> dict:
        """of the last convex(): device ms of `extremes`, `planes` and `count`, host ms of `hull`"""
        ms = (_f32 * len(self.CONVEX_PARTS))()
        self._call("nl_branchfeat_convex_ms", ms)
        return dict(zip(self.CONVEX_PARTS, (float(v) for v in ms)))


def convex_limits() -> dict:
    """the sizes of the convex count kernel: box rows per workgroup, facets per staging chunk, workgroups per launch"""
    lim = np.zeros(3, np.int64)
    load().call("nl_branchfeat_convex_limits", _ptr(lim))
    return dict(zip(("rows_per_workgroup", "facets_per_chunk", "workgroups_per_launch"), (int(v) for v in lim)))


def host_convex_facets(coords) -> np.ndarray:
    """(k, 4) int64 facets (N_z, N_y, N_x, d) of the hull of the diamonds of the voxels `coords` (n, 2 or 3), on the host; k = 0 for
    a flat 3-D set"""
    c = np.ascontiguousarray(coords, dtype=np.int64)
    if c.ndim != 2 or c.shape[1] not in (2, 3) or len(c) == 0:
        raise ValueError(f"coords must be (n >= 1, 2 or 3), got {c.shape}")
    k = _i64(0)
    load().call("nl_host_convex_facets", _ptr(c), len(c), c.shape[1], None, 0, C.byref(k))
    out = np.empty((int(k.value), 4), np.int64)
    load().call("nl_host_convex_facets", _ptr(c), len(c), c.shape[1], _ptr(out), len(out), C.byref(k))
    return out


class Adjacency(_TimedParts, _Handle):
    """Device state of the hierarchy's adjacency maps (include/nellie_amd.h nl_adjacency_*): the three operations its six edge
    lists are made of.  Each returns a C-contiguous (m, 2) int64 array of (row, column) pairs, ascending in the row."""

    PARTS = ("pairs", "expand", "lookup")

    _destroy, _noun, _ms_symbol = "nl_adjacency_destroy", "adjacency object", "nl_adjacency_kernel_ms"

    def __init__(self, device=0):
        self._create("nl_adjacency_create", int(device))

    @staticmethod
    def _labels(a, what, keep32=False):
        """1-D labels as int64 (or as the int32 they are); a cast that would change a value is refused"""
        a = np.asarray(a)
        if a.ndim != 1:
            raise ValueError(f"{what} must be 1-D")
        if a.dtype == np.int64 or (keep32 and a.dtype == np.int32):
            return np.ascontiguousarray(a)
        _refuse_lossy_cast(a, np.dtype(np.int64), what)
        return np.ascontiguousarray(a, dtype=np.int64)

    def _fetch(self, m) -> np.ndarray:
        out = np.empty((int(m.value), 2), np.int64)
        self._call("nl_adjacency_fetch", _ptr(out))
        return out

    def pairs(self, labels, bias=0) -> np.ndarray:
        """(i, labels[i] - bias) for every i with labels[i] > 0"""
        lab = self._labels(labels, "labels", keep32=True)
        m = _i64(0)
        self._call("nl_adjacency_pairs", _ptr(lab), DTYPE_CODES[lab.dtype], lab.size, int(bias), C.byref(m))
        return self._fetch(m)

    def expand(self, offsets, values) -> np.ndarray:
        """(row, value) for every value of the CSR: offsets starts at 0, does not decrease and ends at len(values)"""
        off, val = self._labels(offsets, "offsets"), self._labels(values, "values")
        if off.size < 1 or int(off[-1]) != val.size:
            raise ValueError("offsets must hold at least one entry and end at len(values)")
        m = _i64(0)
        self._call("nl_adjacency_expand", _ptr(off), _ptr(val), off.size - 1, C.byref(m))
        return self._fetch(m)

    def lookup(self, child_labels, parent_labels) -> np.ndarray:
        """(i, j) for every child label that occurs among the parents, j its last position there.  ValueError for a child above
        the parents' largest label (numpy's IndexError in the reference) and for a negative label (which numpy would wrap)."""
        child, parent = self._labels(child_labels, "child labels"), self._labels(parent_labels, "parent labels")
        m = _i64(0)
        self._call("nl_adjacency_lookup", _ptr(child), child.size, _ptr(parent), parent.size, C.byref(m))
        return self._fetch(m)
