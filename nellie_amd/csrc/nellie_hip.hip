// libnellie_hip.so -- hand-written HIP for gfx950 (MI355X): Nellie's Filter -> Label hot path.  This unit: context lifetime, the
// Gaussian cascade, the device chain, the 2-D path and the epilogue (the Hessian walk: nellie_walk.hip, sampling: nellie_sample.hip,
// collectives: nellie_comm.hip).  C-ABI in include/nellie_amd.h.  Compile with -ffp-contract=off: every float operation
// below is meant to round exactly where numpy/scipy round.
#include "nl_host.h"

#include "walk_common.h"
#include "walk_plan.h"
#include "mask_volume.inc"
#include "filter2d.inc"
#include "thresholds.inc"
#include "chain.inc"
#include "percentile.inc"

// =================================================================================================
// host side: context, launch helpers, C-ABI
// =================================================================================================

// fused Y+X Gaussian: tiled / register-blocked X pass (default) or the row-at-a-time kernel (NELLIE_GYX_TILE=0)
bool gyx_tiled() {
    static int on = -1;
    if (on < 0) { const char *e = getenv("NELLIE_GYX_TILE"); on = (e && !atoi(e)) ? 0 : 1; }
    return on != 0;
}

extern "C" const char *nl_version(void) { return NL_VERSION; }

extern "C" int nl_device_count(int *count, char *err, size_t errlen) {
    if (!count) return nl_fail(err, errlen, NL_EINVAL, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return nl_fail(err, errlen, NL_ENODEV, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return NL_OK;
}

extern "C" int nl_device_mem_info(int device, int64_t *free_bytes, int64_t *total_bytes, char *err, size_t errlen) {
    NL_HIP(hipSetDevice(device));
    size_t f = 0, t = 0;
    NL_HIP(hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = (int64_t)f;
    if (total_bytes) *total_bytes = (int64_t)t;
    return NL_OK;
}

extern "C" int nl_device_name(int device, char *name, size_t namelen, char *err, size_t errlen) {
    hipDeviceProp_t p;
    NL_HIP(hipGetDeviceProperties(&p, device));
    if (name && namelen) snprintf(name, namelen, "%s (%s, %d CUs)", p.name, p.gcnArchName, p.multiProcessorCount);
    return NL_OK;
}

extern "C" int64_t nl_ctx_bytes(int64_t nz_local, int64_t ny, int64_t nx) {
    const int64_t n = nz_local * ny * nx;
    const VqAlloc vq = vq_alloc(nz_local, ny, nx);
    return n * (4 * 4 + 3) + vq.entries * 32 + vq.regions * 4 + (1 << 16) + ((n + SCAN_CHUNK - 1) / SCAN_CHUNK + 1) * 4;
}

extern "C" int nl_ctx_destroy(nl_ctx *c) {
    if (!c) return NL_OK;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    for (auto &kv : c->prof) for (auto &r : kv.second) { hipEventDestroy(r.a); hipEventDestroy(r.b); }
    for (auto &r : c->prof_pool) { hipEventDestroy(r.a); hipEventDestroy(r.b); }
    for (int k = 0; k < 4; ++k) if (c->f[k]) hipFree(c->f[k]);
    for (int k = 0; k < 3; ++k) if (c->m[k]) hipFree(c->m[k]);
    if (c->d_small) hipFree(c->d_small);
    if (c->d_input && !c->input_borrowed) hipFree(c->d_input);
    for (int k = 0; k < 2; ++k) { if (c->d_in_slot[k]) hipFree(c->d_in_slot[k]); if (c->ev_in[k]) hipEventDestroy(c->ev_in[k]); }
    if (c->d_stage_fr) hipFree(c->d_stage_fr);
    if (c->d_stage_lab) hipFree(c->d_stage_lab);
    if (c->ev_staged) hipEventDestroy(c->ev_staged);
    if (c->ev_fetched) hipEventDestroy(c->ev_fetched);
    if (c->side) { hipStreamSynchronize(c->side); hipStreamDestroy(c->side); }
    if (c->ev_side) hipEventDestroy(c->ev_side);
    if (c->ev_main) hipEventDestroy(c->ev_main);
    if (c->ev_ahead) hipEventDestroy(c->ev_ahead);
    if (c->copy_in) hipStreamDestroy(c->copy_in);
    if (c->copy_out) hipStreamDestroy(c->copy_out);
    if (c->d_blk) hipFree(c->d_blk);
    for (int k = 0; k < 4; ++k) if (c->d_2d[k]) hipFree(c->d_2d[k]);
    if (c->d_fsq_cache) hipFree(c->d_fsq_cache);
    for (auto &pk : c->fsq_park) if (pk.p) hipFree(pk.p);
    if (c->h_chain_est) hipHostFree(c->h_chain_est);
    if (c->d_vq) hipFree(c->d_vq);
    if (c->mk_scratch) hipFree(c->mk_scratch);
    if (c->mk_act) hipFree(c->mk_act);
    if (c->d_vq_count) hipFree(c->d_vq_count);
    if (c->d_rows) hipFree(c->d_rows);
    if (c->d_ag) hipFree(c->d_ag);
    if (c->d_sl) hipFree(c->d_sl);
    if (c->d_seg_done) hipFree(c->d_seg_done);
    nw_release(c);
    if (c->d_pct) hipFree(c->d_pct);
    if (c->h_pct) hipHostFree(c->h_pct);
    if (c->h_sl) hipHostFree(c->h_sl);
    if (c->d_pack) hipFree(c->d_pack);
    if (c->h_ag) hipHostFree(c->h_ag);
    if (c->gbits[0]) hipFree(c->gbits[0]);
    if (c->gbits[1]) hipFree(c->gbits[1]);
    if (c->grows) hipFree(c->grows);
    if (c->h_small) hipHostFree(c->h_small);
    if (c->h_prefix) hipHostFree(c->h_prefix);
    if (c->t0) hipEventDestroy(c->t0);
    if (c->t1) hipEventDestroy(c->t1);
    if (c->xstream) { hipStreamSynchronize(c->xstream); hipStreamDestroy(c->xstream); }
    if (c->ev_x_main) hipEventDestroy(c->ev_x_main);
    if (c->ev_x_done) hipEventDestroy(c->ev_x_done);
    if (c->d_chain) hipFree(c->d_chain);
    if (c->h_chain) hipHostFree(c->h_chain);
    if (c->ev_chain) hipEventDestroy(c->ev_chain);
    comm_release(c, c->comm2, 2);
    comm_release(c, c->comm, 1);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;
    return NL_OK;
}

extern "C" int nl_ctx_create(nl_ctx **out, int device, int64_t nzl, int64_t ny, int64_t nx,
                             int64_t gz0, int64_t gnz, int64_t own_lo, int64_t own_hi, char *err, size_t errlen) {
    if (!out) return nl_fail(err, errlen, NL_EINVAL, "out is NULL");
    *out = nullptr;
    if (nzl < 1 || ny < 1 || nx < 1) return nl_fail(err, errlen, NL_EINVAL, "empty volume (%lld,%lld,%lld)", (i64)nzl, (i64)ny, (i64)nx);
    if (gz0 < 0 || gz0 + nzl > gnz) return nl_fail(err, errlen, NL_EINVAL, "slab [%lld,%lld) outside the global volume of %lld planes", (i64)gz0, (i64)(gz0 + nzl), (i64)gnz);
    if (own_lo < 0 || own_hi > nzl || own_lo >= own_hi) return nl_fail(err, errlen, NL_EINVAL, "bad owned range [%lld,%lld)", (i64)own_lo, (i64)own_hi);
    const i64 n = (i64)nzl * ny * nx;
    if (n >= ((i64)1 << 31)) return nl_fail(err, errlen, NL_EINVAL, "local slab of %lld voxels exceeds the int32 label index range; shard over Z", n);
    if (ny > 65535 || nzl > 65535) return nl_fail(err, errlen, NL_EINVAL, "Y and local Z extents must be <= 65535");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return nl_fail(err, errlen, NL_ENODEV, "GPU backend requested but no HIP device is available (%s)", e == hipSuccess ? "0 devices" : hipGetErrorString(e));
    if (device < 0 || device >= ndev) return nl_fail(err, errlen, NL_ENODEV, "GPU backend requested but device %d does not exist (%d devices)", device, ndev);
    NL_HIP(hipSetDevice(device));
    nl_ctx *c = new nl_ctx();
    c->device = device; c->nzl = nzl; c->ny = ny; c->nx = nx; c->gz0 = gz0; c->gnz = gnz;
    c->own_lo = own_lo; c->own_hi = own_hi; c->n = n;
    int rc = NL_OK;
    auto alloc = [&](void **p, size_t bytes) -> bool {
        hipError_t ee = hipMalloc(p, bytes);
        if (ee != hipSuccess) {
            rc = nl_fail(err, errlen, ee == hipErrorOutOfMemory ? NL_ENOMEM : NL_EHIP,
                         "hipMalloc(%zu bytes): %s%s", bytes, hipGetErrorString(ee), ee == hipErrorOutOfMemory ? " [out of memory]" : "");
            return false;
        }
        return true;
    };
    bool ok = true;
    for (int k = 0; k < 4 && ok; ++k) ok = alloc((void **)&c->f[k], (size_t)n * 4);
    // m[0] doubles as the cumulative bit mask of Filter: one 64-bit word per 64 x-voxels of a row
    const size_t mask_words = (size_t)NL_MASK_SLOTS * nzl * ny * ((nx + 63) / 64);
    const size_t plane_words_bytes = (size_t)nzl * ny * ((nx + 63) / 64) * 8;     // one bit plane
    for (int k = 0; k < 3 && ok; ++k) {
        size_t bytes = (size_t)n;
        if (k == 0 && mask_words * 8 > bytes) bytes = mask_words * 8;
        if (plane_words_bytes > bytes) bytes = plane_words_bytes;
        ok = alloc((void **)&c->m[k], bytes);
    }
    if (ok) ok = alloc((void **)&c->d_rows, ((size_t)nzl * ny + 2) * 2 * 4);
    if (ok) ok = alloc(&c->d_small, 1 << 16);
    {
        const VqAlloc vq = vq_alloc(nzl, ny, nx);
        if (ok) ok = alloc((void **)&c->d_vq, (size_t)vq.entries * 32);
        if (ok) ok = alloc((void **)&c->d_vq_count, (size_t)vq.regions * 4);
        c->spec_ok = vq.spec_ok;
    }
    c->blk_cap = (n + SCAN_CHUNK - 1) / SCAN_CHUNK + 1;
    if (ok) ok = alloc(&c->d_blk, (size_t)c->blk_cap * 4);
    if (ok && hipHostMalloc(&c->h_small, 1 << 16, hipHostMallocDefault) != hipSuccess) {
        rc = nl_fail(err, errlen, NL_ENOMEM, "hipHostMalloc failed [out of memory]"); ok = false;
    }
    // side stream: the compute-bound resolve kernel runs beside the memory-bound Gaussian of the next scale; NELLIE_SIDE_PRIO
    // (-1 high, 0 normal, 1 low) chooses which of the two the dispatcher serves first
    int side_prio = -1;
    { const char *e = getenv("NELLIE_SIDE_PRIO"); if (e) side_prio = atoi(e); }
    int prio_lo = 0, prio_hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);      // lo = numerically largest = lowest priority
    const int side_p = side_prio < 0 ? prio_hi : (side_prio > 0 ? prio_lo : (prio_lo + prio_hi) / 2);
    if (ok && (hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking, side_p) != hipSuccess ||
               hipEventCreateWithFlags(&c->ev_side, hipEventDisableTiming) != hipSuccess ||
               hipEventCreateWithFlags(&c->ev_main, hipEventDisableTiming) != hipSuccess ||
               hipEventCreateWithFlags(&c->ev_ahead, hipEventDisableTiming) != hipSuccess)) {
        rc = nl_fail(err, errlen, NL_EHIP, "stream/event creation failed"); ok = false;
    }
    if (ok && (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
               hipEventCreate(&c->t0) != hipSuccess || hipEventCreate(&c->t1) != hipSuccess)) {
        rc = nl_fail(err, errlen, NL_EHIP, "stream/event creation failed"); ok = false;
    }
    if (!ok) { nl_ctx_destroy(c); return rc; }
    *out = c;
    return NL_OK;
}

extern "C" int nl_sync(nl_ctx *c, char *err, size_t errlen) {
    if (!c) return nl_fail(err, errlen, NL_EINVAL, "ctx is NULL");
    NL_HIP(hipSetDevice(c->device));
    NL_HIP(hipStreamSynchronize(c->stream));
    NL_HIP(hipStreamSynchronize(c->side));
    if (c->xstream) NL_HIP(hipStreamSynchronize(c->xstream));
    return NL_OK;
}


int upload_convert(nl_ctx *c, const void *host, int dtype, float *dst, i64 count, char *err, size_t errlen) {
    const size_t es = dtype_size(dtype);
    if (!es) return nl_fail(err, errlen, NL_EINVAL, "unsupported dtype code %d", dtype);
    if (dtype == NL_F32) {
        NL_HIP(hipMemcpyAsync(dst, host, (size_t)count * 4, hipMemcpyHostToDevice, c->stream));
        NL_HIP(hipStreamSynchronize(c->stream));
        return NL_OK;
    }
    // stage raw bytes in free float volumes (2 consecutive volumes cover 8-byte types)
    void *raw = nullptr;
    bool own = false;
    // find a free f[] buffer that is not dst's buffer
    for (int k = 0; k < 4 && !raw; ++k) {
        const bool contains = (dst >= c->f[k] && dst < c->f[k] + c->n);
        if (!contains && k != c->i_vmax && es <= 4) raw = c->f[k];
    }
    if (!raw) { NL_HIP(hipMalloc(&raw, (size_t)count * es)); own = true; }
    NL_HIP(hipMemcpyAsync(raw, host, (size_t)count * es, hipMemcpyHostToDevice, c->stream));
    const unsigned int g = grid1d(count);
    switch (dtype) {
        case NL_U8: convert_kernel<uint8_t><<<g, 256, 0, c->stream>>>((const uint8_t *)raw, dst, count); break;
        case NL_I8: convert_kernel<int8_t><<<g, 256, 0, c->stream>>>((const int8_t *)raw, dst, count); break;
        case NL_U16: convert_kernel<uint16_t><<<g, 256, 0, c->stream>>>((const uint16_t *)raw, dst, count); break;
        case NL_I16: convert_kernel<int16_t><<<g, 256, 0, c->stream>>>((const int16_t *)raw, dst, count); break;
        case NL_U32: convert_kernel<uint32_t><<<g, 256, 0, c->stream>>>((const uint32_t *)raw, dst, count); break;
        case NL_I32: convert_kernel<int32_t><<<g, 256, 0, c->stream>>>((const int32_t *)raw, dst, count); break;
        case NL_F64: convert_kernel<double><<<g, 256, 0, c->stream>>>((const double *)raw, dst, count); break;
        case NL_U64: convert_kernel<uint64_t><<<g, 256, 0, c->stream>>>((const uint64_t *)raw, dst, count); break;
        case NL_I64: convert_kernel<int64_t><<<g, 256, 0, c->stream>>>((const int64_t *)raw, dst, count); break;
    }
    NL_CHECK_LAUNCH();
    NL_HIP(hipStreamSynchronize(c->stream));
    if (own) hipFree(raw);
    return NL_OK;
}

extern "C" int nl_filter_load(nl_ctx *c, const void *host, int dtype, int64_t z0, int64_t z1, char *err, size_t errlen) {
    NL_ENTER(c);
    NL_JOIN_SIDE(c);
    if (!host || z0 < 0 || z1 > c->nzl || z0 >= z1) return nl_fail(err, errlen, NL_EINVAL, "bad plane range [%lld,%lld)", (i64)z0, (i64)z1);
    c->i_gauss = 0; c->i_vmax = 3; c->i_labels = -1; c->frangi_ready = 0;
    c->pz_on = 0; c->prezero_used = 0; c->chain_reorder = 0;
    c->gauss_ext = nullptr;
    // a frame abandoned between nl_gauss_step_ahead and nl_gauss_commit (an exception in the host's scale loop) leaves a cascade step on the
    // side stream that still writes the ping-pong volumes: this frame's first kernels come after it
    if (c->ahead_pending) NL_HIP(hipStreamWaitEvent(c->stream, c->ev_ahead, 0));
    c->ahead_pending = 0;
    c->fsq_cache_valid = 0;
    NL_HIP(zero_small((char *)c->d_small + (52 << 10), 4, c->stream));
    c->vmax_zero_lo = c->vmax_zero_hi = 0;
    const i64 plane = c->ny * c->nx;
    int rc = upload_convert(c, host, dtype, c->f[0] + z0 * plane, (z1 - z0) * plane, err, errlen);
    if (rc) return rc;
    // vesselness = zeros, masks = ones (filtering.py:807-808): the first evaluated scale zeroes the vesselness
    // volume and starts the cumulative mask; nl_filter_finish zeroes whatever the masks reject
    c->mask_slots_used = 0;
    NL_HIP(hipStreamSynchronize(c->stream));
    return NL_OK;
}

// Keep the raw frame resident in HBM (any dtype) so that a timed region can start from device memory.
extern "C" int nl_input_load(nl_ctx *c, const void *host, int dtype, int64_t z0, int64_t z1, char *err, size_t errlen) {
    NL_ENTER(c);
    const size_t es = dtype_size(dtype);
    if (!es) return nl_fail(err, errlen, NL_EINVAL, "unsupported dtype code %d", dtype);
    if (!host || z0 < 0 || z1 > c->nzl || z0 >= z1) return nl_fail(err, errlen, NL_EINVAL, "bad plane range [%lld,%lld)", (i64)z0, (i64)z1);
    if (c->d_input && c->input_borrowed) { c->d_input = nullptr; c->input_borrowed = 0; }
    if (c->d_input && c->input_dtype != dtype) { hipFree(c->d_input); c->d_input = nullptr; }
    if (!c->d_input) NL_HIP(hipMalloc(&c->d_input, (size_t)c->n * es));
    c->input_dtype = dtype;
    const i64 plane = c->ny * c->nx;
    NL_HIP(hipMemcpyAsync((char *)c->d_input + (size_t)z0 * plane * es, host, (size_t)(z1 - z0) * plane * es, hipMemcpyHostToDevice, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    return NL_OK;
}

// frame = xp.asarray(resident input, dtype=float32); vesselness = 0; masks = 1.  Asynchronous.
extern "C" int nl_filter_begin(nl_ctx *c, char *err, size_t errlen) {
    NL_ENTER(c);
    NL_JOIN_SIDE(c);
    if (!c->d_input) return nl_fail(err, errlen, NL_ESTATE, "nl_filter_begin before nl_input_load");
    c->i_gauss = 0; c->i_vmax = 3; c->i_labels = -1; c->frangi_ready = 0;
    c->pz_on = 0; c->prezero_used = 0; c->chain_reorder = 0;
    c->mask_slots_used = 0;
    c->gauss_ext = nullptr;
    // a frame abandoned between nl_gauss_step_ahead and nl_gauss_commit (an exception in the host's scale loop) leaves a cascade step on the
    // side stream that still writes the ping-pong volumes: this frame's first kernels come after it
    if (c->ahead_pending) NL_HIP(hipStreamWaitEvent(c->stream, c->ev_ahead, 0));
    c->ahead_pending = 0;
    c->fsq_cache_valid = 0;
    NL_HIP(zero_small((char *)c->d_small + (52 << 10), 4, c->stream));
    c->vmax_zero_lo = c->vmax_zero_hi = 0;
    if (c->input_dtype == NL_F32 && !getenv("NELLIE_COPY_INPUT")) {
        // float32 frames are used where they lie: the cascade never writes its source (ping-pong volumes), so the
        // first Gaussian pass reads the resident input directly (the reference's gauss = frame view, filtering.py:811)
        c->gauss_ext = (float *)c->d_input;
        return NL_OK;
    }
    ProfScope ps(c, "load");
    const unsigned int g = grid1d(c->n);
    switch (c->input_dtype) {
        case NL_U8: convert_kernel<uint8_t><<<g, 256, 0, c->stream>>>((const uint8_t *)c->d_input, c->f[0], c->n); break;
        case NL_I8: convert_kernel<int8_t><<<g, 256, 0, c->stream>>>((const int8_t *)c->d_input, c->f[0], c->n); break;
        case NL_U16: convert_kernel<uint16_t><<<g, 256, 0, c->stream>>>((const uint16_t *)c->d_input, c->f[0], c->n); break;
        case NL_I16: convert_kernel<int16_t><<<g, 256, 0, c->stream>>>((const int16_t *)c->d_input, c->f[0], c->n); break;
        case NL_U32: convert_kernel<uint32_t><<<g, 256, 0, c->stream>>>((const uint32_t *)c->d_input, c->f[0], c->n); break;
        case NL_I32: convert_kernel<int32_t><<<g, 256, 0, c->stream>>>((const int32_t *)c->d_input, c->f[0], c->n); break;
        case NL_F32: convert_kernel<float><<<g, 256, 0, c->stream>>>((const float *)c->d_input, c->f[0], c->n); break;
        case NL_F64: convert_kernel<double><<<g, 256, 0, c->stream>>>((const double *)c->d_input, c->f[0], c->n); break;
        case NL_U64: convert_kernel<uint64_t><<<g, 256, 0, c->stream>>>((const uint64_t *)c->d_input, c->f[0], c->n); break;
        case NL_I64: convert_kernel<int64_t><<<g, 256, 0, c->stream>>>((const int64_t *)c->d_input, c->f[0], c->n); break;
    }
    NL_CHECK_LAUNCH();
    c->mask_slots_used = 0;
    return NL_OK;
}


// Y and X passes in one kernel (gauss_yx_tile_kernel): equal radii up to GM_MAX_R that fit the Y axis
static bool gauss_can_yx(const nl_ctx *c, const double *wy, int ry, const double *wx, int rx) {
    return wy && wx && ry == rx && ry >= 1 && ry <= GM_MAX_R && ry <= c->ny && !getenv("NELLIE_NO_FUSED_YX");
}
// Ping-pong volumes a cascade step writes one after the other: 1 (fused Z+Y+X), 2 (Z, then Y+X) or 3 (one per axis: radii beyond
// GM_MAX_R, unequal in-plane radii).  The third destination of a three-pass step is the step's own SOURCE volume.
static int gauss_step_volumes(const nl_ctx *c, const double *wz, const double *wy, int ry, const double *wx, int rx) {
    return (wz ? 1 : 0) + (gauss_can_yx(c, wy, ry, wx, rx) ? 1 : (wy ? 1 : 0) + (wx ? 1 : 0));
}

// The whole step in one kernel (gauss_zyx.inc)?  See nl_gauss_step.  NELLIE_GAUSS_FUSED=0 / 1: never / whenever the radii allow.
static bool gauss_takes_zyx(const nl_ctx *c, const double *wz, int rz, const double *wy, int ry, const double *wx, int rx) {
    const char *e_fz = getenv("NELLIE_GAUSS_FUSED");
    const bool fused_zyx = e_fz ? atoi(e_fz) != 0 : c->n >= ((i64)1 << 26);
    return fused_zyx && wz && gauss_can_yx(c, wy, ry, wx, rx) && gyx_tiled() && gl_zyx_ok(c, rz, ry, c->f[(c->i_gauss + 1) % 3]) &&
           memcmp(wy, wx, (size_t)(2 * ry + 1) * sizeof(double)) == 0;
}
// ... asked by the host before it plans a frame out of sigma order: *fused = 1 when nl_gauss_step would take the step in one kernel
extern "C" int nl_gauss_step_fused(nl_ctx *c, const double *wz, int rz, const double *wy, int ry, const double *wx, int rx, int *fused,
                                   char *err, size_t errlen) {
    if (!c || !fused) return nl_fail(err, errlen, NL_EINVAL, "ctx or fused is NULL");
    *fused = gauss_takes_zyx(c, wz, rz, wy, ry, wx, rx) ? 1 : 0;
    return NL_OK;
}

extern "C" int nl_gauss_step(nl_ctx *c, const double *wz, int rz, const double *wy, int ry, const double *wx, int rx,
                             int64_t z0, int64_t z1, char *err, size_t errlen) {
    NL_ENTER(c);
    if (c->ahead_pending) return nl_fail(err, errlen, NL_ESTATE, "nl_gauss_step while a step enqueued ahead is uncommitted");
    if (z0 < 0 || z1 > c->nzl || z0 >= z1) return nl_fail(err, errlen, NL_EINVAL, "bad plane range [%lld,%lld)", (i64)z0, (i64)z1);
    if (c->halo_pending) {                       // ghost planes of the source volume still travelling (nl_halo_exchange_at, async)
        // "halo_wait": the event pair brackets nothing but the wait, so its time is what the exchange of this cascade step EXPOSED on the
        // main stream (0 when the planes arrived while the scale's walk ran) -- the figure bench.py's N > 1 line reports per rank
        ProfScope ps(c, "halo_wait");
        NL_HIP(hipStreamWaitEvent(c->stream, c->ev_x_done, 0));
        c->halo_pending = 0;
    }
    const VolGeom v = geom(c);
    // three ping-pong volumes f[0..2]: the source of a pass is dead once the pass has run,
    // so "the next one" is always a legal destination
    const dim3 grid((unsigned)((c->nx + 255) / 256), (unsigned)c->ny, (unsigned)(z1 - z0));
    int src = c->i_gauss;
    const float *srcp = gauss_cur(c);       // the source of the next pass (the borrowed input before the first one)
    GaussW gw;
    int rc;
    const bool can_yx = gauss_can_yx(c, wy, ry, wx, rx);
    bool fused_yx = false;
    // The whole step in one kernel (gauss_zyx.inc) when the radii have an instantiation and Y and X share their weights, which is
    // what Filter asks for (sigma_vec = (s / z_ratio, s, s)) -- on volumes that do not fit the caches: the fused kernel trades HBM
    // traffic for redundant float64 work, and a 128 x 512 x 512 frame (134 MB a volume) streams from the 256 MB Infinity Cache anyway
    // (gauss ms per frame, two kernels / fused: 128 x 512 x 512 0.62 / 0.77; 256 x 512 x 512 1.32 / 1.24; 512^3 2.24 / 2.16; 256 x 1024^2
    // 4.44 / 4.00; 1024^3 17.7 / 15.3).
    // NELLIE_GAUSS_FUSED=0 / 1: never / whenever the radii allow (tests run the fused kernel on small volumes that way).
    // A chain that walks its scales out of sigma order (nl_chain_begin: reorder) keeps the Gaussians of its pending scales: the step
    // writes a volume that holds none of them, and it is the fused step or nothing -- every other form needs a second free volume.
    const bool reorder = c->chain_reorder && c->chain_n > 0;
    int dst_zyx = (src + 1) % 3;
    if (reorder) {
        if (c->vol_scale[dst_zyx] >= 0) dst_zyx = (src + 2) % 3;
        if (c->vol_scale[dst_zyx] >= 0 || c->stream == c->side || !gauss_takes_zyx(c, wz, rz, wy, ry, wx, rx))
            return nl_fail(err, errlen, NL_ESTATE, c->vol_scale[dst_zyx] >= 0 ? "no free Gaussian volume: three scales wait for their walk"
                                                                                : "a chain out of sigma order takes fused cascade steps only");
    }
    if (gauss_takes_zyx(c, wz, rz, wy, ry, wx, rx)) {
        GaussW gy;
        if ((rc = fill_gw(gw, wz, rz, err, errlen)) || (rc = fill_gw(gy, wy, ry, err, errlen))) return rc;
        if ((z0 - rz < 0 && c->gz0 > 0) || (z1 - 1 + rz >= c->nzl && c->gz0 + c->nzl < c->gnz))
            return nl_fail(err, errlen, NL_EINVAL, "Z pass of radius %d on planes [%lld,%lld) reaches outside the local slab", rz, (i64)z0, (i64)z1);
        const int dst = dst_zyx;
        char scope[32];
        snprintf(scope, sizeof scope, "gauss_zyx<%d,%d>", rz, ry);        // one timer per kernel instantiation, as a profiler lists them
        ProfScope ps(c, scope);
        // the frame's first step also zeroes the running scale maximum on its planes (see gauss_zyx.inc: zero_out)
        static int zero_in_passing = -1;
        if (zero_in_passing < 0) { const char *e = getenv("NELLIE_ZERO_IN_GAUSS"); zero_in_passing = (e && !atoi(e)) ? 0 : 1; }
        const bool zero = zero_in_passing && c->mask_slots_used == 0 && c->vmax_zero_hi == 0 && c->stream != c->side;
        // ... and the chain's last step the volume Label will paint into: the third ping-pong volume, dead since the step before and
        // for the rest of the frame (nl_chain_begin: pz_on).  A step running ahead is enqueued one nl_chain_scale earlier.
        const bool ahead = c->stream == c->side;
        // Out of sigma order the steps are counted, and the third volume must hold no scale that still waits for its walk (the host
        // holds the last step back until then; where an explicit order does not, the labels are written densely as before).
        const int i_third = 3 - src - dst;
        const bool last = reorder ? (c->chain_steps == c->chain_n - 1 && c->vol_scale[i_third] < 0)
                                  : c->chain_k == c->chain_n - (ahead ? 2 : 1);
        const bool prezero = !zero && c->pz_on && c->chain_n > 0 && last && z0 == 0 && z1 == c->nzl;
        float *third = c->f[i_third];
        (void)gl_zyx(c, rz, ry, srcp, c->f[dst], v, z0, z1, gauss_ws_of(gw), gauss_ws_of(gy), zero ? c->f[c->i_vmax] : (prezero ? third : nullptr));
        if (zero) { c->vmax_zero_lo = z0; c->vmax_zero_hi = z1; }
        NL_CHECK_LAUNCH();
        if (prezero) pz_set(c, third);
        src = dst; srcp = c->f[dst];
        fused_yx = true;
        wz = nullptr;
    }
    if (wz) {
        if ((rc = fill_gw(gw, wz, rz, err, errlen))) return rc;
        // every tap must land inside the local slab unless it reflects at a true face
        if ((z0 - rz < 0 && c->gz0 > 0) || (z1 - 1 + rz >= c->nzl && c->gz0 + c->nzl < c->gnz))
            return nl_fail(err, errlen, NL_EINVAL, "Z pass of radius %d on planes [%lld,%lld) reaches outside the local slab", rz, (i64)z0, (i64)z1);
        const int dst = (src + 1) % 3;
        ProfScope ps(c, "gauss_z");
        if (!gl_fast(0, c, srcp, c->f[dst], v, z0, z1, gw)) gl_axis(0, false, c, grid, srcp, c->f[dst], v, z0, z1, gw);
        NL_CHECK_LAUNCH();
        src = dst; srcp = c->f[dst];
    }
    if (!fused_yx && can_yx) {
        GaussW gy, gx;
        if ((rc = fill_gw(gy, wy, ry, err, errlen))) return rc;
        if ((rc = fill_gw(gx, wx, rx, err, errlen))) return rc;
        const GaussWS wsy = gauss_ws_of(gy), wsx = gauss_ws_of(gx);
        const int dst = (src + 1) % 3;
        ProfScope ps(c, "gauss_yx");
        const dim3 g2((unsigned)((c->nx + GYX_COLS - 1) / GYX_COLS), (unsigned)((c->ny + v.chunk - 1) / v.chunk), (unsigned)(z1 - z0));
        (void)gl_yx(c, gyx_tiled(), false, ry, srcp, c->f[dst], v, z0, z1, wsy, wsx, g2);
        NL_CHECK_LAUNCH();
        src = dst; srcp = c->f[dst];
        fused_yx = true;
    }
    if (wy && !fused_yx) {
        if ((rc = fill_gw(gw, wy, ry, err, errlen))) return rc;
        const int dst = (src + 1) % 3;
        ProfScope ps(c, "gauss_y");
        if (!gl_fast(1, c, srcp, c->f[dst], v, z0, z1, gw)) gl_axis(1, false, c, grid, srcp, c->f[dst], v, z0, z1, gw);
        NL_CHECK_LAUNCH();
        src = dst; srcp = c->f[dst];
    }
    if (wx && !fused_yx) {
        if ((rc = fill_gw(gw, wx, rx, err, errlen))) return rc;
        const int dst = (src + 1) % 3;
        ProfScope ps(c, "gauss_x");
        if (!gl_fast(2, c, srcp, c->f[dst], v, z0, z1, gw)) gl_axis(2, false, c, grid, srcp, c->f[dst], v, z0, z1, gw);
        NL_CHECK_LAUNCH();
        src = dst; srcp = c->f[dst];
    }
    c->i_gauss = src;
    c->fsq_cache_valid = 0;
    if (srcp != c->gauss_ext) c->gauss_ext = nullptr;      // a cascade step ran: the Gaussian now lives in f[src]
    if (reorder) ++c->chain_steps;
    return NL_OK;
}

// The cascade step of scale s+1 only reads the Gaussian of scale s -- like everything else scale s does -- so it can run
// beside it.  nl_gauss_step_ahead enqueues the step on the side stream into the two free ping-pong volumes without
// making it current; nl_gauss_commit (before anything of scale s+1) orders the main stream after it and switches.
// Between the two calls no entry point that uses a free Gaussian volume as scratch may be called (nl_sample_gather,
// nl_mask_volume*, Label); the per-scale calls of Filter do not.
extern "C" int nl_gauss_step_ahead(nl_ctx *c, const double *wz, int rz, const double *wy, int ry, const double *wx, int rx,
                                   int64_t z0, int64_t z1, char *err, size_t errlen) {
    NL_ENTER(c);
    if (c->ahead_pending) return nl_fail(err, errlen, NL_ESTATE, "a step enqueued ahead is already pending");
    // A step of three passes would write its third pass into the volume it started from -- the Gaussian the current scale is
    // still reading (found by the fuzzer's explicit sigma lists, round 5: radii beyond GM_MAX_R).  Callers ask
    // nl_ctx_info("gauss_yx_max_r") and run such steps in order.
    if (gauss_step_volumes(c, wz, wy, ry, wx, rx) > 2)
        return nl_fail(err, errlen, NL_ESTATE, "a cascade step of three passes (radii %d / %d / %d) cannot run ahead: it needs the current Gaussian's volume", rz, ry, rx);
    NL_HIP(hipEventRecord(c->ev_main, c->stream));
    hipStream_t ahead_stream = c->side;
    NL_HIP(hipStreamWaitEvent(ahead_stream, c->ev_main, 0));
    const int cur_idx = c->i_gauss;
    float *cur_ext = c->gauss_ext;
    hipStream_t main_stream = c->stream;
    c->stream = ahead_stream;                  // the launch helpers use c->stream
    const int rc = nl_gauss_step(c, wz, rz, wy, ry, wx, rx, z0, z1, err, errlen);
    c->stream = main_stream;
    if (rc) { c->i_gauss = cur_idx; c->gauss_ext = cur_ext; return rc; }
    c->ahead_gauss = c->i_gauss;
    c->i_gauss = cur_idx; c->gauss_ext = cur_ext;
    NL_HIP(hipEventRecord(c->ev_ahead, ahead_stream));
    c->ahead_pending = 1;
    return NL_OK;
}

extern "C" int nl_gauss_commit(nl_ctx *c, char *err, size_t errlen) {
    NL_ENTER_KEEP_PZ(c);
    if (!c->ahead_pending) return nl_fail(err, errlen, NL_ESTATE, "nl_gauss_commit without nl_gauss_step_ahead");
    NL_HIP(hipStreamWaitEvent(c->stream, c->ev_ahead, 0));
    c->i_gauss = c->ahead_gauss;
    c->gauss_ext = nullptr;
    c->ahead_pending = 0;
    c->fsq_cache_valid = 0;
    return NL_OK;
}


// ---- device-resident threshold chain (chain.inc) -----------------------------------------------------------------------------
static inline unsigned int f2u(float x) { unsigned int u; memcpy(&u, &x, 4); return u; }
static inline float u2f(unsigned int u) { float x; memcpy(&x, &u, 4); return x; }
static inline float py_min_f(float a, float b) { return b < a ? b : a; }       // python's min(a, b)

// The host repeats what the chain's kernels decided for one scale, with the code of the synchronous path, and compares bit for
// bit.  Returns the record's flags, NL_CF_VERIFY added on any difference.
static int chain_verify(const ChainScale &s, double division, double margin, double test_scale) {
    if (s.flags) return s.flags;
    int bad = 0;
    double tri, otsu; int st;
    {   // gamma
        hist_thresholds_host<float>((const int64_t *)s.h_gauss.counts, s.h_gauss.edges, NL_CHAIN_BINS, &tri, &otsu, &st);
        const float g = py_min_f((float)tri, (float)otsu);
        const float gamma = g > 0.0f ? g : 1.1920929e-07f;
        const float gamma_sq = (float)(2.0 * std::pow((double)gamma, 2.0));
        if (st || f2u(gamma) != f2u(s.gamma) || f2u(gamma_sq) != f2u(s.gamma_sq)) bad = 1;
        float e[NL_CHAIN_BINS + 1];
        host_edges(u2f(s.h_gauss.res[0]), u2f(s.h_gauss.res[1]), NL_CHAIN_BINS, e);
        if (memcmp(e, s.h_gauss.edges, sizeof(e))) bad = 1;
    }
    {   // bracket
        hist_thresholds_host<float>((const int64_t *)s.h_raw.counts, s.h_raw.edges, NL_CHAIN_BINS, &tri, &otsu, &st);
        const double t = (double)py_min_f((float)tri, (float)otsu) * test_scale / division;
        const float lo = (float)(t * t * (1.0 - margin)), hi = (float)(t * t * (1.0 + margin));
        if (st || f2u(lo) != f2u(s.fsq_lo) || f2u(hi) != f2u(s.fsq_hi)) bad = 1;
        float e[NL_CHAIN_BINS + 1];
        host_edges(u2f(s.h_raw.res[0]), u2f(s.h_raw.res[1]), NL_CHAIN_BINS, e);
        if (memcmp(e, s.h_raw.edges, sizeof(e))) bad = 1;
    }
    {   // statistics -> normalisation -> exact threshold -> mask test
        const float max_abs32 = u2f(s.stats[0]), max_fsq32 = u2f(s.stats[1]);
        const float max_abs = max_abs32 <= 0.0f ? 1.0f : max_abs32;
        volatile float mf = sqrtf(max_fsq32); mf = mf / max_abs;
        volatile float mn = u2f(s.h_raw.res[0]) / max_abs, mx = u2f(s.h_raw.res[1]) / max_abs;
        if (f2u(max_abs) != f2u(s.max_abs) || f2u((float)mf) != f2u(s.max_frob) || f2u((float)mn) != f2u(s.nmn) || f2u((float)mx) != f2u(s.nmx) ||
            f2u(s.norm[0]) != f2u(max_abs) || s.norm[1] != 0.0f) bad = 1;
        float e[NL_CHAIN_BINS + 1];
        host_edges((float)mn, (float)mx, NL_CHAIN_BINS, e);
        if (memcmp(e, s.h_exact.edges, sizeof(e))) bad = 1;
        hist_thresholds_host<float>((const int64_t *)s.h_exact.counts, s.h_exact.edges, NL_CHAIN_BINS, &tri, &otsu, &st);
        const float thr = py_min_f((float)tri, (float)otsu);
        const float thr_cmp = (float)((double)thr / division);
        const float fsq_min = mask_threshold_on_fsq(max_abs, 1, thr_cmp);
        if (st || f2u(thr) != f2u(s.thr) || f2u(thr_cmp) != f2u(s.thr_cmp) || f2u(fsq_min) != f2u(s.fsq_min) || s.m_inf != ((0.0f > thr_cmp) ? 1 : 0)) bad = 1;
        if (!(fsq_min >= s.fsq_lo && fsq_min <= s.fsq_hi) || !((float)mf > thr_cmp)) bad = 1;      // (the kernel would have flagged these)
    }
    return bad ? NL_CF_VERIFY : 0;
}

extern "C" int nl_chain_begin(nl_ctx *c, int n_scales, char *err, size_t errlen) {
    NL_ENTER(c);
    if (n_scales < 1 || n_scales > NL_CHAIN_MAX_SCALES) return nl_fail(err, errlen, NL_EINVAL, "a chain holds 1..%d scales", NL_CHAIN_MAX_SCALES);
    if (!c->two_d && (!c->spec_ok || walk_plan(c, 2, c->own_lo, c->own_hi).family == WALK_ONE_VOXEL)) return nl_fail(err, errlen, NL_ESTATE, "the device-resident chain needs the 3-D one-pass walk");
    if (!c->d_chain) {
        NL_HIP(hipMalloc(&c->d_chain, sizeof(ChainScale) * NL_CHAIN_MAX_SCALES));
        NL_HIP(hipHostMalloc(&c->h_chain, sizeof(ChainScale) * NL_CHAIN_MAX_SCALES, hipHostMallocDefault));
        NL_HIP(hipEventCreateWithFlags(&c->ev_chain, hipEventDisableTiming));
    }
    chain_init_kernel<<<16, 256, 0, c->stream>>>((ChainScale *)c->d_chain, n_scales);
    chain_init2_kernel<<<1, 64, 0, c->stream>>>((ChainScale *)c->d_chain, n_scales);
    NL_CHECK_LAUNCH();
    c->chain_n = n_scales; c->chain_k = 0; c->chain_copy_pending = 0;
    c->def_resolve = 0;
    c->chain_reorder = 0; c->chain_steps = 0; c->chain_walked = 0;
    for (int v = 0; v < 3; ++v) { c->vol_scale[v] = -1; c->fsq_park[v].valid = 0; }
    // NELLIE_PREZERO=0: the frame's outputs are written densely, as before (read per frame: one process can run both ways).  A whole
    // 3-D volume on one context only: slabs, images and everything outside the chain keep the dense kernels.
    const char *e_pz = getenv("NELLIE_PREZERO");
    c->pz_on = (e_pz ? atoi(e_pz) != 0 : NL_PREZERO_DEFAULT) && !c->two_d && !c->comm && c->own_lo == 0 && c->own_hi == c->nzl && c->nzl == c->gnz;
    return NL_OK;
}

static int chain_first_round(nl_ctx *c, ChainScale *cs, i64 sz, i64 sy, i64 sx, double division, double margin, double test_scale, char *err, size_t errlen);
static int chain_walk_resolve(nl_ctx *c, ChainScale *cs, const double spacing[3], i64 sz, i64 sy, i64 sx, double alpha_sq, double beta_sq, double division,
                              int64_t z0, int64_t z1, char *err, size_t errlen);

// One scale of the frame, enqueued without a single wait: see chain.inc.  The Gaussian of the scale is current (nl_gauss_step).
extern "C" int nl_chain_scale(nl_ctx *c, const double spacing[3], int64_t sz, int64_t sy, int64_t sx, double alpha_sq, double beta_sq,
                              double division, double margin, double test_scale, int64_t z0, int64_t z1, char *err, size_t errlen) {
    NL_ENTER_KEEP_PZ(c);          // (the threshold kernels, the walk and the resolve kernel use no free volume)
    if (!c->d_chain || c->chain_k >= c->chain_n) return nl_fail(err, errlen, NL_ESTATE, "nl_chain_scale outside nl_chain_begin .. nl_chain_finish");
    if (!(division != 0.0)) return nl_fail(err, errlen, NL_EINVAL, "the chain needs a non-zero threshold division");
    int rc;
    if ((rc = set_spacing(c, spacing, err, errlen))) return rc;
    // the resolve kernel of the previous scale, held back until now: beside this scale's threshold kernels, behind its cascade step
    if ((rc = resolve_deferred_launch(c, true, err, errlen))) return rc;
    ChainScale *cs = (ChainScale *)c->d_chain + c->chain_k;
    c->chain_par[c->chain_k][0] = division; c->chain_par[c->chain_k][1] = margin; c->chain_par[c->chain_k][2] = test_scale;
    ++c->chain_k;
    c->frob_max_abs = 1.0f; c->frob_max_finite = 0.0f;                    // the bracket round: max_abs := 1 (pipeline.py _fsq_bracket)
    if (c->two_d) {
        // Round 6: images (im_info.no_z; filtering.py:675-690, 732-741) through the same records -- two passes, no walk and no queue: the
        // raw round only measures the sample range the exact round's edges are derived from (its "bracket" decides nothing: the caller passes
        // a margin of 1), the statistics kernel stands where the walk stands, and the vesselness kernel reads gamma_sq / fsq_min / m_inf
        // from the record as the resolve kernel does.  ~20 host round trips of a 2048^2 frame gone.
        if ((rc = sample_first_round(c, NL_FIELD_GAUSS, NL_FIELD_FROB, sz, sy, sx, NL_CHAIN_BINS, (char *)&cs->h_gauss, (char *)&cs->h_raw, nullptr, nullptr, true, err, errlen))) return rc;
        chain_thr1_kernel<<<2, 64, 0, c->stream>>>(cs, division, margin, test_scale, 0.0);
        if ((rc = hessian2d_stats_enqueue(c, cs->stats, err, errlen))) return rc;
        chain_post_kernel<<<1, 64, 0, c->stream>>>(cs);
        NL_CHECK_LAUNCH();
        // the exact round (an image lives on one context: no reduction)
        if ((rc = sample_exact_round(c, sz, sy, sx, NL_CHAIN_BINS, (char *)&cs->h_exact, cs->norm, c->stream, false, err, errlen))) return rc;
        chain_thr2_kernel<<<1, 64, 0, c->stream>>>(cs, division);
        NL_CHECK_LAUNCH();
        VessP vp{};
        vp.alpha_sq = (float)alpha_sq; vp.beta_sq = (float)beta_sq; vp.use_thr = 1;
        vp.cnt_lo = (int)c->own_lo; vp.cnt_hi = (int)c->own_hi;
        vp.first = c->mask_slots_used == 0 ? 1 : 0;
        vp.nan_flag = (unsigned int *)((char *)c->d_small + NL_NAN_FLAG_OFF);
        c->spec_valid = 0;
        return vesselness2d_enqueue(c, vp, &cs->cnt_resolve, (const float *)cs, err, errlen);
    }
    if ((rc = chain_first_round(c, cs, sz, sy, sx, division, margin, test_scale, err, errlen))) return rc;
    return chain_walk_resolve(c, cs, spacing, sz, sy, sx, alpha_sq, beta_sq, division, z0, z1, err, errlen);
}

// The two halves of a 3-D scale.  The first depends on the scale's Gaussian alone: the lattice samples (which fill the frob_sq cache),
// gamma, the bracket and the forecast of the mask fraction ...
static int chain_first_round(nl_ctx *c, ChainScale *cs, i64 sz, i64 sy, i64 sx, double division, double margin, double test_scale, char *err, size_t errlen) {
    int rc;
    if ((rc = sample_first_round(c, NL_FIELD_GAUSS, NL_FIELD_FROB, sz, sy, sx, NL_CHAIN_BINS, (char *)&cs->h_gauss, (char *)&cs->h_raw, nullptr, nullptr, true, err, errlen))) return rc;
    const i64 g_lo = c->gz0 + c->own_lo, g_hi = c->gz0 + c->own_hi;
    const i64 cz = (g_hi + sz - 1) / sz - (g_lo + sz - 1) / sz;
    const double n_lattice = (double)((cz > 0 ? cz : 0) * ((c->ny + sy - 1) / sy) * ((c->nx + sx - 1) / sx));
    chain_thr1_kernel<<<2, 64, 0, c->stream>>>(cs, division, margin, test_scale, n_lattice);
    NL_CHECK_LAUNCH();
    return NL_OK;
}
// ... the second joins the frame: the walk inside the masks of the scales walked so far, the exact threshold, the resolve kernel.
static int chain_walk_resolve(nl_ctx *c, ChainScale *cs, const double spacing[3], i64 sz, i64 sy, i64 sx, double alpha_sq, double beta_sq, double division,
                              int64_t z0, int64_t z1, char *err, size_t errlen) {
    int rc;
    if ((rc = spec_enqueue(c, spacing, 0.0f, 0.0f, z0, z1, cs->stats, &cs->cnt_walk, &cs->fsq_lo, err, errlen))) return rc;
    // (With the resolve kernel held back, the exact round of the scale on the side stream as well was measured: no gain, docs/HISTORY.md.)
    const bool defer = resolve_defer_ok(c) && c->fsq_cache_valid;     // (the cache is this scale's: the exact round below launches nothing to fill it)
    hipStream_t st = c->stream;
    chain_post_kernel<<<1, 64, 0, st>>>(cs);
    NL_CHECK_LAUNCH();
    // the exact round: edges from the normalised range, histogram of the cached frob_sq under the device's normalisation
    if ((rc = sample_exact_round(c, sz, sy, sx, NL_CHAIN_BINS, (char *)&cs->h_exact, cs->norm, st, true, err, errlen))) return rc;
    chain_thr2_kernel<<<1, 64, 0, st>>>(cs, division);
    NL_CHECK_LAUNCH();
    VessP vp{};
    vp.alpha_sq = (float)alpha_sq; vp.beta_sq = (float)beta_sq; vp.use_thr = 1;
    vp.cnt_lo = (int)c->own_lo; vp.cnt_hi = (int)c->own_hi;
    vp.first = c->mask_slots_used == 0 ? 1 : 0;
    if (defer) {
        memcpy(c->def_vp, &vp, sizeof(VessP));
        c->def_cnt = &cs->cnt_resolve; c->def_params = (const float *)cs; c->def_resolve = 1;
        return NL_OK;
    }
    return resolve_enqueue(c, vp, &cs->cnt_resolve, (const float *)cs, err, errlen);
}

// ---- the scales of a frame walked out of sigma order ---------------------------------------------------------------------------
// The frame's result is max_s(v_s) * AND_s(m_s): any walk order gives the same bits, and a walk queues only the voxels alive in the masks
// walked before it -- so the most selective masks should come first.  The cascade itself runs in sigma order; what can be delayed is a
// scale's walk, for as long as its Gaussian survives: the fused cascade step reads one ping-pong volume and writes one, so three
// consecutive Gaussians coexist.  nl_chain_begin_unordered starts such a frame.  After every nl_gauss_step the host calls nl_chain_sample(k)
// -- k in sigma order -- which makes scale k PENDING: its Gaussian stays in the volume the step wrote and its lattice cache is parked
// beside it.  nl_chain_walk(k) walks any pending scale and frees its volume.  nl_chain_estimates brings the forecasts of the mask
// fractions to the host, which picks the order (pipeline.py); the records, the flags and nl_chain_finish stay by sigma index.
extern "C" int nl_chain_begin_unordered(nl_ctx *c, int n_scales, char *err, size_t errlen) {
    int rc = nl_chain_begin(c, n_scales, err, errlen);
    if (rc) return rc;
    if (c->two_d || c->comm) { c->chain_n = 0; return nl_fail(err, errlen, NL_ESTATE, "scales out of sigma order: whole 3-D volumes on one context only"); }
    c->chain_reorder = 1;
    return NL_OK;
}

static void fsq_swap_parked(nl_ctx *c, int v) {
    nl_ctx::FsqPark &pk = c->fsq_park[v];
    std::swap(pk.p, c->d_fsq_cache); std::swap(pk.cap, c->fsq_cache_cap); std::swap(pk.valid, c->fsq_cache_valid);
    for (int i = 0; i < 3; ++i) std::swap(pk.key[i], c->fsq_cache_key[i]);
}

extern "C" int nl_chain_sample(nl_ctx *c, int k, const double spacing[3], int64_t sz, int64_t sy, int64_t sx, double division, double margin,
                               double test_scale, char *err, size_t errlen) {
    NL_ENTER_KEEP_PZ(c);
    if (!c->d_chain || !c->chain_reorder || c->chain_n < 1) return nl_fail(err, errlen, NL_ESTATE, "nl_chain_sample outside nl_chain_begin_unordered .. nl_chain_finish");
    if (k != c->chain_k || k >= c->chain_n) return nl_fail(err, errlen, NL_ESTATE, "nl_chain_sample(%d): scale %d is the next in sigma order", k, c->chain_k);
    if (c->chain_steps != k + 1 || c->gauss_ext) return nl_fail(err, errlen, NL_ESTATE, "nl_chain_sample(%d) without a cascade step of its own", k);
    if (!(division != 0.0)) return nl_fail(err, errlen, NL_EINVAL, "the chain needs a non-zero threshold division");
    int rc;
    if ((rc = set_spacing(c, spacing, err, errlen))) return rc;
    // the resolve kernel of the last walk, held back until now: beside these threshold kernels, behind the cascade step
    if ((rc = resolve_deferred_launch(c, true, err, errlen))) return rc;
    c->chain_par[k][0] = division; c->chain_par[k][1] = margin; c->chain_par[k][2] = test_scale;
    c->frob_max_abs = 1.0f; c->frob_max_finite = 0.0f;
    if ((rc = chain_first_round(c, (ChainScale *)c->d_chain + k, sz, sy, sx, division, margin, test_scale, err, errlen))) return rc;
    const int v = c->i_gauss;
    fsq_swap_parked(c, v);               // the cache just filled waits with the Gaussian; the buffer that comes back is nobody's
    c->fsq_cache_valid = 0;
    c->vol_scale[v] = k; c->chain_vol[k] = v;
    ++c->chain_k;
    return NL_OK;
}

// frac[0 .. n): the forecast mask fraction of every scale sampled so far (chain_thr1_kernel), < 0 where there is none (yet).  Waits for
// the sampling round of the newest scale -- the one wait a decision about the order costs; nothing the frame computes depends on it.
extern "C" int nl_chain_estimates(nl_ctx *c, float *frac, int n, char *err, size_t errlen) {
    NL_ENTER_KEEP_PZ(c);
    if (!c->d_chain || !c->chain_reorder || c->chain_n < 1) return nl_fail(err, errlen, NL_ESTATE, "nl_chain_estimates outside nl_chain_begin_unordered .. nl_chain_finish");
    if (!frac || n < 0 || n > NL_CHAIN_MAX_SCALES) return nl_fail(err, errlen, NL_EINVAL, "bad arguments");
    if (!c->h_chain_est) NL_HIP(hipHostMalloc((void **)&c->h_chain_est, sizeof(float) * NL_CHAIN_MAX_SCALES, hipHostMallocDefault));
    const int have = c->chain_k < n ? c->chain_k : n;
    for (int k = 0; k < have; ++k)
        NL_HIP(hipMemcpyAsync(c->h_chain_est + k, &((const ChainScale *)c->d_chain)[k].pred_frac, sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (have) NL_HIP(hipStreamSynchronize(c->stream));
    for (int k = 0; k < n; ++k) frac[k] = k < have ? c->h_chain_est[k] : -1.0f;
    return NL_OK;
}

extern "C" int nl_chain_walk(nl_ctx *c, int k, const double spacing[3], int64_t sz, int64_t sy, int64_t sx, double alpha_sq, double beta_sq,
                             double division, int64_t z0, int64_t z1, char *err, size_t errlen) {
    NL_ENTER_KEEP_PZ(c);
    if (!c->d_chain || !c->chain_reorder || c->chain_n < 1) return nl_fail(err, errlen, NL_ESTATE, "nl_chain_walk outside nl_chain_begin_unordered .. nl_chain_finish");
    if (k < 0 || k >= c->chain_k || ((c->chain_walked >> k) & 1u)) return nl_fail(err, errlen, NL_ESTATE, "nl_chain_walk(%d): the scale is not pending", k);
    const int v = c->chain_vol[k];
    if (c->vol_scale[v] != k) return nl_fail(err, errlen, NL_ESTATE, "nl_chain_walk(%d): its Gaussian is gone", k);
    int rc;
    if ((rc = set_spacing(c, spacing, err, errlen))) return rc;
    // two walks back to back, no sampling round in between: the resolve kernel of the first runs in line
    if ((rc = resolve_deferred_launch(c, false, err, errlen))) return rc;
    fsq_swap_parked(c, v);               // this scale's lattice cache becomes the current one
    c->frob_max_abs = 1.0f; c->frob_max_finite = 0.0f;
    const int newest = c->i_gauss;
    c->i_gauss = v;                      // gauss_cur(): the walk and the exact round read this scale's Gaussian
    rc = chain_walk_resolve(c, (ChainScale *)c->d_chain + k, spacing, sz, sy, sx, alpha_sq, beta_sq, division, z0, z1, err, errlen);
    c->i_gauss = newest;
    c->fsq_cache_valid = 0;              // (the cache describes volume v, no longer the current Gaussian)
    if (rc) return rc;
    c->vol_scale[v] = -1;
    c->chain_walked |= 1u << k;
    return NL_OK;
}

// Optional, before nl_chain_finish: start the download of the records now, so that work enqueued after this call (the samples
// of the frame's percentile threshold) runs on the device while nl_chain_finish waits for the records only and repeats the
// decisions on the host.
extern "C" int nl_chain_flush(nl_ctx *c, char *err, size_t errlen) {
    NL_ENTER_KEEP_PZ(c);
    if (!c->d_chain || c->chain_k < 1) return nl_fail(err, errlen, NL_ESTATE, "nl_chain_flush without scales");
    { int rcd = resolve_deferred_launch(c, false, err, errlen); if (rcd) return rcd; }       // the last scale's: nothing left to run beside
    NL_JOIN_SIDE(c);
    NL_HIP(hipMemcpyAsync(c->h_chain, c->d_chain, sizeof(ChainScale) * (size_t)c->chain_k, hipMemcpyDeviceToHost, c->stream));
    NL_HIP(hipEventRecord(c->ev_chain, c->stream));
    c->chain_copy_pending = 1;
    return NL_OK;
}

// The one wait of the frame: per scale flags (0 = the chain's result stands), gamma, max |H|, the Frobenius threshold and this
// context's h_mask count.  Any non-zero flag: redo the frame the synchronous way.
extern "C" int nl_chain_finish(nl_ctx *c, int *flags, double *gamma, double *max_abs, double *thr, int64_t *mask_count, char *err, size_t errlen) {
    NL_ENTER_KEEP_PZ(c);
    if (!c->d_chain || c->chain_k < 1) return nl_fail(err, errlen, NL_ESTATE, "nl_chain_finish without scales");
    const int n = c->chain_k;
    if (c->chain_reorder && c->chain_walked != (1u << n) - 1u) return nl_fail(err, errlen, NL_ESTATE, "nl_chain_finish while a sampled scale waits for its walk");
    if (!c->chain_copy_pending) { int rcd = resolve_deferred_launch(c, false, err, errlen); if (rcd) return rcd; }
    if (c->chain_copy_pending) {
        NL_HIP(hipEventSynchronize(c->ev_chain));
        c->chain_copy_pending = 0;
    } else {
        NL_JOIN_SIDE(c);
        NL_HIP(hipMemcpyAsync(c->h_chain, c->d_chain, sizeof(ChainScale) * (size_t)n, hipMemcpyDeviceToHost, c->stream));
        NL_HIP(hipStreamSynchronize(c->stream));
    }
    const ChainScale *h = (const ChainScale *)c->h_chain;
    for (int k = 0; k < n; ++k) {
        const int f = chain_verify(h[k], c->chain_par[k][0], c->chain_par[k][1], c->chain_par[k][2]);
        if (flags) flags[k] = f;
        if (gamma) gamma[k] = (double)h[k].gamma;
        if (max_abs) max_abs[k] = (double)h[k].max_abs;
        if (thr) thr[k] = (double)h[k].thr;
        if (mask_count) mask_count[k] = (int64_t)(h[k].cnt_walk + h[k].cnt_resolve);
    }
    c->chain_n = 0; c->pz_on = 0; c->chain_reorder = 0;
    return NL_OK;
}

// Test hook: the logged record of scale k after nl_chain_finish -- which: 0 Gaussian samples, 1 raw Frobenius samples, 2 normalised
// Frobenius samples; counts[256], edges[257], range[2] (min, max of the positive samples), scalars[8] = fsq_lo, fsq_hi, gamma_sq,
// fsq_min, thr_cmp, max_frob, tri, otsu (of that histogram).
extern "C" int nl_chain_log(nl_ctx *c, int k, int which, int64_t *counts, float *edges, float *range, double *scalars, char *err, size_t errlen) {
    if (!c || !c->h_chain || k < 0 || k >= NL_CHAIN_MAX_SCALES || which < 0 || which > 2) return nl_fail(err, errlen, NL_EINVAL, "bad chain log request");
    const ChainScale &s = ((const ChainScale *)c->h_chain)[k];
    const ChainHist &h = which == 0 ? s.h_gauss : (which == 1 ? s.h_raw : s.h_exact);
    if (counts) memcpy(counts, h.counts, sizeof(h.counts));
    if (edges) memcpy(edges, h.edges, sizeof(h.edges));
    if (range) { range[0] = u2f(h.res[0]); range[1] = u2f(h.res[1]); }
    if (scalars) {
        scalars[0] = s.fsq_lo; scalars[1] = s.fsq_hi; scalars[2] = s.gamma_sq; scalars[3] = s.fsq_min; scalars[4] = s.thr_cmp; scalars[5] = s.max_frob;
        scalars[6] = s.tri[which]; scalars[7] = s.otsu[which];
    }
    return NL_OK;
}

// ---- 2-D images (im_info.no_z) -----------------------------------------------------------------------------
int hessian2d_stats_enqueue(nl_ctx *c, unsigned int *res, char *err, size_t errlen) {
    ProfScope ps(c, "hessian_stats");
    hessian2d_stats_kernel<<<grid2d_rows(c->nx, c->ny), 256, 0, c->stream>>>(gauss_cur(c), geom(c), hessp(c), res);
    NL_CHECK_LAUNCH();
    return NL_OK;
}
int vesselness2d_enqueue(nl_ctx *c, const VessP &vp0, unsigned long long *d_cnt, const float *dev_params, char *err, size_t errlen) {
    VessP vp = vp0;
    ProfScope ps(c, "vesselness");
    const int k_scale = c->mask_slots_used++;
    vp.have_prev = k_scale > 0;
    const MaskSlots ms = mask_slots(c, k_scale);
    if (vp.first && !vmax_is_zero(c, 0, c->nzl)) NL_HIP(hipMemsetAsync(c->f[c->i_vmax], 0, (size_t)c->n * 4, c->stream));
    c->vmax_zero_hi = 0;
    vesselness2d_kernel<<<grid2d_rows((i64)ms.wpr * 64, c->ny), 256, 0, c->stream>>>(gauss_cur(c), c->f[c->i_vmax], ms.cm, ms.pm, ms.wpr, geom(c), hessp(c), vp, d_cnt,
                                                                                      dev_params);
    NL_CHECK_LAUNCH();
    return NL_OK;
}

extern "C" int nl_set_ndim(nl_ctx *c, int ndim, char *err, size_t errlen) {
    NL_ENTER(c);
    if (ndim != 2 && ndim != 3) return nl_fail(err, errlen, NL_EINVAL, "ndim must be 2 or 3");
    if (ndim == 2 && (c->nzl != 1 || c->gnz != 1)) return nl_fail(err, errlen, NL_EINVAL, "a 2-D context has exactly one plane");
    c->two_d = ndim == 2;
    c->fsq_cache_valid = 0;
    return NL_OK;
}

// One sigma of filtering.py:779-789.  w?2 / w?0 = scipy's order-2 / order-0 Gaussian kernels (2r+1 float64 weights,
// symmetric) for the Y and X axes; s2 = float32(sigma**2).
extern "C" int nl_log2d_step(nl_ctx *c, const double *wy2, const double *wy0, const double *wx2, const double *wx0, int r,
                             float s2, int first, int use_mask, char *err, size_t errlen) {
    NL_ENTER(c);
    if (!c->two_d) return nl_fail(err, errlen, NL_ESTATE, "nl_log2d_step on a 3-D context");
    if (!wy2 || !wy0 || !wx2 || !wx0) return nl_fail(err, errlen, NL_EINVAL, "weights are NULL");
    NL_JOIN_SIDE(c);
    for (int k = 0; k < 4; ++k)
        if (!c->d_2d[k]) NL_HIP(hipMalloc((void **)&c->d_2d[k], (size_t)c->n * 4));
    GaussW gy2, gy0, gx2, gx0;
    int rc;
    if ((rc = fill_gw(gy2, wy2, r, err, errlen)) || (rc = fill_gw(gy0, wy0, r, err, errlen)) ||
        (rc = fill_gw(gx2, wx2, r, err, errlen)) || (rc = fill_gw(gx0, wx0, r, err, errlen))) return rc;
    const VolGeom v = geom(c);
    const dim3 grid((unsigned)((c->nx + 255) / 256), (unsigned)c->ny, 1);
    ProfScope ps(c, "log2d");
    const float *src = gauss_cur(c);
    float *t = c->d_2d[0], *A = c->d_2d[1], *B = c->d_2d[2], *lap = c->d_2d[3];
    // gaussian_laplace: second derivative along Y (then plain Gaussian along X), plus the one along X.  Both terms in one walk over
    // the image (the pair kernel of Markers' LoG: A = XY(gy2, gx0) + XY(gy0, gx2), the float32 sum the combine kernel forms) when
    // the radius allows; four one-axis passes otherwise.
    bool summed = false;
    if (gyx_tiled() && r >= 1 && r <= GM_MAX_R && r <= c->ny && r <= c->nx) {
        const GaussWS wya = gauss_ws_of(gy2), wxa = gauss_ws_of(gx0), wyb = gauss_ws_of(gy0), wxb = gauss_ws_of(gx2);
        const dim3 g2((unsigned)((c->nx + GYX_COLS - 1) / GYX_COLS), (unsigned)((c->ny + v.chunk - 1) / v.chunk), 1);
        (void)gl_yx_dual(c, false, r, src, A, v, 0, 1, wya, wxa, wyb, wxb, g2);
        summed = true;
    } else {
        gl_axis(1, false, c, grid, src, t, v, 0, 1, gy2);
        gl_axis(2, false, c, grid, t, A, v, 0, 1, gx0);
        gl_axis(1, false, c, grid, src, t, v, 0, 1, gy0);
        gl_axis(2, false, c, grid, t, B, v, 0, 1, gx2);
    }
    const int wpr = (int)((c->nx + 63) / 64);
    const i64 slot_words = c->nzl * c->ny * wpr;
    const unsigned long long *mask = c->mask_slots_used > 0
        ? (const unsigned long long *)c->m[0] + (i64)((c->mask_slots_used - 1) & 1) * slot_words : nullptr;
    log2d_combine_kernel<<<grid2d_rows(c->nx, c->ny), 256, 0, c->stream>>>(A, summed ? nullptr : B, s2, use_mask ? mask : nullptr, wpr, v, first, lap);
    NL_CHECK_LAUNCH();
    return NL_OK;
}

// filtering.py:792-795 and 928-930: scale the blob response to [0, 0.1] and take the maximum with NL_FIELD_FRANGI
// (call after nl_filter_finish).
extern "C" int nl_log2d_finish(nl_ctx *c, int64_t *n_positive, char *err, size_t errlen) {
    NL_ENTER(c);
    if (!c->two_d || !c->d_2d[3]) return nl_fail(err, errlen, NL_ESTATE, "nl_log2d_finish before nl_log2d_step");
    unsigned int *res = (unsigned int *)c->d_small;
    unsigned long long *d_pos = (unsigned long long *)c->d_small + 2;
    NL_HIP(zero_small(res, 32, c->stream));
    ProfScope ps(c, "log2d");
    // (1024 workgroups: both kernels end in one atomic per workgroup on one word -- 8192 of them were 80 of the apply kernel's 99 us at 2048^2)
    log2d_clip_max_kernel<<<grid1d(c->n, 256, 1024), 256, 0, c->stream>>>(c->d_2d[3], c->n, res);
    NL_CHECK_LAUNCH();
    NL_HIP(hipMemcpyAsync(c->h_small, res, 4, hipMemcpyDeviceToHost, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    float mx;
    memcpy(&mx, c->h_small, 4);
    const float denom = mx + 1e-12f;                      // float32 + weak python float
    log2d_apply_kernel<<<grid1d(c->n, 256, 1024), 256, 0, c->stream>>>(c->d_2d[3], denom, c->f[c->i_vmax], c->n, d_pos);
    NL_CHECK_LAUNCH();
    NL_HIP(hipMemcpyAsync(c->h_small, d_pos, 8, hipMemcpyDeviceToHost, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    if (n_positive) *n_positive = (int64_t)(*(unsigned long long *)c->h_small);
    return NL_OK;
}

extern "C" int nl_filter_finish(nl_ctx *c, int64_t z0, int64_t z1, int64_t *n_positive, char *err, size_t errlen) {
    NL_ENTER(c);
    if (z0 < 0 && z1 < 0) { z0 = c->own_lo; z1 = c->own_hi; }
    if (z0 < 0 || z1 > c->nzl || z0 >= z1) return nl_fail(err, errlen, NL_EINVAL, "bad plane range [%lld,%lld)", (i64)z0, (i64)z1);
    NL_JOIN_SIDE(c);
    unsigned long long *d_cnt = (unsigned long long *)c->d_small;
    NL_HIP(zero_small(d_cnt, 8, c->stream));
    const i64 plane = c->ny * c->nx;
    if (c->mask_slots_used == 0 && !vmax_is_zero(c, z0, z1))       // every scale was skipped: vesselness was never written
        NL_HIP(hipMemsetAsync(c->f[c->i_vmax] + z0 * plane, 0, (size_t)(z1 - z0) * plane * 4, c->stream));
    c->vmax_zero_hi = 0;
    {
        ProfScope ps(c, "finish");
        const int wpr = (int)((c->nx + 63) / 64);
        const i64 quads = (z1 - z0) * c->ny * ((c->nx + 3) / 4);
        const i64 slot_words = c->nzl * c->ny * wpr;
        const int last = c->mask_slots_used > 0 ? ((c->mask_slots_used - 1) & 1) : 0;      // the slot of the last scale = AND of all
        finish_kernel<<<grid1d(quads, 256, 256 * 16), 256, 0, c->stream>>>(c->f[c->i_vmax], (const unsigned long long *)c->m[0] + last * slot_words,
                                                               c->mask_slots_used > 0 ? 1 : 0, slot_words, wpr, geom(c), z0, z1, c->own_lo, c->own_hi, d_cnt);
        NL_CHECK_LAUNCH();
    }
    NL_HIP(hipMemcpyAsync(c->h_small, d_cnt, 8, hipMemcpyDeviceToHost, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    if (n_positive) *n_positive = (int64_t)(*(unsigned long long *)c->h_small);
    c->frangi_ready = 1;
    return NL_OK;
}

// filtering.py:931-932, 969-1000: `_remove_edges` on the resident `vesselness * masks` frame (after nl_filter_finish),
// owned planes; *n_positive = values > 0 left on them.
extern "C" int nl_remove_edges(nl_ctx *c, int margin, int64_t *n_positive, char *err, size_t errlen) {
    NL_ENTER(c);
    NL_JOIN_SIDE(c);
    if (!c->frangi_ready) return nl_fail(err, errlen, NL_ESTATE, "nl_remove_edges before a Frangi frame exists");
    if (margin < 0) return nl_fail(err, errlen, NL_EINVAL, "margin %d is negative", margin);
    unsigned long long *d_cnt = (unsigned long long *)c->d_small;
    NL_HIP(zero_small(d_cnt, 8, c->stream));
    {
        ProfScope ps(c, "finish");
        // the same planes nl_filter_finish materialises: nl_mask_volume thresholds and opens own +- 2, so the ghost planes
        // of a Z slab must lose their edge rows too (each plane is trimmed on its own: no cross-plane dependency)
        const i64 r0 = c->own_lo - 2 > 0 ? c->own_lo - 2 : 0, r1 = c->own_hi + 2 < c->nzl ? c->own_hi + 2 : c->nzl;
        remove_edges_kernel<<<(unsigned)(r1 - r0), 256, 0, c->stream>>>(c->f[c->i_vmax], geom(c), r0, margin, c->own_lo, c->own_hi, d_cnt);
        NL_CHECK_LAUNCH();
    }
    NL_HIP(hipMemcpyAsync(c->h_small, d_cnt, 8, hipMemcpyDeviceToHost, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    if (n_positive) *n_positive = (int64_t)(*(unsigned long long *)c->h_small);
    return NL_OK;
}

// filtering.py:964-966 on the finished frame; thr_dev != NULL: the threshold is read from device memory (nl_mask_volume_dev)
static int mask_volume_enqueue(nl_ctx *c, float thr, const float *thr_dev, int *dst_out, char *err, size_t errlen) {
    // result goes to a free gauss volume, which then becomes the Frangi volume
    int dst = -1;
    for (int k = 0; k < 3; ++k) if (k != c->i_gauss) { dst = k; break; }
    *dst_out = dst;
    ProfScope ps(c, "mask_volume");
    const int wpr = (int)((c->nx + 63) / 64);
    const VolGeom v = geom(c);
    // planes whose bits exist: own +-2 clipped to the slab (ghost planes beyond a true face do not exist)
    const i64 m0 = c->own_lo - 2 > 0 ? c->own_lo - 2 : 0, m1 = c->own_hi + 2 < c->nzl ? c->own_hi + 2 : c->nzl;
    const i64 e0 = c->own_lo - 1 > 0 ? c->own_lo - 1 : 0, e1 = c->own_hi + 1 < c->nzl ? c->own_hi + 1 : c->nzl;
    unsigned long long *bM = (unsigned long long *)c->m[1], *bE = (unsigned long long *)c->m[2], *bD = (unsigned long long *)c->m[0];
    nl_launch_threshold_pack(grid1d((m1 - m0) * c->ny * 64, 256, (i64)1 << 22), c->stream,
        c->f[c->i_vmax] + m0 * c->ny * c->nx, nullptr, bM + m0 * c->ny * wpr, 1, thr, (int)c->nx, (m1 - m0) * c->ny, wpr, thr_dev);
    NL_CHECK_LAUNCH();
    bits_morph6_kernel<0><<<(unsigned)(((e1 - e0) * c->ny * wpr + 255) / 256), 256, 0, c->stream>>>(bM, bE, v, wpr, e0, e1, c->two_d);
    NL_CHECK_LAUNCH();
    bits_morph6_kernel<1><<<(unsigned)(((c->own_hi - c->own_lo) * c->ny * wpr + 255) / 256), 256, 0, c->stream>>>(bE, bD, v, wpr, c->own_lo, c->own_hi, c->two_d);
    NL_CHECK_LAUNCH();
    apply_bits_kernel<<<grid1d((c->own_hi - c->own_lo) * c->ny * ((c->nx + 3) / 4), 256, 256 * 32), 256, 0, c->stream>>>(
        c->f[c->i_vmax], bD, c->f[dst], v, wpr, c->own_lo, c->own_hi);
    NL_CHECK_LAUNCH();
    return NL_OK;
}
static void mask_volume_commit(nl_ctx *c, int dst) {       // swap roles: the old vmax volume joins the gauss ping-pong set
    float *tmp = c->f[c->i_vmax];
    c->f[c->i_vmax] = c->f[dst];
    c->f[dst] = tmp;
}

extern "C" int nl_mask_volume(nl_ctx *c, float thr, char *err, size_t errlen) {
    NL_ENTER(c);
    int dst, rc;
    if ((rc = mask_volume_enqueue(c, thr, nullptr, &dst, err, errlen))) return rc;
    mask_volume_commit(c, dst);
    return NL_OK;
}

// The kernels of the fused epilogue; thr_dev != NULL: the threshold is read from device memory (nl_tail_enqueue).
// Writes the masked frame into the free volume *dst_out; the caller commits it (swap with i_vmax) or not.
static int mask_volume_fused_enqueue(nl_ctx *c, float thr, const float *thr_dev, unsigned long long *d_cnt, int *dst_out, char *err, size_t errlen) {
    int dst = -1;
    for (int k = 0; k < 3; ++k) if (k != c->i_gauss && !pz_is(c, c->f[k])) { dst = k; break; }      // (not the pre-zeroed label volume)
    if (dst < 0) for (int k = 0; k < 3; ++k) if (k != c->i_gauss) { dst = k; break; }
    pz_touch(c, c->f[dst]);
    *dst_out = dst;
    NL_HIP(zero_small(d_cnt, 8, c->stream));
    ProfScope ps(c, "mask_volume");
    const int wpr = (int)((c->nx + 63) / 64);
    const VolGeom v = geom(c);
    const i64 slot_words = c->nzl * c->ny * wpr;
    const int last = (c->mask_slots_used - 1) & 1;
    const unsigned long long *alive = (const unsigned long long *)c->m[0] + (i64)last * slot_words;
    // the threshold bits may not overwrite the mask slot they are computed from: m[1] / m[2] hold them, the free
    // slot of m[0] takes the opened mask
    const i64 m0 = c->own_lo - 2 > 0 ? c->own_lo - 2 : 0, m1 = c->own_hi + 2 < c->nzl ? c->own_hi + 2 : c->nzl;
    const i64 e0 = c->own_lo - 1 > 0 ? c->own_lo - 1 : 0, e1 = c->own_hi + 1 < c->nzl ? c->own_hi + 1 : c->nzl;
    unsigned long long *bM = (unsigned long long *)c->m[1], *bE = (unsigned long long *)c->m[2];
    unsigned long long *bD = (unsigned long long *)c->m[0] + (i64)(last ^ 1) * slot_words;
    pack_masked_kernel<<<grid1d((m1 - m0) * c->ny * 64, 256, 256 * 16), 256, 0, c->stream>>>(    // one atomic per workgroup: small grid
        c->f[c->i_vmax], alive, bM, thr, thr_dev, (int)c->nx, m0 * c->ny, m1 * c->ny, wpr, c->own_lo * c->ny, c->own_hi * c->ny, d_cnt);
    NL_CHECK_LAUNCH();
    bits_morph6_kernel<0><<<(unsigned)(((e1 - e0) * c->ny * wpr + 255) / 256), 256, 0, c->stream>>>(bM, bE, v, wpr, e0, e1, c->two_d);
    NL_CHECK_LAUNCH();
    bits_morph6_kernel<1><<<(unsigned)(((c->own_hi - c->own_lo) * c->ny * wpr + 255) / 256), 256, 0, c->stream>>>(bE, bD, v, wpr, c->own_lo, c->own_hi, c->two_d);
    NL_CHECK_LAUNCH();
    apply_bits_pos_kernel<<<grid1d(((c->own_hi - c->own_lo) * c->ny + APPLY_ROWS - 1) / APPLY_ROWS * 64, 256, (i64)1 << 22), 256, 0, c->stream>>>(    // a wave takes APPLY_ROWS rows
        c->f[c->i_vmax], bD, c->f[dst], v, wpr, c->own_lo, c->own_hi);
    NL_CHECK_LAUNCH();
    // a fused communicator: the count comes back GLOBAL (one collective on the stream instead of a host-level all-reduce behind the call)
    if (fused(c)) return reduce_u64_sum(c, d_cnt, 1, err, errlen);
    return NL_OK;
}
static void mask_volume_fused_commit(nl_ctx *c, int dst) {
    float *tmp = c->f[c->i_vmax];
    c->f[c->i_vmax] = c->f[dst];
    c->f[dst] = tmp;
    c->frangi_ready = 1;
    // valid as long as only NL_KEEP_SUPPORT entry points follow; on a slab it describes the OWNED planes (all nl_slab_label_pack reads)
    c->d_support = (const unsigned long long *)c->m[0] + (i64)(((c->mask_slots_used - 1) & 1) ^ 1) * (c->nzl * c->ny * (i64)((c->nx + 63) / 64));
    c->support_epoch = c->epoch.load();
}

extern "C" int nl_mask_volume_fused(nl_ctx *c, float thr, int64_t *n_positive, char *err, size_t errlen) {
    NL_ENTER_KEEP_PZ(c);
    if (c->mask_slots_used == 0) return nl_fail(err, errlen, NL_ESTATE, "nl_mask_volume_fused before any scale was evaluated");
    NL_JOIN_SIDE(c);
    unsigned long long *d_cnt = (unsigned long long *)c->d_small;
    int dst, rc;
    if ((rc = mask_volume_fused_enqueue(c, thr, nullptr, d_cnt, &dst, err, errlen))) return rc;
    NL_HIP(hipMemcpyAsync(c->h_small, d_cnt, 8, hipMemcpyDeviceToHost, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    if (n_positive) *n_positive = (int64_t)(*(unsigned long long *)c->h_small);
    mask_volume_fused_commit(c, dst);
    return NL_OK;
}

// ---- the frame's epilogue without a host decision in it (percentile.inc) ------------------------------------------------------
// layout of d_pct: [PctRec 64 B][sample counter 4 B, pad][voxel counter 8 B][hist 2 x PCT_BINS u32]
static int pct_buffers(nl_ctx *c, char *err, size_t errlen) {
    if (!c->d_pct) {
        NL_HIP(hipMalloc(&c->d_pct, 128 + (size_t)2 * PCT_BINS * 4));
        NL_HIP(hipHostMalloc(&c->h_pct, 128, hipHostMallocDefault));
    }
    return NL_OK;
}
// numpy.percentile(samples[0 .. *d_n), q) -> rec->thr, selected on the device (all-reduced across a fused communicator)
static int pct_enqueue(nl_ctx *c, const float *samples, const unsigned int *d_n, i64 max_n, float q, char *err, size_t errlen) {
    PctRec *rec = (PctRec *)c->d_pct;
    unsigned int *hist = (unsigned int *)((char *)c->d_pct + 128);
    NL_HIP(hipMemcpyAsync(&rec->n, d_n, 4, hipMemcpyDeviceToDevice, c->stream));
    NL_HIP(hipMemcpyAsync(&rec->n_local, d_n, 4, hipMemcpyDeviceToDevice, c->stream));
    int rc;
    if (fused(c) && (rc = reduce_u32_sum(c, &rec->n, 1, err, errlen))) return rc;
    ProfScope ps(c, "sample");
    pct_begin_kernel<<<1, 64, 0, c->stream>>>(rec, q);
    const unsigned grid = grid1d(max_n > 0 ? max_n : 1, 256, 256 * 256);
#define NL_PCT_LEVEL(L)                                                                                            \
    NL_HIP(hipMemsetAsync(hist, 0, (size_t)2 * PCT_BINS * 4, c->stream));                                           \
    pct_hist_kernel<L><<<grid, 256, 0, c->stream>>>(samples, d_n, rec, hist);                                       \
    if (fused(c) && (rc = reduce_u32_sum(c, hist, (size_t)2 * PCT_BINS, err, errlen))) return rc;                    \
    pct_select_kernel<L><<<1, 256, 0, c->stream>>>(rec, hist);
    NL_PCT_LEVEL(0) NL_PCT_LEVEL(1) NL_PCT_LEVEL(2)
#undef NL_PCT_LEVEL
    NL_CHECK_LAUNCH();
    return NL_OK;
}

/* filtering.py:926 + 952-967 in one enqueue, no host decision inside: the positive lattice samples of `vesselness * masks`
   (strides sz, sy, sx), their q-th percentile (numpy's float32 'linear' rule, selected on the device), the percentile mask, its
   opening and the product.  Nothing is committed yet: nl_tail_finish waits, reports and (commit != 0) makes the result the frame. */
extern "C" int nl_tail_enqueue(nl_ctx *c, int64_t sz, int64_t sy, int64_t sx, double q, char *err, size_t errlen) {
    NL_ENTER_KEEP_PZ(c);
    if (c->mask_slots_used == 0) return nl_fail(err, errlen, NL_ESTATE, "nl_tail_enqueue before any scale was evaluated");
    if (c->two_d) return nl_fail(err, errlen, NL_EINVAL, "nl_tail_enqueue is the 3-D epilogue");
    int rc;
    if ((rc = pct_buffers(c, err, errlen))) return rc;
    float *stage = c->f[(c->i_gauss + 1) % 3];
    if (stage == c->f[c->i_vmax]) return nl_fail(err, errlen, NL_ESTATE, "no free volume for the samples");
    // the pre-zeroed label volume is that very volume (the one after the current Gaussian): the samples borrow its first `total` words,
    // which are zeroed again once the percentile is selected (a few MB)
    const bool stage_pz = pz_is(c, stage);
    unsigned int *d_n = (unsigned int *)((char *)c->d_pct + 64);
    unsigned long long *d_cnt = (unsigned long long *)((char *)c->d_pct + 72);
    i64 total;
    if ((rc = sample_gather_pos_enqueue(c, NL_FIELD_VESSELNESS, sz, sy, sx, stage, d_n, c->n, &total, err, errlen))) return rc;       // (joins the side stream)
    if (total > c->n) return nl_fail(err, errlen, NL_EINVAL, "lattice larger than the volume");
    if ((rc = pct_enqueue(c, stage, d_n, total, (float)q, err, errlen))) return rc;
    if (stage_pz && total > 0) NL_HIP(hipMemsetAsync(stage, 0, (size_t)total * 4, c->stream));
    // the samples sit in a volume the epilogue may write (dst): the selection above is complete before it does (stream order)
    int dst;
    if ((rc = mask_volume_fused_enqueue(c, 0.0f, &((PctRec *)c->d_pct)->thr, d_cnt, &dst, err, errlen))) return rc;
    NL_HIP(hipMemcpyAsync(c->h_pct, c->d_pct, 80, hipMemcpyDeviceToHost, c->stream));
    c->tail_pending = 1; c->tail_dst = dst;
    return NL_OK;
}

extern "C" int nl_tail_finish(nl_ctx *c, int commit, int64_t *n_samples, float *a, float *b, float *gamma, float *thr, int64_t *n_positive,
                              char *err, size_t errlen) {
    NL_ENTER_KEEP_PZ(c);
    if (!c->tail_pending) return nl_fail(err, errlen, NL_ESTATE, "nl_tail_finish without nl_tail_enqueue");
    NL_HIP(hipStreamSynchronize(c->stream));
    c->tail_pending = 0;
    const PctRec *rec = (const PctRec *)c->h_pct;
    if (n_samples) *n_samples = rec->n;
    if (a) *a = rec->a;
    if (b) *b = rec->b;
    if (gamma) *gamma = rec->gamma;
    if (thr) *thr = rec->thr;
    if (n_positive) *n_positive = (int64_t)(*(const unsigned long long *)((const char *)c->h_pct + 72));
    if (commit && rec->n > 0) mask_volume_fused_commit(c, c->tail_dst);
    return NL_OK;
}

/* _mask_volume (filtering.py:952-967) on the finished frame with the percentile selected on the device: the positive lattice samples
   of the Frangi frame, their q-th percentile, `frame > thr`, the opening and the product, one wait.  n_samples = 0: nothing was
   changed (the reference returns the frame as it is).  The epilogue of 2-D images, of remove_edges runs, of slabs without the
   fused epilogue; 3-D frames normally take nl_tail_enqueue. */
extern "C" int nl_mask_volume_dev(nl_ctx *c, int64_t sz, int64_t sy, int64_t sx, double q, int64_t *n_samples, float *a, float *b, float *gamma,
                                  float *thr, char *err, size_t errlen) {
    NL_ENTER(c);
    int rc;
    if ((rc = pct_buffers(c, err, errlen))) return rc;
    float *stage = nullptr;                                  // a free volume: neither the frame nor the current Gaussian
    for (int k = 0; k < 3; ++k) if (k != c->i_gauss && c->f[k] != c->f[c->i_vmax]) stage = c->f[k];
    if (!stage) return nl_fail(err, errlen, NL_ESTATE, "no free volume for the samples");
    unsigned int *d_n = (unsigned int *)((char *)c->d_pct + 64);
    i64 total;
    if ((rc = sample_gather_pos_enqueue(c, NL_FIELD_FRANGI, sz, sy, sx, stage, d_n, c->n, &total, err, errlen))) return rc;
    if (total > c->n) return nl_fail(err, errlen, NL_EINVAL, "lattice larger than the volume");
    if ((rc = pct_enqueue(c, stage, d_n, total, (float)q, err, errlen))) return rc;
    int dst;
    if ((rc = mask_volume_enqueue(c, 0.0f, &((PctRec *)c->d_pct)->thr, &dst, err, errlen))) return rc;
    NL_HIP(hipMemcpyAsync(c->h_pct, c->d_pct, 64, hipMemcpyDeviceToHost, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    const PctRec *rec = (const PctRec *)c->h_pct;
    if (n_samples) *n_samples = rec->n;
    if (a) *a = rec->a;
    if (b) *b = rec->b;
    if (gamma) *gamma = rec->gamma;
    if (thr) *thr = rec->thr;
    if (rec->n > 0) mask_volume_commit(c, dst);
    return NL_OK;
}

/* numpy.percentile(values, q) by the device's selection (tests): values > 0, n < the context's voxel count */
extern "C" int nl_debug_percentile(nl_ctx *c, const float *values, int64_t n, double q, float *thr, float *a, float *b, char *err, size_t errlen) {
    NL_ENTER(c);
    if (!values || n < 1 || n > c->n) return nl_fail(err, errlen, NL_EINVAL, "bad sample array");
    int rc;
    if ((rc = pct_buffers(c, err, errlen))) return rc;
    float *stage = c->f[(c->i_gauss + 1) % 3];
    unsigned int *d_n = (unsigned int *)((char *)c->d_pct + 64);
    const unsigned int un = (unsigned int)n;
    NL_HIP(hipMemcpyAsync(stage, values, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    NL_HIP(hipMemcpyAsync(d_n, &un, 4, hipMemcpyHostToDevice, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    const int keep = c->fuse_reduce; c->fuse_reduce = 0;                 // a local array: no collective
    rc = pct_enqueue(c, stage, d_n, n, (float)q, err, errlen);
    c->fuse_reduce = keep;
    if (rc) return rc;
    NL_HIP(hipMemcpyAsync(c->h_pct, c->d_pct, 64, hipMemcpyDeviceToHost, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    const PctRec *rec = (const PctRec *)c->h_pct;
    if (thr) *thr = rec->thr;
    if (a) *a = rec->a;
    if (b) *b = rec->b;
    return NL_OK;
}

int store_planes(nl_ctx *c, const void *dev_base, void *host, size_t elem, int64_t z0, int64_t z1, char *err, size_t errlen) {
    if (!host || z0 < 0 || z1 > c->nzl || z0 >= z1) return nl_fail(err, errlen, NL_EINVAL, "bad plane range [%lld,%lld)", (i64)z0, (i64)z1);
    const i64 plane = c->ny * c->nx;
    NL_HIP(hipMemcpyAsync(host, (const char *)dev_base + (size_t)z0 * plane * elem, (size_t)(z1 - z0) * plane * elem,
                          hipMemcpyDeviceToHost, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    return NL_OK;
}

extern "C" int nl_filter_store(nl_ctx *c, float *host, int64_t z0, int64_t z1, char *err, size_t errlen) {
    NL_ENTER_KEEP_PZ(c);
    NL_KEEP_LABBITS(c);
    NL_KEEP_SUPPORT(c);
    return store_planes(c, c->f[c->i_vmax], host, 4, z0, z1, err, errlen);
}
extern "C" int nl_gauss_store(nl_ctx *c, float *host, int64_t z0, int64_t z1, char *err, size_t errlen) {
    NL_ENTER(c);
    return store_planes(c, gauss_cur(c), host, 4, z0, z1, err, errlen);
}

// ------------------------------------------------------------------------------ slab helpers ----

extern "C" int nl_planes_get(nl_ctx *c, int field, int64_t z0, int64_t z1, float *host, char *err, size_t errlen) {
    NL_ENTER(c);
    float *p = field_ptr(c, field);
    if (!p) return nl_fail(err, errlen, NL_EINVAL, "nl_planes_get: field %d has no volume", field);
    return store_planes(c, p, host, 4, z0, z1, err, errlen);
}

extern "C" int nl_planes_put(nl_ctx *c, int field, int64_t z0, int64_t z1, const float *host, char *err, size_t errlen) {
    NL_ENTER(c);
    float *p = field_ptr(c, field);
    c->fsq_cache_valid = 0;
    if (!p || !host || z0 < 0 || z1 > c->nzl || z0 >= z1) return nl_fail(err, errlen, NL_EINVAL, "nl_planes_put: bad field or plane range");
    const i64 plane = c->ny * c->nx;
    NL_HIP(hipMemcpyAsync(p + z0 * plane, host, (size_t)(z1 - z0) * plane * 4, hipMemcpyHostToDevice, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    return NL_OK;
}



// ---------------------------------------------------------------------------------- debug -------
extern "C" int nl_ctx_info(nl_ctx *c, const char *key, double *value) {
    if (!c || !key || !value) return NL_EINVAL;
    if (!strcmp(key, "fast_div")) *value = c->fast_div2 ? 2 : c->fast_div;      // 2: two-instruction division proven, 1: three, 0: float64
    else if (!strcmp(key, "hessian_tile_rows")) *value = walk_plan(c, 0, c->own_lo, c->own_hi).ty;
    else if (!strcmp(key, "hv_variants")) *value = NL_HV_VARIANTS;               // 1: a build with the rejected forms of the walk (nellie_hv.hip)
    else if (!strcmp(key, "vesselness_one_pass")) *value = c->spec_ok;
    else if (!strcmp(key, "chain_available")) *value = (c->two_d || (c->spec_ok && walk_plan(c, 2, c->own_lo, c->own_hi).family != WALK_ONE_VOXEL)) ? 1 : 0;   // nl_chain_begin's own precondition
    else if (!strcmp(key, "last_fsq_min")) *value = c->last_fsq_min;
    else if (!strcmp(key, "last_spec_overflow")) *value = c->last_spec_overflow;
    else if (!strcmp(key, "last_label_sparse")) *value = c->last_label_sparse;
    else if (!strcmp(key, "last_label_path")) *value = c->last_label_path;     // which implementation nl_label_run's last frame used (nl_common.h)
    else if (!strcmp(key, "prezero_used")) *value = c->prezero_used;        // bit 1: the last frame's labels were painted into a pre-zeroed volume (bit 0, the Frangi volume: never)
    else if (!strcmp(key, "device_bytes")) *value = (double)nl_ctx_bytes(c->nzl, c->ny, c->nx);
    else if (!strcmp(key, "gauss_yx_max_r")) *value = getenv("NELLIE_NO_FUSED_YX") ? 0 : GM_MAX_R;   // largest in-plane radius whose Y and X passes share a kernel
    else if (!strcmp(key, "queue_entries")) {
        // entries the last one-pass walk (nl_vesselness_spec / a chain scale) left in the eigen queue: the sum of the per-wave region counts
        // (waits for the stream; bench.py's fused-design byte model prices the walk's stores and the resolve kernel's reads with it)
        if (hipSetDevice(c->device) != hipSuccess) return NL_EHIP;
        if (c->side_pending && hipStreamSynchronize(c->side) != hipSuccess) return NL_EHIP;
        const unsigned nreg = c->spec_nregions;
        std::vector<unsigned int> h(nreg);
        if (nreg && (hipMemcpyAsync(h.data(), c->d_vq_count, (size_t)nreg * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                     hipStreamSynchronize(c->stream) != hipSuccess)) return NL_EHIP;
        double t = 0.0;
        for (unsigned k = 0; k < nreg; ++k) t += (double)h[k];
        *value = t;
    }
    else if (!strcmp(key, "nan_hessian")) {
        // Filter.run(mask=False) only: 1 if a Hessian with a NaN entry reached the eigen-solver since the frame began (waits for the stream)
        if (hipSetDevice(c->device) != hipSuccess) return NL_EHIP;
        unsigned int flag = 0;
        if (c->side_pending && hipStreamSynchronize(c->side) != hipSuccess) return NL_EHIP;
        if (hipMemcpyAsync(&flag, (char *)c->d_small + NL_NAN_FLAG_OFF, 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess) return NL_EHIP;
        *value = flag ? 1.0 : 0.0;
    }
    else return NL_EINVAL;
    return NL_OK;
}

// --------------------------------------------------------------------------------- timing -------
extern "C" int nl_timer_begin(nl_ctx *c, char *err, size_t errlen) {
    NL_ENTER(c);
    NL_HIP(hipEventRecord(c->t0, c->stream));
    return NL_OK;
}
extern "C" int nl_timer_end_ms(nl_ctx *c, float *ms, char *err, size_t errlen) {
    NL_ENTER(c);
    NL_HIP(hipEventRecord(c->t1, c->stream));
    NL_HIP(hipEventSynchronize(c->t1));
    float t = 0;
    NL_HIP(hipEventElapsedTime(&t, c->t0, c->t1));
    if (ms) *ms = t;
    return NL_OK;
}
extern "C" int nl_prof_enable(nl_ctx *c, int on) {
    if (!c) return NL_OK;
    if (on && !c->prof_on) {                 // stock the pool outside the timed region
        hipSetDevice(c->device);
        size_t used = 0;
        for (auto &kv : c->prof) used += kv.second.size();
        while (c->prof_pool.size() + used < 1024) {
            ProfRec r;
            if (hipEventCreate(&r.a) != hipSuccess) break;
            if (hipEventCreate(&r.b) != hipSuccess) { hipEventDestroy(r.a); break; }
            c->prof_pool.push_back(r);
        }
    }
    c->prof_on = on;
    return NL_OK;
}
extern "C" int nl_prof_reset(nl_ctx *c) {
    if (!c) return NL_OK;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    hipStreamSynchronize(c->side);
    for (auto &kv : c->prof) for (auto &r : kv.second) c->prof_pool.push_back(r);       // kept for the next scopes
    c->prof.clear();
    c->prof_sum.clear();
    return NL_OK;
}
extern "C" int nl_prof_get(nl_ctx *c, const char *name, double *ms, int64_t *launches) {
    if (!c || !name) return NL_EINVAL;
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    hipStreamSynchronize(c->side);
    if (c->xstream) hipStreamSynchronize(c->xstream);
    prof_harvest(c, true);
    double tot = 0; int64_t k = 0;
    auto it = c->prof_sum.find(name);
    if (it != c->prof_sum.end()) { tot = it->second.first; k = it->second.second; }
    if (ms) *ms = tot;
    if (launches) *launches = k;
    return NL_OK;
}
