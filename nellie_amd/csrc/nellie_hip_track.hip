// Translation unit of libnellie_hip.so (gfx950): Hu-moment marker tracking (nellie/tracking/hu_tracking.py).  C-ABI in
// include/nellie_amd.h; kernels in track.inc.  A tracker owns its buffers and stream: it needs none of a Filter context's volumes.
#include "nl_stage.h"
#include "track.inc"

struct TrkSlot {
    int *coord = nullptr;    // (cap, 3) int32 z, y, x (z = 0 for 2-D)
    double *phys = nullptr;  // (cap, 3)
    int *rad = nullptr;      // (cap)
    float *stats = nullptr;  // (cap, 4)
    double *hu = nullptr;    // (cap, 18)
    i64 n = 0, cap = 0;
};

struct nl_track : StageBase {      // times nothing: no event pair
    int two_d = 0;
    i64 nz = 0, ny = 0, nx = 0, n = 0;
    void *d_int = nullptr; i64 int_bytes = 0;
    float *d_fr = nullptr, *d_dist = nullptr;
    uint8_t *d_mk = nullptr;
    unsigned int *d_blk = nullptr;
    unsigned int *d_small = nullptr, *h_small = nullptr;   // [0] marker total, [1] frangi min key, [2] max radius
    double *d_scale = nullptr;
    TrkSlot slot[2];
    int cur = 0, frames = 0;
    double *d_part = nullptr; i64 part_cap = 0;            // per-row partial sums of a frame pair
    double *d_mom = nullptr;                                // means / stds (2 x 23)
    int *d_idx = nullptr; float *d_val = nullptr; i64 res_cap = 0;   // row results | column results
};

extern "C" int nl_track_destroy(nl_track *t) {
    if (!t) return NL_OK;
    std::vector<void *> ps = {t->d_int, t->d_fr, t->d_dist, t->d_mk, t->d_blk, t->d_small, t->d_scale, t->d_part, t->d_mom, t->d_idx, t->d_val};
    for (const TrkSlot &s : t->slot) ps.insert(ps.end(), {s.coord, s.phys, s.rad, s.stats, s.hu});
    stage_close(*t, ps, {t->h_small});
    delete t;
    return NL_OK;
}

extern "C" int nl_track_create(nl_track **out, int device, int ndim, int64_t nz, int64_t ny, int64_t nx, const double *spacing,
                               char *err, size_t errlen) {
    if (!out) return nl_fail(err, errlen, NL_EINVAL, "out is NULL");
    *out = nullptr;
    if (ndim == 2) nz = 1;
    if (int rc = stage_check_frame(ndim, spacing, nz, ny, nx, err, errlen)) return rc;
    if (ny > INT32_MAX || nx > INT32_MAX || nz > INT32_MAX || nz * ny * nx > ((i64)1 << 40)) return nl_fail(err, errlen, NL_EINVAL, "bad frame shape");
    if (int rc = stage_check_device(device, err, errlen)) return rc;
    nl_track *t = new nl_track();
    t->two_d = ndim == 2;
    t->nz = nz; t->ny = ny; t->nx = nx; t->n = nz * ny * nx;
    if (int rc = stage_open(*t, device, false, err, errlen)) { nl_track_destroy(t); return rc; }
    const i64 nblk = (t->n + TRK_CHUNK - 1) / TRK_CHUNK;
    STAGE_HIP(stage_alloc(&t->d_fr, t->n, 4), nl_track_destroy(t));
    STAGE_HIP(stage_alloc(&t->d_dist, t->n, 4), nl_track_destroy(t));
    STAGE_HIP(stage_alloc(&t->d_mk, t->n, 1), nl_track_destroy(t));
    STAGE_HIP(stage_alloc(&t->d_blk, nblk, 4), nl_track_destroy(t));
    STAGE_HIP(stage_alloc(&t->d_small, 16, 4), nl_track_destroy(t));
    STAGE_HIP(hipHostMalloc((void **)&t->h_small, 64, hipHostMallocDefault), nl_track_destroy(t));
    STAGE_HIP(stage_alloc(&t->d_scale, 3, 8), nl_track_destroy(t));
    STAGE_HIP(stage_alloc(&t->d_mom, 2 * TRK_NF_MAX, 8), nl_track_destroy(t));
    double sc[3] = {ndim == 2 ? 1.0 : spacing[0], spacing[ndim == 2 ? 0 : 1], spacing[ndim == 2 ? 1 : 2]};
    STAGE_HIP(hipMemcpy(t->d_scale, sc, 24, hipMemcpyHostToDevice), nl_track_destroy(t));
    *out = t;
    return NL_OK;
}

// Uploads one frame, computes its features into the current slot; the previous frame's features stay resident as "pre".
extern "C" int nl_track_frame(nl_track *t, const void *intensity, int dtype, const float *frangi, const float *distance,
                              const uint8_t *marker, int64_t *n_markers, char *err, size_t errlen) {
    STAGE_ENTER(t, "tracker");
    if (!intensity || !frangi || !distance || !marker) return nl_fail(err, errlen, NL_EINVAL, "NULL frame");
    if (dtype != NL_U8 && dtype != NL_U16 && dtype != NL_F32)
        return nl_fail(err, errlen, NL_EINVAL, "tracking intensities must be uint8, uint16 or float32 (dtype code %d)", dtype);
    const size_t esz = dtype_size(dtype);
    if (int rc = stage_grow(&t->int_bytes, t->n * (i64)esz, t->n * (i64)esz, {{&t->d_int, 1}}, err, errlen)) return rc;
    hipStream_t st = t->stream;
    NL_HIP(hipMemcpyAsync(t->d_int, intensity, (size_t)t->n * esz, hipMemcpyHostToDevice, st));
    NL_HIP(hipMemcpyAsync(t->d_fr, frangi, (size_t)t->n * 4, hipMemcpyHostToDevice, st));
    NL_HIP(hipMemcpyAsync(t->d_dist, distance, (size_t)t->n * 4, hipMemcpyHostToDevice, st));
    NL_HIP(hipMemcpyAsync(t->d_mk, marker, (size_t)t->n, hipMemcpyHostToDevice, st));
    NL_HIP(hipMemsetAsync(t->d_small, 0, 16, st));
    NL_HIP(hipMemsetAsync(t->d_small + 1, 0xff, 4, st));
    const i64 nblk = (t->n + TRK_CHUNK - 1) / TRK_CHUNK;
    trk_mark_count_kernel<<<(unsigned)nblk, 256, 0, st>>>(t->d_mk, t->n, t->d_blk);
    NL_CHECK_LAUNCH();
    trk_scan_kernel<<<1, 1024, 0, st>>>(t->d_blk, nblk, t->d_small);
    NL_CHECK_LAUNCH();
    NL_HIP(hipMemcpyAsync(t->h_small, t->d_small, 4, hipMemcpyDeviceToHost, st));
    NL_HIP(hipStreamSynchronize(st));
    const i64 n = t->h_small[0];
    if (t->frames > 0) t->cur ^= 1;
    ++t->frames;
    TrkSlot &s = t->slot[t->cur];
    s.n = 0;
    *n_markers = n;
    if (n == 0) return NL_OK;
    if (int rc = stage_grow(&s.cap, n, stage_doubled(s.cap, n), {{&s.coord, 12}, {&s.phys, 24}, {&s.rad, 4}, {&s.stats, 16}, {&s.hu, 8 * TRK_NH_MAX}},
                            err, errlen)) return rc;
    trk_mark_write_kernel<<<(unsigned)nblk, 256, 0, st>>>(t->d_mk, t->n, t->d_blk, s.coord, (int)t->ny, (int)t->nx);
    NL_CHECK_LAUNCH();
    trk_frangi_log_kernel<<<grid1d(t->n), 256, 0, st>>>(t->d_fr, t->n, t->d_small + 1);
    NL_CHECK_LAUNCH();
    trk_frangi_shift_kernel<<<grid1d(t->n), 256, 0, st>>>(t->d_fr, t->n, t->d_small + 1);
    NL_CHECK_LAUNCH();
    trk_radius_kernel<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(s.coord, (int)n, t->d_dist, (int)t->nz, (int)t->ny, (int)t->nx,
                                                                    t->d_scale, s.phys, s.rad, (int *)(t->d_small + 2));
    NL_CHECK_LAUNCH();
    NL_HIP(hipMemcpyAsync(t->h_small + 2, t->d_small + 2, 4, hipMemcpyDeviceToHost, st));
    NL_HIP(hipStreamSynchronize(st));
    const int rmax = (int)t->h_small[2];
    const int R = 2 * rmax + 1;
    if (R > 125)
        return nl_fail(err, errlen, NL_EINVAL, "marker radius %d exceeds the feature kernel's ROI tile (distance values above 31)", rmax);
    TrkFrame F{(int)t->nz, (int)t->ny, (int)t->nx, t->two_d, R, t->d_fr, s.coord, s.rad, s.stats, s.hu};
    const size_t lds = (size_t)R * R * 4;
    switch (dtype) {
        case NL_U8: trk_features_kernel<uint8_t><<<(unsigned)n, 256, lds, st>>>((const uint8_t *)t->d_int, F); break;
        case NL_U16: trk_features_kernel<uint16_t><<<(unsigned)n, 256, lds, st>>>((const uint16_t *)t->d_int, F); break;
        default: trk_features_kernel<float><<<(unsigned)n, 256, lds, st>>>((const float *)t->d_int, F); break;
    }
    NL_CHECK_LAUNCH();
    s.n = n;
    return NL_OK;
}

// Downloads a slot's features (which = 0: the last frame, 1: the one before): coords (n, ndim) int64, stats (n, 4) float32,
// log-Hu (n, 6 | 18) float64.  NULL pointers are skipped.
extern "C" int nl_track_features(nl_track *t, int which, int64_t *coords, float *stats, double *hu, char *err, size_t errlen) {
    STAGE_ENTER(t, "tracker");
    if (which != 0 && which != 1) return nl_fail(err, errlen, NL_EINVAL, "which must be 0 or 1");
    if (which == 1 && t->frames < 2) return nl_fail(err, errlen, NL_ESTATE, "no previous frame");
    TrkSlot &s = t->slot[which == 0 ? t->cur : t->cur ^ 1];
    if (s.n == 0) return NL_OK;
    const int nh = t->two_d ? 6 : 18;
    if (coords) {
        std::vector<int> c((size_t)s.n * 3);
        NL_HIP(hipMemcpyAsync(c.data(), s.coord, c.size() * 4, hipMemcpyDeviceToHost, t->stream));
        NL_HIP(hipStreamSynchronize(t->stream));
        const int d = t->two_d ? 2 : 3;
        for (i64 k = 0; k < s.n; ++k)
            for (int a = 0; a < d; ++a) coords[k * d + a] = c[k * 3 + 3 - d + a];
    }
    if (stats) NL_HIP(hipMemcpyAsync(stats, s.stats, (size_t)s.n * 16, hipMemcpyDeviceToHost, t->stream));
    if (hu) NL_HIP(hipMemcpyAsync(hu, s.hu, (size_t)s.n * nh * 8, hipMemcpyDeviceToHost, t->stream));
    NL_HIP(hipStreamSynchronize(t->stream));
    return NL_OK;
}

// Matches the last frame (post, rows) against the one before (pre, columns).  mode 0: dense, 1: sparse.  Outputs: row_idx /
// row_cost (n_post) and col_idx / col_cost (n_pre); an index of -1 has no candidate (sparse).  full (dense only, may be NULL):
// the (n_post, n_pre) float16 cost matrix.
extern "C" int nl_track_match(nl_track *t, int mode, double max_distance, int32_t *row_idx, float *row_cost, int32_t *col_idx,
                              float *col_cost, uint16_t *full, char *err, size_t errlen) {
    STAGE_ENTER(t, "tracker");
    if (t->frames < 2) return nl_fail(err, errlen, NL_ESTATE, "nl_track_match needs two frames");
    if (mode != 0 && mode != 1) return nl_fail(err, errlen, NL_EINVAL, "mode must be 0 (dense) or 1 (sparse)");
    if (mode == 1 && full) return nl_fail(err, errlen, NL_EINVAL, "the full cost matrix is a dense-mode output");
    const TrkSlot &a = t->slot[t->cur], &b = t->slot[t->cur ^ 1];
    if (a.n == 0 || b.n == 0) return NL_OK;
    const int nh = t->two_d ? 6 : 18, nf = 5 + nh;
    TrkPair P{(int)a.n, (int)b.n, t->two_d ? 2 : 3, nh, a.phys, b.phys, a.stats, b.stats, a.hu, b.hu, max_distance};
    hipStream_t st = t->stream;
    const i64 pw = mode == 0 ? 1 + nf : 1 + 2 * nf;
    if (int rc = stage_grow(&t->part_cap, a.n * pw, stage_doubled(t->part_cap, a.n * pw), {{&t->d_part, 8}}, err, errlen)) return rc;
    if (int rc = stage_grow(&t->res_cap, a.n + b.n, stage_doubled(t->res_cap, a.n + b.n), {{&t->d_idx, 4}, {&t->d_val, 4}}, err, errlen)) return rc;
    uint16_t *d_full = nullptr;
    const unsigned gr = (unsigned)((a.n + 127) / 128), gc = (unsigned)((b.n + 127) / 128);
    if (mode == 0) {
        if (full) NL_HIP(hipMalloc((void **)&d_full, (size_t)a.n * b.n * 2));
        trk_dense_rowsum_kernel<<<gr, 128, 0, st>>>(P, nullptr, t->d_part);
        trk_colsum_kernel<<<1, 64, 0, st>>>(t->d_part, (int)a.n, nf, 0, t->d_mom);
        trk_dense_rowsum_kernel<<<gr, 128, 0, st>>>(P, t->d_mom, t->d_part);
        trk_colsum_kernel<<<1, 64, 0, st>>>(t->d_part, (int)a.n, nf, 1, t->d_mom + TRK_NF_MAX);
        trk_dense_min_kernel<<<gr, 128, 0, st>>>(P, t->d_mom, t->d_mom + TRK_NF_MAX, 0, t->d_idx, t->d_val, d_full);
        trk_dense_min_kernel<<<gc, 128, 0, st>>>(P, t->d_mom, t->d_mom + TRK_NF_MAX, 1, t->d_idx + a.n, t->d_val + a.n, nullptr);
    } else {
        trk_sparse_rowsum_kernel<<<gr, 128, 0, st>>>(P, t->d_part);
        trk_sparse_moments_kernel<<<1, 64, 0, st>>>(t->d_part, (int)a.n, nf, t->d_mom);
        trk_sparse_min_kernel<<<gr, 128, 0, st>>>(P, t->d_mom, 0, t->d_idx, t->d_val);
        trk_sparse_min_kernel<<<gc, 128, 0, st>>>(P, t->d_mom, 1, t->d_idx + a.n, t->d_val + a.n);
    }
    hipError_t le = hipGetLastError();
    if (le != hipSuccess) {
        if (d_full) hipFree(d_full);
        return nl_fail(err, errlen, NL_EHIP, "tracking match launch: %s", hipGetErrorString(le));
    }
    NL_HIP(hipMemcpyAsync(row_idx, t->d_idx, (size_t)a.n * 4, hipMemcpyDeviceToHost, st));
    NL_HIP(hipMemcpyAsync(row_cost, t->d_val, (size_t)a.n * 4, hipMemcpyDeviceToHost, st));
    NL_HIP(hipMemcpyAsync(col_idx, t->d_idx + a.n, (size_t)b.n * 4, hipMemcpyDeviceToHost, st));
    NL_HIP(hipMemcpyAsync(col_cost, t->d_val + a.n, (size_t)b.n * 4, hipMemcpyDeviceToHost, st));
    if (d_full) NL_HIP(hipMemcpyAsync(full, d_full, (size_t)a.n * b.n * 2, hipMemcpyDeviceToHost, st));
    hipError_t se = hipStreamSynchronize(st);
    if (d_full) hipFree(d_full);
    NL_HIP(se);
    return NL_OK;
}

// Host copies of the float16 helpers the dense matcher runs on the device (checked against numpy by the CPU tests).
extern "C" int nl_host_half_round(const double *in, uint16_t *out, int64_t n, char *err, size_t errlen) {
    if ((!in || !out) && n > 0) return nl_fail(err, errlen, NL_EINVAL, "NULL buffer");
    for (int64_t i = 0; i < n; ++i) out[i] = trk_f64_to_f16(in[i]);
    return NL_OK;
}

extern "C" int nl_host_half_nansum(const uint16_t *in, int64_t rows, int k, uint16_t *out, char *err, size_t errlen) {
    if (k < 1 || k > TRK_NF_MAX) return nl_fail(err, errlen, NL_EINVAL, "row length must be 1..%d", TRK_NF_MAX);
    if ((!in || !out) && rows > 0) return nl_fail(err, errlen, NL_EINVAL, "NULL buffer");
    for (int64_t r = 0; r < rows; ++r) out[r] = trk_half_nansum(in + r * k, k);
    return NL_OK;
}

// Host copy of numpy's float32 np.sum of a flat array, the order of the feature kernel's float stats.
extern "C" int nl_host_np_sum_f32(const float *in, int64_t n, float *out, char *err, size_t errlen) {
    if (!out || (!in && n > 0) || n < 0) return nl_fail(err, errlen, NL_EINVAL, "NULL buffer or negative length");
    *out = trk_np_sum_f32(in, n);
    return NL_OK;
}
