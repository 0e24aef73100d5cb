// Translation unit of libnellie_hip.so (gfx950): the analysis overlay (nellie_napari/nellie_analysis.py:955-1218).  C-ABI in
// include/nellie_amd.h; kernels in overlay.inc.  An overlay handle is made for one frame shape and owns its buffers and stream: the
// 1-bit mask of the loaded frame with its scanned word populations, the rows' groups, the column, the rows' values and the painted
// frame.  The label frame is uploaded into the painted frame's buffer: it is not needed once the mask stands.
#include "nl_stage.h"
#include "overlay.inc"

#define OV_MAX_ROWS ((i64)1 << 30)          // labelled voxels per frame: rows are ints
#define OV_MAX_GROUP ((i64)0x7ffffffe)      // group indices are ints below OV_NO_GROUP
#define OV_MS_PARTS 3                       // load, values, paint

struct nl_overlay : StageBase {
    int ndim = 3;
    i64 n = 0, words = 0;             // voxels; mask words (a multiple of 4: one workgroup of rank_mask_kernel writes 4)
    u64 *d_bits = nullptr;
    int *d_wcount = nullptr, *d_wpre = nullptr;
    RankScan scan;
    void *d_out = nullptr;            // n x 8 bytes: the painted frame; the label frame on its way to the mask
    i64 V = -1;                       // rows of the loaded frame, -1: none
    int *d_group = nullptr; i64 *d_off = nullptr; double *d_val = nullptr; i64 row_cap = 0;
    int *d_idx = nullptr; i64 idx_cap = 0;
    double *d_attr = nullptr; i64 attr_cap = 0;
    int grouping = 0;                 // 0 none, 1 one group per row, 2 CSR
    i64 max_group = -1;
    bool valued = false;
    int painted = -1;                 // the element kind of d_out: 0 float64, 1 float32, 2 uint64; -1: not painted
    float ms[OV_MS_PARTS] = {0.f, 0.f, 0.f};
};

extern "C" int nl_overlay_destroy(nl_overlay *h) {
    if (!h) return NL_OK;
    stage_close(*h, {h->d_bits, h->d_wcount, h->d_wpre, h->scan.d_bsum, h->scan.d_total, h->d_out, h->d_group, h->d_off, h->d_val, h->d_idx, h->d_attr},
                {h->scan.h_total});
    delete h;
    return NL_OK;
}

extern "C" int nl_overlay_create(nl_overlay **out, int device, int ndim, int64_t nz, int64_t ny, int64_t nx, char *err, size_t errlen) {
    if (!out) return nl_fail(err, errlen, NL_EINVAL, "out is NULL");
    *out = nullptr;
    const double unit[3] = {1.0, 1.0, 1.0};
    if (int rc = stage_check_frame(ndim, unit, nz, ny, nx, err, errlen)) return rc;
    if (int rc = stage_check_device(device, err, errlen)) return rc;
    nl_overlay *h = new nl_overlay();
    h->ndim = ndim;
    h->n = nz * ny * nx;
    h->words = ((h->n + 255) / 256) * 4;
    if (int rc = stage_open(*h, device, true, err, errlen)) { nl_overlay_destroy(h); return rc; }
    STAGE_HIP(stage_alloc(&h->d_bits, h->words, 8), nl_overlay_destroy(h));
    STAGE_HIP(stage_alloc(&h->d_wcount, h->words, 4), nl_overlay_destroy(h));
    STAGE_HIP(stage_alloc(&h->d_wpre, h->words, 4), nl_overlay_destroy(h));
    STAGE_HIP(stage_alloc((char **)&h->d_out, h->n, 8), nl_overlay_destroy(h));
    STAGE_HIP(stage_alloc(&h->scan.d_bsum, rank_scan_sums(h->words), 8), nl_overlay_destroy(h));
    STAGE_HIP(stage_alloc(&h->scan.d_total, 1, 8), nl_overlay_destroy(h));
    STAGE_HIP(hipHostMalloc((void **)&h->scan.h_total, 8, hipHostMallocDefault), nl_overlay_destroy(h));
    *out = h;
    return NL_OK;
}

// The label frame (int32, the handle's shape) goes up; its labels > 0 mask and the scan of the word populations give every set
// voxel its row.  n_rows = V, the labelled voxels.  Forgets the groups, the values and the painted frame of the frame before.
extern "C" int nl_overlay_load(nl_overlay *h, const int32_t *labels, int64_t *n_rows, char *err, size_t errlen) {
    STAGE_ENTER(h, "overlay");
    if (!labels || !n_rows) return nl_fail(err, errlen, NL_EINVAL, "labels or n_rows is NULL");
    *n_rows = 0;
    h->V = -1;
    h->grouping = 0;
    h->valued = false;
    h->painted = -1;
    for (float &m : h->ms) m = 0.f;
    hipStream_t st = h->stream;
    int *frame = (int *)h->d_out;
    NL_HIP(hipMemcpyAsync(frame, labels, (size_t)h->n * 4, hipMemcpyHostToDevice, st));
    if (int rc = stage_start(*h, err, errlen)) return rc;
    rank_mask_kernel<<<(unsigned)((h->n + 255) / 256), 256, 0, st>>>(OvLabelled{frame}, h->n, h->d_bits, h->d_wcount);
    NL_CHECK_LAUNCH();
    i64 total = 0;
    if (int rc = rank_scan(h->scan, st, h->d_wcount, h->words, h->d_wpre, OV_MAX_ROWS, "labelled voxels in one frame", &total, err, errlen)) return rc;
    if (int rc = stage_stop(*h, &h->ms[0], err, errlen)) return rc;
    if (int rc = stage_grow(&h->row_cap, total + 1, total + 1, {{&h->d_group, 4}, {&h->d_off, 8}, {&h->d_val, 8}}, err, errlen)) return rc;
    h->V = total;
    *n_rows = total;
    return NL_OK;
}

// The groups of the rows: group != NULL: one per row (V ints, -1: none); else a CSR: offsets (V + 1, from 0, not decreasing, ending
// at n_idx) and idx (n_idx group indices).  A group index is 0 .. 2^31 - 2.  Stays until the next nl_overlay_load.
extern "C" int nl_overlay_groups(nl_overlay *h, const int32_t *group, const int64_t *offsets, const int32_t *idx, int64_t n_idx, char *err,
                                 size_t errlen) {
    STAGE_ENTER(h, "overlay");
    if (h->V < 0) return nl_fail(err, errlen, NL_ESTATE, "nl_overlay_groups needs nl_overlay_load");
    h->grouping = 0;
    h->valued = false;
    const i64 V = h->V;
    i64 top = -1;
    if (group) {
        for (i64 r = 0; r < V; ++r) {
            if (group[r] < -1 || (i64)group[r] > OV_MAX_GROUP) return nl_fail(err, errlen, NL_EINVAL, "row %lld holds group %d", (long long)r, (int)group[r]);
            if (group[r] > top) top = group[r];
        }
        if (V > 0) NL_HIP(hipMemcpyAsync(h->d_group, group, (size_t)V * 4, hipMemcpyHostToDevice, h->stream));
    } else {
        if (!offsets || n_idx < 0 || (n_idx > 0 && !idx)) return nl_fail(err, errlen, NL_EINVAL, "neither groups nor a CSR");
        if (offsets[0] != 0 || offsets[V] != n_idx) return nl_fail(err, errlen, NL_EINVAL, "the offsets start at 0 and end at n_idx");
        for (i64 r = 0; r < V; ++r)
            if (offsets[r + 1] < offsets[r]) return nl_fail(err, errlen, NL_EINVAL, "the offsets decrease at row %lld", (long long)r);
        for (i64 j = 0; j < n_idx; ++j) {
            if (idx[j] < 0 || (i64)idx[j] > OV_MAX_GROUP) return nl_fail(err, errlen, NL_EINVAL, "edge %lld holds group %d", (long long)j, (int)idx[j]);
            if (idx[j] > top) top = idx[j];
        }
        if (int rc = stage_grow(&h->idx_cap, n_idx, n_idx, {{&h->d_idx, 4}}, err, errlen)) return rc;
        NL_HIP(hipMemcpyAsync(h->d_off, offsets, (size_t)(V + 1) * 8, hipMemcpyHostToDevice, h->stream));
        if (n_idx > 0) NL_HIP(hipMemcpyAsync(h->d_idx, idx, (size_t)n_idx * 4, hipMemcpyHostToDevice, h->stream));
    }
    NL_HIP(hipStreamSynchronize(h->stream));            // the host arrays may go away after the call
    h->grouping = group ? 1 : 2;
    h->max_group = top;
    return NL_OK;
}

// The rows' values.  direct = 0: attr is the column by group index (n_attr entries, above the largest group index of the rows): a
// row gets the mean over its distinct groups whose entry is not NaN, NaN without one.  The sum is np.sum's over the dense column
// (absent and NaN entries +0.0): pairwise = 0: one add per entry in ascending order; else pairwise trees over pieces of 8192 entries.
// direct != 0: attr holds the rows' values themselves (n_attr = V; the voxel level).
extern "C" int nl_overlay_values(nl_overlay *h, const double *attr, int64_t n_attr, int direct, int pairwise, char *err, size_t errlen) {
    STAGE_ENTER(h, "overlay");
    if (h->V < 0) return nl_fail(err, errlen, NL_ESTATE, "nl_overlay_values needs nl_overlay_load");
    if (n_attr < 0 || (n_attr > 0 && !attr)) return nl_fail(err, errlen, NL_EINVAL, "attr is NULL");
    h->valued = false;
    hipStream_t st = h->stream;
    const i64 V = h->V;
    h->ms[1] = 0.f;
    if (direct) {
        if (n_attr != V) return nl_fail(err, errlen, NL_EINVAL, "%lld values for %lld rows", (long long)n_attr, (long long)V);
        if (V > 0) NL_HIP(hipMemcpyAsync(h->d_val, attr, (size_t)V * 8, hipMemcpyHostToDevice, st));
        NL_HIP(hipStreamSynchronize(st));
    } else {
        if (!h->grouping) return nl_fail(err, errlen, NL_ESTATE, "nl_overlay_values needs nl_overlay_groups");
        if (n_attr <= h->max_group)
            return nl_fail(err, errlen, NL_EINVAL, "a column of %lld entries for group indices up to %lld", (long long)n_attr, (long long)h->max_group);
        if (int rc = stage_upload(*h, (void **)&h->d_attr, &h->attr_cap, attr, n_attr, 8, err, errlen)) return rc;
        if (int rc = stage_start(*h, err, errlen)) return rc;
        if (V > 0) {
            const unsigned gv = (unsigned)((V + 255) / 256);
            if (h->grouping == 1) ov_values_single_kernel<<<gv, 256, 0, st>>>(h->d_group, V, h->d_attr, n_attr, h->d_val);
            else ov_values_csr_kernel<<<gv, 256, 0, st>>>(h->d_off, h->d_idx, V, h->d_attr, n_attr, pairwise ? 1 : 0, h->d_val);
            NL_CHECK_LAUNCH();
        }
        if (int rc = stage_stop(*h, &h->ms[1], err, errlen)) return rc;
    }
    h->valued = true;
    return NL_OK;
}

// The dense frame: the value of its row at every labelled voxel; kind 0: float64, NaN elsewhere; 1: float32 (the float64 value
// rounded once), NaN elsewhere; 2: uint64 labels -- the truncated value, 0 where it is NaN, negative, infinite or 2^64 and above,
// and 0 elsewhere.
extern "C" int nl_overlay_paint(nl_overlay *h, int kind, char *err, size_t errlen) {
    STAGE_ENTER(h, "overlay");
    if (kind < 0 || kind > 2) return nl_fail(err, errlen, NL_EINVAL, "kind must be 0, 1 or 2");
    if (h->V < 0 || !h->valued) return nl_fail(err, errlen, NL_ESTATE, "nl_overlay_paint needs nl_overlay_load and nl_overlay_values");
    hipStream_t st = h->stream;
    h->painted = -1;
    h->ms[2] = 0.f;
    const i64 per = kind == 1 ? 4 : 2;
    const unsigned grid = (unsigned)(((h->n + per - 1) / per + 255) / 256);
    if (int rc = stage_start(*h, err, errlen)) return rc;
    if (kind == 0) ov_paint_kernel<double><<<grid, 256, 0, st>>>(h->d_bits, h->d_wpre, h->d_val, h->n, (double *)h->d_out);
    else if (kind == 1) ov_paint_kernel<float><<<grid, 256, 0, st>>>(h->d_bits, h->d_wpre, h->d_val, h->n, (float *)h->d_out);
    else ov_paint_kernel<u64><<<grid, 256, 0, st>>>(h->d_bits, h->d_wpre, h->d_val, h->n, (u64 *)h->d_out);
    NL_CHECK_LAUNCH();
    if (int rc = stage_stop(*h, &h->ms[2], err, errlen)) return rc;
    h->painted = kind;
    return NL_OK;
}

// The rows' values, V float64.
extern "C" int nl_overlay_fetch_values(nl_overlay *h, double *values, char *err, size_t errlen) {
    STAGE_ENTER(h, "overlay");
    if (h->V < 0 || !h->valued) return nl_fail(err, errlen, NL_ESTATE, "nl_overlay_fetch_values needs nl_overlay_values");
    if (h->V > 0) {
        if (!values) return nl_fail(err, errlen, NL_EINVAL, "values is NULL");
        NL_HIP(hipMemcpyAsync(values, h->d_val, (size_t)h->V * 8, hipMemcpyDeviceToHost, h->stream));
        NL_HIP(hipStreamSynchronize(h->stream));
    }
    return NL_OK;
}

// The painted frame in the element type of the last nl_overlay_paint, the handle's shape.
extern "C" int nl_overlay_fetch_frame(nl_overlay *h, void *frame, char *err, size_t errlen) {
    STAGE_ENTER(h, "overlay");
    if (h->painted < 0) return nl_fail(err, errlen, NL_ESTATE, "nl_overlay_fetch_frame needs nl_overlay_paint");
    if (!frame) return nl_fail(err, errlen, NL_EINVAL, "frame is NULL");
    NL_HIP(hipMemcpyAsync(frame, h->d_out, (size_t)h->n * (h->painted == 1 ? 4 : 8), hipMemcpyDeviceToHost, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));
    return NL_OK;
}

// Device time (ms) of the kernels: ms[0] the mask and scan of the last nl_overlay_load, [1] the last nl_overlay_values, [2] the last
// nl_overlay_paint.  Transfers excluded.
extern "C" int nl_overlay_kernel_ms(nl_overlay *h, float *ms, char *err, size_t errlen) {
    if (!h || !ms) return nl_fail(err, errlen, NL_EINVAL, "overlay or ms is NULL");
    for (int j = 0; j < OV_MS_PARTS; ++j) ms[j] = h->ms[j];
    return NL_OK;
}
