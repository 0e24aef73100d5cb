// Translation unit of libnellie_hip.so (gfx950): flow-vector interpolation (nellie/tracking/flow_interpolation.py).  C-ABI in
// include/nellie_amd.h; kernels in flow.inc.  A flow field owns its buffers and stream: it needs none of a Filter context's volumes.
#include "nl_stage.h"
#include "flow.inc"

#define FLOW_CHUNK ((i64)1 << 22)      // query rows per launch: 96 MB in and 96 MB out on the device at D = 3

struct nl_flow : StageBase {
    int ndim = 3;
    FlowSpacing sp{{1.0, 1.0, 1.0}};
    double r = 0.5;
    i64 n_rows = 0, row_cap = 0;
    i64 max_cells = 0;                 // the cell budget the last load's plan was given
    double *d_in = nullptr;            // uploaded rows: coords (n, D) | vectors (n, D) | costs (n)
    int *d_cell = nullptr, *d_perm = nullptr;
    FlowRow *d_rows = nullptr;
    FlowGrid *d_grid = nullptr;
    int *d_start = nullptr, *d_cursor = nullptr;      // FLOW_MAX_CELLS + 1 entries
    double *d_q = nullptr, *d_out = nullptr; i64 q_cap = 0;
    unsigned long long *d_found = nullptr, *h_found = nullptr;
    float kernel_ms = 0.f;             // device time of the last nl_flow_interpolate's kernels
};

extern "C" int nl_flow_destroy(nl_flow *f) {
    if (!f) return NL_OK;
    stage_close(*f, {f->d_in, f->d_cell, f->d_perm, f->d_rows, f->d_grid, f->d_start, f->d_cursor, f->d_q, f->d_out, f->d_found}, {f->h_found});
    delete f;
    return NL_OK;
}

extern "C" int nl_flow_create(nl_flow **out, int device, int ndim, const double *spacing, double r, char *err, size_t errlen) {
    if (!out) return nl_fail(err, errlen, NL_EINVAL, "out is NULL");
    *out = nullptr;
    if (int rc = stage_check_frame(ndim, spacing, 1, 1, 1, err, errlen)) return rc;
    if (int rc = stage_check_positive(r, "the radius", err, errlen)) return rc;
    if (int rc = stage_check_device(device, err, errlen)) return rc;
    nl_flow *f = new nl_flow();
    f->ndim = ndim;
    f->r = r;
    for (int a = 0; a < ndim; ++a) f->sp.s[3 - ndim + a] = spacing[a];
    if (int rc = stage_open(*f, device, true, err, errlen)) { nl_flow_destroy(f); return rc; }
    STAGE_HIP(stage_alloc(&f->d_grid, 1, sizeof(FlowGrid)), nl_flow_destroy(f));
    STAGE_HIP(stage_alloc(&f->d_start, FLOW_MAX_CELLS + 1, 4), nl_flow_destroy(f));
    STAGE_HIP(stage_alloc(&f->d_cursor, FLOW_MAX_CELLS + 1, 4), nl_flow_destroy(f));
    STAGE_HIP(stage_alloc(&f->d_found, 1, 8), nl_flow_destroy(f));
    STAGE_HIP(hipHostMalloc((void **)&f->h_found, 8, hipHostMallocDefault), nl_flow_destroy(f));
    *out = f;
    return NL_OK;
}

// The rows of one time point and direction: check coordinates (n, ndim) in voxels (the row's position, forward; position +
// vector, backward), vectors (n, ndim), costs (n), all float64.  They replace the rows loaded before and stay on the device.
extern "C" int nl_flow_load(nl_flow *f, const double *coords, const double *vectors, const double *costs, int64_t n, char *err, size_t errlen) {
    STAGE_ENTER(f, "flow field");
    if (n < 0 || n > (i64)1 << 30) return nl_fail(err, errlen, NL_EINVAL, "row count must be 0 .. 2^30");
    if (n > 0 && (!coords || !vectors || !costs)) return nl_fail(err, errlen, NL_EINVAL, "NULL rows");
    f->n_rows = 0;
    if (n == 0) return NL_OK;
    const int D = f->ndim;
    const i64 W = 2 * D + 1;
    if (int rc = stage_grow(&f->row_cap, n, stage_doubled(f->row_cap, n),
                            {{&f->d_in, (size_t)W * 8}, {&f->d_cell, 4}, {&f->d_perm, 4}, {&f->d_rows, sizeof(FlowRow)}}, err, errlen)) return rc;
    hipStream_t st = f->stream;
    double *d_c = f->d_in, *d_v = f->d_in + n * D, *d_k = f->d_in + 2 * n * D;
    NL_HIP(hipMemcpyAsync(d_c, coords, (size_t)n * D * 8, hipMemcpyHostToDevice, st));
    NL_HIP(hipMemcpyAsync(d_v, vectors, (size_t)n * D * 8, hipMemcpyHostToDevice, st));
    NL_HIP(hipMemcpyAsync(d_k, costs, (size_t)n * 8, hipMemcpyHostToDevice, st));
    i64 cells = 8 * n;                  // more cells than a few per row only lengthen the scan
    if (cells < FLOW_MIN_CELLS) cells = FLOW_MIN_CELLS;
    if (cells > FLOW_MAX_CELLS) cells = FLOW_MAX_CELLS;
    const unsigned gn = (unsigned)((n + 255) / 256);
    flow_grid_kernel<<<1, 1024, 0, st>>>(d_c, D, (int)n, f->sp, f->r, (int)cells, f->d_grid, f->d_start);
    NL_CHECK_LAUNCH();
    flow_count_kernel<<<gn, 256, 0, st>>>(d_c, D, (int)n, f->sp, f->d_grid, f->d_start, f->d_cell);
    NL_CHECK_LAUNCH();
    flow_scan_kernel<<<1, 1024, 0, st>>>(f->d_grid, f->d_start, f->d_cursor);
    NL_CHECK_LAUNCH();
    flow_place_kernel<<<gn, 256, 0, st>>>((int)n, f->d_cell, f->d_cursor, f->d_perm);
    NL_CHECK_LAUNCH();
    flow_sort_write_kernel<<<grid1d(cells, 256, 256), 256, 0, st>>>(d_c, d_v, d_k, D, f->sp, f->d_grid, f->d_start, f->d_perm, f->d_rows);
    NL_CHECK_LAUNCH();
    NL_HIP(hipStreamSynchronize(st));   // the host arrays may go away after the call
    f->n_rows = n;
    f->max_cells = cells;
    return NL_OK;
}

// The plan of the rows that are loaded, read back from the device (not on any hot path): dims[3], the number of cells, the cell
// edge per axis in um (1 / inv; 0 where the plan resolves nothing), the cell budget the plan was given and the number of rows in
// the fullest cell.  A 2-D field reports a leading axis of one cell.  With no rows loaded everything is 0.
extern "C" int nl_flow_grid_info(nl_flow *f, int *dims, int64_t *ncell, double *edge, int64_t *max_cells, int64_t *fullest, char *err, size_t errlen) {
    STAGE_ENTER(f, "flow field");
    if (!dims || !ncell || !edge || !max_cells || !fullest) return nl_fail(err, errlen, NL_EINVAL, "NULL output");
    for (int a = 0; a < 3; ++a) { dims[a] = 0; edge[a] = 0.0; }
    *ncell = *max_cells = *fullest = 0;
    if (f->n_rows == 0) return NL_OK;
    FlowGrid g;
    NL_HIP(hipMemcpyAsync(&g, f->d_grid, sizeof(FlowGrid), hipMemcpyDeviceToHost, f->stream));
    NL_HIP(hipStreamSynchronize(f->stream));
    if (g.ncell < 1 || g.ncell > FLOW_MAX_CELLS) return nl_fail(err, errlen, NL_ESTATE, "the flow grid holds %d cells", g.ncell);
    std::vector<int> start((size_t)g.ncell + 1);
    NL_HIP(hipMemcpyAsync(start.data(), f->d_start, start.size() * 4, hipMemcpyDeviceToHost, f->stream));
    NL_HIP(hipStreamSynchronize(f->stream));
    for (int a = 0; a < 3; ++a) {
        dims[a] = g.dims[a];
        edge[a] = g.inv[a] > 0.0 ? 1.0 / g.inv[a] : 0.0;
    }
    *ncell = g.ncell;
    *max_cells = f->max_cells;
    for (int c = 0; c < g.ncell; ++c)
        if (start[c + 1] - start[c] > *fullest) *fullest = start[c + 1] - start[c];
    return NL_OK;
}

// Interpolates n query rows (n, ndim) float64 (voxels) into out (n, ndim) float64; a row without a neighbour (a NaN row
// included) is NaN.  n_found = rows that found a neighbour.  Longer inputs run in chunks of FLOW_CHUNK rows.
extern "C" int nl_flow_interpolate(nl_flow *f, const double *queries, int64_t n, double *out, int64_t *n_found, char *err, size_t errlen) {
    STAGE_ENTER(f, "flow field");
    if (n < 0) return nl_fail(err, errlen, NL_EINVAL, "negative query count");
    if (!n_found) return nl_fail(err, errlen, NL_EINVAL, "n_found is NULL");
    if (n > 0 && (!queries || !out)) return nl_fail(err, errlen, NL_EINVAL, "NULL queries or output");
    *n_found = 0;
    f->kernel_ms = 0.f;
    if (n == 0) return NL_OK;
    const int D = f->ndim;
    if (f->n_rows == 0) {               // no rows for this time point: every query row is NaN
        const double nan = __builtin_nan("");
        for (i64 i = 0; i < n * D; ++i) out[i] = nan;
        return NL_OK;
    }
    const i64 chunk = n < FLOW_CHUNK ? n : FLOW_CHUNK;
    if (int rc = stage_grow(&f->q_cap, chunk, chunk, {{&f->d_q, (size_t)D * 8}, {&f->d_out, (size_t)D * 8}}, err, errlen)) return rc;
    hipStream_t st = f->stream;
    NL_HIP(hipMemsetAsync(f->d_found, 0, 8, st));
    const double r2 = f->r * f->r;
    for (i64 at = 0; at < n; at += chunk) {
        const i64 m = n - at < chunk ? n - at : chunk;
        NL_HIP(hipMemcpyAsync(f->d_q, queries + at * D, (size_t)m * D * 8, hipMemcpyHostToDevice, st));
        if (int rc = stage_start(*f, err, errlen)) return rc;
        const unsigned g = (unsigned)((m + 255) / 256);
        if (D == 3) flow_interp_kernel<3><<<g, 256, 0, st>>>(f->d_q, m, f->d_rows, f->d_start, f->d_grid, f->sp, r2, f->d_out, f->d_found);
        else flow_interp_kernel<2><<<g, 256, 0, st>>>(f->d_q, m, f->d_rows, f->d_start, f->d_grid, f->sp, r2, f->d_out, f->d_found);
        NL_CHECK_LAUNCH();
        if (int rc = stage_stop_record(*f, err, errlen)) return rc;
        NL_HIP(hipMemcpyAsync(out + at * D, f->d_out, (size_t)m * D * 8, hipMemcpyDeviceToHost, st));
        if (int rc = stage_stop_wait(*f, &f->kernel_ms, err, errlen)) return rc;
    }
    NL_HIP(hipMemcpyAsync(f->h_found, f->d_found, 8, hipMemcpyDeviceToHost, st));
    NL_HIP(hipStreamSynchronize(st));
    *n_found = (int64_t)*f->h_found;
    return NL_OK;
}

// nl_flow_interpolate for queries and results that are already on this field's device: n rows (n, ndim) float64 at d_queries ->
// d_out, in one launch, nothing crosses the host.  The caller's work on d_queries must be complete; the call returns when d_out
// is.  With no rows loaded nothing is written and n_found = 0.
extern "C" int nl_flow_interpolate_dev(nl_flow *f, const double *d_queries, int64_t n, double *d_out, int64_t *n_found, char *err, size_t errlen) {
    STAGE_ENTER(f, "flow field");
    if (n < 0 || n > (i64)1 << 31) return nl_fail(err, errlen, NL_EINVAL, "query count must be 0 .. 2^31");
    if (!n_found) return nl_fail(err, errlen, NL_EINVAL, "n_found is NULL");
    if (n > 0 && (!d_queries || !d_out)) return nl_fail(err, errlen, NL_EINVAL, "NULL queries or output");
    *n_found = 0;
    f->kernel_ms = 0.f;
    if (n == 0 || f->n_rows == 0) return NL_OK;
    hipStream_t st = f->stream;
    NL_HIP(hipMemsetAsync(f->d_found, 0, 8, st));
    const double r2 = f->r * f->r;
    if (int rc = stage_start(*f, err, errlen)) return rc;
    const unsigned g = (unsigned)((n + 255) / 256);
    if (f->ndim == 3) flow_interp_kernel<3><<<g, 256, 0, st>>>(d_queries, n, f->d_rows, f->d_start, f->d_grid, f->sp, r2, d_out, f->d_found);
    else flow_interp_kernel<2><<<g, 256, 0, st>>>(d_queries, n, f->d_rows, f->d_start, f->d_grid, f->sp, r2, d_out, f->d_found);
    NL_CHECK_LAUNCH();
    if (int rc = stage_stop_record(*f, err, errlen)) return rc;
    NL_HIP(hipMemcpyAsync(f->h_found, f->d_found, 8, hipMemcpyDeviceToHost, st));
    if (int rc = stage_stop_wait(*f, &f->kernel_ms, err, errlen)) return rc;
    *n_found = (int64_t)*f->h_found;
    return NL_OK;
}

// Device time (ms) of the kernels of the last nl_flow_interpolate / nl_flow_interpolate_dev call (transfers excluded).
extern "C" int nl_flow_kernel_ms(nl_flow *f, float *ms, char *err, size_t errlen) {
    if (!f || !ms) return nl_fail(err, errlen, NL_EINVAL, "flow field or ms is NULL");
    *ms = f->kernel_ms;
    return NL_OK;
}
