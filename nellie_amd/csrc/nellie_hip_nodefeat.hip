// Translation unit of libnellie_hip.so (gfx950): node-level features (Nodes and aggregate_stats_for_class of
// nellie/feature_extraction/hierarchical.py).  C-ABI in include/nellie_amd.h; kernels in nodefeat.inc.  The object owns its
// buffers and stream.  It keeps one frame's node list and border mask, and one set of groups (a CSR of indices into value arrays)
// that any number of value arrays are then aggregated over.
#include <math.h>
#include <string.h>
#include "nl_stage.h"
#include "nodefeat.inc"

#define NF_MAX_ROWS ((i64)1 << 30)          // nodes per frame: ranks are ints
#define NF_MAX_IDX (((i64)1 << 31) - 1)     // indices in all groups together, and groups: a group's length and L are ints
#define NF_WIDE_FROM (4 * NF_BLOCK + 1)      // groups of at least that many values are summed a buffer block per wave: measured, DESIGN.md section 19
enum { NF_MS_LIST, NF_MS_THICKNESS, NF_MS_STATS, NF_MS_AGGREGATE, NF_MS_PARTS };

struct nl_nodefeat : StageBase {
    int ndim = 3;
    NfGeom g{};
    i64 words = 0;                                  // mask words per frame (a multiple of 4: one workgroup of the mask kernels writes 4)
    void *d_in = nullptr; i64 in_cap = 0;           // the frame or value array being uploaded, bytes
    u64 *nbits = nullptr, *bbits = nullptr;         // masks: nodes, border
    int *npre = nullptr, *d_wcount = nullptr, *d_any = nullptr;
    RankScan scan;
    // nodes
    i64 m = 0, node_cap = 0; bool has_frame = false; int comp_size = 1, branch_size = 1;
    i64 *node_vox = nullptr, *coords = nullptr; void *lab_c = nullptr, *lab_b = nullptr; double *thick = nullptr;
    // groups
    i64 groups = 0, total = 0, L = 0, idx_min = 0, idx_max = -1, grp_cap = 0, idx_cap = 0, sc_cap = 0; bool has_groups = false;
    i64 *d_off = nullptr, *d_idx = nullptr; double *d_scratch = nullptr, *d_out = nullptr;
    // the wide groups of the loaded set: their (group, block) items, one slot of partial results per item and per group
    i64 wide_from = NF_WIDE_FROM, listed_from = 0, n_wide = 0, n_items = 0, wide_cap = 0, item_cap = 0;
    i64 *d_wide = nullptr, *d_items = nullptr, *d_pcount = nullptr, *d_wtotal = nullptr; int *d_plo_at = nullptr, *d_phi_at = nullptr;
    double *d_psum = nullptr, *d_plo = nullptr, *d_phi = nullptr, *d_wmean = nullptr;
    // the voxels' coordinates and vectors of nl_nodefeat_node_stats
    i64 *d_vcoords = nullptr; float *d_v01 = nullptr, *d_v12 = nullptr; i64 vox_cap = 0;
    float ms[NF_MS_PARTS] = {0.f, 0.f, 0.f, 0.f};
};

extern "C" int nl_nodefeat_destroy(nl_nodefeat *h) {
    if (!h) return NL_OK;
    stage_close(*h, {h->d_in, h->nbits, h->bbits, h->npre, h->d_wcount, h->d_any, h->scan.d_bsum, h->scan.d_total, h->node_vox, h->coords, h->lab_c,
                     h->lab_b, h->thick, h->d_off, h->d_idx, h->d_scratch, h->d_out, h->d_vcoords, h->d_v01, h->d_v12, h->d_wide, h->d_items, h->d_pcount, h->d_wtotal,
                     h->d_plo_at, h->d_phi_at, h->d_psum, h->d_plo, h->d_phi, h->d_wmean},
                {h->scan.h_total});
    delete h;
    return NL_OK;
}

extern "C" int nl_nodefeat_create(nl_nodefeat **out, int device, int ndim, int64_t nz, int64_t ny, int64_t nx, const double *spacing, char *err,
                                  size_t errlen) {
    if (!out) return nl_fail(err, errlen, NL_EINVAL, "out is NULL");
    *out = nullptr;
    if (int rc = stage_check_frame(ndim, spacing, nz, ny, nx, err, errlen)) return rc;
    if (int rc = stage_check_device(device, err, errlen)) return rc;
    nl_nodefeat *h = new nl_nodefeat();
    h->ndim = ndim;
    h->g.nz = nz; h->g.ny = ny; h->g.nx = nx; h->g.n = nz * ny * nx;
    for (int a = 0; a < 3; ++a) h->g.s[a] = a < ndim ? spacing[a] : 1.0;
    for (int a = 0; a < 3; ++a) h->g.s3[a] = ndim == 3 ? spacing[a] : spacing[a > 0 ? a - 1 : 0];
    h->words = ((h->g.n + 255) / 256) * 4;
    if (int rc = stage_open(*h, device, true, err, errlen)) { nl_nodefeat_destroy(h); return rc; }
    STAGE_HIP(stage_alloc(&h->nbits, h->words, 8), nl_nodefeat_destroy(h));
    STAGE_HIP(stage_alloc(&h->bbits, h->words, 8), nl_nodefeat_destroy(h));
    STAGE_HIP(stage_alloc(&h->npre, h->words, 4), nl_nodefeat_destroy(h));
    STAGE_HIP(stage_alloc(&h->d_wcount, h->words, 4), nl_nodefeat_destroy(h));
    STAGE_HIP(stage_alloc(&h->d_any, 1, 4), nl_nodefeat_destroy(h));
    STAGE_HIP(stage_alloc(&h->scan.d_bsum, rank_scan_sums(h->words), 8), nl_nodefeat_destroy(h));
    STAGE_HIP(stage_alloc(&h->scan.d_total, 1, 8), nl_nodefeat_destroy(h));
    STAGE_HIP(hipHostMalloc((void **)&h->scan.h_total, 8, hipHostMallocDefault), nl_nodefeat_destroy(h));
    *out = h;
    return NL_OK;
}

// A frame: pixel class, component labels, branch labels and border mask of the object's shape, each in its own dtype (NL_U8 ..
// NL_I64).  The voxels with pixel class > 0 become the nodes, in raster order; their two labels are gathered and their thickness
// (twice the distance in um to the nearest voxel with border != 0, NaN in a frame without one) is computed.  n_nodes = their number.
extern "C" int nl_nodefeat_frame(nl_nodefeat *h, const void *pixel_class, int class_dtype, const void *comp, int comp_dtype, const void *branch,
                                 int branch_dtype, const void *border, int border_dtype, int64_t *n_nodes, char *err, size_t errlen) {
    STAGE_ENTER(h, "node-feature object");
    if (!pixel_class || !comp || !branch || !border || !n_nodes) return nl_fail(err, errlen, NL_EINVAL, "NULL frame or n_nodes");
    const size_t ps = dtype_size(class_dtype), cs = dtype_size(comp_dtype), bs = dtype_size(branch_dtype), os = dtype_size(border_dtype);
    if (!ps || !cs || !bs || !os) return nl_fail(err, errlen, NL_EINVAL, "unsupported dtype code");
    hipStream_t st = h->stream;
    const i64 n = h->g.n;
    h->has_frame = false;
    h->m = 0;
    *n_nodes = 0;
    h->ms[NF_MS_LIST] = h->ms[NF_MS_THICKNESS] = h->ms[NF_MS_STATS] = 0.f;
    const unsigned gv = (unsigned)((n + 255) / 256);
    if (int rc = stage_upload(*h, &h->d_in, &h->in_cap, pixel_class, n, ps, err, errlen)) return rc;
    if (int rc = stage_start(*h, err, errlen)) return rc;
    rank_mask_kernel<<<gv, 256, 0, st>>>(NfSet{h->d_in, class_dtype, true}, n, h->nbits, h->d_wcount);
    NL_CHECK_LAUNCH();
    i64 m = 0;
    if (int rc = rank_scan(h->scan, st, h->d_wcount, h->words, h->npre, NF_MAX_ROWS, "nodes in one frame", &m, err, errlen)) return rc;
    if (int rc = stage_grow(&h->node_cap, m, m, {{&h->node_vox, 8}, {&h->coords, 3 * 8}, {&h->lab_c, 8}, {&h->lab_b, 8}, {&h->thick, 8}}, err, errlen)) return rc;
    const unsigned gm = (unsigned)((m + 255) / 256);
    if (m > 0) {
        nf_compact_kernel<<<gv, 256, 0, st>>>(n, h->nbits, h->npre, h->node_vox);
        NL_CHECK_LAUNCH();
        nf_coords_kernel<<<gm, 256, 0, st>>>(h->node_vox, m, h->g, h->ndim, h->coords);
        NL_CHECK_LAUNCH();
    }
    if (int rc = stage_stop(*h, &h->ms[NF_MS_LIST], err, errlen)) return rc;
    const void *frames[2] = {comp, branch};
    const size_t sizes[2] = {cs, bs};
    void *dst[2] = {h->lab_c, h->lab_b};
    for (int f = 0; f < 2 && m > 0; ++f) {
        if (int rc = stage_upload(*h, &h->d_in, &h->in_cap, frames[f], n, sizes[f], err, errlen)) return rc;
        if (int rc = stage_start(*h, err, errlen)) return rc;
        nf_gather_kernel<<<gm, 256, 0, st>>>(h->d_in, (int)sizes[f], h->node_vox, m, dst[f]);
        NL_CHECK_LAUNCH();
        if (int rc = stage_stop(*h, &h->ms[NF_MS_LIST], err, errlen)) return rc;
    }
    if (m > 0) {
        if (int rc = stage_upload(*h, &h->d_in, &h->in_cap, border, n, os, err, errlen)) return rc;
        NL_HIP(hipMemsetAsync(h->d_any, 0, 4, st));
        if (int rc = stage_start(*h, err, errlen)) return rc;
        nf_border_kernel<<<gv, 256, 0, st>>>(NfSet{h->d_in, border_dtype, false}, n, h->bbits, h->d_any);
        NL_CHECK_LAUNCH();
        nf_thickness_kernel<<<(unsigned)m, 64, 0, st>>>(h->node_vox, m, h->g, h->bbits, h->d_any, h->thick);
        NL_CHECK_LAUNCH();
        if (int rc = stage_stop(*h, &h->ms[NF_MS_THICKNESS], err, errlen)) return rc;
    }
    NL_HIP(hipStreamSynchronize(st));                                  // the host arrays may go away after the call
    h->m = m;
    h->comp_size = (int)cs;
    h->branch_size = (int)bs;
    h->has_frame = true;
    *n_nodes = m;
    return NL_OK;
}

// Downloads the loaded frame's nodes: coordinates (n_nodes, D) int64, component and branch labels (n_nodes elements of the
// uploaded dtypes) and thickness (n_nodes float64).  NULL pointers are skipped.
extern "C" int nl_nodefeat_fetch(nl_nodefeat *h, int64_t *coords, void *comp, void *branch, double *thickness, char *err, size_t errlen) {
    STAGE_ENTER(h, "node-feature object");
    if (!h->has_frame) return nl_fail(err, errlen, NL_ESTATE, "no frame loaded");
    hipStream_t st = h->stream;
    const size_t m = (size_t)h->m;
    if (m > 0) {
        if (coords) NL_HIP(hipMemcpyAsync(coords, h->coords, m * h->ndim * 8, hipMemcpyDeviceToHost, st));
        if (comp) NL_HIP(hipMemcpyAsync(comp, h->lab_c, m * h->comp_size, hipMemcpyDeviceToHost, st));
        if (branch) NL_HIP(hipMemcpyAsync(branch, h->lab_b, m * h->branch_size, hipMemcpyDeviceToHost, st));
        if (thickness) NL_HIP(hipMemcpyAsync(thickness, h->thick, m * 8, hipMemcpyDeviceToHost, st));
    }
    NL_HIP(hipStreamSynchronize(st));
    return NL_OK;
}

// The groups of the calls that follow: group j holds idx[offsets[j] .. offsets[j + 1]), indices into the value arrays, in the
// order given (neither sorted nor disjoint).  offsets has n_groups + 1 entries and starts at 0.  *longest = L, the longest group.
extern "C" int nl_nodefeat_groups(nl_nodefeat *h, const int64_t *offsets, const int64_t *idx, int64_t n_groups, int64_t *longest, char *err,
                                  size_t errlen) {
    STAGE_ENTER(h, "node-feature object");
    if (!offsets || !longest || n_groups < 0) return nl_fail(err, errlen, NL_EINVAL, "NULL offsets or longest, or a negative group count");
    h->has_groups = false;
    *longest = 0;
    if (n_groups > NF_MAX_IDX) return nl_fail(err, errlen, NL_EINVAL, "more than %lld groups", (long long)NF_MAX_IDX);
    if (offsets[0] != 0) return nl_fail(err, errlen, NL_EINVAL, "offsets must start at 0");
    i64 L = 0;
    for (i64 j = 0; j < n_groups; ++j) {
        const i64 k = offsets[j + 1] - offsets[j];
        if (k < 0) return nl_fail(err, errlen, NL_EINVAL, "offsets must not decrease");
        L = k > L ? k : L;
    }
    const i64 total = offsets[n_groups];
    if (total > NF_MAX_IDX) return nl_fail(err, errlen, NL_EINVAL, "more than %lld indices in the groups of one call", (long long)NF_MAX_IDX);
    if (total > 0 && !idx) return nl_fail(err, errlen, NL_EINVAL, "idx is NULL");
    i64 lo = 0, hi = -1;
    for (i64 q = 0; q < total; ++q) {
        lo = q == 0 || idx[q] < lo ? idx[q] : lo;
        hi = q == 0 || idx[q] > hi ? idx[q] : hi;
    }
    if (lo < 0) return nl_fail(err, errlen, NL_EINVAL, "negative index in a group");
    // the wide groups: (group, first item) each, and an item (row of that list, block) for every buffer block that starts below k
    std::vector<i64> wide, items;
    for (i64 j = 0; j < n_groups && h->wide_from > 0; ++j) {
        const i64 k = offsets[j + 1] - offsets[j];
        if (k == 0 || k < h->wide_from) continue;
        const i64 w = (i64)wide.size() / 2;
        wide.push_back(j);
        wide.push_back((i64)items.size() / 2);
        for (i64 b = 0; b * NF_BLOCK < k; ++b) {
            items.push_back(w);
            items.push_back(b);
        }
    }
    const i64 n_wide = (i64)wide.size() / 2, n_items = (i64)items.size() / 2;
    if (n_items > NF_MAX_IDX) return nl_fail(err, errlen, NL_EINVAL, "more than %lld buffer blocks in the wide groups of one call", (long long)NF_MAX_IDX);
    hipStream_t st = h->stream;
    if (int rc = stage_grow(&h->wide_cap, n_wide, n_wide, {{&h->d_wide, 2 * 8}, {&h->d_wmean, 8}, {&h->d_wtotal, 8}}, err, errlen)) return rc;
    if (int rc = stage_grow(&h->item_cap, n_items, n_items, {{&h->d_items, 2 * 8}, {&h->d_psum, 8}, {&h->d_pcount, 8}, {&h->d_plo, 8}, {&h->d_phi, 8},
                                                               {&h->d_plo_at, 4}, {&h->d_phi_at, 4}}, err, errlen)) return rc;
    if (n_wide > 0) {
        NL_HIP(hipMemcpyAsync(h->d_wide, wide.data(), (size_t)n_wide * 16, hipMemcpyHostToDevice, st));
        NL_HIP(hipMemcpyAsync(h->d_items, items.data(), (size_t)n_items * 16, hipMemcpyHostToDevice, st));
    }
    const i64 scratch = total / 64 + 2 * n_groups + 2;
    if (int rc = stage_grow(&h->grp_cap, n_groups + 1, n_groups + 1, {{&h->d_off, 8}, {&h->d_out, 6 * 8}}, err, errlen)) return rc;
    if (int rc = stage_grow(&h->idx_cap, total, total, {{&h->d_idx, 8}}, err, errlen)) return rc;
    if (int rc = stage_grow(&h->sc_cap, scratch, scratch, {{&h->d_scratch, 8}}, err, errlen)) return rc;
    NL_HIP(hipMemcpyAsync(h->d_off, offsets, (size_t)(n_groups + 1) * 8, hipMemcpyHostToDevice, st));
    if (total > 0) NL_HIP(hipMemcpyAsync(h->d_idx, idx, (size_t)total * 8, hipMemcpyHostToDevice, st));
    NL_HIP(hipStreamSynchronize(st));
    h->groups = n_groups;
    h->total = total;
    h->L = L;
    h->idx_min = lo;
    h->idx_max = hi;
    h->listed_from = h->wide_from;
    h->n_wide = n_wide;
    h->n_items = n_items;
    h->has_groups = true;
    h->ms[NF_MS_AGGREGATE] = 0.f;
    *longest = L;
    return NL_OK;
}

// From the next nl_nodefeat_groups on, groups of at least wide_from values are aggregated a buffer block per wave (nodefeat.inc,
// nf_wide_block_kernel), the others a group per wave; 0: none.  Either way the values are the same bits.
extern "C" int nl_nodefeat_set_wide_from(nl_nodefeat *h, int64_t wide_from, char *err, size_t errlen) {
    if (!h) return nl_fail(err, errlen, NL_EINVAL, "node-feature object is NULL");
    if (wide_from < 0) return nl_fail(err, errlen, NL_EINVAL, "wide_from must be 0 (never) or at least 1");
    h->wide_from = wide_from;
    return NL_OK;
}

// One statistic over the loaded groups: values (n_values elements, NL_F32, NL_F64 or an integer dtype of at most 32 bits) are
// converted exactly to float64.  out (5, n_groups) float64: mean, std_dev, min, max, sum of every group as numpy's nanmean, nanstd,
// nanmin, nanmax, nansum give them for the rows of a matrix padded with NaN to L columns.
extern "C" int nl_nodefeat_aggregate(nl_nodefeat *h, const void *values, int dtype, int64_t n_values, double *out, char *err, size_t errlen) {
    STAGE_ENTER(h, "node-feature object");
    if (!out || n_values < 0 || (n_values > 0 && !values)) return nl_fail(err, errlen, NL_EINVAL, "NULL values or out");
    if (!h->has_groups) return nl_fail(err, errlen, NL_ESTATE, "no groups loaded");
    const size_t vs = dtype_size(dtype);
    if (!vs || dtype == NL_U64 || dtype == NL_I64) return nl_fail(err, errlen, NL_EINVAL, "values must be float32, float64 or integers of at most 32 bits");
    if (h->idx_max >= n_values) return nl_fail(err, errlen, NL_EINVAL, "index %lld in a group, but %lld values", (long long)h->idx_max, (long long)n_values);
    if (h->groups == 0) return NL_OK;
    hipStream_t st = h->stream;
    if (int rc = stage_upload(*h, &h->d_in, &h->in_cap, values, n_values, vs, err, errlen)) return rc;
    if (int rc = stage_start(*h, err, errlen)) return rc;
    const i64 wide_from = h->n_wide > 0 ? h->listed_from : 0;          // the threshold the loaded groups were listed under
    nf_aggregate_kernel<<<(unsigned)h->groups, 64, 0, st>>>(h->d_in, dtype, n_values, h->d_off, h->d_idx, h->groups, (int)h->L, wide_from, h->d_scratch,
                                                            h->d_out);
    NL_CHECK_LAUNCH();
    if (h->n_wide > 0) {
        const NfWide W{h->d_items, h->d_wide, h->d_psum, h->d_pcount, h->d_plo, h->d_phi, h->d_plo_at, h->d_phi_at, h->d_wmean, h->d_wtotal};
        const unsigned gi = (unsigned)h->n_items, gw = (unsigned)h->n_wide;
        nf_wide_block_kernel<false><<<gi, 64, 0, st>>>(h->d_in, dtype, n_values, h->d_off, h->d_idx, (int)h->L, W, h->n_items);
        NL_CHECK_LAUNCH();
        nf_wide_chain_kernel<false><<<gw, 64, 0, st>>>(h->d_off, h->groups, W, h->n_wide, h->d_out);
        NL_CHECK_LAUNCH();
        nf_wide_block_kernel<true><<<gi, 64, 0, st>>>(h->d_in, dtype, n_values, h->d_off, h->d_idx, (int)h->L, W, h->n_items);
        NL_CHECK_LAUNCH();
        nf_wide_chain_kernel<true><<<gw, 64, 0, st>>>(h->d_off, h->groups, W, h->n_wide, h->d_out);
        NL_CHECK_LAUNCH();
    }
    if (int rc = stage_stop_record(*h, err, errlen)) return rc;
    NL_HIP(hipMemcpyAsync(out, h->d_out, (size_t)h->groups * 5 * 8, hipMemcpyDeviceToHost, st));
    return stage_stop_wait(*h, &h->ms[NF_MS_AGGREGATE], err, errlen);
}

// The statistics of the loaded frame's nodes over the loaded groups, group j being node j's voxels: indices into coords
// (n_vox, D) int64 and vec01 / vec12 (n_vox, D) float32 (NULL: every vector of that direction is NaN).  out (6, n_nodes) float64:
// z, y, x (the mean voxel coordinate times the spacing; z NaN in 2-D), divergence, convergence, vergere.
extern "C" int nl_nodefeat_node_stats(nl_nodefeat *h, const int64_t *coords, const float *vec01, const float *vec12, int64_t n_vox, double *out,
                                      char *err, size_t errlen) {
    STAGE_ENTER(h, "node-feature object");
    if (!out || n_vox < 0 || (n_vox > 0 && !coords)) return nl_fail(err, errlen, NL_EINVAL, "NULL coords or out");
    if (!h->has_frame) return nl_fail(err, errlen, NL_ESTATE, "no frame loaded");
    if (!h->has_groups) return nl_fail(err, errlen, NL_ESTATE, "no groups loaded");
    if (h->groups != h->m) return nl_fail(err, errlen, NL_EINVAL, "%lld groups for %lld nodes", (long long)h->groups, (long long)h->m);
    if (h->idx_max >= n_vox) return nl_fail(err, errlen, NL_EINVAL, "index %lld in a group, but %lld voxels", (long long)h->idx_max, (long long)n_vox);
    h->ms[NF_MS_STATS] = 0.f;
    const i64 m = h->m;
    if (m == 0) return NL_OK;
    hipStream_t st = h->stream;
    const int D = h->ndim;
    if (int rc = stage_grow(&h->vox_cap, n_vox, n_vox, {{&h->d_vcoords, 3 * 8}, {&h->d_v01, 3 * 4}, {&h->d_v12, 3 * 4}}, err, errlen)) return rc;
    if (n_vox > 0) {
        NL_HIP(hipMemcpyAsync(h->d_vcoords, coords, (size_t)n_vox * D * 8, hipMemcpyHostToDevice, st));
        if (vec01) NL_HIP(hipMemcpyAsync(h->d_v01, vec01, (size_t)n_vox * D * 4, hipMemcpyHostToDevice, st));
        if (vec12) NL_HIP(hipMemcpyAsync(h->d_v12, vec12, (size_t)n_vox * D * 4, hipMemcpyHostToDevice, st));
    }
    if (int rc = stage_start(*h, err, errlen)) return rc;
    const float *v01 = vec01 ? h->d_v01 : nullptr, *v12 = vec12 ? h->d_v12 : nullptr;
    if (D == 3) nf_node_stats_kernel<3><<<(unsigned)m, 64, 0, st>>>(h->node_vox, m, h->g, h->d_vcoords, n_vox, v01, v12, h->d_off, h->d_idx, h->d_scratch, h->d_out);
    else nf_node_stats_kernel<2><<<(unsigned)m, 64, 0, st>>>(h->node_vox, m, h->g, h->d_vcoords, n_vox, v01, v12, h->d_off, h->d_idx, h->d_scratch, h->d_out);
    NL_CHECK_LAUNCH();
    if (int rc = stage_stop_record(*h, err, errlen)) return rc;
    NL_HIP(hipMemcpyAsync(out, h->d_out, (size_t)m * 6 * 8, hipMemcpyDeviceToHost, st));
    return stage_stop_wait(*h, &h->ms[NF_MS_STATS], err, errlen);
}

// Device time (ms) of the kernels, per part: ms[0] node list and labels, [1] border mask and thickness, [2] node statistics (all
// three since the last nl_nodefeat_frame), [3] aggregation since the last nl_nodefeat_groups.  Transfers excluded.
extern "C" int nl_nodefeat_kernel_ms(nl_nodefeat *h, float *ms, char *err, size_t errlen) {
    if (!h || !ms) return nl_fail(err, errlen, NL_EINVAL, "node-feature object or ms is NULL");
    for (int j = 0; j < NF_MS_PARTS; ++j) ms[j] = h->ms[j];
    return NL_OK;
}
