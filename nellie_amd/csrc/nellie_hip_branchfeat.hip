// Translation unit of libnellie_hip.so (gfx950): branch-level features (Branches of nellie/feature_extraction/hierarchical.py).
// C-ABI in include/nellie_amd.h; kernels in branchfeat.inc.  The object owns its buffers and stream.  It keeps one frame's
// skeleton list with everything per skeleton voxel and per skeleton label, and one frame's regions (the labels of the full
// branch-label volume) with their sums and, on request, their convex counts (convex.inc, convex_hull.h).
#include <math.h>
#include <string.h>
#include <chrono>
#include <vector>
#include "nl_stage.h"
#include "branchfeat.inc"
#include "convex.inc"
#include "convex_hull.h"

#define BF_MAX_ROWS ((i64)1 << 30)          // skeleton voxels, distinct labels, region voxels of one frame: ranks and offsets are ints
#define BF_MAX_LABEL (((i64)1 << 31) - 2)   // label values: the presence table has one bit per value
#define BF_MAX_DIM ((i64)1 << 15)           // extent of a frame whose region sums are taken (branchfeat.inc, bf_region_kernel)
enum { BF_MS_LIST, BF_MS_DEGREE, BF_MS_RADII, BF_MS_LISTS, BF_MS_REGIONS, BF_MS_PARTS };
enum { CV_MS_EXTREMES, CV_MS_PLANES, CV_MS_COUNT, CV_MS_HULL, CV_MS_PARTS };
#define CV_MAX_ROWS ((i64)1 << 28)          // box rows of all regions of one frame (two ints each come back to the host)

struct nl_branchfeat : StageBase {
    int ndim = 3, noff = BF_NOFF3;
    NfGeom g{};
    i64 words = 0;                                  // mask words per frame (a multiple of 4: one workgroup of the mask kernels writes 4)
    void *d_lab = nullptr; i64 lab_cap = 0;         // the label frame that stays (skeleton, then branch labels), bytes
    void *d_in = nullptr; i64 in_cap = 0;           // the frame that passes through (component labels, border, reassigned labels), bytes
    u64 *sbits = nullptr, *bbits = nullptr, *tbits = nullptr;      // masks: skeleton, border, tips (over the skeleton list)
    int *spre = nullptr, *tpre = nullptr, *d_wcount = nullptr, *d_any = nullptr;
    u64 *d_word = nullptr;                          // one word: the largest label, the append cursor
    RankScan scan; i64 bsum_cap = 0;
    // the presence table of the labels being ranked
    u64 *pres = nullptr; int *lpre = nullptr, *lwcount = nullptr; i64 pres_cap = 0;
    // skeleton voxels
    i64 m = 0, vox_cap = 0; bool has_frame = false; int comp_size = 1; bool has_border = false;
    i64 *vox = nullptr, *coords = nullptr, *label = nullptr, *tips = nullptr, *lone = nullptr; int *rank = nullptr; uint8_t *deg = nullptr;
    double *radius = nullptr; i64 n_tips = 0, n_lone = 0;
    BfKey2 *keys2 = nullptr; i64 keys2_cap = 0;
    // skeleton labels
    i64 B = 0, lab_rows = 0;
    i64 *uniq = nullptr, *first_vox = nullptr; u64 *first = nullptr; int *count = nullptr, *off = nullptr; unsigned int *edges = nullptr;
    void *comp_l = nullptr; double *median = nullptr;
    // regions
    i64 R = 0, reg_rows = 0, acc_fields = 0; bool has_regions = false, has_mode = false;
    i64 *runiq = nullptr; u64 *acc = nullptr, *best = nullptr; u64 *keys = nullptr; i64 keys_cap = 0;
    float ms[BF_MS_PARTS] = {0.f, 0.f, 0.f, 0.f, 0.f};
    // convex counts of the regions (convex.inc): d_lab still holds the regions' frame while lab_regions
    bool lab_regions = false, has_convex = false; int reg_dtype = 0;
    CvBox *cbox = nullptr; i64 *crowoff = nullptr, *cplaneoff = nullptr, *cfacetoff = nullptr; u64 *ccount = nullptr; i64 cv_cap = 0;     // per region (+ 1)
    int *cxmin = nullptr, *cxmax = nullptr, *ckeep_lo = nullptr, *ckeep_hi = nullptr; i64 crow_cap = 0;                                      // per box row
    i64 *cfacets = nullptr; i64 cfacet_cap = 0; CvTask *ctasks = nullptr; i64 ctask_cap = 0;
    std::vector<i64> cv_nfacets, cv_nrows;
    float cms[CV_MS_PARTS] = {0.f, 0.f, 0.f, 0.f};
};

extern "C" int nl_branchfeat_destroy(nl_branchfeat *h) {
    if (!h) return NL_OK;
    stage_close(*h, {h->d_lab, h->d_in, h->sbits, h->bbits, h->tbits, h->spre, h->tpre, h->d_wcount, h->d_any, h->d_word, h->scan.d_bsum, h->scan.d_total,
                     h->pres, h->lpre, h->lwcount, h->vox, h->coords, h->label, h->tips, h->lone, h->rank, h->deg, h->radius, h->keys2, h->uniq,
                     h->first_vox, h->first, h->count, h->off, h->edges, h->comp_l, h->median, h->runiq, h->acc, h->best, h->keys,
                     h->cbox, h->crowoff, h->cplaneoff, h->cfacetoff, h->ccount, h->cxmin, h->cxmax, h->ckeep_lo, h->ckeep_hi, h->cfacets, h->ctasks},
                {h->scan.h_total});
    delete h;
    return NL_OK;
}

extern "C" int nl_branchfeat_create(nl_branchfeat **out, int device, int ndim, int64_t nz, int64_t ny, int64_t nx, const double *spacing, char *err,
                                    size_t errlen) {
    if (!out) return nl_fail(err, errlen, NL_EINVAL, "out is NULL");
    *out = nullptr;
    if (int rc = stage_check_frame(ndim, spacing, nz, ny, nx, err, errlen)) return rc;
    if (int rc = stage_check_device(device, err, errlen)) return rc;
    nl_branchfeat *h = new nl_branchfeat();
    h->ndim = ndim;
    h->noff = ndim == 3 ? BF_NOFF3 : BF_NOFF2;
    h->acc_fields = 1 + 3 * ndim + ndim * (ndim + 1) / 2;
    h->g.nz = nz; h->g.ny = ny; h->g.nx = nx; h->g.n = nz * ny * nx;
    for (int a = 0; a < 3; ++a) h->g.s[a] = a < ndim ? spacing[a] : 1.0;
    for (int a = 0; a < 3; ++a) h->g.s3[a] = ndim == 3 ? spacing[a] : spacing[a > 0 ? a - 1 : 0];
    h->words = ((h->g.n + 255) / 256) * 4;
    if (int rc = stage_open(*h, device, true, err, errlen)) { nl_branchfeat_destroy(h); return rc; }
    STAGE_HIP(stage_alloc(&h->sbits, h->words, 8), nl_branchfeat_destroy(h));
    STAGE_HIP(stage_alloc(&h->bbits, h->words, 8), nl_branchfeat_destroy(h));
    STAGE_HIP(stage_alloc(&h->tbits, h->words, 8), nl_branchfeat_destroy(h));
    STAGE_HIP(stage_alloc(&h->spre, h->words, 4), nl_branchfeat_destroy(h));
    STAGE_HIP(stage_alloc(&h->tpre, h->words, 4), nl_branchfeat_destroy(h));
    STAGE_HIP(stage_alloc(&h->d_wcount, h->words, 4), nl_branchfeat_destroy(h));
    STAGE_HIP(stage_alloc(&h->d_any, 2, 4), nl_branchfeat_destroy(h));
    STAGE_HIP(stage_alloc(&h->d_word, 1, 8), nl_branchfeat_destroy(h));
    h->bsum_cap = rank_scan_sums(h->words);
    STAGE_HIP(stage_alloc(&h->scan.d_bsum, h->bsum_cap, 8), nl_branchfeat_destroy(h));
    STAGE_HIP(stage_alloc(&h->scan.d_total, 1, 8), nl_branchfeat_destroy(h));
    STAGE_HIP(hipHostMalloc((void **)&h->scan.h_total, 8, hipHostMallocDefault), nl_branchfeat_destroy(h));
    *out = h;
    return NL_OK;
}

static bool bf_label_dtype(int dt) { return dtype_size(dt) && dt != NL_F32 && dt != NL_F64; }
static unsigned bf_grid(i64 n) { return (unsigned)((n + 255) / 256); }

// the scan's workgroup sums hold a scan of `longest` counts afterwards
static int bf_scan_reserve(nl_branchfeat *h, i64 longest, char *err, size_t errlen) {
    const i64 need = rank_scan_sums(longest);
    return stage_grow(&h->bsum_cap, need, need, {{&h->scan.d_bsum, 8}}, err, errlen);
}

// one word from the device, through the scan's pinned word.  Synchronises the stream.
static int bf_fetch_word(nl_branchfeat *h, const void *dev, i64 *value, char *err, size_t errlen) {
    NL_HIP(hipMemcpyAsync(h->scan.h_total, dev, 8, hipMemcpyDeviceToHost, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));
    *value = *h->scan.h_total;
    return NL_OK;
}

// The distinct labels > 0 of lab(0 .. n), ascending, into *uniq (grown under *rows, with `extra` buffers of the same capacity);
// afterwards ra_rank(h->pres, h->lpre, l) is the rank of a label l among them.  Synchronises the stream.
static int bf_distinct(nl_branchfeat *h, BfLabels lab, i64 n, i64 **uniq, i64 *rows, std::initializer_list<StageBuf> extra, i64 *count, char *err,
                       size_t errlen) {
    hipStream_t st = h->stream;
    *count = 0;
    i64 top = 0;
    if (n > 0) {
        NL_HIP(hipMemsetAsync(h->d_word, 0, 8, st));
        bf_max_kernel<<<bf_grid(n), 256, 0, st>>>(lab, n, h->d_word);
        NL_CHECK_LAUNCH();
        if (int rc = bf_fetch_word(h, h->d_word, &top, err, errlen)) return rc;
    }
    if (top > BF_MAX_LABEL) return nl_fail(err, errlen, NL_EINVAL, "label %lld is above %lld", (long long)top, (long long)BF_MAX_LABEL);
    i64 found = 0;
    if (top > 0) {
        const i64 lwords = (top + 64) / 64;                            // the values 0 .. top
        if (int rc = stage_grow(&h->pres_cap, lwords, lwords, {{&h->pres, 8}, {&h->lpre, 4}, {&h->lwcount, 4}}, err, errlen)) return rc;
        if (int rc = bf_scan_reserve(h, lwords, err, errlen)) return rc;
        NL_HIP(hipMemsetAsync(h->pres, 0, (size_t)lwords * 8, st));
        bf_present_kernel<<<bf_grid(n), 256, 0, st>>>(lab, n, h->pres);
        NL_CHECK_LAUNCH();
        bf_popc_kernel<<<bf_grid(lwords), 256, 0, st>>>(h->pres, lwords, h->lwcount);
        NL_CHECK_LAUNCH();
        if (int rc = rank_scan(h->scan, st, h->lwcount, lwords, h->lpre, BF_MAX_ROWS, "distinct labels in one frame", &found, err, errlen)) return rc;
    }
    if (found > *rows) {
        std::vector<StageBuf> bufs(extra);
        *rows = 0;
        NL_HIP(stage_alloc(uniq, found, 8));
        for (const StageBuf &b : bufs) NL_HIP(stage_alloc(b.p, found, b.elem));
        *rows = found;
    }
    if (found > 0) {
        bf_uniq_kernel<<<bf_grid(top + 1), 256, 0, st>>>(h->pres, h->lpre, top + 1, *uniq);
        NL_CHECK_LAUNCH();
    }
    *count = found;
    return NL_OK;
}

template <typename K> static int bf_sort(hipStream_t st, K *keys, i64 P, char *err, size_t errlen) {
    for (i64 kk = 2; kk <= P; kk <<= 1)
        for (i64 j = kk >> 1; j > 0; j >>= 1) {
            bf_bitonic_kernel<K><<<bf_grid(P), 256, 0, st>>>(keys, P, j, kk);
            NL_CHECK_LAUNCH();
        }
    return NL_OK;
}
static i64 bf_pow2(i64 n) { i64 p = 1; while (p < n) p <<= 1; return p; }

// the set bits of a mask over the skeleton list (degree == want), as positions in the list, in order
static int bf_pick(nl_branchfeat *h, i64 m, int want, i64 *out, i64 *count, char *err, size_t errlen) {
    hipStream_t st = h->stream;
    const i64 mwords = ((m + 255) / 256) * 4;                // at most the frame's: m <= n
    rank_mask_kernel<<<bf_grid(m), 256, 0, st>>>(BfDegreeIs{h->deg, want}, m, h->tbits, h->d_wcount);
    NL_CHECK_LAUNCH();
    if (int rc = rank_scan(h->scan, st, h->d_wcount, mwords, h->tpre, BF_MAX_ROWS, "tips in one frame", count, err, errlen)) return rc;
    if (*count > 0) {
        bf_positions_kernel<<<bf_grid(m), 256, 0, st>>>(m, h->tbits, h->tpre, out);
        NL_CHECK_LAUNCH();
    }
    return NL_OK;
}

// A frame: skeleton labels, component labels and border mask of the object's shape, each in its own dtype (labels: an integer
// dtype).  The voxels with skeleton label > 0 become the skeleton list, in raster order; see include/nellie_amd.h for what is
// computed from it.
extern "C" int nl_branchfeat_frame(nl_branchfeat *h, const void *skel, int skel_dtype, const void *comp, int comp_dtype, const void *border,
                                   int border_dtype, int64_t *n_voxels, int64_t *n_labels, int64_t *n_tips, int64_t *n_lone, char *err, size_t errlen) {
    STAGE_ENTER(h, "branch-feature object");
    if (!skel || !comp || !border || !n_voxels || !n_labels || !n_tips || !n_lone) return nl_fail(err, errlen, NL_EINVAL, "NULL frame or count");
    const size_t ss = dtype_size(skel_dtype), cs = dtype_size(comp_dtype), os = dtype_size(border_dtype);
    if (!ss || !cs || !os) return nl_fail(err, errlen, NL_EINVAL, "unsupported dtype code");
    if (!bf_label_dtype(skel_dtype)) return nl_fail(err, errlen, NL_EINVAL, "skeleton labels must have an integer dtype");
    hipStream_t st = h->stream;
    const i64 n = h->g.n;
    h->has_frame = false;
    h->lab_regions = false;                                            // the skeleton takes the regions' place on the device
    h->m = h->B = h->n_tips = h->n_lone = 0;
    *n_voxels = *n_labels = *n_tips = *n_lone = 0;
    for (int j = BF_MS_LIST; j <= BF_MS_LISTS; ++j) h->ms[j] = 0.f;
    // ---- the list, its labels and their ranks
    if (int rc = stage_upload(*h, &h->d_lab, &h->lab_cap, skel, n, ss, err, errlen)) return rc;
    if (int rc = bf_scan_reserve(h, h->words, err, errlen)) return rc;
    if (int rc = stage_start(*h, err, errlen)) return rc;
    rank_mask_kernel<<<bf_grid(n), 256, 0, st>>>(BfPositive{h->d_lab, skel_dtype}, n, h->sbits, h->d_wcount);
    NL_CHECK_LAUNCH();
    i64 m = 0;
    if (int rc = rank_scan(h->scan, st, h->d_wcount, h->words, h->spre, BF_MAX_ROWS, "skeleton voxels in one frame", &m, err, errlen)) return rc;
    if (int rc = stage_grow(&h->vox_cap, m, m, {{&h->vox, 8}, {&h->coords, 3 * 8}, {&h->label, 8}, {&h->tips, 8}, {&h->lone, 8}, {&h->rank, 4},
                                                {&h->deg, 1}, {&h->radius, 8}}, err, errlen)) return rc;
    if (m > 0) {
        nf_compact_kernel<<<bf_grid(n), 256, 0, st>>>(n, h->sbits, h->spre, h->vox);
        NL_CHECK_LAUNCH();
        nf_coords_kernel<<<bf_grid(m), 256, 0, st>>>(h->vox, m, h->g, h->ndim, h->coords);
        NL_CHECK_LAUNCH();
    }
    const BfLabels lab{h->d_lab, skel_dtype, h->vox};
    i64 B = 0;
    if (int rc = bf_distinct(h, lab, m, &h->uniq, &h->lab_rows, {{&h->first_vox, 8}, {&h->first, 8}, {&h->count, 4}, {&h->off, 4},
                                                                 {&h->edges, BF_NOFF3 * 4}, {&h->comp_l, 8}, {&h->median, 8}}, &B, err, errlen)) return rc;
    if (m > 0) {
        NL_HIP(hipMemsetAsync(h->first, 0xff, (size_t)B * 8, st));
        NL_HIP(hipMemsetAsync(h->count, 0, (size_t)B * 4, st));
        NL_HIP(hipMemsetAsync(h->edges, 0, (size_t)B * h->noff * 4, st));
        bf_list_kernel<<<bf_grid(m), 256, 0, st>>>(lab, m, h->pres, h->lpre, h->label, h->rank, h->count, h->first);
        NL_CHECK_LAUNCH();
        bf_first_voxel_kernel<<<bf_grid(B), 256, 0, st>>>(h->first, h->vox, B, h->first_vox);
        NL_CHECK_LAUNCH();
    }
    if (int rc = stage_stop(*h, &h->ms[BF_MS_LIST], err, errlen)) return rc;
    // ---- degree and edge counts (the skeleton frame is still there)
    if (m > 0) {
        if (int rc = stage_start(*h, err, errlen)) return rc;
        if (h->ndim == 3) bf_degree_kernel<3><<<bf_grid(m), 256, 0, st>>>(h->d_lab, skel_dtype, h->vox, h->rank, m, h->g, h->deg, h->edges);
        else bf_degree_kernel<2><<<bf_grid(m), 256, 0, st>>>(h->d_lab, skel_dtype, h->vox, h->rank, m, h->g, h->deg, h->edges);
        NL_CHECK_LAUNCH();
        if (int rc = stage_stop(*h, &h->ms[BF_MS_DEGREE], err, errlen)) return rc;
        // ---- the component label at every label's first voxel
        if (int rc = stage_upload(*h, &h->d_in, &h->in_cap, comp, n, cs, err, errlen)) return rc;
        if (int rc = stage_start(*h, err, errlen)) return rc;
        nf_gather_kernel<<<bf_grid(B), 256, 0, st>>>(h->d_in, (int)cs, h->first_vox, B, h->comp_l);
        NL_CHECK_LAUNCH();
        if (int rc = stage_stop(*h, &h->ms[BF_MS_LIST], err, errlen)) return rc;
        // ---- radii
        if (int rc = stage_upload(*h, &h->d_in, &h->in_cap, border, n, os, err, errlen)) return rc;
        NL_HIP(hipMemsetAsync(h->d_any, 0, 4, st));
        if (int rc = stage_start(*h, err, errlen)) return rc;
        nf_border_kernel<<<bf_grid(n), 256, 0, st>>>(NfSet{h->d_in, border_dtype, false}, n, h->bbits, h->d_any);
        NL_CHECK_LAUNCH();
        bf_radius_kernel<<<(unsigned)m, 64, 0, st>>>(h->vox, m, h->g, h->bbits, h->d_any, h->radius);
        NL_CHECK_LAUNCH();
        if (int rc = stage_stop(*h, &h->ms[BF_MS_RADII], err, errlen)) return rc;
        int any = 0;
        NL_HIP(hipMemcpyAsync(&any, h->d_any, 4, hipMemcpyDeviceToHost, st));
        NL_HIP(hipStreamSynchronize(st));
        h->has_border = any != 0;
        // ---- per-label lists: offsets, the sorted values and their median; tips and lone tips
        const i64 P = bf_pow2(m);
        if (int rc = stage_grow(&h->keys2_cap, P, P, {{&h->keys2, sizeof(BfKey2)}}, err, errlen)) return rc;
        if (int rc = bf_scan_reserve(h, B, err, errlen)) return rc;
        if (int rc = stage_start(*h, err, errlen)) return rc;
        i64 total = 0;
        if (int rc = rank_scan(h->scan, st, h->count, B, h->off, BF_MAX_ROWS, "skeleton voxels in one frame", &total, err, errlen)) return rc;
        if (h->has_border) {
            bf_median_keys_kernel<<<bf_grid(P), 256, 0, st>>>(h->rank, h->radius, m, P, h->keys2);
            NL_CHECK_LAUNCH();
            if (int rc = bf_sort(st, h->keys2, P, err, errlen)) return rc;
            bf_median_kernel<<<bf_grid(B), 256, 0, st>>>(h->keys2, h->off, h->count, B, h->median);
            NL_CHECK_LAUNCH();
        }
        if (int rc = bf_pick(h, m, 1, h->tips, &h->n_tips, err, errlen)) return rc;
        if (int rc = bf_pick(h, m, 0, h->lone, &h->n_lone, err, errlen)) return rc;
        if (int rc = stage_stop(*h, &h->ms[BF_MS_LISTS], err, errlen)) return rc;
    }
    NL_HIP(hipStreamSynchronize(st));                                  // the host arrays may go away after the call
    h->m = m;
    h->B = B;
    h->comp_size = (int)cs;
    h->has_frame = true;
    *n_voxels = m;
    *n_labels = B;
    *n_tips = h->n_tips;
    *n_lone = h->n_lone;
    return NL_OK;
}

// Downloads the loaded frame's skeleton list and labels; NULL pointers are skipped (layouts: include/nellie_amd.h).
extern "C" int nl_branchfeat_fetch(nl_branchfeat *h, int64_t *coords, int64_t *labels, uint8_t *degree, double *radius, int64_t *tips, int64_t *lone,
                                   int64_t *branch_label, void *comp, uint32_t *edges, int32_t *count, double *median, char *err, size_t errlen) {
    STAGE_ENTER(h, "branch-feature object");
    if (!h->has_frame) return nl_fail(err, errlen, NL_ESTATE, "no frame loaded");
    hipStream_t st = h->stream;
    const size_t m = (size_t)h->m, B = (size_t)h->B;
    if (m > 0) {
        if (coords) NL_HIP(hipMemcpyAsync(coords, h->coords, m * h->ndim * 8, hipMemcpyDeviceToHost, st));
        if (labels) NL_HIP(hipMemcpyAsync(labels, h->label, m * 8, hipMemcpyDeviceToHost, st));
        if (degree) NL_HIP(hipMemcpyAsync(degree, h->deg, m, hipMemcpyDeviceToHost, st));
        if (radius) NL_HIP(hipMemcpyAsync(radius, h->radius, m * 8, hipMemcpyDeviceToHost, st));
        if (tips && h->n_tips > 0) NL_HIP(hipMemcpyAsync(tips, h->tips, (size_t)h->n_tips * 8, hipMemcpyDeviceToHost, st));
        if (lone && h->n_lone > 0) NL_HIP(hipMemcpyAsync(lone, h->lone, (size_t)h->n_lone * 8, hipMemcpyDeviceToHost, st));
        if (branch_label) NL_HIP(hipMemcpyAsync(branch_label, h->uniq, B * 8, hipMemcpyDeviceToHost, st));
        if (comp) NL_HIP(hipMemcpyAsync(comp, h->comp_l, B * h->comp_size, hipMemcpyDeviceToHost, st));
        if (edges) NL_HIP(hipMemcpyAsync(edges, h->edges, B * h->noff * 4, hipMemcpyDeviceToHost, st));
        if (count) NL_HIP(hipMemcpyAsync(count, h->count, B * 4, hipMemcpyDeviceToHost, st));
        if (median && h->has_border) NL_HIP(hipMemcpyAsync(median, h->median, B * 8, hipMemcpyDeviceToHost, st));
    }
    NL_HIP(hipStreamSynchronize(st));
    if (median && !h->has_border)
        for (size_t b = 0; b < B; ++b) median[b] = NAN;
    return NL_OK;
}

// The regions of a label volume of the object's shape (an integer dtype): its distinct labels > 0 with their sums, and, when
// `reassigned` is not NULL (an integer dtype, values in [0, 2^31)), the most frequent reassigned label over every region.  `rows`
// picks the sum kernel (one lane per voxel, or one head lane per run along X: the same sums); everything else is shared.
// Needs no frame: every buffer it uses is grown here.
static int bf_regions(nl_branchfeat *h, bool rows, const void *labels, int dtype, const void *reassigned, int reassigned_dtype, int64_t *n_regions,
                      char *err, size_t errlen) {
    STAGE_ENTER(h, "branch-feature object");
    if (!labels || !n_regions) return nl_fail(err, errlen, NL_EINVAL, "NULL labels or n_regions");
    const size_t ls = dtype_size(dtype), rs = reassigned ? dtype_size(reassigned_dtype) : 1;
    if (!ls || !bf_label_dtype(dtype)) return nl_fail(err, errlen, NL_EINVAL, "branch labels must have an integer dtype");
    if (reassigned && (!rs || !bf_label_dtype(reassigned_dtype))) return nl_fail(err, errlen, NL_EINVAL, "reassigned labels must have an integer dtype");
    if (h->g.nz > BF_MAX_DIM || h->g.ny > BF_MAX_DIM || h->g.nx > BF_MAX_DIM)
        return nl_fail(err, errlen, NL_EINVAL, "region sums need every extent of the frame to be at most %lld", (long long)BF_MAX_DIM);
    hipStream_t st = h->stream;
    const i64 n = h->g.n;
    h->has_regions = h->has_mode = h->has_convex = h->lab_regions = false;
    h->R = 0;
    *n_regions = 0;
    h->ms[BF_MS_REGIONS] = 0.f;
    if (int rc = stage_upload(*h, &h->d_lab, &h->lab_cap, labels, n, ls, err, errlen)) return rc;
    if (int rc = stage_start(*h, err, errlen)) return rc;
    const BfLabels lab{h->d_lab, dtype, nullptr};
    i64 R = 0;
    const i64 F = h->acc_fields;
    if (int rc = bf_distinct(h, lab, n, &h->runiq, &h->reg_rows, {{&h->acc, 16 * 8}, {&h->best, 8}}, &R, err, errlen)) return rc;
    std::vector<u64> counts;
    i64 total = 0;
    if (R > 0) {
        NL_HIP(hipMemsetAsync(h->acc, 0, (size_t)(F * R) * 8, st));
        NL_HIP(hipMemsetAsync(h->acc + R, 0xff, (size_t)(h->ndim * R) * 8, st));      // the smallest coordinates
        const i64 bands = (h->g.ny + BF_ROWS_BAND - 1) / BF_ROWS_BAND;        // nz * bands <= 2^15 * 2^11 workgroups
        if (rows && h->ndim == 3) bf_region_rows_kernel<3><<<(unsigned)(h->g.nz * bands), 256, 0, st>>>(lab, h->g, bands, h->pres, h->lpre, R, h->acc);
        else if (rows) bf_region_rows_kernel<2><<<(unsigned)(h->g.nz * bands), 256, 0, st>>>(lab, h->g, bands, h->pres, h->lpre, R, h->acc);
        else if (h->ndim == 3) bf_region_kernel<3><<<bf_grid(n), 256, 0, st>>>(lab, n, h->g, h->pres, h->lpre, R, h->acc);
        else bf_region_kernel<2><<<bf_grid(n), 256, 0, st>>>(lab, n, h->g, h->pres, h->lpre, R, h->acc);
        NL_CHECK_LAUNCH();
        counts.resize((size_t)R);
        NL_HIP(hipMemcpyAsync(counts.data(), h->acc, (size_t)R * 8, hipMemcpyDeviceToHost, st));
        NL_HIP(hipStreamSynchronize(st));
        for (u64 c : counts) total += (i64)c;
        if (total > BF_MAX_ROWS) return nl_fail(err, errlen, NL_EINVAL, "more than %lld region voxels in one frame", (long long)BF_MAX_ROWS);
    }
    if (int rc = stage_stop(*h, &h->ms[BF_MS_REGIONS], err, errlen)) return rc;
    if (reassigned && R > 0) {
        const i64 P = bf_pow2(total);
        if (int rc = stage_grow(&h->keys_cap, P, P, {{&h->keys, 8}}, err, errlen)) return rc;
        if (int rc = stage_upload(*h, &h->d_in, &h->in_cap, reassigned, n, rs, err, errlen)) return rc;
        NL_HIP(hipMemsetAsync(h->keys, 0xff, (size_t)P * 8, st));     // above every key
        NL_HIP(hipMemsetAsync(h->d_word, 0, 8, st));
        NL_HIP(hipMemsetAsync(h->d_any + 1, 0, 4, st));
        NL_HIP(hipMemsetAsync(h->best, 0, (size_t)R * 8, st));
        if (int rc = stage_start(*h, err, errlen)) return rc;
        bf_mode_keys_kernel<<<bf_grid(n), 256, 0, st>>>(lab, BfLabels{h->d_in, reassigned_dtype, nullptr}, n, h->pres, h->lpre, h->keys, P, h->d_word,
                                                        h->d_any + 1);
        NL_CHECK_LAUNCH();
        int bad = 0;
        NL_HIP(hipMemcpyAsync(&bad, h->d_any + 1, 4, hipMemcpyDeviceToHost, st));
        i64 appended = 0;
        if (int rc = bf_fetch_word(h, h->d_word, &appended, err, errlen)) return rc;
        // a refused label appended no key: the slots past `appended` hold the padding, which belongs to no region
        if (bad || appended != total) return nl_fail(err, errlen, NL_EINVAL, "a reassigned label is negative or above 2^31 - 1");
        if (int rc = bf_sort(st, h->keys, P, err, errlen)) return rc;
        bf_mode_kernel<<<bf_grid(appended), 256, 0, st>>>(h->keys, appended, R, h->best);
        NL_CHECK_LAUNCH();
        if (int rc = stage_stop(*h, &h->ms[BF_MS_REGIONS], err, errlen)) return rc;
        h->has_mode = true;
    }
    NL_HIP(hipStreamSynchronize(st));
    h->R = R;
    h->has_regions = h->lab_regions = true;
    h->reg_dtype = dtype;
    *n_regions = R;
    return NL_OK;
}

extern "C" int nl_branchfeat_regions(nl_branchfeat *h, const void *labels, int dtype, const void *reassigned, int reassigned_dtype, int64_t *n_regions,
                                     char *err, size_t errlen) {
    return bf_regions(h, false, labels, dtype, reassigned, reassigned_dtype, n_regions, err, errlen);
}

extern "C" int nl_branchfeat_regions_rows(nl_branchfeat *h, const void *labels, int dtype, const void *reassigned, int reassigned_dtype,
                                          int64_t *n_regions, char *err, size_t errlen) {
    return bf_regions(h, true, labels, dtype, reassigned, reassigned_dtype, n_regions, err, errlen);
}

// Downloads the loaded regions: labels (R) int64 ascending, sums (fields, R) int64 with fields = 1 + 3 D + D (D + 1) / 2 (n, the
// smallest and the largest coordinate per axis, S_a, Q_ab for a <= b), mode (R) int64, -1 where no reassigned labels were given.
extern "C" int nl_branchfeat_fetch_regions(nl_branchfeat *h, int64_t *labels, int64_t *sums, int64_t *mode, char *err, size_t errlen) {
    STAGE_ENTER(h, "branch-feature object");
    if (!h->has_regions) return nl_fail(err, errlen, NL_ESTATE, "no regions loaded");
    hipStream_t st = h->stream;
    const size_t R = (size_t)h->R;
    std::vector<u64> best(mode && h->has_mode ? R : 0);
    if (R > 0) {
        if (labels) NL_HIP(hipMemcpyAsync(labels, h->runiq, R * 8, hipMemcpyDeviceToHost, st));
        if (sums) NL_HIP(hipMemcpyAsync(sums, h->acc, R * (size_t)h->acc_fields * 8, hipMemcpyDeviceToHost, st));
        if (!best.empty()) NL_HIP(hipMemcpyAsync(best.data(), h->best, R * 8, hipMemcpyDeviceToHost, st));
    }
    NL_HIP(hipStreamSynchronize(st));
    if (mode)
        for (size_t r = 0; r < R; ++r) mode[r] = best.empty() ? -1 : (int64_t)(0xffffffffull - (best[r] & 0xffffffffull));
    return NL_OK;
}

// Device time (ms) of the kernels, per part: ms[0] skeleton list, labels and component labels, [1] degree and edge counts, [2] border
// mask and radii, [3] per-label lists, medians and tips (all four since the last nl_branchfeat_frame), [4] region sums and the
// most frequent reassigned label (since the last nl_branchfeat_regions).  Transfers excluded.
extern "C" int nl_branchfeat_kernel_ms(nl_branchfeat *h, float *ms, char *err, size_t errlen) {
    if (!h || !ms) return nl_fail(err, errlen, NL_EINVAL, "branch-feature object or ms is NULL");
    for (int j = 0; j < BF_MS_PARTS; ++j) ms[j] = h->ms[j];
    return NL_OK;
}

// ---- convex counts ---------------------------------------------------------------------------------------------------------------
// The convex counts of the loaded regions: works on the label frame the last nl_branchfeat_regions /
// _regions_rows call left on the device and on its region table, so it follows that call directly (nl_branchfeat_frame in
// between replaces the frame: NL_ESTATE).  Device: the candidates (row extremes, per-plane hulls) and the count; host: the hull of
// every region from its candidates (convex_hull.h).
extern "C" int nl_branchfeat_convex(nl_branchfeat *h, char *err, size_t errlen) {
    STAGE_ENTER(h, "branch-feature object");
    if (!h->has_regions || !h->lab_regions) return nl_fail(err, errlen, NL_ESTATE, "no regions loaded, or a frame was loaded after them");
    hipStream_t st = h->stream;
    const i64 R = h->R, n = h->g.n;
    const int D = h->ndim;
    h->has_convex = false;
    for (int j = 0; j < CV_MS_PARTS; ++j) h->cms[j] = 0.f;
    h->cv_nfacets.assign((size_t)R, 0);
    h->cv_nrows.assign((size_t)R, 0);
    if (R == 0) { h->has_convex = true; return NL_OK; }
    // ---- boxes, row and plane offsets
    std::vector<u64> lohi((size_t)(2 * D * R));
    NL_HIP(hipMemcpyAsync(lohi.data(), h->acc + R, lohi.size() * 8, hipMemcpyDeviceToHost, st));
    NL_HIP(hipStreamSynchronize(st));
    std::vector<CvBox> box((size_t)R);
    std::vector<i64> rowoff((size_t)R + 1, 0), planeoff((size_t)R + 1, 0);
    for (i64 r = 0; r < R; ++r) {
        CvBox &b = box[(size_t)r];
        for (int a = 0; a < 3; ++a) {
            const int k = a - (3 - D);                                 // the axis among the frame's own
            b.lo[a] = k < 0 ? 0 : (int)lohi[(size_t)(k * R + r)];
            b.ext[a] = k < 0 ? 1 : (int)(lohi[(size_t)((D + k) * R + r)] - lohi[(size_t)(k * R + r)]) + 1;
        }
        h->cv_nrows[(size_t)r] = (i64)b.ext[0] * b.ext[1];
        rowoff[(size_t)r + 1] = rowoff[(size_t)r] + h->cv_nrows[(size_t)r];
        planeoff[(size_t)r + 1] = planeoff[(size_t)r] + b.ext[0];
        if (rowoff[(size_t)r + 1] > CV_MAX_ROWS)
            return nl_fail(err, errlen, NL_EINVAL, "the regions' bounding boxes hold more than %lld rows", (long long)CV_MAX_ROWS);
    }
    const i64 rows = rowoff[(size_t)R], planes = planeoff[(size_t)R];
    if (int rc = stage_grow(&h->cv_cap, R + 1, R + 1, {{&h->cbox, sizeof(CvBox)}, {&h->crowoff, 8}, {&h->cplaneoff, 8}, {&h->cfacetoff, 8}, {&h->ccount, 8}},
                            err, errlen)) return rc;
    if (int rc = stage_grow(&h->crow_cap, rows, rows, {{&h->cxmin, 4}, {&h->cxmax, 4}, {&h->ckeep_lo, 4}, {&h->ckeep_hi, 4}}, err, errlen)) return rc;
    NL_HIP(hipMemcpyAsync(h->cbox, box.data(), (size_t)R * sizeof(CvBox), hipMemcpyHostToDevice, st));
    NL_HIP(hipMemcpyAsync(h->crowoff, rowoff.data(), ((size_t)R + 1) * 8, hipMemcpyHostToDevice, st));
    NL_HIP(hipMemcpyAsync(h->cplaneoff, planeoff.data(), ((size_t)R + 1) * 8, hipMemcpyHostToDevice, st));
    NL_HIP(hipMemsetAsync(h->cxmin, 0x7f, (size_t)rows * 4, st));
    NL_HIP(hipMemsetAsync(h->cxmax, 0xff, (size_t)rows * 4, st));
    NL_HIP(hipMemsetAsync(h->ccount, 0, (size_t)R * 8, st));
    // ---- step 1: candidates
    const BfLabels lab{h->d_lab, h->reg_dtype, nullptr};
    if (int rc = stage_start(*h, err, errlen)) return rc;
    cv_extremes_kernel<<<bf_grid(n), 256, 0, st>>>(lab, n, h->g, h->pres, h->lpre, h->cbox, h->crowoff, h->cxmin, h->cxmax);
    NL_CHECK_LAUNCH();
    if (int rc = stage_stop(*h, &h->cms[CV_MS_EXTREMES], err, errlen)) return rc;
    if (int rc = stage_start(*h, err, errlen)) return rc;
    cv_plane_kernel<<<bf_grid(planes), 256, 0, st>>>(planes, R, h->cplaneoff, h->cbox, h->crowoff, h->cxmin, h->cxmax, h->ckeep_lo, h->ckeep_hi);
    NL_CHECK_LAUNCH();
    if (int rc = stage_stop(*h, &h->cms[CV_MS_PLANES], err, errlen)) return rc;
    std::vector<int> xmin((size_t)rows), xmax((size_t)rows);
    NL_HIP(hipMemcpyAsync(xmin.data(), h->cxmin, (size_t)rows * 4, hipMemcpyDeviceToHost, st));
    NL_HIP(hipMemcpyAsync(xmax.data(), h->cxmax, (size_t)rows * 4, hipMemcpyDeviceToHost, st));
    NL_HIP(hipStreamSynchronize(st));
    // ---- step 2: the hulls
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<nl_convex::Facet> facets;
    std::vector<i64> facetoff((size_t)R + 1, 0), cand;
    std::vector<CvTask> tasks;
    for (i64 r = 0; r < R; ++r) {
        const CvBox &b = box[(size_t)r];
        cand.clear();
        for (i64 row = 0; row < h->cv_nrows[(size_t)r]; ++row) {
            const int lo = xmin[(size_t)(rowoff[(size_t)r] + row)], hi = xmax[(size_t)(rowoff[(size_t)r] + row)];
            const i64 z = row / b.ext[1], y = row % b.ext[1];
            for (int e = 0; e < 2; ++e) {
                const int x = e ? hi : lo;
                if (x < 0 || x == CV_NO_MIN || (e && hi == lo)) continue;
                if (D == 3) cand.push_back(z);
                cand.push_back(y);
                cand.push_back((i64)x - b.lo[2]);
            }
        }
        nl_convex::ch_facets(cand.data(), (i64)cand.size() / D, D, facets);
        facetoff[(size_t)r + 1] = (i64)facets.size();
        h->cv_nfacets[(size_t)r] = facetoff[(size_t)r + 1] - facetoff[(size_t)r];
        if (h->cv_nfacets[(size_t)r] > 0)
            for (i64 row0 = 0; row0 < h->cv_nrows[(size_t)r]; row0 += CV_WG) tasks.push_back(CvTask{(int)r, (int)row0});
    }
    h->cms[CV_MS_HULL] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    // ---- step 3: the count
    const i64 nf = (i64)facets.size(), nt = (i64)tasks.size();
    if (nt > 0) {
        if (int rc = stage_grow(&h->cfacet_cap, nf, stage_doubled(h->cfacet_cap, nf), {{&h->cfacets, 4 * 8}}, err, errlen)) return rc;
        if (int rc = stage_grow(&h->ctask_cap, nt, stage_doubled(h->ctask_cap, nt), {{&h->ctasks, sizeof(CvTask)}}, err, errlen)) return rc;
        static_assert(sizeof(nl_convex::Facet) == 4 * 8, "a facet is four int64");
        NL_HIP(hipMemcpyAsync(h->cfacets, facets.data(), (size_t)nf * 32, hipMemcpyHostToDevice, st));
        NL_HIP(hipMemcpyAsync(h->ctasks, tasks.data(), (size_t)nt * sizeof(CvTask), hipMemcpyHostToDevice, st));
        NL_HIP(hipMemcpyAsync(h->cfacetoff, facetoff.data(), ((size_t)R + 1) * 8, hipMemcpyHostToDevice, st));
        if (int rc = stage_start(*h, err, errlen)) return rc;
        cv_count_kernel<<<(unsigned)(nt < CV_MAX_GRID ? nt : CV_MAX_GRID), CV_WG, 0, st>>>(h->ctasks, nt, h->cbox, h->cfacetoff, h->cfacets, h->ccount);
        NL_CHECK_LAUNCH();
        if (int rc = stage_stop(*h, &h->cms[CV_MS_COUNT], err, errlen)) return rc;
    }
    NL_HIP(hipStreamSynchronize(st));                                  // the host vectors go away
    h->has_convex = true;
    return NL_OK;
}

// Downloads the convex counts of the loaded regions: count (R) int64, 0 for a 3-D region whose voxel centres lie in one plane;
// facets (R) int64 = the facets of every region's hull, rows (R) int64 = the rows of its bounding box.  NULL pointers are skipped.
extern "C" int nl_branchfeat_fetch_convex(nl_branchfeat *h, int64_t *count, int64_t *facets, int64_t *rows, char *err, size_t errlen) {
    STAGE_ENTER(h, "branch-feature object");
    if (!h->has_convex) return nl_fail(err, errlen, NL_ESTATE, "no convex counts taken");
    const size_t R = (size_t)h->R;
    if (R > 0 && count) {
        NL_HIP(hipMemcpyAsync(count, h->ccount, R * 8, hipMemcpyDeviceToHost, h->stream));
        NL_HIP(hipStreamSynchronize(h->stream));
    }
    for (size_t r = 0; r < R; ++r) {
        if (facets) facets[r] = h->cv_nfacets[r];
        if (rows) rows[r] = h->cv_nrows[r];
    }
    return NL_OK;
}

// ms[4] of the last nl_branchfeat_convex: device time of the row extremes, of the per-plane hulls and of the count (transfers
// excluded), then the host time of the hulls.
extern "C" int nl_branchfeat_convex_ms(nl_branchfeat *h, float *ms, char *err, size_t errlen) {
    if (!h || !ms) return nl_fail(err, errlen, NL_EINVAL, "branch-feature object or ms is NULL");
    for (int j = 0; j < CV_MS_PARTS; ++j) ms[j] = h->cms[j];
    return NL_OK;
}

// limits[3]: the box rows of one workgroup of the count kernel, the facets of one staging chunk, the workgroups of one launch.
extern "C" int nl_branchfeat_convex_limits(int64_t *limits, char *err, size_t errlen) {
    if (!limits) return nl_fail(err, errlen, NL_EINVAL, "limits is NULL");
    limits[0] = CV_WG; limits[1] = CV_CHUNK; limits[2] = CV_MAX_GRID;
    return NL_OK;
}

// Host only: the facets (N_z, N_y, N_x, d), N . p <= d inside in doubled coordinates, of the hull of the diamonds of `n` voxels
// coords (n, ndim) int64 with 0 <= c < 2^15; none for a 3-D set of affine rank < 3.  Writes at most `cap` facets, *n_facets = how
// many there are.
extern "C" int nl_host_convex_facets(const int64_t *coords, int64_t n, int ndim, int64_t *facets, int64_t cap, int64_t *n_facets, char *err,
                                     size_t errlen) {
    if (!coords || !n_facets || n < 1 || (ndim != 2 && ndim != 3) || (cap > 0 && !facets)) return nl_fail(err, errlen, NL_EINVAL, "bad arguments");
    for (int64_t i = 0; i < n * ndim; ++i)
        if (coords[i] < 0 || coords[i] >= BF_MAX_DIM) return nl_fail(err, errlen, NL_EINVAL, "coordinates must lie in [0, %lld)", (long long)BF_MAX_DIM);
    std::vector<nl_convex::Facet> f;
    nl_convex::ch_facets((const nl_convex::ci64 *)coords, n, ndim, f);
    *n_facets = (int64_t)f.size();
    for (int64_t k = 0; k < cap && k < (int64_t)f.size(); ++k) {
        facets[4 * k] = f[(size_t)k].nz; facets[4 * k + 1] = f[(size_t)k].ny; facets[4 * k + 2] = f[(size_t)k].nx; facets[4 * k + 3] = f[(size_t)k].d;
    }
    return NL_OK;
}
