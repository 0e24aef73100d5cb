// Translation unit of libnellie_hip.so (gfx950): the edge lists of the hierarchy's adjacency maps (_save_adjacency_maps of
// nellie/feature_extraction/hierarchical.py).  C-ABI in include/nellie_amd.h; kernels in adjacency.inc.  The object owns its buffers
// and stream and has no frame shape: every call brings its own row count.  An operation leaves its (m, 2) int64 rows on the device;
// nl_adjacency_fetch downloads them.
#include <string.h>
#include "nl_stage.h"
#include "adjacency.inc"

#define ADJ_MAX_ROWS ((i64)1 << 36)            // rows of one call: the mask kernels' grid
#define ADJ_MAX_EDGES (((i64)1 << 31) - 1)     // edges of one call: ranks are ints
#define ADJ_MAX_LABEL (((i64)1 << 31) - 2)     // the largest parent label: the table has one entry per label up to it
enum { ADJ_MS_PAIRS, ADJ_MS_EXPAND, ADJ_MS_LOOKUP, ADJ_MS_PARTS };

struct nl_adjacency : StageBase {
    void *d_in = nullptr; i64 in_cap = 0;           // the labels, the CSR's values or the children being uploaded, bytes
    void *d_aux = nullptr; i64 aux_cap = 0;         // the CSR's offsets or the parents, bytes
    i64 *d_table = nullptr; i64 table_cap = 0;      // lookup: label -> position
    i64 *d_bad = nullptr, *h_bad = nullptr;         // lookup: the first child above the table, and its pinned landing place
    u64 *d_bits = nullptr; int *d_wcount = nullptr, *d_pre = nullptr; i64 word_cap = 0;
    RankScan scan; i64 sum_cap = 0;
    longlong2 *d_out = nullptr; i64 out_cap = 0;
    i64 m = 0; bool has_rows = false;
    float ms[ADJ_MS_PARTS] = {0.f, 0.f, 0.f};
};

extern "C" int nl_adjacency_destroy(nl_adjacency *h) {
    if (!h) return NL_OK;
    stage_close(*h, {h->d_in, h->d_aux, h->d_table, h->d_bad, h->d_bits, h->d_wcount, h->d_pre, h->scan.d_bsum, h->scan.d_total, h->d_out},
                {h->scan.h_total, h->h_bad});
    delete h;
    return NL_OK;
}

extern "C" int nl_adjacency_create(nl_adjacency **out, int device, char *err, size_t errlen) {
    if (!out) return nl_fail(err, errlen, NL_EINVAL, "out is NULL");
    *out = nullptr;
    if (int rc = stage_check_device(device, err, errlen)) return rc;
    nl_adjacency *h = new nl_adjacency();
    if (int rc = stage_open(*h, device, true, err, errlen)) { nl_adjacency_destroy(h); return rc; }
    STAGE_HIP(stage_alloc(&h->d_bad, 1, 8), nl_adjacency_destroy(h));
    STAGE_HIP(stage_alloc(&h->scan.d_total, 1, 8), nl_adjacency_destroy(h));
    STAGE_HIP(hipHostMalloc((void **)&h->scan.h_total, 8, hipHostMallocDefault), nl_adjacency_destroy(h));
    STAGE_HIP(hipHostMalloc((void **)&h->h_bad, 8, hipHostMallocDefault), nl_adjacency_destroy(h));
    *out = h;
    return NL_OK;
}

// the mask words of n rows (a multiple of 4: one workgroup of the mask kernel writes 4) and the buffers of a scan over them
static int adj_words(nl_adjacency *h, i64 n, i64 *words, char *err, size_t errlen) {
    *words = ((n + 255) / 256) * 4;
    if (int rc = stage_grow(&h->word_cap, *words, stage_doubled(h->word_cap, *words), {{&h->d_bits, 8}, {&h->d_wcount, 4}, {&h->d_pre, 4}}, err, errlen)) return rc;
    const i64 sums = rank_scan_sums(h->word_cap);
    return stage_grow(&h->sum_cap, sums, sums, {{&h->scan.d_bsum, 8}}, err, errlen);
}

// Ranks the rows of the mask in d_bits / d_wcount and makes room for their pairs.
static int adj_rank(nl_adjacency *h, i64 words, i64 *m, char *err, size_t errlen) {
    if (int rc = rank_scan(h->scan, h->stream, h->d_wcount, words, h->d_pre, ADJ_MAX_EDGES, "edges in one list", m, err, errlen)) return rc;
    return stage_grow(&h->out_cap, *m, stage_doubled(h->out_cap, *m), {{&h->d_out, 16}}, err, errlen);
}

// The rows (i, labels[i] - bias) of every i with labels[i] > 0, ascending in i.  labels: n elements of NL_I32 or NL_I64.
extern "C" int nl_adjacency_pairs(nl_adjacency *h, const void *labels, int dtype, int64_t n, int64_t bias, int64_t *n_edges, char *err, size_t errlen) {
    STAGE_ENTER(h, "adjacency object");
    if (!n_edges || n < 0 || (n > 0 && !labels)) return nl_fail(err, errlen, NL_EINVAL, "NULL labels or n_edges, or a negative row count");
    if (dtype != NL_I32 && dtype != NL_I64) return nl_fail(err, errlen, NL_EINVAL, "labels must be int32 or int64");
    if (n > ADJ_MAX_ROWS) return nl_fail(err, errlen, NL_EINVAL, "more than %lld rows", (long long)ADJ_MAX_ROWS);
    h->has_rows = false;
    h->m = 0;
    h->ms[ADJ_MS_PAIRS] = 0.f;
    *n_edges = 0;
    i64 m = 0;
    if (n > 0) {
        hipStream_t st = h->stream;
        i64 words = 0;
        if (int rc = adj_words(h, n, &words, err, errlen)) return rc;
        if (int rc = stage_upload(*h, &h->d_in, &h->in_cap, labels, n, dtype_size(dtype), err, errlen)) return rc;
        const AdjLabels lab{h->d_in, dtype == NL_I64};
        const unsigned gv = (unsigned)((n + 255) / 256);
        if (int rc = stage_start(*h, err, errlen)) return rc;
        rank_mask_kernel<<<gv, 256, 0, st>>>(AdjPositive{lab}, n, h->d_bits, h->d_wcount);
        NL_CHECK_LAUNCH();
        if (int rc = adj_rank(h, words, &m, err, errlen)) return rc;
        if (m > 0) {
            adj_pairs_write_kernel<<<gv, 256, 0, st>>>(lab, n, bias, h->d_pre, h->d_out);
            NL_CHECK_LAUNCH();
        }
        if (int rc = stage_stop(*h, &h->ms[ADJ_MS_PAIRS], err, errlen)) return rc;      // synchronises: the host array may go away
    }
    h->m = m;
    h->has_rows = true;
    *n_edges = m;
    return NL_OK;
}

// The CSR (offsets of n_rows + 1 entries, values) as rows (r, values[e]) for every e of row r: rows ascend, values keep their order.
extern "C" int nl_adjacency_expand(nl_adjacency *h, const int64_t *offsets, const int64_t *values, int64_t n_rows, int64_t *n_edges, char *err,
                                   size_t errlen) {
    STAGE_ENTER(h, "adjacency object");
    if (!offsets || !n_edges || n_rows < 0) return nl_fail(err, errlen, NL_EINVAL, "NULL offsets or n_edges, or a negative row count");
    h->has_rows = false;
    h->m = 0;
    h->ms[ADJ_MS_EXPAND] = 0.f;
    *n_edges = 0;
    if (offsets[0] != 0) return nl_fail(err, errlen, NL_EINVAL, "offsets must start at 0");
    for (i64 r = 0; r < n_rows; ++r)
        if (offsets[r + 1] < offsets[r]) return nl_fail(err, errlen, NL_EINVAL, "offsets must not decrease (row %lld)", (long long)r);
    const i64 E = offsets[n_rows];
    if (E > ADJ_MAX_EDGES) return nl_fail(err, errlen, NL_EINVAL, "more than %lld edges in one list", (long long)ADJ_MAX_EDGES);
    if (E > 0 && !values) return nl_fail(err, errlen, NL_EINVAL, "values is NULL");
    if (E > 0) {
        hipStream_t st = h->stream;
        if (int rc = stage_grow(&h->out_cap, E, stage_doubled(h->out_cap, E), {{&h->d_out, 16}}, err, errlen)) return rc;
        if (int rc = stage_upload(*h, &h->d_aux, &h->aux_cap, offsets, n_rows + 1, 8, err, errlen)) return rc;
        if (int rc = stage_upload(*h, &h->d_in, &h->in_cap, values, E, 8, err, errlen)) return rc;
        if (int rc = stage_start(*h, err, errlen)) return rc;
        adj_expand_kernel<<<(unsigned)((E + 255) / 256), 256, 0, st>>>((const i64 *)h->d_aux, n_rows, (const i64 *)h->d_in, E, h->d_out);
        NL_CHECK_LAUNCH();
        if (int rc = stage_stop(*h, &h->ms[ADJ_MS_EXPAND], err, errlen)) return rc;
    }
    h->m = E;
    h->has_rows = true;
    *n_edges = E;
    return NL_OK;
}

// The rows (i, j) where j is the last position of child[i] in parent, for every child listed there, ascending in i.  Labels are
// int64 and not negative; a child above the largest parent label is an error that names its row.
extern "C" int nl_adjacency_lookup(nl_adjacency *h, const int64_t *child, int64_t n, const int64_t *parent, int64_t p, int64_t *n_edges, char *err,
                                   size_t errlen) {
    STAGE_ENTER(h, "adjacency object");
    if (!n_edges || n < 0 || p < 0 || (n > 0 && !child) || (p > 0 && !parent)) return nl_fail(err, errlen, NL_EINVAL, "NULL labels or n_edges, or a negative count");
    if (n > ADJ_MAX_ROWS || p > ADJ_MAX_ROWS) return nl_fail(err, errlen, NL_EINVAL, "more than %lld rows", (long long)ADJ_MAX_ROWS);
    h->has_rows = false;
    h->m = 0;
    h->ms[ADJ_MS_LOOKUP] = 0.f;
    *n_edges = 0;
    i64 max_label = -1;
    for (i64 j = 0; j < p; ++j) {
        if (parent[j] < 0) return nl_fail(err, errlen, NL_EINVAL, "parent row %lld holds the negative label %lld", (long long)j, (long long)parent[j]);
        max_label = parent[j] > max_label ? parent[j] : max_label;
    }
    for (i64 i = 0; i < n; ++i)
        if (child[i] < 0) return nl_fail(err, errlen, NL_EINVAL, "row %lld holds the negative label %lld", (long long)i, (long long)child[i]);
    if (max_label > ADJ_MAX_LABEL) return nl_fail(err, errlen, NL_EINVAL, "parent label %lld above %lld", (long long)max_label, (long long)ADJ_MAX_LABEL);
    i64 m = 0;
    if (p > 0 && n > 0) {
        hipStream_t st = h->stream;
        i64 words = 0;
        if (int rc = adj_words(h, n, &words, err, errlen)) return rc;
        if (int rc = stage_grow(&h->table_cap, max_label + 1, stage_doubled(h->table_cap, max_label + 1), {{&h->d_table, 8}}, err, errlen)) return rc;
        if (int rc = stage_upload(*h, &h->d_aux, &h->aux_cap, parent, p, 8, err, errlen)) return rc;
        if (int rc = stage_upload(*h, &h->d_in, &h->in_cap, child, n, 8, err, errlen)) return rc;
        NL_HIP(hipMemsetAsync(h->d_table, 0xFF, (size_t)(max_label + 1) * 8, st));       // every entry -1
        NL_HIP(hipMemsetAsync(h->d_bad, 0x7F, 8, st));                                   // above every row
        const unsigned gv = (unsigned)((n + 255) / 256);
        if (int rc = stage_start(*h, err, errlen)) return rc;
        adj_table_kernel<<<(unsigned)((p + 255) / 256), 256, 0, st>>>((const i64 *)h->d_aux, p, h->d_table);
        NL_CHECK_LAUNCH();
        rank_mask_kernel<<<gv, 256, 0, st>>>(AdjListed{(const i64 *)h->d_in, h->d_table, max_label, h->d_bad}, n, h->d_bits, h->d_wcount);
        NL_CHECK_LAUNCH();
        NL_HIP(hipMemcpyAsync(h->h_bad, h->d_bad, 8, hipMemcpyDeviceToHost, st));
        NL_HIP(hipStreamSynchronize(st));
        const i64 bad = *h->h_bad;
        if (bad < n)
            return nl_fail(err, errlen, NL_EINVAL, "row %lld holds label %lld, above the parents' largest label %lld", (long long)bad, (long long)child[bad],
                           (long long)max_label);
        if (int rc = adj_rank(h, words, &m, err, errlen)) return rc;
        if (m > 0) {
            adj_lookup_write_kernel<<<gv, 256, 0, st>>>((const i64 *)h->d_in, n, h->d_table, h->d_pre, h->d_out);
            NL_CHECK_LAUNCH();
        }
        if (int rc = stage_stop(*h, &h->ms[ADJ_MS_LOOKUP], err, errlen)) return rc;
    }
    h->m = m;
    h->has_rows = true;
    *n_edges = m;
    return NL_OK;
}

// Downloads the rows of the last operation: out (n_edges, 2) int64.
extern "C" int nl_adjacency_fetch(nl_adjacency *h, int64_t *out, char *err, size_t errlen) {
    STAGE_ENTER(h, "adjacency object");
    if (!h->has_rows) return nl_fail(err, errlen, NL_ESTATE, "no edge list computed");
    if (h->m > 0) {
        if (!out) return nl_fail(err, errlen, NL_EINVAL, "out is NULL");
        NL_HIP(hipMemcpyAsync(out, h->d_out, (size_t)h->m * 16, hipMemcpyDeviceToHost, h->stream));
        NL_HIP(hipStreamSynchronize(h->stream));
    }
    return NL_OK;
}

// Device time (ms) of the kernels of the last call of each operation: ms[0] pairs, [1] expand, [2] lookup.  Transfers excluded.
extern "C" int nl_adjacency_kernel_ms(nl_adjacency *h, float *ms, char *err, size_t errlen) {
    if (!h || !ms) return nl_fail(err, errlen, NL_EINVAL, "adjacency object or ms is NULL");
    for (int j = 0; j < ADJ_MS_PARTS; ++j) ms[j] = h->ms[j];
    return NL_OK;
}
