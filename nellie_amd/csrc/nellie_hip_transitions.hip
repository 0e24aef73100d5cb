// Translation unit of libnellie_hip.so (gfx950): label transition counts from voxel matches (the consumer of `voxel_matches`,
// scripts/voxel_reassignment_demo.py of the reference).  C-ABI in include/nellie_amd.h; kernels in
// transitions.inc.  A handle is made for one frame shape and owns its buffers and stream: two label frames (the later one of a pair
// becomes the earlier one of the next without a second upload), the coordinates of the rows in flight, the counting table with its
// occupancy mask and scan, the compacted entries and the relabelled frame.
#include "nl_stage.h"
#include "transitions.inc"

#define TR_MAX_ROWS ((i64)1 << 31)             // rows of one launch
#define TR_MAX_SLOTS ((i64)1 << 34)            // slots of the table: the mask kernels' grid
#define TR_MAX_ENTRIES (((i64)1 << 31) - 1)    // distinct keys of a pair: ranks are ints
enum { TR_MS_CLEAR, TR_MS_COUNT, TR_MS_COMPACT, TR_MS_RELABEL, TR_MS_PARTS };

struct TrFrame {
    void *d = nullptr; i64 cap = 0;   // the labels, bytes
    int wide = 0;                     // int64 elements
    bool loaded = false;
    i64 top = 0; bool has_top = false;      // the largest label, once asked for
};

struct nl_trans : StageBase {
    int ndim = 3;
    i64 nz = 1, ny = 1, nx = 1, n = 0;
    TrFrame fr[2];                    // [0]: frame t ("prev"), [1]: frame t + 1 ("next")
    void *d_coord = nullptr; i64 coord_cap = 0;      // both ends of the rows of one launch, bytes
    ulonglong2 *d_table = nullptr; i64 table_cap = 0, slots = 0;
    u64 *d_bits = nullptr; int *d_wcount = nullptr, *d_pre = nullptr; i64 word_cap = 0;
    RankScan scan; i64 sum_cap = 0;
    ulonglong2 *d_entries = nullptr; i64 entry_cap = 0;
    i64 *d_words = nullptr, *h_words = nullptr;      // TR_WORDS words and the largest label; their pinned landing place
    int *d_lut = nullptr; i64 lut_cap = 0;
    int *d_out = nullptr; i64 out_cap = 0;
    bool counting = false, overflowed = false, relabelled = false;
    i64 entries = -1;                 // of the finished pair, -1: none
    float ms[TR_MS_PARTS] = {0.f, 0.f, 0.f, 0.f};
};

extern "C" int nl_trans_destroy(nl_trans *h) {
    if (!h) return NL_OK;
    stage_close(*h, {h->fr[0].d, h->fr[1].d, h->d_coord, h->d_table, h->d_bits, h->d_wcount, h->d_pre, h->scan.d_bsum, h->scan.d_total, h->d_entries, h->d_words,
                     h->d_lut, h->d_out}, {h->scan.h_total, h->h_words});
    delete h;
    return NL_OK;
}

extern "C" int nl_trans_create(nl_trans **out, int device, int ndim, int64_t nz, int64_t ny, int64_t nx, char *err, size_t errlen) {
    if (!out) return nl_fail(err, errlen, NL_EINVAL, "out is NULL");
    *out = nullptr;
    const double unit[3] = {1.0, 1.0, 1.0};
    if (int rc = stage_check_frame(ndim, unit, nz, ny, nx, err, errlen)) return rc;
    if (int rc = stage_check_device(device, err, errlen)) return rc;
    nl_trans *h = new nl_trans();
    h->ndim = ndim;
    h->nz = nz; h->ny = ny; h->nx = nx;
    h->n = nz * ny * nx;
    if (int rc = stage_open(*h, device, true, err, errlen)) { nl_trans_destroy(h); return rc; }
    STAGE_HIP(stage_alloc(&h->d_words, TR_WORDS + 1, 8), nl_trans_destroy(h));
    STAGE_HIP(stage_alloc(&h->scan.d_total, 1, 8), nl_trans_destroy(h));
    STAGE_HIP(hipHostMalloc((void **)&h->scan.h_total, 8, hipHostMallocDefault), nl_trans_destroy(h));
    STAGE_HIP(hipHostMalloc((void **)&h->h_words, (TR_WORDS + 1) * 8, hipHostMallocDefault), nl_trans_destroy(h));
    *out = h;
    return NL_OK;
}

// The next label frame (the handle's shape, NL_I32 or NL_I64): the frame that was "next" becomes "prev", this one "next".  A pair
// that was being counted is abandoned.
extern "C" int nl_trans_frame(nl_trans *h, const void *labels, int dtype, char *err, size_t errlen) {
    STAGE_ENTER(h, "transitions object");
    if (!labels) return nl_fail(err, errlen, NL_EINVAL, "labels is NULL");
    if (dtype != NL_I32 && dtype != NL_I64) return nl_fail(err, errlen, NL_EINVAL, "labels must be int32 or int64");
    h->counting = false;
    h->entries = -1;
    h->relabelled = false;
    // the new frame goes into the slot of the frame that leaves, and the slots change places once it stands: after a failed upload
    // "next" is still "next" and "prev" holds nothing
    TrFrame &f = h->fr[0];
    f.loaded = f.has_top = false;
    f.wide = dtype == NL_I64;
    if (int rc = stage_upload(*h, &f.d, &f.cap, labels, h->n, dtype_size(dtype), err, errlen)) return rc;
    NL_HIP(hipStreamSynchronize(h->stream));            // the host array may go away after the call
    f.loaded = true;
    std::swap(h->fr[0], h->fr[1]);
    return NL_OK;
}

// Begins a pair: a table of `slots` slots (a power of two, at least 2), every slot free; the words and the times of the pair reset.
extern "C" int nl_trans_begin(nl_trans *h, int64_t slots, char *err, size_t errlen) {
    STAGE_ENTER(h, "transitions object");
    if (slots < 2 || slots > TR_MAX_SLOTS || (slots & (slots - 1))) return nl_fail(err, errlen, NL_EINVAL, "table_slots must be a power of two from 2 to 2^34, got %lld", (long long)slots);
    if (!h->fr[0].loaded || !h->fr[1].loaded) return nl_fail(err, errlen, NL_ESTATE, "nl_trans_begin needs two label frames (nl_trans_frame)");
    h->counting = false;
    h->entries = -1;
    h->ms[TR_MS_CLEAR] = h->ms[TR_MS_COUNT] = h->ms[TR_MS_COMPACT] = 0.f;
    if (int rc = stage_grow(&h->table_cap, slots, slots, {{&h->d_table, 16}}, err, errlen)) return rc;
    const i64 words = ((slots + 255) / 256) * 4;
    if (int rc = stage_grow(&h->word_cap, words, words, {{&h->d_bits, 8}, {&h->d_wcount, 4}, {&h->d_pre, 4}}, err, errlen)) return rc;
    const i64 sums = rank_scan_sums(h->word_cap);
    if (int rc = stage_grow(&h->sum_cap, sums, sums, {{&h->scan.d_bsum, 8}}, err, errlen)) return rc;
    h->slots = slots;
    if (int rc = stage_start(*h, err, errlen)) return rc;
    tr_clear_kernel<<<grid1d(slots), 256, 0, h->stream>>>(h->d_table, slots, h->d_words);
    NL_CHECK_LAUNCH();
    if (int rc = stage_stop(*h, &h->ms[TR_MS_CLEAR], err, errlen)) return rc;
    h->counting = true;
    h->overflowed = false;
    return NL_OK;
}

template <typename Coord>
static void tr_launch_count(nl_trans *h, i64 n, i64 row0, int D) {
    const Coord *prev = (const Coord *)h->d_coord, *next = prev + n * D;
    tr_gather_count_kernel<Coord><<<grid1d(n, 256, 4096), 256, 0, h->stream>>>(prev, next, n, row0, D, h->nz, h->ny, h->nx, TrLabels{h->fr[0].d, h->fr[0].wide},
                                                                              TrLabels{h->fr[1].d, h->fr[1].wide}, h->d_table, (u64)(h->slots - 1), h->d_words);
}

// Counts the rows row0 .. row0 + n of the pair: prev and next are (n, ndim) coordinates of NL_U16, NL_U32 or NL_U64, in frame t
// and frame t + 1.  A coordinate outside the frame is NL_EINVAL naming the lowest such row (chunks come in ascending order); the pair
// is then over.  *overflow: a probe sequence ran through the whole table -- what follows of this pair need not be sent.
extern "C" int nl_trans_count(nl_trans *h, const void *prev, const void *next, int coord_dtype, int64_t n, int64_t row0, int *overflow, char *err,
                              size_t errlen) {
    STAGE_ENTER(h, "transitions object");
    if (!overflow || n < 0 || row0 < 0 || (n > 0 && (!prev || !next))) return nl_fail(err, errlen, NL_EINVAL, "NULL coordinates or overflow, or a negative row count");
    if (coord_dtype != NL_U16 && coord_dtype != NL_U32 && coord_dtype != NL_U64) return nl_fail(err, errlen, NL_EINVAL, "coordinates must be uint16, uint32 or uint64");
    if (n > TR_MAX_ROWS) return nl_fail(err, errlen, NL_EINVAL, "more than %lld rows in one launch", (long long)TR_MAX_ROWS);
    if (!h->counting) return nl_fail(err, errlen, NL_ESTATE, "nl_trans_count needs nl_trans_begin");
    *overflow = h->overflowed ? 1 : 0;
    if (n == 0) return NL_OK;
    const int D = h->ndim;
    const i64 half = n * D * (i64)dtype_size(coord_dtype);
    if (int rc = stage_grow(&h->coord_cap, 2 * half, 2 * half, {{&h->d_coord, 1}}, err, errlen)) return rc;
    NL_HIP(hipMemcpyAsync(h->d_coord, prev, (size_t)half, hipMemcpyHostToDevice, h->stream));
    NL_HIP(hipMemcpyAsync((char *)h->d_coord + half, next, (size_t)half, hipMemcpyHostToDevice, h->stream));
    if (int rc = stage_start(*h, err, errlen)) return rc;
    if (coord_dtype == NL_U16) tr_launch_count<unsigned short>(h, n, row0, D);
    else if (coord_dtype == NL_U32) tr_launch_count<unsigned int>(h, n, row0, D);
    else tr_launch_count<u64>(h, n, row0, D);
    NL_CHECK_LAUNCH();
    if (int rc = stage_stop_record(*h, err, errlen)) return rc;
    NL_HIP(hipMemcpyAsync(h->h_words, h->d_words, TR_WORDS * 8, hipMemcpyDeviceToHost, h->stream));
    if (int rc = stage_stop_wait(*h, &h->ms[TR_MS_COUNT], err, errlen)) return rc;      // synchronises: the host arrays may go away
    const i64 bad = h->h_words[TR_W_BAD_COORD];
    if (bad != TR_NO_ROW) {
        h->counting = false;
        return nl_fail(err, errlen, NL_EINVAL, "row %lld holds a coordinate outside the frame (%lld, %lld, %lld)", (long long)bad, (long long)h->nz, (long long)h->ny,
                       (long long)h->nx);
    }
    h->overflowed = h->h_words[TR_W_OVERFLOW] != 0;
    *overflow = h->overflowed ? 1 : 0;
    return NL_OK;
}

// Ends the pair.  A gathered label below 0 or above 2^31 - 1 is NL_EINVAL naming the lowest such row.  *overflow != 0: the table was
// too small, nothing else is valid and the pair is to be repeated with more slots.  Else the occupied slots are compacted:
// *n_entries distinct (prev label, next label) keys, *n_dropped rows with a label of 0 at either end, *n_heads runs that touched the table.
extern "C" int nl_trans_finish(nl_trans *h, int64_t *n_entries, int64_t *n_dropped, int64_t *n_heads, int *overflow, char *err, size_t errlen) {
    STAGE_ENTER(h, "transitions object");
    if (!n_entries || !n_dropped || !n_heads || !overflow) return nl_fail(err, errlen, NL_EINVAL, "an output pointer is NULL");
    if (!h->counting) return nl_fail(err, errlen, NL_ESTATE, "nl_trans_finish needs nl_trans_begin");
    h->counting = false;
    *n_entries = *n_dropped = *n_heads = 0;
    hipStream_t st = h->stream;
    NL_HIP(hipMemcpyAsync(h->h_words, h->d_words, TR_WORDS * 8, hipMemcpyDeviceToHost, st));
    NL_HIP(hipStreamSynchronize(st));
    const i64 bad = h->h_words[TR_W_BAD_LABEL];
    if (bad != TR_NO_ROW) return nl_fail(err, errlen, NL_EINVAL, "row %lld gathers a label outside [0, 2^31 - 1]", (long long)bad);
    *overflow = h->h_words[TR_W_OVERFLOW] != 0;
    if (*overflow) return NL_OK;
    *n_dropped = h->h_words[TR_W_DROPPED];
    *n_heads = h->h_words[TR_W_HEADS];
    const i64 words = ((h->slots + 255) / 256) * 4;
    const unsigned gv = (unsigned)((h->slots + 255) / 256);
    i64 m = 0;
    if (int rc = stage_start(*h, err, errlen)) return rc;
    rank_mask_kernel<<<gv, 256, 0, st>>>(TrOccupied{h->d_table}, h->slots, h->d_bits, h->d_wcount);
    NL_CHECK_LAUNCH();
    if (int rc = rank_scan(h->scan, st, h->d_wcount, words, h->d_pre, TR_MAX_ENTRIES, "distinct label pairs in one frame pair", &m, err, errlen)) return rc;
    if (int rc = stage_grow(&h->entry_cap, m, stage_doubled(h->entry_cap, m), {{&h->d_entries, 16}}, err, errlen)) return rc;
    if (m > 0) {
        tr_entries_write_kernel<<<gv, 256, 0, st>>>(h->d_table, h->slots, h->d_pre, h->d_entries);
        NL_CHECK_LAUNCH();
    }
    if (int rc = stage_stop(*h, &h->ms[TR_MS_COMPACT], err, errlen)) return rc;
    h->entries = m;
    *n_entries = m;
    return NL_OK;
}

// The entries of the finished pair: out (n_entries, 2) uint64 rows (key = prev label << 32 | next label, count), in slot order.
extern "C" int nl_trans_fetch(nl_trans *h, uint64_t *out, char *err, size_t errlen) {
    STAGE_ENTER(h, "transitions object");
    if (h->entries < 0) return nl_fail(err, errlen, NL_ESTATE, "nl_trans_fetch needs nl_trans_finish");
    if (h->entries > 0) {
        if (!out) return nl_fail(err, errlen, NL_EINVAL, "out is NULL");
        NL_HIP(hipMemcpyAsync(out, h->d_entries, (size_t)h->entries * 16, hipMemcpyDeviceToHost, h->stream));
        NL_HIP(hipStreamSynchronize(h->stream));
    }
    return NL_OK;
}

// The largest label of the "next" frame (computed on the device once per frame).
extern "C" int nl_trans_label_max(nl_trans *h, int64_t *top, char *err, size_t errlen) {
    STAGE_ENTER(h, "transitions object");
    if (!top) return nl_fail(err, errlen, NL_EINVAL, "top is NULL");
    TrFrame &f = h->fr[1];
    if (!f.loaded) return nl_fail(err, errlen, NL_ESTATE, "nl_trans_label_max needs a label frame (nl_trans_frame)");
    if (!f.has_top) {
        hipStream_t st = h->stream;
        i64 *d_top = h->d_words + TR_WORDS, *h_top = h->h_words + TR_WORDS;
        *h_top = -TR_NO_ROW - 1;
        NL_HIP(hipMemcpyAsync(d_top, h_top, 8, hipMemcpyHostToDevice, st));
        tr_label_max_kernel<<<grid1d(h->n, 256, 2048), 256, 0, st>>>(TrLabels{f.d, f.wide}, h->n, d_top);
        NL_CHECK_LAUNCH();
        NL_HIP(hipMemcpyAsync(h_top, d_top, 8, hipMemcpyDeviceToHost, st));
        NL_HIP(hipStreamSynchronize(st));
        f.top = *h_top;
        f.has_top = true;
    }
    *top = f.top;
    return NL_OK;
}

// The "next" frame through lut (n_lut int32 entries): a voxel of label b in (0, n_lut) becomes lut[b], every other voxel 0.
extern "C" int nl_trans_relabel(nl_trans *h, const int32_t *lut, int64_t n_lut, char *err, size_t errlen) {
    STAGE_ENTER(h, "transitions object");
    if (n_lut < 0 || n_lut > TR_MAX_LABEL + 1 || (n_lut > 0 && !lut)) return nl_fail(err, errlen, NL_EINVAL, "lut is NULL or its length is outside [0, 2^31]");
    const TrFrame &f = h->fr[1];
    if (!f.loaded) return nl_fail(err, errlen, NL_ESTATE, "nl_trans_relabel needs a label frame (nl_trans_frame)");
    h->relabelled = false;
    h->ms[TR_MS_RELABEL] = 0.f;
    hipStream_t st = h->stream;
    if (int rc = stage_grow(&h->out_cap, h->n, h->n, {{&h->d_out, 4}}, err, errlen)) return rc;
    if (int rc = stage_grow(&h->lut_cap, n_lut, stage_doubled(h->lut_cap, n_lut), {{&h->d_lut, 4}}, err, errlen)) return rc;
    if (n_lut > 0) NL_HIP(hipMemcpyAsync(h->d_lut, lut, (size_t)n_lut * 4, hipMemcpyHostToDevice, st));
    if (int rc = stage_start(*h, err, errlen)) return rc;
    const unsigned grid = grid1d((h->n + 3) / 4, 256, 8192);
    if (f.wide) tr_relabel_kernel<true><<<grid, 256, 0, st>>>(f.d, h->n, h->d_lut, n_lut, h->d_out);
    else tr_relabel_kernel<false><<<grid, 256, 0, st>>>(f.d, h->n, h->d_lut, n_lut, h->d_out);
    NL_CHECK_LAUNCH();
    if (int rc = stage_stop(*h, &h->ms[TR_MS_RELABEL], err, errlen)) return rc;         // synchronises: the host array may go away
    h->relabelled = true;
    return NL_OK;
}

// The relabelled frame, int32, the handle's shape.
extern "C" int nl_trans_fetch_frame(nl_trans *h, int32_t *frame, char *err, size_t errlen) {
    STAGE_ENTER(h, "transitions object");
    if (!h->relabelled) return nl_fail(err, errlen, NL_ESTATE, "nl_trans_fetch_frame needs nl_trans_relabel");
    if (!frame) return nl_fail(err, errlen, NL_EINVAL, "frame is NULL");
    NL_HIP(hipMemcpyAsync(frame, h->d_out, (size_t)h->n * 4, hipMemcpyDeviceToHost, h->stream));
    NL_HIP(hipStreamSynchronize(h->stream));
    return NL_OK;
}

// Device time (ms) of the kernels: ms[0] the table's clear, [1] the gather-and-count launches and [2] the compaction of the last
// pair, [3] the last nl_trans_relabel.  Transfers excluded, but for one: the compaction's scan brings its total to the host between
// its kernels (rank_scan), and that round trip of one word lies inside ms[2].
extern "C" int nl_trans_kernel_ms(nl_trans *h, float *ms, char *err, size_t errlen) {
    if (!h || !ms) return nl_fail(err, errlen, NL_EINVAL, "transitions object or ms is NULL");
    for (int j = 0; j < TR_MS_PARTS; ++j) ms[j] = h->ms[j];
    return NL_OK;
}
