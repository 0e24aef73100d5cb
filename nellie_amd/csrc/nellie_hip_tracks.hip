// Translation unit of libnellie_hip.so (gfx950): voxel tracks of a label stack (nellie/tracking/all_tracks_for_label.py).  C-ABI in
// include/nellie_amd.h; kernels in tracks.inc.  A track set owns its buffers and stream: the 1-bit masks of the frames the caller
// keeps resident, the seeds, the coordinates on their way through the stack and the rows they leave.  The flow vectors come from a
// flow field (nellie_hip_flow.hip) through nl_flow_interpolate_dev, device to device; the surviving rows come down once.
#include "nl_stage.h"
#include "tracks.inc"

#define TK_MAX_SEEDS ((i64)1 << 30)         // set voxels per frame: ranks are ints
#define TK_MAX_ROWS ((i64)0x7fffffff)       // rows of one run: positions are ints
#define TK_MAX_ID 4503599627370496.0        // 2^52: ids are exact in the float64 rows
#define TK_MS_PARTS 6                       // mask, seed, flow, step, filter, compact

struct TkStep {                       // a step that emitted rows [begin, end)
    i64 begin, end;
    int backward, first, ord;         // ord: the rows each of its tracks had emitted before it
    i64 frame_from, frame_to;
};

struct nl_tracks : StageBase {
    int ndim = 3, slots = 0;
    TkGeom g{};
    i64 words = 0;                    // mask words per frame (a multiple of 4: one workgroup of rank_mask_kernel writes 4)
    u64 *d_masks = nullptr;           // slots x words
    std::vector<char> slot_valid;
    int *d_frame = nullptr;           // the label frame being uploaded
    u64 *d_sel = nullptr;             // the seed predicate's mask when it is not a frame mask (label == label_num)
    int *d_wcount = nullptr, *d_wpre = nullptr;
    RankScan scan; i64 scan_cap = 0;
    // a run
    i64 n = 0, seed_cap = 0;          // seeds
    double *d_seed = nullptr;
    double *d_cur = nullptr, *d_vec = nullptr, *d_old = nullptr; int *d_per_id = nullptr, *d_start = nullptr; i64 coord_cap = 0;
    u64 *d_keep = nullptr; int *d_kcount = nullptr, *d_kpre = nullptr; i64 kw_cap = 0;
    double *d_rows = nullptr, *d_out = nullptr; int *d_src = nullptr, *d_flag = nullptr, *d_pre = nullptr; i64 row_cap = 0;
    i64 run_cap = 0, n_rows = 0, n_back = 0, n_out = 0;
    double id0 = 0.0;
    int dir_ord = 0;
    bool begun = false, forward_seen = false, ordered = false, finished = false;
    std::vector<TkStep> steps;
    float ms[TK_MS_PARTS] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
};

extern "C" int nl_tracks_destroy(nl_tracks *h) {
    if (!h) return NL_OK;
    stage_close(*h, {h->d_masks, h->d_frame, h->d_sel, h->d_wcount, h->d_wpre, h->scan.d_bsum, h->scan.d_total, h->d_seed, h->d_cur, h->d_vec,
                     h->d_old, h->d_per_id, h->d_start, h->d_keep, h->d_kcount, h->d_kpre, h->d_rows, h->d_out, h->d_src, h->d_flag, h->d_pre},
                {h->scan.h_total});
    delete h;
    return NL_OK;
}

// the workgroup sums of the scans hold a scan of m counts afterwards
static int tk_scan_reserve(nl_tracks *h, i64 m, char *err, size_t errlen) {
    const i64 need = rank_scan_sums(m);
    return stage_grow(&h->scan_cap, need, need, {{&h->scan.d_bsum, 8}}, err, errlen);
}

extern "C" int nl_tracks_create(nl_tracks **out, int device, int ndim, int64_t nz, int64_t ny, int64_t nx, int mask_slots, char *err, size_t errlen) {
    if (!out) return nl_fail(err, errlen, NL_EINVAL, "out is NULL");
    *out = nullptr;
    const double unit[3] = {1.0, 1.0, 1.0};
    if (int rc = stage_check_frame(ndim, unit, nz, ny, nx, err, errlen)) return rc;
    if (mask_slots < 1 || mask_slots > (1 << 20)) return nl_fail(err, errlen, NL_EINVAL, "mask_slots must be 1 .. 2^20");
    if (int rc = stage_check_device(device, err, errlen)) return rc;
    nl_tracks *h = new nl_tracks();
    h->ndim = ndim;
    h->slots = mask_slots;
    h->slot_valid.assign((size_t)mask_slots, 0);
    h->g.nz = nz; h->g.ny = ny; h->g.nx = nx; h->g.n = nz * ny * nx;
    h->words = ((h->g.n + 255) / 256) * 4;
    if (int rc = stage_open(*h, device, true, err, errlen)) { nl_tracks_destroy(h); return rc; }
    STAGE_HIP(stage_alloc(&h->d_masks, h->words * (i64)mask_slots, 8), nl_tracks_destroy(h));
    STAGE_HIP(stage_alloc(&h->d_frame, h->g.n, 4), nl_tracks_destroy(h));
    STAGE_HIP(stage_alloc(&h->d_sel, h->words, 8), nl_tracks_destroy(h));
    STAGE_HIP(stage_alloc(&h->d_wcount, h->words, 4), nl_tracks_destroy(h));
    STAGE_HIP(stage_alloc(&h->d_wpre, h->words, 4), nl_tracks_destroy(h));
    STAGE_HIP(stage_alloc(&h->scan.d_total, 1, 8), nl_tracks_destroy(h));
    STAGE_HIP(hipHostMalloc((void **)&h->scan.h_total, 8, hipHostMallocDefault), nl_tracks_destroy(h));
    if (int rc = tk_scan_reserve(h, h->words, err, errlen)) { nl_tracks_destroy(h); return rc; }
    *out = h;
    return NL_OK;
}

// uploads a label frame and writes its labels > 0 mask into `slot` (d_wcount holds the word counts afterwards)
static int tk_build_mask(nl_tracks *h, int slot, const int32_t *labels, char *err, size_t errlen) {
    hipStream_t st = h->stream;
    h->slot_valid[(size_t)slot] = 0;
    NL_HIP(hipMemcpyAsync(h->d_frame, labels, (size_t)h->g.n * 4, hipMemcpyHostToDevice, st));
    if (int rc = stage_start(*h, err, errlen)) return rc;
    rank_mask_kernel<<<(unsigned)((h->g.n + 255) / 256), 256, 0, st>>>(TkLabelled{h->d_frame}, h->g.n, h->d_masks + (i64)slot * h->words, h->d_wcount);
    NL_CHECK_LAUNCH();
    if (int rc = stage_stop(*h, &h->ms[0], err, errlen)) return rc;      // synchronises: the host array may go away after the call
    h->slot_valid[(size_t)slot] = 1;
    return NL_OK;
}

#define TK_CHECK_SLOT(slot) \
    if ((slot) < 0 || (slot) >= h->slots) return nl_fail(err, errlen, NL_EINVAL, "mask slot %d is not in 0 .. %d", (int)(slot), h->slots - 1);

// The labels > 0 mask of a frame (int32, the frame's shape) into `slot`, replacing what the slot held.
extern "C" int nl_tracks_mask(nl_tracks *h, int slot, const int32_t *labels, char *err, size_t errlen) {
    STAGE_ENTER(h, "track set");
    TK_CHECK_SLOT(slot);
    if (!labels) return nl_fail(err, errlen, NL_EINVAL, "labels is NULL");
    return tk_build_mask(h, slot, labels, err, errlen);
}

// The seeds of a run: every skip-th voxel, in raster order, of the start frame's mask in `slot` (use_label = 0) or of
// labels == label (use_label != 0).  labels != NULL: the start frame, uploaded for this call; it also (re)builds the slot's mask.
extern "C" int nl_tracks_seed(nl_tracks *h, int slot, const int32_t *labels, int use_label, int32_t label, int skip, int64_t *n_seeds,
                              char *err, size_t errlen) {
    STAGE_ENTER(h, "track set");
    TK_CHECK_SLOT(slot);
    if (!n_seeds) return nl_fail(err, errlen, NL_EINVAL, "n_seeds is NULL");
    if (skip < 1) return nl_fail(err, errlen, NL_EINVAL, "skip must be at least 1");
    if (use_label && !labels) return nl_fail(err, errlen, NL_EINVAL, "seeding by label needs the start frame");
    *n_seeds = 0;
    h->n = 0;
    h->begun = false;
    for (float &m : h->ms) m = 0.f;
    hipStream_t st = h->stream;
    if (labels) {
        if (int rc = tk_build_mask(h, slot, labels, err, errlen)) return rc;
    } else if (!h->slot_valid[(size_t)slot]) {
        return nl_fail(err, errlen, NL_ESTATE, "mask slot %d holds no frame", slot);
    }
    const u64 *bits = h->d_masks + (i64)slot * h->words;
    if (int rc = stage_start(*h, err, errlen)) return rc;
    if (use_label) {
        rank_mask_kernel<<<(unsigned)((h->g.n + 255) / 256), 256, 0, st>>>(TkIsLabel{h->d_frame, (int)label}, h->g.n, h->d_sel, h->d_wcount);
        NL_CHECK_LAUNCH();
        bits = h->d_sel;
    } else if (!labels) {
        tk_popcount_kernel<<<(unsigned)((h->words + 255) / 256), 256, 0, st>>>(bits, h->words, h->d_wcount);
        NL_CHECK_LAUNCH();
    }
    i64 total = 0;
    if (int rc = rank_scan(h->scan, st, h->d_wcount, h->words, h->d_wpre, TK_MAX_SEEDS, "seed voxels in one frame", &total, err, errlen)) return rc;
    const i64 n = (total + skip - 1) / skip;
    if (int rc = stage_grow(&h->seed_cap, n, n, {{&h->d_seed, (size_t)h->ndim * 8}}, err, errlen)) return rc;
    if (n > 0) {
        const unsigned gv = (unsigned)((h->g.n + 255) / 256);
        if (h->ndim == 3) tk_seed_kernel<3><<<gv, 256, 0, st>>>(bits, h->d_wpre, h->g, skip, h->d_seed);
        else tk_seed_kernel<2><<<gv, 256, 0, st>>>(bits, h->d_wpre, h->g, skip, h->d_seed);
        NL_CHECK_LAUNCH();
    }
    if (int rc = stage_stop(*h, &h->ms[1], err, errlen)) return rc;
    h->n = n;
    *n_seeds = n;
    return NL_OK;
}

// Sizes the buffers of a run before any of its work: n * (steps + 1) rows per direction (0 steps: the direction does not run).
// Ids are id0 + the seed's index.  What does not fit is NL_ENOMEM.
extern "C" int nl_tracks_begin(nl_tracks *h, int64_t fw_steps, int64_t bw_steps, int64_t id0, char *err, size_t errlen) {
    STAGE_ENTER(h, "track set");
    if (fw_steps < 0 || bw_steps < 0) return nl_fail(err, errlen, NL_EINVAL, "negative step count");
    if (h->n <= 0) return nl_fail(err, errlen, NL_ESTATE, "nl_tracks_begin needs seeds");
    if (!((double)id0 > -TK_MAX_ID && (double)id0 + (double)h->n < TK_MAX_ID)) return nl_fail(err, errlen, NL_EINVAL, "track ids beyond 2^52");
    h->begun = false;
    const double rows = (double)h->n * ((fw_steps ? (double)fw_steps + 1.0 : 0.0) + (bw_steps ? (double)bw_steps + 1.0 : 0.0));
    if (rows > (double)TK_MAX_ROWS)
        return nl_fail(err, errlen, NL_ENOMEM, "%lld seeds over %lld + %lld steps are more than %lld track rows [out of memory]", (long long)h->n,
                       (long long)fw_steps, (long long)bw_steps, (long long)TK_MAX_ROWS);
    const i64 cap = (i64)rows, n = h->n, W = 2 + h->ndim, kw = ((n + 255) / 256) * 4;
    const size_t D8 = (size_t)h->ndim * 8;
    if (int rc = stage_grow(&h->coord_cap, n, n, {{&h->d_cur, D8}, {&h->d_vec, D8}, {&h->d_old, D8}, {&h->d_per_id, 4}, {&h->d_start, 4}}, err, errlen)) return rc;
    if (int rc = stage_grow(&h->kw_cap, kw, kw, {{&h->d_keep, 8}, {&h->d_kcount, 4}, {&h->d_kpre, 4}}, err, errlen)) return rc;
    if (int rc = stage_grow(&h->row_cap, cap, cap, {{&h->d_rows, (size_t)W * 8}, {&h->d_out, (size_t)W * 8}, {&h->d_src, 4}, {&h->d_flag, 4}, {&h->d_pre, 4}},
                            err, errlen)) return rc;
    i64 longest = cap > n ? cap : n;
    if (h->words > longest) longest = h->words;
    if (kw > longest) longest = kw;
    if (int rc = tk_scan_reserve(h, longest, err, errlen)) return rc;
    h->run_cap = cap;
    h->n_rows = h->n_back = h->n_out = 0;
    h->id0 = (double)id0;
    h->dir_ord = 0;
    h->forward_seen = h->ordered = h->finished = false;
    h->steps.clear();
    for (int j = 2; j < TK_MS_PARTS; ++j) h->ms[j] = 0.f;
    h->begun = true;
    return NL_OK;
}

// One frame of one direction.  first != 0: the direction's first frame -- the coordinates start from the seeds, and a kept
// coordinate emits its start row [id, frame_from, coord] before its new one.  flow: the field with the direction's rows of
// frame_from loaded, NULL when it has none.  Nothing changes and nothing is emitted (n_rows = 0) when no coordinate finds a row.
// The backward steps of a run come before its forward steps.
extern "C" int nl_tracks_step(nl_tracks *h, nl_flow *flow, int backward, int first, int64_t frame_from, int64_t frame_to, int64_t *n_rows,
                              char *err, size_t errlen) {
    STAGE_ENTER(h, "track set");
    if (!n_rows) return nl_fail(err, errlen, NL_EINVAL, "n_rows is NULL");
    *n_rows = 0;
    if (!h->begun || h->ordered) return nl_fail(err, errlen, NL_ESTATE, "nl_tracks_step needs nl_tracks_begin, and comes before nl_tracks_filter");
    if (backward && h->forward_seen) return nl_fail(err, errlen, NL_ESTATE, "the backward steps come before the forward steps");
    if (!backward) h->forward_seen = true;
    hipStream_t st = h->stream;
    const i64 n = h->n;
    const int D = h->ndim;
    if (first) {
        NL_HIP(hipMemcpyAsync(h->d_cur, h->d_seed, (size_t)n * D * 8, hipMemcpyDeviceToDevice, st));
        if (backward) NL_HIP(hipMemsetAsync(h->d_per_id, 0, (size_t)n * 4, st));
        h->dir_ord = 0;
    }
    if (!flow) return NL_OK;
    NL_HIP(hipStreamSynchronize(st));                   // the coordinates are complete before the field reads them
    int64_t found = 0;
    if (int rc = nl_flow_interpolate_dev(flow, h->d_cur, n, h->d_vec, &found, err, errlen)) return rc;
    float ms = 0.f;
    if (int rc = nl_flow_kernel_ms(flow, &ms, err, errlen)) return rc;
    h->ms[2] += ms;
    NL_HIP(hipSetDevice(h->device));
    if (found == 0) return NL_OK;
    const unsigned gn = (unsigned)((n + 255) / 256);
    const i64 kw = (i64)gn * 4;
    const double sign = backward ? -1.0 : 1.0;
    int *per_id = backward ? h->d_per_id : nullptr;
    if (int rc = stage_start(*h, err, errlen)) return rc;
    if (D == 3) tk_update_kernel<3><<<gn, 256, 0, st>>>(h->d_cur, h->d_vec, n, sign, first ? 1 : 0, h->d_old, per_id, h->d_keep, h->d_kcount);
    else tk_update_kernel<2><<<gn, 256, 0, st>>>(h->d_cur, h->d_vec, n, sign, first ? 1 : 0, h->d_old, per_id, h->d_keep, h->d_kcount);
    NL_CHECK_LAUNCH();
    i64 kept = 0;
    if (int rc = rank_scan(h->scan, st, h->d_kcount, kw, h->d_kpre, TK_MAX_SEEDS, "kept coordinates", &kept, err, errlen)) return rc;
    const i64 rows = first ? 2 * kept : kept;
    if (h->n_rows + rows > h->run_cap) return nl_fail(err, errlen, NL_ESTATE, "more steps than nl_tracks_begin was told");
    if (rows > 0) {
        const double ff = (double)frame_from, ft = (double)frame_to;
        if (D == 3) tk_emit_kernel<3><<<gn, 256, 0, st>>>(h->d_cur, h->d_old, n, h->d_keep, h->d_kpre, h->n_rows, first ? 1 : 0, h->id0, ff, ft, h->d_rows);
        else tk_emit_kernel<2><<<gn, 256, 0, st>>>(h->d_cur, h->d_old, n, h->d_keep, h->d_kpre, h->n_rows, first ? 1 : 0, h->id0, ff, ft, h->d_rows);
        NL_CHECK_LAUNCH();
    }
    if (int rc = stage_stop(*h, &h->ms[3], err, errlen)) return rc;
    if (rows > 0) {
        h->steps.push_back(TkStep{h->n_rows, h->n_rows + rows, backward ? 1 : 0, first ? 1 : 0, h->dir_ord, frame_from, frame_to});
        h->n_rows += rows;
        if (backward) h->n_back = h->n_rows;
    }
    h->dir_ord += first ? 2 : 1;
    *n_rows = rows;
    return NL_OK;
}

// The final filter for the rows of one frame, in every step that emitted some: slot holds the frame's mask, slot < 0: the frame
// lies outside the stack and its rows go.  Also gives each of those rows its place in the defined order.  Called once for every
// frame that has rows, after the last step.
extern "C" int nl_tracks_filter(nl_tracks *h, int64_t frame, int slot, char *err, size_t errlen) {
    STAGE_ENTER(h, "track set");
    if (!h->begun || h->finished) return nl_fail(err, errlen, NL_ESTATE, "nl_tracks_filter comes between the steps and nl_tracks_finish");
    if (slot >= h->slots) return nl_fail(err, errlen, NL_EINVAL, "mask slot %d is not in 0 .. %d", slot, h->slots - 1);
    if (slot >= 0 && !h->slot_valid[(size_t)slot]) return nl_fail(err, errlen, NL_ESTATE, "mask slot %d holds no frame", slot);
    hipStream_t st = h->stream;
    if (int rc = stage_start(*h, err, errlen)) return rc;
    if (!h->ordered) {
        if (h->n_back > 0) {
            i64 total = 0;
            if (int rc = rank_scan(h->scan, st, h->d_per_id, h->n, h->d_start, TK_MAX_ROWS, "backward rows", &total, err, errlen)) return rc;
            if (total != h->n_back) return nl_fail(err, errlen, NL_ESTATE, "the backward rows and their counts per id disagree");
        }
        h->ordered = true;
    }
    const u64 *bits = slot >= 0 ? h->d_masks + (i64)slot * h->words : nullptr;
    for (const TkStep &s : h->steps) {
        if (s.frame_to != frame && !(s.first && s.frame_from == frame)) continue;
        const unsigned gr = (unsigned)((s.end - s.begin + 255) / 256);
        if (h->ndim == 3)
            tk_filter_kernel<3><<<gr, 256, 0, st>>>(h->d_rows, s.begin, s.end, (double)frame, h->g, bits, s.backward, s.first, s.ord, h->id0, h->d_start,
                                                    h->d_per_id, h->d_src, h->d_flag);
        else
            tk_filter_kernel<2><<<gr, 256, 0, st>>>(h->d_rows, s.begin, s.end, (double)frame, h->g, bits, s.backward, s.first, s.ord, h->id0, h->d_start,
                                                    h->d_per_id, h->d_src, h->d_flag);
        NL_CHECK_LAUNCH();
    }
    return stage_stop(*h, &h->ms[4], err, errlen);
}

// One scan over the flags of all rows and one compaction.  n_rows = the rows that stay.
extern "C" int nl_tracks_finish(nl_tracks *h, int64_t *n_rows, char *err, size_t errlen) {
    STAGE_ENTER(h, "track set");
    if (!n_rows) return nl_fail(err, errlen, NL_EINVAL, "n_rows is NULL");
    *n_rows = 0;
    if (!h->begun || h->finished) return nl_fail(err, errlen, NL_ESTATE, "nl_tracks_finish needs nl_tracks_begin, once");
    if (h->n_rows > 0 && !h->ordered) return nl_fail(err, errlen, NL_ESTATE, "nl_tracks_finish needs nl_tracks_filter for every frame with rows");
    hipStream_t st = h->stream;
    i64 total = 0;
    if (h->n_rows > 0) {
        if (int rc = stage_start(*h, err, errlen)) return rc;
        if (int rc = rank_scan(h->scan, st, h->d_flag, h->n_rows, h->d_pre, TK_MAX_ROWS, "track rows", &total, err, errlen)) return rc;
        if (total > 0) {
            const unsigned gr = (unsigned)((h->n_rows + 255) / 256);
            if (h->ndim == 3) tk_compact_kernel<3><<<gr, 256, 0, st>>>(h->d_rows, h->n_rows, h->d_src, h->d_flag, h->d_pre, h->d_out);
            else tk_compact_kernel<2><<<gr, 256, 0, st>>>(h->d_rows, h->n_rows, h->d_src, h->d_flag, h->d_pre, h->d_out);
            NL_CHECK_LAUNCH();
        }
        if (int rc = stage_stop(*h, &h->ms[5], err, errlen)) return rc;
    }
    h->n_out = total;
    h->finished = true;
    *n_rows = total;
    return NL_OK;
}

// The rows that stayed, (n_rows, 2 + ndim) float64: [id, frame, (z,) y, x], in the defined order.
extern "C" int nl_tracks_fetch(nl_tracks *h, double *rows, char *err, size_t errlen) {
    STAGE_ENTER(h, "track set");
    if (!h->finished) return nl_fail(err, errlen, NL_ESTATE, "nl_tracks_fetch needs nl_tracks_finish");
    if (h->n_out > 0) {
        if (!rows) return nl_fail(err, errlen, NL_EINVAL, "rows is NULL");
        NL_HIP(hipMemcpyAsync(rows, h->d_out, (size_t)h->n_out * (2 + h->ndim) * 8, hipMemcpyDeviceToHost, h->stream));
        NL_HIP(hipStreamSynchronize(h->stream));
    }
    return NL_OK;
}

// Device time (ms) of the kernels since the last nl_tracks_seed, per part: ms[0] frame masks, [1] seeding, [2] flow
// interpolation, [3] steps, [4] filter and order, [5] scan and compaction.  Transfers excluded.
extern "C" int nl_tracks_kernel_ms(nl_tracks *h, float *ms, char *err, size_t errlen) {
    if (!h || !ms) return nl_fail(err, errlen, NL_EINVAL, "track set or ms is NULL");
    for (int j = 0; j < TK_MS_PARTS; ++j) ms[j] = h->ms[j];
    return NL_OK;
}
