// Translation unit of libnellie_hip.so (gfx950): voxel reassignment (nellie/tracking/voxel_reassignment.py).  C-ABI in
// include/nellie_amd.h; kernels in reassign.inc.  A reassigner owns its buffers and stream and keeps the last two frames on the
// device; the flow vectors come from two flow fields (nellie_hip_flow.hip) through nl_flow_interpolate_dev, device to device.
#include <algorithm>
#include <math.h>
#include "nl_stage.h"
#include "reassign.inc"

#define RA_MAX_OFFSETS ((i64)1 << 22)
#define RA_MAX_ROWS ((i64)1 << 30)          // labelled voxels per frame: ranks, candidate ids and their sums are ints

struct RaSlot {                       // one frame
    i64 n = 0, cap = 0;               // labelled voxels
    u64 *bits = nullptr;
    int *pre = nullptr;
    i64 *vox = nullptr;
    int *lab_b = nullptr, *lab_o = nullptr, *re_b = nullptr, *re_o = nullptr;
};

struct nl_reassign : StageBase {
    int ndim = 3;
    RaGeom g{};
    double r = 0.5, half_diag = 0.0;
    i64 words = 0;                    // mask words per frame (a multiple of 4: one workgroup of rank_mask_kernel writes 4)
    RaOffset *d_table = nullptr; int ntab = 0;
    int *d_branch = nullptr, *d_obj = nullptr;       // the frame being loaded
    int *d_wcount = nullptr;
    RankScan scan;
    RaSlot slot[2]; int cur = 0, frames = 0;
    // temporaries of a pair
    double *d_q = nullptr, *d_v = nullptr; i64 q_cap = 0;
    int *d_fw_match = nullptr, *d_bw_match = nullptr; float *d_fw_d = nullptr, *d_bw_d = nullptr; i64 fw_cap = 0, bw_cap = 0;
    int *d_cnt = nullptr, *d_start = nullptr, *d_cursor = nullptr, *d_best = nullptr; i64 t_cap = 0;
    int *d_ent = nullptr; i64 ent_cap = 0;
    bool has_best = false;
    float kernel_ms = 0.f;
};

extern "C" int nl_reassign_destroy(nl_reassign *h) {
    if (!h) return NL_OK;
    std::vector<void *> ps = {h->d_table, h->d_branch, h->d_obj, h->d_wcount, h->scan.d_bsum, h->scan.d_total, h->d_q, h->d_v, h->d_fw_match,
                              h->d_bw_match, h->d_fw_d, h->d_bw_d, h->d_cnt, h->d_start, h->d_cursor, h->d_best, h->d_ent};
    for (const RaSlot &s : h->slot) ps.insert(ps.end(), {s.bits, s.pre, s.vox, s.lab_b, s.lab_o, s.re_b, s.re_o});
    stage_close(*h, ps, {h->scan.h_total});
    delete h;
    return NL_OK;
}

// The lattice offsets of scaled length <= reach, by ascending (length, dz, dy, dx).  false: more than RA_MAX_OFFSETS.
static bool ra_offsets(int ndim, const double *s, double reach, std::vector<RaOffset> &out) {
    i64 k[3];
    double count = 1.0;
    for (int a = 0; a < 3; ++a) {
        k[a] = (a == 0 && ndim == 2) ? 0 : (i64)floor(reach / s[a]);
        count *= (double)(2 * k[a] + 1);
    }
    if (count > 8.0 * (double)RA_MAX_OFFSETS) return false;
    for (i64 dz = -k[0]; dz <= k[0]; ++dz)
        for (i64 dy = -k[1]; dy <= k[1]; ++dy)
            for (i64 dx = -k[2]; dx <= k[2]; ++dx) {
                const double ez = (double)dz * s[0], ey = (double)dy * s[1], ex = (double)dx * s[2];
                const double len = sqrt(ez * ez + ey * ey + ex * ex);
                if (len <= reach) out.push_back(RaOffset{(int)dz, (int)dy, (int)dx, 0, len});
            }
    if ((i64)out.size() > RA_MAX_OFFSETS) return false;
    std::sort(out.begin(), out.end(), [](const RaOffset &a, const RaOffset &b) {
        if (a.len != b.len) return a.len < b.len;
        if (a.dz != b.dz) return a.dz < b.dz;
        if (a.dy != b.dy) return a.dy < b.dy;
        return a.dx < b.dx;
    });
    return true;
}

extern "C" int nl_reassign_create(nl_reassign **out, int device, int ndim, int64_t nz, int64_t ny, int64_t nx, const double *spacing, double r,
                                  char *err, size_t errlen) {
    if (!out) return nl_fail(err, errlen, NL_EINVAL, "out is NULL");
    *out = nullptr;
    if (int rc = stage_check_frame(ndim, spacing, nz, ny, nx, err, errlen)) return rc;
    if (int rc = stage_check_positive(r, "the radius", err, errlen)) return rc;
    if (int rc = stage_check_device(device, err, errlen)) return rc;
    double s[3] = {1.0, 1.0, 1.0};
    for (int a = 0; a < ndim; ++a) s[3 - ndim + a] = spacing[a];
    double diag2 = 0.0;
    for (int a = 3 - ndim; a < 3; ++a) diag2 += s[a] * s[a];
    const double diag = sqrt(diag2);
    std::vector<RaOffset> table;
    if (!ra_offsets(ndim, s, r + diag, table))
        return nl_fail(err, errlen, NL_EINVAL, "the radius spans too many voxels (more than %lld lattice offsets)", (long long)RA_MAX_OFFSETS);
    nl_reassign *h = new nl_reassign();
    h->ndim = ndim;
    h->r = r;
    h->half_diag = 0.5 * diag;
    h->g.nz = nz; h->g.ny = ny; h->g.nx = nx; h->g.n = nz * ny * nx;
    for (int a = 0; a < 3; ++a) h->g.s[a] = s[a];
    h->words = ((h->g.n + 255) / 256) * 4;
    h->ntab = (int)table.size();
    if (int rc = stage_open(*h, device, true, err, errlen)) { nl_reassign_destroy(h); return rc; }
    STAGE_HIP(stage_alloc(&h->d_table, (i64)table.size(), sizeof(RaOffset)), nl_reassign_destroy(h));
    STAGE_HIP(hipMemcpy(h->d_table, table.data(), table.size() * sizeof(RaOffset), hipMemcpyHostToDevice), nl_reassign_destroy(h));
    STAGE_HIP(stage_alloc(&h->d_branch, h->g.n, 4), nl_reassign_destroy(h));
    STAGE_HIP(stage_alloc(&h->d_obj, h->g.n, 4), nl_reassign_destroy(h));
    STAGE_HIP(stage_alloc(&h->d_wcount, h->words, 4), nl_reassign_destroy(h));
    // the workgroup sums are sized once for the longest scan a frame of this shape can ask for
    STAGE_HIP(stage_alloc(&h->scan.d_bsum, rank_scan_sums(h->words > h->g.n ? h->words : h->g.n), 8), nl_reassign_destroy(h));
    STAGE_HIP(stage_alloc(&h->scan.d_total, 1, 8), nl_reassign_destroy(h));
    STAGE_HIP(hipHostMalloc((void **)&h->scan.h_total, 8, hipHostMallocDefault), nl_reassign_destroy(h));
    for (RaSlot &sl : h->slot) {
        STAGE_HIP(stage_alloc(&sl.bits, h->words, 8), nl_reassign_destroy(h));
        STAGE_HIP(stage_alloc(&sl.pre, h->words, 4), nl_reassign_destroy(h));
    }
    *out = h;
    return NL_OK;
}

// The next frame of the stack: branch and object labels (int32, the frame's shape).  The frame loaded before becomes "prev".
// seed != 0: its reassigned labels are its own labels (frame 0); otherwise they are 0 until nl_reassign_pair votes.
extern "C" int nl_reassign_frame(nl_reassign *h, const int32_t *branch, const int32_t *obj, int seed, int64_t *n_vox, char *err, size_t errlen) {
    STAGE_ENTER(h, "reassigner");
    if (!branch || !obj || !n_vox) return nl_fail(err, errlen, NL_EINVAL, "NULL labels or n_vox");
    hipStream_t st = h->stream;
    const i64 n = h->g.n;
    // the new frame is built in the slot of the frame before the last, which is lost from here on; the last frame stays valid
    // and `cur` moves only once the new one is complete, so after an error the handle holds one frame, not a half-written one
    const int into = h->cur ^ 1;
    if (h->frames > 1) h->frames = 1;
    h->has_best = false;
    RaSlot &s = h->slot[into];
    s.n = 0;
    NL_HIP(hipMemcpyAsync(h->d_branch, branch, (size_t)n * 4, hipMemcpyHostToDevice, st));
    NL_HIP(hipMemcpyAsync(h->d_obj, obj, (size_t)n * 4, hipMemcpyHostToDevice, st));
    const unsigned gv = (unsigned)((n + 255) / 256);
    rank_mask_kernel<<<gv, 256, 0, st>>>(RaLabelled{h->d_branch, h->d_obj}, n, s.bits, h->d_wcount);
    NL_CHECK_LAUNCH();
    i64 total = 0;
    if (int rc = rank_scan(h->scan, st, h->d_wcount, h->words, s.pre, RA_MAX_ROWS, "labelled voxels in one frame", &total, err, errlen)) return rc;
    if (int rc = stage_grow(&s.cap, total, total, {{&s.vox, 8}, {&s.lab_b, 4}, {&s.lab_o, 4}, {&s.re_b, 4}, {&s.re_o, 4}}, err, errlen)) return rc;
    if (total > 0) {
        ra_compact_kernel<<<gv, 256, 0, st>>>(h->d_branch, h->d_obj, n, s.bits, s.pre, seed ? 1 : 0, s.vox, s.lab_b, s.lab_o, s.re_b, s.re_o);
        NL_CHECK_LAUNCH();
    }
    NL_HIP(hipStreamSynchronize(st));                   // the host arrays may go away after the call
    s.n = total;
    h->cur = into;
    if (h->frames < 2) ++h->frames;
    *n_vox = total;
    return NL_OK;
}

// One direction: queries = the voxels of slot q, matched against the mask of slot m.  found = 0 leaves every match at -1.
static int ra_direction(nl_reassign *h, nl_flow *flow, const RaSlot &q, const RaSlot &m, double sign, int *match, float *dist, char *err, size_t errlen) {
    hipStream_t st = h->stream;
    const unsigned gq = (unsigned)((q.n + 255) / 256);
    int64_t found = 0;
    if (flow) {
        if (int rc = stage_start(*h, err, errlen)) return rc;
        rank_coords_kernel<<<gq, 256, 0, st>>>(q.vox, q.n, h->g.ny, h->g.nx, h->ndim, h->d_q);
        NL_CHECK_LAUNCH();
        if (int rc = stage_stop(*h, &h->kernel_ms, err, errlen)) return rc;      // the queries are complete before the field reads them
        if (int rc = nl_flow_interpolate_dev(flow, h->d_q, q.n, h->d_v, &found, err, errlen)) return rc;
        float ms = 0.f;
        if (int rc = nl_flow_kernel_ms(flow, &ms, err, errlen)) return rc;
        h->kernel_ms += ms;
        NL_HIP(hipSetDevice(h->device));
    }
    if (found == 0) {
        NL_HIP(hipMemsetAsync(match, 0xff, (size_t)q.n * 4, st));
        return NL_OK;
    }
    if (int rc = stage_start(*h, err, errlen)) return rc;
    if (h->ndim == 3) ra_search_kernel<3><<<gq, 256, 0, st>>>(q.vox, q.n, h->d_v, sign, h->g, m.bits, m.pre, h->d_table, h->ntab, h->half_diag, h->r, match, dist);
    else ra_search_kernel<2><<<gq, 256, 0, st>>>(q.vox, q.n, h->d_v, sign, h->g, m.bits, m.pre, h->d_table, h->ntab, h->half_diag, h->r, match, dist);
    NL_CHECK_LAUNCH();
    return stage_stop(*h, &h->kernel_ms, err, errlen);
}

// Matches the last two frames: forward candidates from the flow field `fw` (rows of t loaded), backward ones from `bw` (rows of
// t + 1 loaded); a NULL field gives no candidates of its direction.  Then the best pair and the two votes per voxel of the
// later frame, whose reassigned labels are written.  n_candidates = 0: no candidate at all (the caller's loop stops).
extern "C" int nl_reassign_pair(nl_reassign *h, nl_flow *fw, nl_flow *bw, int64_t *n_candidates, char *err, size_t errlen) {
    STAGE_ENTER(h, "reassigner");
    if (!n_candidates) return nl_fail(err, errlen, NL_EINVAL, "n_candidates is NULL");
    *n_candidates = 0;
    if (h->frames < 2) return nl_fail(err, errlen, NL_ESTATE, "nl_reassign_pair needs two frames");
    RaSlot &nx = h->slot[h->cur], &pv = h->slot[h->cur ^ 1];
    h->kernel_ms = 0.f;
    h->has_best = false;
    if (pv.n == 0 || nx.n == 0) return NL_OK;
    hipStream_t st = h->stream;
    const i64 n0 = pv.n, n1 = nx.n, big = n0 > n1 ? n0 : n1;
    const int D = h->ndim;
    if (int rc = stage_grow(&h->q_cap, big, big, {{&h->d_q, (size_t)D * 8}, {&h->d_v, (size_t)D * 8}}, err, errlen)) return rc;
    if (int rc = stage_grow(&h->fw_cap, n0, n0, {{&h->d_fw_match, 4}, {&h->d_fw_d, 4}}, err, errlen)) return rc;
    if (int rc = stage_grow(&h->bw_cap, n1, n1, {{&h->d_bw_match, 4}, {&h->d_bw_d, 4}}, err, errlen)) return rc;
    if (int rc = stage_grow(&h->t_cap, n1, n1, {{&h->d_cnt, 4}, {&h->d_start, 4}, {&h->d_cursor, 4}, {&h->d_best, 4}}, err, errlen)) return rc;
    if (int rc = stage_grow(&h->ent_cap, n0 + n1, n0 + n1, {{&h->d_ent, 4}}, err, errlen)) return rc;
    if (int rc = ra_direction(h, fw, pv, nx, 1.0, h->d_fw_match, h->d_fw_d, err, errlen)) return rc;
    if (int rc = ra_direction(h, bw, nx, pv, -1.0, h->d_bw_match, h->d_bw_d, err, errlen)) return rc;
    const unsigned gc = (unsigned)((n0 + n1 + 255) / 256), gt = (unsigned)((n1 + 255) / 256);
    if (int rc = stage_start(*h, err, errlen)) return rc;
    NL_HIP(hipMemsetAsync(h->d_cnt, 0, (size_t)n1 * 4, st));
    ra_count_kernel<<<gc, 256, 0, st>>>(h->d_fw_match, n0, h->d_bw_match, n1, h->d_cnt);
    NL_CHECK_LAUNCH();
    i64 total = 0;
    if (int rc = rank_scan(h->scan, st, h->d_cnt, n1, h->d_start, 2 * RA_MAX_ROWS - 1, "candidates in one frame pair", &total, err, errlen)) return rc;
    *n_candidates = total;
    if (total == 0) return NL_OK;
    NL_HIP(hipMemcpyAsync(h->d_cursor, h->d_start, (size_t)n1 * 4, hipMemcpyDeviceToDevice, st));
    ra_place_kernel<<<gc, 256, 0, st>>>(h->d_fw_match, n0, h->d_bw_match, n1, h->d_cursor, h->d_ent);
    NL_CHECK_LAUNCH();
    RaCand cd{h->d_fw_match, h->d_bw_match, h->d_fw_d, h->d_bw_d, (int)n0};
    ra_vote_kernel<<<gt, 256, 0, st>>>(n1, cd, h->d_start, h->d_cnt, h->d_ent, pv.re_b, pv.re_o, nx.lab_b, nx.lab_o, nx.re_b, nx.re_o, h->d_best);
    NL_CHECK_LAUNCH();
    if (int rc = stage_stop(*h, &h->kernel_ms, err, errlen)) return rc;
    h->has_best = true;
    return NL_OK;
}

// Downloads what the host keeps of a frame (which: 0 the last frame, 1 the one before): the linear indices of its labelled
// voxels in raster order (n), their reassigned labels, and -- last frame only, after a pair with candidates -- per voxel the rank
// of the best pair's source among the voxels of the frame before, -1 without a candidate.  NULL pointers are skipped.
extern "C" int nl_reassign_fetch(nl_reassign *h, int which, int64_t *vox, int32_t *re_branch, int32_t *re_obj, int32_t *best_src,
                                 char *err, size_t errlen) {
    STAGE_ENTER(h, "reassigner");
    if (which != 0 && which != 1) return nl_fail(err, errlen, NL_EINVAL, "which must be 0 or 1");
    if (h->frames < 1 + which) return nl_fail(err, errlen, NL_ESTATE, "no such frame");
    if (best_src && (which != 0 || !h->has_best)) return nl_fail(err, errlen, NL_ESTATE, "no best pairs to fetch");
    const RaSlot &s = h->slot[h->cur ^ which];
    hipStream_t st = h->stream;
    if (s.n > 0) {
        if (vox) NL_HIP(hipMemcpyAsync(vox, s.vox, (size_t)s.n * 8, hipMemcpyDeviceToHost, st));
        if (re_branch) NL_HIP(hipMemcpyAsync(re_branch, s.re_b, (size_t)s.n * 4, hipMemcpyDeviceToHost, st));
        if (re_obj) NL_HIP(hipMemcpyAsync(re_obj, s.re_o, (size_t)s.n * 4, hipMemcpyDeviceToHost, st));
        if (best_src) NL_HIP(hipMemcpyAsync(best_src, h->d_best, (size_t)s.n * 4, hipMemcpyDeviceToHost, st));
    }
    NL_HIP(hipStreamSynchronize(st));
    return NL_OK;
}

// Device time (ms) of the kernels of the last nl_reassign_pair call, the flow interpolation included, transfers excluded.
extern "C" int nl_reassign_kernel_ms(nl_reassign *h, float *ms, char *err, size_t errlen) {
    if (!h || !ms) return nl_fail(err, errlen, NL_EINVAL, "reassigner or ms is NULL");
    *ms = h->kernel_ms;
    return NL_OK;
}
