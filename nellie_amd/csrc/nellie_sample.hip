// Part of libnellie_hip.so (gfx950): the samples the thresholds are made from -- the strided lattice of a field (Filter) and the flat
// strided samples of a volume (Label), gathered, compacted, ranged and binned on the device -- and the histogram thresholds on the
// host.  The only unit that includes sampling.inc.  C-ABI in include/nellie_amd.h; what the Filter unit calls is declared in nl_host.h.
#include "nl_host.h"
#include "sampling.inc"
#include "thresholds.inc"

// NELLIE_CHAIN_UNFUSED_SAMPLING=1: the first round of a scale as two separate range + histogram sequences (A/B, tests)
static bool chain_unfused_sampling() {
    static int v = -1;
    if (v < 0) { const char *e = getenv("NELLIE_CHAIN_UNFUSED_SAMPLING"); v = (e && e[0] == '1') ? 1 : 0; }
    return v == 1;
}
// workgroups of the lattice reductions (range, histogram): every workgroup ends with atomics on the same few words, which
// retire ~10 ns apart -- 1024 workgroups spent 10-30 us on that alone (a 1e6-point gather is not longer); NELLIE_SAMPLE_GRID
static i64 sample_grid_cap() {
    static i64 v = 0;
    if (!v) { const char *e = getenv("NELLIE_SAMPLE_GRID"); v = (e && atoll(e) > 0) ? atoll(e) : 256; }
    return v;
}

static int make_field(nl_ctx *c, int field, FieldSrc &fs, char *err, size_t errlen) {
    fs.field = field; fs.hp = hessp(c); fs.max_abs = c->frob_max_abs; fs.max_finite = c->frob_max_finite;
    fs.two_d = c->two_d; fs.bits = nullptr; fs.wpr = 0; fs.fsq_cache = nullptr; fs.norm_dev = nullptr;
    if (field == NL_FIELD_GAUSS) fs.p = gauss_cur(c);
    else if (field == NL_FIELD_FROB) {
        if (!c->have_spacing) return nl_fail(err, errlen, NL_ESTATE, "NL_FIELD_FROB before nl_hessian_stats");
        fs.p = gauss_cur(c);
    } else if (field == NL_FIELD_FRANGI) fs.p = c->f[c->i_vmax];
    else if (field == NL_FIELD_VESSELNESS) {
        if (c->mask_slots_used == 0) return nl_fail(err, errlen, NL_ESTATE, "NL_FIELD_VESSELNESS before any scale was evaluated");
        NL_JOIN_SIDE(c);
        fs.p = c->f[c->i_vmax];
        fs.wpr = (int)((c->nx + 63) / 64);
        fs.bits = (const unsigned long long *)c->m[0] + (i64)((c->mask_slots_used - 1) & 1) * (c->nzl * c->ny * fs.wpr);
    } else return nl_fail(err, errlen, NL_EINVAL, "unknown field %d", field);
    return NL_OK;
}

static int fsq_reserve(nl_ctx *c, i64 total, char *err, size_t errlen) {
    if (total <= c->fsq_cache_cap) return NL_OK;
    if (c->d_fsq_cache) NL_HIP(hipFree(c->d_fsq_cache));
    c->d_fsq_cache = nullptr; c->fsq_cache_cap = 0;
    NL_HIP(hipMalloc((void **)&c->d_fsq_cache, (size_t)total * 4));
    c->fsq_cache_cap = total;
    return NL_OK;
}
static bool fsq_cached(const nl_ctx *c, i64 sz, i64 sy, i64 sx) {
    return c->fsq_cache_valid && c->fsq_cache_key[0] == sz && c->fsq_cache_key[1] == sy && c->fsq_cache_key[2] == sx;
}
static void fsq_filled(nl_ctx *c, const Lattice &L) {
    c->fsq_cache_key[0] = L.sz; c->fsq_cache_key[1] = L.sy; c->fsq_cache_key[2] = L.sx;
    c->fsq_cache_valid = 1;
}

// Where a sampling call reads: the lattice of the strides on the owned planes, the field's source and the number of points.
// NL_FIELD_FROB is sampled up to four times per scale (threshold bracket and exact threshold, min/max and histogram each) with
// different normalisations of the same frob_sq: the Hessian is evaluated at the lattice points once, into the context's cache,
// which the source then reads (cache = false: left unattached -- the pair kernel of the first round fills it in passing).
struct Site { Lattice L; FieldSrc fs; i64 total; };
static int site_setup(nl_ctx *c, int field, i64 sz, i64 sy, i64 sx, Site &s, char *err, size_t errlen, bool cache = true) {
    if (sz < 1 || sy < 1 || sx < 1) return nl_fail(err, errlen, NL_EINVAL, "strides must be >= 1");
    Lattice &L = s.L;
    L.sz = sz; L.sy = sy; L.sx = sx;
    // owned global planes [g_lo, g_hi): lattice planes are global z = k*sz
    const i64 g_lo = c->gz0 + c->own_lo, g_hi = c->gz0 + c->own_hi;
    const i64 k_lo = (g_lo + sz - 1) / sz, k_hi = (g_hi + sz - 1) / sz;   // k in [k_lo, k_hi)
    L.cz = k_hi > k_lo ? k_hi - k_lo : 0;
    L.zfirst = k_lo * sz - c->gz0;
    L.cy = (c->ny + sy - 1) / sy;
    L.cx = (c->nx + sx - 1) / sx;
    int rc;
    if ((rc = make_field(c, field, s.fs, err, errlen))) return rc;
    s.total = L.cz * L.cy * L.cx;
    if (field != NL_FIELD_FROB || !cache || s.total == 0) return NL_OK;
    if (!fsq_cached(c, sz, sy, sx)) {
        if ((rc = fsq_reserve(c, s.total, err, errlen))) return rc;
        ProfScope ps(c, "sample");
        sample_fsq_kernel<<<(unsigned)((s.total + 255) / 256), 256, 0, c->stream>>>(s.fs, geom(c), L, c->d_fsq_cache);
        NL_CHECK_LAUNCH();
        fsq_filled(c, L);
    }
    s.fs.fsq_cache = c->d_fsq_cache;
    return NL_OK;
}

// the grid-stride reductions over a site (the caller holds the ProfScope and checks the launches)
static void launch_minmax(nl_ctx *c, const Site &s, unsigned int *res) {
    sample_minmax_kernel<<<grid1d(s.total, 256, sample_grid_cap()), 256, 0, c->stream>>>(s.fs, geom(c), s.L, res);
}
static size_t hist_lds(int nbins) { return (size_t)(nbins + 2) * 4 + (size_t)nbins * 4; }
static void launch_hist(nl_ctx *c, const Site &s, const float *edges, int nbins, unsigned long long *counts, const unsigned int *flag, hipStream_t st) {
    sample_hist_kernel<<<grid1d(s.total, 256, sample_grid_cap()), 256, hist_lds(nbins), st>>>(s.fs, geom(c), s.L, edges, nbins, counts, flag);
}

extern "C" int nl_sample_gather(nl_ctx *c, int field, int64_t sz, int64_t sy, int64_t sx, float *out, int64_t cap,
                                int64_t *n, char *err, size_t errlen) {
    NL_ENTER(c);
    Site s; int rc;
    if ((rc = site_setup(c, field, sz, sy, sx, s, err, errlen))) return rc;
    const i64 total = s.total;
    if (n) *n = total;
    if (total == 0 || (!out && cap == 0)) return NL_OK;   // size query
    if (!out || cap < total) return nl_fail(err, errlen, NL_EINVAL, "output capacity %lld < %lld samples", (i64)cap, total);
    // a free float volume as staging: whichever of f[0..2] is not the current gauss
    float *stage = c->f[(c->i_gauss + 1) % 3];
    if (total > c->n) return nl_fail(err, errlen, NL_EINVAL, "lattice larger than the volume");
    {
        ProfScope ps(c, "sample");
        sample_gather_kernel<<<(unsigned)((total + 255) / 256), 256, 0, c->stream>>>(s.fs, geom(c), s.L, stage);
        NL_CHECK_LAUNCH();
    }
    NL_HIP(hipMemcpyAsync(out, stage, (size_t)total * 4, hipMemcpyDeviceToHost, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    return NL_OK;
}

int sample_gather_pos_enqueue(nl_ctx *c, int field, i64 sz, i64 sy, i64 sx, float *dst, unsigned int *d_n, i64 cap, i64 *total, char *err, size_t errlen) {
    Site s; int rc;
    if ((rc = site_setup(c, field, sz, sy, sx, s, err, errlen))) return rc;
    *total = s.total;
    if (s.total > cap) return NL_OK;
    NL_HIP(zero_small(d_n, 4, c->stream));
    if (s.total > 0) {
        ProfScope ps(c, "sample");
        sample_gather_pos_kernel<<<(unsigned)((s.total + 255) / 256), 256, 0, c->stream>>>(s.fs, geom(c), s.L, dst, d_n);
        NL_CHECK_LAUNCH();
    }
    return NL_OK;
}

// The positive samples of the same lattice, compacted on the device: only they cross PCIe (the consumers take
// arr[arr > 0] first anyway: filtering.py:357, 957-959).  Order unspecified.  cap >= number of lattice points.
// A positive gather leaves its samples in `stage` and their number in *d_n.  Fetching them used to be two round trips (the count,
// then that many samples); the count and the first NL_PREFIX samples now travel together into pinned memory, and only a longer
// list costs a second transfer.  *n = the count; out[0 .. n) = the samples.
#define NL_PREFIX 32768
int fetch_counted(nl_ctx *c, const float *stage, const unsigned int *d_n, i64 max_count, float *out, i64 cap, int64_t *n, char *err, size_t errlen) {
    if (!c->h_prefix) NL_HIP(hipHostMalloc(&c->h_prefix, (size_t)NL_PREFIX * 4 + 64, hipHostMallocDefault));
    unsigned int *h_n = (unsigned int *)c->h_prefix;
    float *h_s = (float *)((char *)c->h_prefix + 64);
    const i64 first = max_count < NL_PREFIX ? max_count : NL_PREFIX;
    NL_HIP(hipMemcpyAsync(h_n, d_n, 4, hipMemcpyDeviceToHost, c->stream));
    if (first > 0) NL_HIP(hipMemcpyAsync(h_s, stage, (size_t)first * 4, hipMemcpyDeviceToHost, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    const i64 k = (i64)*h_n;
    if (n) *n = 0;
    if (k > cap || (k && !out)) return nl_fail(err, errlen, NL_EINVAL, "output capacity %lld < %lld positive samples", (i64)cap, k);
    if (k > max_count) return nl_fail(err, errlen, NL_ESTATE, "positive gather counted %lld of at most %lld samples", k, max_count);
    if (k) memcpy(out, h_s, (size_t)(k < first ? k : first) * 4);
    if (k > first) {
        NL_HIP(hipMemcpyAsync(out + first, stage + first, (size_t)(k - first) * 4, hipMemcpyDeviceToHost, c->stream));
        NL_HIP(hipStreamSynchronize(c->stream));
    }
    if (n) *n = k;
    return NL_OK;
}

// The positive lattice samples in two halves, so that the host can do other work (nl_chain_finish: wait for the chain's
// records, repeat its decisions) while the kernel runs: _begin enqueues the kernel and the download of the count, _end waits and
// fetches the samples.  No other call on this context in between except nl_chain_finish / nl_chain_log.
extern "C" int nl_sample_gather_positive_begin(nl_ctx *c, int field, int64_t sz, int64_t sy, int64_t sx, int64_t *n_lattice, char *err, size_t errlen) {
    NL_ENTER(c);
    c->gp_total = -1;
    c->gp_stage = c->f[(c->i_gauss + 1) % 3];
    i64 total; int rc;
    if ((rc = sample_gather_pos_enqueue(c, field, sz, sy, sx, c->gp_stage, (unsigned int *)c->d_small, c->n, &total, err, errlen))) return rc;
    if (n_lattice) *n_lattice = total;
    if (total > c->n) return nl_fail(err, errlen, NL_EINVAL, "lattice larger than the volume");
    c->gp_total = total;
    return NL_OK;
}
extern "C" int nl_sample_gather_positive_end(nl_ctx *c, float *out, int64_t cap, int64_t *n, char *err, size_t errlen) {
    NL_ENTER(c);
    if (c->gp_total < 0) return nl_fail(err, errlen, NL_ESTATE, "nl_sample_gather_positive_end without _begin");
    const i64 total = c->gp_total;
    c->gp_total = -1;
    if (n) *n = 0;
    if (total == 0) return NL_OK;
    return fetch_counted(c, c->gp_stage, (const unsigned int *)c->d_small, total, out, cap, n, err, errlen);
}
extern "C" int nl_sample_gather_positive(nl_ctx *c, int field, int64_t sz, int64_t sy, int64_t sx, float *out, int64_t cap,
                                         int64_t *n, char *err, size_t errlen) {
    int64_t total = 0;
    if (n) *n = 0;
    int rc = nl_sample_gather_positive_begin(c, field, sz, sy, sx, &total, err, errlen);
    if (rc) return rc;
    if (total > 0 && (!out || cap < total)) { c->gp_total = -1; return nl_fail(err, errlen, NL_EINVAL, "output capacity %lld < %lld lattice points", (i64)cap, (i64)total); }
    return nl_sample_gather_positive_end(c, out, cap, n, err, errlen);
}

// The initial state of a range: no sample yet (min = all ones, max, count and flag zero), uploaded from the pinned words `h`.
static int range_reset(nl_ctx *c, unsigned int *res, unsigned int *h, char *err, size_t errlen) {
    h[0] = 0xffffffffu; h[1] = 0; h[2] = 0; h[3] = 0; h[4] = 0;
    NL_HIP(hipMemcpyAsync(res, h, 20, hipMemcpyHostToDevice, c->stream));
    return NL_OK;
}
// ... and of a whole record at d0 (pinned mirror h0): that range, zero counts
static int record_reset(nl_ctx *c, char *d0, char *h0, int nbins, char *err, size_t errlen) {
    const size_t off_res = hist_layout(nbins).off_res;
    int rc = range_reset(c, (unsigned int *)(d0 + off_res), (unsigned int *)(h0 + off_res), err, errlen);
    if (rc) return rc;
    NL_HIP(zero_small(d0, (size_t)nbins * 8, c->stream));
    return NL_OK;
}

extern "C" int nl_sample_minmax(nl_ctx *c, int field, int64_t sz, int64_t sy, int64_t sx, float *mn, float *mx,
                                int64_t *npos, char *err, size_t errlen) {
    NL_ENTER(c);
    Site s; int rc;
    if ((rc = site_setup(c, field, sz, sy, sx, s, err, errlen))) return rc;
    unsigned int *res = (unsigned int *)c->d_small;
    unsigned int *h = (unsigned int *)c->h_small;
    if ((rc = range_reset(c, res, h, err, errlen))) return rc;
    if (s.total > 0) {
        ProfScope ps(c, "sample");
        launch_minmax(c, s, res);
        NL_CHECK_LAUNCH();
    }
    if (fused(c) && (rc = reduce_range(c, res, nullptr, err, errlen))) return rc;
    NL_HIP(hipMemcpyAsync(h, res, 16, hipMemcpyDeviceToHost, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    const unsigned long long cnt = *(unsigned long long *)(h + 2);
    if (npos) *npos = (int64_t)cnt;
    if (cnt) {
        if (mn) memcpy(mn, &h[0], 4);
        if (mx) memcpy(mx, &h[1], 4);
    }
    return NL_OK;
}

extern "C" int nl_sample_hist(nl_ctx *c, int field, int64_t sz, int64_t sy, int64_t sx, const float *edges, int nbins,
                              int64_t *counts, char *err, size_t errlen) {
    NL_ENTER(c);
    if (!edges || !counts || nbins < 1 || nbins > 4096) return nl_fail(err, errlen, NL_EINVAL, "bad histogram arguments (nbins=%d)", nbins);
    Site s; int rc;
    if ((rc = site_setup(c, field, sz, sy, sx, s, err, errlen))) return rc;
    // d_small layout: [0, 32K) counts (u64 x nbins), [32K, 64K) edges (f32 x nbins+1)
    unsigned long long *d_counts = (unsigned long long *)c->d_small;
    float *d_edges = (float *)((char *)c->d_small + (1 << 15));
    NL_HIP(zero_small(d_counts, (size_t)nbins * 8, c->stream));
    memcpy((char *)c->h_small + (1 << 15), edges, (size_t)(nbins + 1) * 4);
    NL_HIP(hipMemcpyAsync(d_edges, (char *)c->h_small + (1 << 15), (size_t)(nbins + 1) * 4, hipMemcpyHostToDevice, c->stream));
    if (s.total > 0) {
        ProfScope ps(c, "sample");
        launch_hist(c, s, d_edges, nbins, d_counts, nullptr, c->stream);
        NL_CHECK_LAUNCH();
    }
    if (fused(c) && (rc = reduce_u64_sum(c, d_counts, (size_t)nbins, err, errlen))) return rc;
    NL_HIP(hipMemcpyAsync(c->h_small, d_counts, (size_t)nbins * 8, hipMemcpyDeviceToHost, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    memcpy(counts, c->h_small, (size_t)nbins * 8);
    return NL_OK;
}

// nl_sample_minmax + nl_sample_hist in one go: the bin edges numpy would build from the range are formed on the
// device, so the two passes need no host round trip in between.  The kernels of one range + edges + histogram sequence, enqueued.
// d0: the record in device memory (hist_layout); h0: its pinned mirror (the initial state is uploaded from there), or NULL when the
// record was initialised by the caller (chain_init_kernel)
static int range_hist_enqueue(nl_ctx *c, int field, i64 sz, i64 sy, i64 sx, int nbins, char *d0, char *h0, char *err, size_t errlen) {
    Site s; int rc;
    if ((rc = site_setup(c, field, sz, sy, sx, s, err, errlen))) return rc;
    const HistLayout lay = hist_layout(nbins);
    unsigned long long *d_counts = (unsigned long long *)d0;
    float *d_edges = (float *)(d0 + lay.off_edges);
    unsigned int *res = (unsigned int *)(d0 + lay.off_res);
    if (h0 && (rc = record_reset(c, d0, h0, nbins, err, errlen))) return rc;
    if (s.total > 0 || fused(c)) {
        // fused: a rank without lattice points of its own still takes part in the collectives and builds the same edges
        ProfScope ps(c, "sample");
        if (s.total > 0) launch_minmax(c, s, res);
        if (fused(c) && (rc = reduce_range(c, res, nullptr, err, errlen))) return rc;
        sample_edges_kernel<<<1, 64, 0, c->stream>>>(res, nbins, d_edges, res + 4);
        if (s.total > 0) launch_hist(c, s, d_edges, nbins, d_counts, res + 4, c->stream);
        NL_CHECK_LAUNCH();
        if (fused(c) && (rc = reduce_u64_sum(c, d_counts, (size_t)nbins, err, errlen))) return rc;
    }
    return NL_OK;
}
// The Gaussian and the raw-Frobenius records of one scale in three launches instead of seven: one pass fills the frob_sq
// cache and both ranges, one builds both edge arrays, one bins both.  With fused reductions: two grouped collectives instead of four.
static int range_hist_pair_enqueue(nl_ctx *c, i64 sz, i64 sy, i64 sx, int nbins, char *dG, char *dF, char *hG, char *hF, char *err, size_t errlen) {
    Site g, f; int rc;
    if ((rc = site_setup(c, NL_FIELD_GAUSS, sz, sy, sx, g, err, errlen))) return rc;
    if ((rc = site_setup(c, NL_FIELD_FROB, sz, sy, sx, f, err, errlen, false))) return rc;
    const i64 total = g.total;
    const HistLayout lay = hist_layout(nbins);
    unsigned int *resG = (unsigned int *)(dG + lay.off_res), *resF = (unsigned int *)(dF + lay.off_res);
    float *edgesG = (float *)(dG + lay.off_edges), *edgesF = (float *)(dF + lay.off_edges);
    if (hG && (rc = record_reset(c, dG, hG, nbins, err, errlen))) return rc;
    if (hF && (rc = record_reset(c, dF, hF, nbins, err, errlen))) return rc;
    if ((rc = fsq_reserve(c, total, err, errlen))) return rc;
    if (total == 0 && !fused(c)) return NL_OK;
    ProfScope ps(c, "sample");
    if (total > 0) {
        sample_minmax2_kernel<<<grid1d(total, 256, sample_grid_cap()), 256, 0, c->stream>>>(g.fs, f.fs, geom(c), g.L, resG, resF, c->d_fsq_cache);
        fsq_filled(c, g.L);
        f.fs.fsq_cache = c->d_fsq_cache;
    }
    if (fused(c) && (rc = reduce_range(c, resG, resF, err, errlen))) return rc;
    sample_edges2_kernel<<<2, 64, 0, c->stream>>>(resG, edgesG, resG + 4, resF, edgesF, resF + 4, nbins);
    if (total > 0)
        sample_hist2_kernel<<<grid1d(total, 256, sample_grid_cap()), 256, 2 * hist_lds(nbins), c->stream>>>(g.fs, f.fs, geom(c), g.L, nbins, edgesG, (unsigned long long *)dG, resG + 4,
                                                                                                           edgesF, (unsigned long long *)dF, resF + 4);
    NL_CHECK_LAUNCH();
    if (fused(c) && (rc = reduce_u64_sum(c, (unsigned long long *)dG, (size_t)nbins, err, errlen, (unsigned long long *)dF))) return rc;
    return NL_OK;
}

int sample_first_round(nl_ctx *c, int field_a, int field_b, i64 sz, i64 sy, i64 sx, int nbins, char *dA, char *dB, char *hA, char *hB, bool pair_ok,
                       char *err, size_t errlen) {
    if (pair_ok && field_a == NL_FIELD_GAUSS && field_b == NL_FIELD_FROB && !chain_unfused_sampling())
        return range_hist_pair_enqueue(c, sz, sy, sx, nbins, dA, dB, hA, hB, err, errlen);
    int rc = range_hist_enqueue(c, field_a, sz, sy, sx, nbins, dA, hA, err, errlen);
    return rc ? rc : range_hist_enqueue(c, field_b, sz, sy, sx, nbins, dB, hB, err, errlen);
}

int sample_exact_round(nl_ctx *c, i64 sz, i64 sy, i64 sx, int nbins, char *rec, const float *norm_dev, hipStream_t st, bool reduce, char *err, size_t errlen) {
    Site s; int rc;
    if ((rc = site_setup(c, NL_FIELD_FROB, sz, sy, sx, s, err, errlen))) return rc;
    s.fs.norm_dev = norm_dev;
    const HistLayout lay = hist_layout(nbins);
    unsigned long long *counts = (unsigned long long *)rec;
    float *edges = (float *)(rec + lay.off_edges);
    unsigned int *res = (unsigned int *)(rec + lay.off_res);
    ProfScope ps(c, "sample", st);
    sample_edges_kernel<<<1, 64, 0, st>>>(res, nbins, edges, res + 4);
    if (s.total > 0) launch_hist(c, s, edges, nbins, counts, res + 4, st);
    NL_CHECK_LAUNCH();
    if (reduce && fused(c) && (rc = reduce_u64_sum(c, counts, (size_t)nbins, err, errlen))) return rc;
    return NL_OK;
}

// The synchronous forms work in the two halves of the small scratch (device and pinned): record k at k * NL_RH_SLOT.
// *valid: 0 no positive sample, 1 ok, 2 range not finite (the caller raises numpy's ValueError then).  edges (may be NULL)
// receives the nbins + 1 device-built edges.
#define NL_RH_SLOT 32768
static int range_hist_fetch(nl_ctx *c, int nbins, int records, char *err, size_t errlen) {
    for (int k = 0; k < records; ++k)
        NL_HIP(hipMemcpyAsync((char *)c->h_small + (size_t)k * NL_RH_SLOT, (char *)c->d_small + (size_t)k * NL_RH_SLOT, hist_layout(nbins).bytes, hipMemcpyDeviceToHost, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    return NL_OK;
}
static void range_hist_read(const nl_ctx *c, int nbins, int slot, float *mn, float *mx, int64_t *npos, int64_t *counts, float *edges, int *valid) {
    const HistLayout lay = hist_layout(nbins);
    const char *h0 = (const char *)c->h_small + (size_t)slot * NL_RH_SLOT;
    const unsigned int *hr = (const unsigned int *)(h0 + lay.off_res);
    const unsigned long long cnt = *(const unsigned long long *)(hr + 2);
    if (npos) *npos = (int64_t)cnt;
    *valid = (int)hr[4];
    if (cnt) {
        if (mn) memcpy(mn, &hr[0], 4);
        if (mx) memcpy(mx, &hr[1], 4);
    }
    memcpy(counts, h0, (size_t)nbins * 8);
    if (edges) memcpy(edges, h0 + lay.off_edges, (size_t)(nbins + 1) * 4);
}

extern "C" int nl_sample_range_hist(nl_ctx *c, int field, int64_t sz, int64_t sy, int64_t sx, int nbins, float *mn, float *mx,
                                    int64_t *npos, int64_t *counts, float *edges, int *valid, char *err, size_t errlen) {
    NL_ENTER(c);
    if (!counts || !valid || nbins < 1 || nbins > 2048) return nl_fail(err, errlen, NL_EINVAL, "bad histogram arguments (nbins=%d)", nbins);
    int rc;
    if ((rc = range_hist_enqueue(c, field, sz, sy, sx, nbins, (char *)c->d_small, (char *)c->h_small, err, errlen))) return rc;
    if ((rc = range_hist_fetch(c, nbins, 1, err, errlen))) return rc;
    range_hist_read(c, nbins, 0, mn, mx, npos, counts, edges, valid);
    return NL_OK;
}

// Two independent fields in one round trip (the gamma samples of the Gaussian and the raw Frobenius samples of a scale:
// filtering.py:365-380 and 421-444 need nothing from each other).  Arrays of two: [0] = field_a, [1] = field_b.
extern "C" int nl_sample_range_hist2(nl_ctx *c, int field_a, int field_b, int64_t sz, int64_t sy, int64_t sx, int nbins, float *mn, float *mx,
                                     int64_t *npos, int64_t *counts, float *edges, int *valid, char *err, size_t errlen) {
    NL_ENTER(c);
    if (!counts || !valid || !mn || !mx || !npos || nbins < 1 || nbins > 2048) return nl_fail(err, errlen, NL_EINVAL, "bad histogram arguments (nbins=%d)", nbins);
    int rc;
    // the pair of a scale's first round (filtering.py:365-380, 421-444) in one pass over the lattice, while no cache exists yet
    if ((rc = sample_first_round(c, field_a, field_b, sz, sy, sx, nbins, (char *)c->d_small, (char *)c->d_small + NL_RH_SLOT, (char *)c->h_small,
                                 (char *)c->h_small + NL_RH_SLOT, !fsq_cached(c, sz, sy, sx) && nbins <= 1024, err, errlen))) return rc;
    if ((rc = range_hist_fetch(c, nbins, 2, err, errlen))) return rc;
    for (int k = 0; k < 2; ++k)
        range_hist_read(c, nbins, k, mn + k, mx + k, npos + k, counts + (size_t)k * nbins, edges ? edges + (size_t)k * (nbins + 1) : nullptr, valid + k);
    return NL_OK;
}

extern "C" int nl_hist_thresholds(const int64_t *counts, const float *edges, int nbins, double *triangle, double *otsu, int *status,
                                  char *err, size_t errlen) {
    if (!counts || !edges || !triangle || !otsu || !status || nbins < 1 || nbins > (1 << 20))
        return nl_fail(err, errlen, NL_EINVAL, "bad histogram arguments (nbins=%d)", nbins);
    hist_thresholds_host<float>(counts, edges, nbins, triangle, otsu, status);
    return NL_OK;
}

void host_edges(float first, float last, int nbins, float *edges) {
    if (first == last) { first = first - 0.5f; last = last + 0.5f; }
    volatile float delta = last - first;
    const float div = (float)nbins;
    volatile float step = delta / div;
    for (int i = 0; i <= nbins; ++i) {
        volatile float y = (float)i;
        if (step == 0.0f) { y = y / div; y = y * delta; } else y = y * step;
        y = y + first;
        edges[i] = (i == nbins) ? last : y;
    }
}
// np.histogram(values, bins=nbins, range=(min, max)) of float32 host data + the two thresholds of that histogram, in one call
// (labelling.py:448-455 after the log10: the samples are a few 10^4 values, numpy spends ~0.2-0.6 ms on them while the GPU
// waits).  Same float32 arithmetic as sample_edges_kernel / sample_hist_kernel, which are pinned against numpy.  *status: 0 ok,
// 1 degenerate triangle (numpy's ValueError), 2 range not finite (numpy's ValueError).  counts / edges: optional copies.
extern "C" int nl_host_hist_thresholds_f32(const float *values, int64_t n, int nbins, double *triangle, double *otsu, int *status,
                                           int64_t *counts_out, float *edges_out, char *err, size_t errlen) {
    if (!values || n < 1 || !triangle || !otsu || !status || nbins < 1 || nbins > (1 << 20))
        return nl_fail(err, errlen, NL_EINVAL, "bad histogram arguments (n=%lld, nbins=%d)", (long long)n, nbins);
    float mn = values[0], mx = values[0];
    bool nan = false;
    for (int64_t i = 0; i < n; ++i) {
        const float a = values[i];
        if (a != a) nan = true;
        if (a < mn) mn = a;
        if (a > mx) mx = a;
    }
    *status = 0; *triangle = 0.0; *otsu = 0.0;
    if (nan || !(fabsf(mn) <= 3.402823466e38f) || !(fabsf(mx) <= 3.402823466e38f)) { *status = 2; return NL_OK; }
    std::vector<float> edges((size_t)nbins + 1);
    std::vector<int64_t> counts((size_t)nbins, 0);
    host_edges(mn, mx, nbins, edges.data());
    volatile float first = mn, last = mx;
    if (mn == mx) { first = mn - 0.5f; last = mx + 0.5f; }
    const float f0 = first, f1 = last;
    volatile float denom = f1 - f0;
    const float dn = denom, nb = (float)nbins;
    for (int64_t i = 0; i < n; ++i) {
        const float a = values[i];
        if (!(a >= f0 && a <= f1)) continue;
        const float t = ((a - f0) / dn) * nb;          // float32 throughout (x86-64 SSE, -ffp-contract=off): numpy's expression
        int idx = (int)t;
        if (idx == nbins) idx -= 1;
        if (a < edges[idx]) idx -= 1;
        if (a >= edges[idx + 1] && idx != nbins - 1) idx += 1;
        counts[idx] += 1;
    }
    hist_thresholds_host<float>(counts.data(), edges.data(), nbins, triangle, otsu, status, nullptr);
    if (counts_out) memcpy(counts_out, counts.data(), (size_t)nbins * 8);
    if (edges_out) memcpy(edges_out, edges.data(), ((size_t)nbins + 1) * 4);
    return NL_OK;
}

extern "C" int nl_hist_thresholds_ex(const int64_t *counts, const void *edges, int edges_f64, int nbins, double *triangle, double *otsu,
                                     double *otsu_var, int *status, char *err, size_t errlen) {
    if (!counts || !edges || !triangle || !otsu || !status || nbins < 1 || nbins > (1 << 20))
        return nl_fail(err, errlen, NL_EINVAL, "bad histogram arguments (nbins=%d)", nbins);
    if (edges_f64) hist_thresholds_host<double>(counts, (const double *)edges, nbins, triangle, otsu, status, otsu_var);
    else hist_thresholds_host<float>(counts, (const float *)edges, nbins, triangle, otsu, status, otsu_var);
    return NL_OK;
}

// ---- flat strided samples of a volume (Label's threshold sampling, labelling.py:426-433) ----------------------------------------
// The flat index offset + k * step runs over the GLOBAL volume; this rank contributes the indices inside its owned planes:
// `count` of them from `first` on (local flat index = global - gz0 * plane).
static void owned_flat_range(const nl_ctx *c, i64 offset, i64 step, i64 &first, i64 &count) {
    const i64 plane = c->ny * c->nx;
    const i64 g_begin = (c->gz0 + c->own_lo) * plane, g_end = (c->gz0 + c->own_hi) * plane;
    const i64 k0 = g_begin > offset ? (g_begin - offset + step - 1) / step : 0;
    const i64 k1 = g_end > offset ? (g_end - offset + step - 1) / step : 0;    // k in [k0, k1)
    first = offset + k0 * step;
    count = k1 > k0 ? k1 - k0 : 0;
}
static int flat_args(nl_ctx *c, int field, i64 offset, i64 step, char *err, size_t errlen) {
    if (step < 1 || offset < 0) return nl_fail(err, errlen, NL_EINVAL, "bad offset/step");
    if (field != NL_FIELD_FRANGI && field != NL_FIELD_GAUSS) return nl_fail(err, errlen, NL_EINVAL, "flat sampling supports GAUSS/FRANGI");
    return NL_OK;
}
// a free staging volume -- neither the current Gaussian nor `src` --, not the pre-zeroed one while there is another
static float *free_stage(nl_ctx *c, const float *src) {
    float *stage = nullptr;
    for (int k = 0; k < 3; ++k) if (k != c->i_gauss && c->f[k] != src && !pz_is(c, c->f[k])) { stage = c->f[k]; break; }
    if (!stage) for (int k = 0; k < 3; ++k) if (k != c->i_gauss && c->f[k] != src) { stage = c->f[k]; break; }
    pz_touch(c, stage);
    return stage;
}

extern "C" int nl_flat_sample_gather(nl_ctx *c, int field, int64_t offset, int64_t step, float *out, int64_t cap, int64_t *n,
                                     char *err, size_t errlen) {
    NL_ENTER_KEEP_PZ(c);
    NL_KEEP_SUPPORT(c);
    int rc;
    if ((rc = flat_args(c, field, offset, step, err, errlen))) return rc;
    i64 first, count;
    owned_flat_range(c, offset, step, first, count);
    if (n) *n = count;
    if (count == 0 || (!out && cap == 0)) return NL_OK;   // size query
    if (!out || cap < count) return nl_fail(err, errlen, NL_EINVAL, "output capacity %lld < %lld samples", (i64)cap, count);
    const float *src = field_ptr(c, field);
    float *stage = free_stage(c, src);
    {
        ProfScope ps(c, "sample");
        flat_gather_kernel<<<(unsigned)((count + 255) / 256), 256, 0, c->stream>>>(src, -c->gz0 * c->ny * c->nx, first, step, count, stage);
        NL_CHECK_LAUNCH();
    }
    NL_HIP(hipMemcpyAsync(out, stage, (size_t)count * 4, hipMemcpyDeviceToHost, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    return NL_OK;
}

// nl_flat_sample_gather restricted to the positive samples, compacted on the device (labelling.py:426-433 takes
// values[values > 0]); order unspecified.  cap >= the count nl_flat_sample_gather reports.
extern "C" int nl_flat_sample_gather_positive(nl_ctx *c, int field, int64_t offset, int64_t step, float *out, int64_t cap,
                                              int64_t *n, char *err, size_t errlen) {
    NL_ENTER_KEEP_PZ(c);
    NL_KEEP_SUPPORT(c);
    int rc;
    if ((rc = flat_args(c, field, offset, step, err, errlen))) return rc;
    i64 first, count;
    owned_flat_range(c, offset, step, first, count);
    if (n) *n = 0;
    if (count == 0) return NL_OK;
    if (!out || cap < count) return nl_fail(err, errlen, NL_EINVAL, "output capacity %lld < %lld samples", (i64)cap, count);
    const float *src = field_ptr(c, field);
    float *stage = free_stage(c, src);
    unsigned int *d_n = (unsigned int *)c->d_small;
    NL_HIP(zero_small(d_n, 4, c->stream));
    {
        ProfScope ps(c, "sample");
        flat_gather_pos_kernel<<<(unsigned)((count + 255) / 256), 256, 0, c->stream>>>(src, -c->gz0 * c->ny * c->nx, first, step, count, stage, d_n);
        NL_CHECK_LAUNCH();
    }
    return fetch_counted(c, stage, d_n, count, out, cap, n, err, errlen);
}

// The positive samples of ALL ranks in one call with one wait (round 4): every rank compacts its samples into a block
// [count | samples ...] of block_items + 1 floats (block_items: a bound on any rank's sample points that the callers derive from
// the global geometry, identical everywhere), the blocks are all-gathered over RCCL on the context stream and land in page-locked
// memory.  mode 0: the lattice arr[::a, ::b, ::c] of `field` (filtering.py:348-363), mode 1: flat[a::b] (labelling.py:418-433).
// out receives the samples rank by rank, counts[r] how many rank r contributed.  Before: a download, then nl_allgather_var's two
// collectives with a wait each.
extern "C" int nl_positive_samples_world(nl_ctx *c, int field, int mode, int64_t a, int64_t b, int64_t cc, int64_t block_items,
                                         float *out, int64_t cap, int64_t *counts, char *err, size_t errlen) {
    NL_ENTER(c);
    NL_KEEP_SUPPORT(c);
    if (!c->comm) return nl_fail(err, errlen, NL_ESTATE, "nl_positive_samples_world before nl_comm_init");
    if (block_items < 0 || !counts || (mode != 0 && mode != 1)) return nl_fail(err, errlen, NL_EINVAL, "bad arguments");
    const int W = c->world;
    const size_t blk = (size_t)block_items + 1;                       // floats per rank
    int rc;
    if ((rc = ag_reserve(c, blk * (size_t)(W + 1) * 4, blk * W * 4, err, errlen))) return rc;
    float *d_send = (float *)c->d_ag, *d_recv = d_send + blk;
    i64 points = 0;
    if (mode == 0) {
        if ((rc = sample_gather_pos_enqueue(c, field, a, b, cc, d_send + 1, (unsigned int *)d_send, block_items, &points, err, errlen))) return rc;
        if (points > block_items) return nl_fail(err, errlen, NL_EINVAL, "%lld lattice points in this slab, block of %lld", (long long)points, (long long)block_items);
    } else {
        if ((rc = flat_args(c, field, a, b, err, errlen))) return rc;
        i64 first;
        owned_flat_range(c, a, b, first, points);
        if (points > block_items) return nl_fail(err, errlen, NL_EINVAL, "%lld sample points in this slab, block of %lld", (long long)points, (long long)block_items);
        NL_HIP(zero_small(d_send, 4, c->stream));
        if (points) {
            ProfScope ps(c, "sample");
            flat_gather_pos_kernel<<<(unsigned)((points + 255) / 256), 256, 0, c->stream>>>(field_ptr(c, field), -c->gz0 * c->ny * c->nx, first, b, points, d_send + 1, (unsigned int *)d_send);
            NL_CHECK_LAUNCH();
        }
    }
    {
        ProfScope ps(c, "halo");
        NL_NCCL(rccl().AllGather(d_send, d_recv, blk, ncclFloat, (ncclComm_t)c->comm, c->stream));
    }
    NL_HIP(hipMemcpyAsync(c->h_ag, d_recv, blk * W * 4, hipMemcpyDeviceToHost, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    i64 total = 0;
    const float *h = (const float *)c->h_ag;
    for (int r = 0; r < W; ++r) {
        unsigned int k; memcpy(&k, h + (size_t)r * blk, 4);
        if ((i64)k > block_items) return nl_fail(err, errlen, NL_ESTATE, "rank %d reports %u samples in a block of %lld", r, k, (long long)block_items);
        counts[r] = (int64_t)k;
        if (total + (i64)k > cap || (k && !out)) return nl_fail(err, errlen, NL_EINVAL, "output capacity %lld too small", (long long)cap);
        if (k) memcpy(out + total, h + (size_t)r * blk + 1, (size_t)k * 4);
        total += (i64)k;
    }
    return NL_OK;
}
