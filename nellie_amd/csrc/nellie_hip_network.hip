// Translation unit of libnellie_hip.so (gfx950): the Network stage behind the thinning (nellie/segmentation/networking.py:828-851).
// C-ABI in include/nellie_amd.h; kernels in network_relabel.inc; the classes and the branch labels are nellie_label.hip's, the thinning
// (nl_network_load_thin) is nellie_hip_thin.hip's.  The calls
// live on the context because that is where the pixel-class and branch-label kernels keep their volumes: one frame goes up
// (nl_network_load), stays in HBM through clean, seed, classes and relabel, and comes down once (nl_network_fetch).
//   f[0]  skel = labels * mask, later the relabelled volume     f[2]  pixel classes (uint8)
//   f[3]  cleaned + seeded skeleton, later the branch labels    f[0], f[1]  run records of the branch labelling in between
#include <algorithm>
#include "nl_host.h"
#include "network_relabel.inc"

#define NW_MAX_SCRATCH ((i64)1 << 38)       // slots of a batch: the launches count them in an unsigned number of 256-thread workgroups

void nw_release(nl_ctx *c) {
    for (void *p : {(void *)c->nw_lab, (void *)c->nw_fr, (void *)c->nw_mask, c->nw_tab, (void *)c->nw_feat, (void *)c->nw_stk, c->nw_objs})
        if (p) hipFree(p);
    for (hipEvent_t e : c->nw_ev) if (e) hipEventDestroy(e);
    for (hipEvent_t e : c->thin_ev) if (e) hipEventDestroy(e);
}

static inline unsigned long long *nw_best(nl_ctx *c) { return (unsigned long long *)c->nw_tab; }
static inline int *nw_box(nl_ctx *c) { return (int *)(nw_best(c) + (c->nw_tab_cap + 1)); }
static inline int *nw_has(nl_ctx *c) { return nw_box(c) + 6 * (c->nw_tab_cap + 1); }
static inline int *nw_seeded(nl_ctx *c) { return nw_has(c) + (c->nw_tab_cap + 1); }

static int nw_grow(void **p, i64 *cap, i64 need, size_t elem, hipStream_t st, char *err, size_t errlen) {
    if (*p && need <= *cap) return NL_OK;
    if (*p) { NL_HIP(hipStreamSynchronize(st)); NL_HIP(hipFree(*p)); *p = nullptr; *cap = 0; }
    NL_HIP(hipMalloc(p, (size_t)(need > 0 ? need : 1) * elem));
    *cap = need;
    return NL_OK;
}

static int nw_check(nl_ctx *c, int ndim, char *err, size_t errlen) {
    if (c->own_lo != 0 || c->own_hi != c->nzl || c->gnz != c->nzl) return nl_fail(err, errlen, NL_EINVAL, "the Network kernels run on a whole volume");
    if (ndim != 2 && ndim != 3) return nl_fail(err, errlen, NL_EINVAL, "ndim must be 2 or 3");
    if (ndim == 2 && c->nzl != 1) return nl_fail(err, errlen, NL_EINVAL, "a 2-D frame needs a context of shape (1, ny, nx)");
    if (c->n >= ((i64)1 << 31)) return nl_fail(err, errlen, NL_EINVAL, "the Network stage holds voxel indices in 32 bits: frames of 2^31 voxels or more are not supported");
    return NL_OK;
}

static int nw_begin(nl_ctx *c, char *err, size_t errlen) {
    for (hipEvent_t &e : c->nw_ev) if (!e) NL_HIP(hipEventCreate(&e));
    if (!c->nw_lab) NL_HIP(hipMalloc((void **)&c->nw_lab, (size_t)c->n * 4));
    c->nw_stage = 0;
    c->nw_has_classes = 0;
    c->thin_valid = 0;
    for (float &m : c->nw_ms) m = 0.f;
    // the frame takes over the four volumes and the mask planes
    c->i_labels = -1; c->frangi_ready = 0; c->gauss_ext = nullptr; c->fsq_cache_valid = 0; c->mk_state = 0; c->nw_state = 0;
    return NL_OK;
}

static NwGeom nw_geom(const nl_ctx *c) {
    NwGeom g;
    g.nz = (int)c->nzl; g.ny = (int)c->ny; g.nx = (int)c->nx; g.ndim = c->nw_ndim;
    g.s[0] = g.s[1] = g.s[2] = 1.0;
    return g;
}

// stats (two ints in d_small, zeroed by the caller's kernel order): the largest label and the smallest; sizes the per-label tables
static int nw_labels_done(nl_ctx *c, int64_t *max_label, char *err, size_t errlen) {
    int *d_stats = (int *)c->d_small + 8;
    NL_HIP(hipMemcpyAsync(c->h_small, d_stats, 8, hipMemcpyDeviceToHost, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    const int mx = ((int *)c->h_small)[0], mn = ((int *)c->h_small)[1];
    if (mn < 0) return nl_fail(err, errlen, NL_EINVAL, "labels hold %d: object labels are not negative", mn);
    c->nw_max_label = mx;
    if (!c->nw_tab || mx > c->nw_tab_cap) {
        const i64 cap = std::max<i64>(mx, 1024);
        if (c->nw_tab) { NL_HIP(hipFree(c->nw_tab)); c->nw_tab = nullptr; c->nw_tab_cap = 0; }
        NL_HIP(hipMalloc(&c->nw_tab, (size_t)(cap + 1) * (8 + 6 * 4 + 4 + 4)));
        c->nw_tab_cap = cap;
    }
    if (max_label) *max_label = mx;
    return NL_OK;
}

static inline int nw_t0(nl_ctx *c, char *err, size_t errlen) { NL_HIP(hipEventRecord(c->nw_ev[0], c->stream)); return NL_OK; }
static inline int nw_t1(nl_ctx *c, int which, char *err, size_t errlen) {
    NL_HIP(hipEventRecord(c->nw_ev[1], c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    float t = 0.f;
    NL_HIP(hipEventElapsedTime(&t, c->nw_ev[0], c->nw_ev[1]));
    c->nw_ms[which] += t;
    return NL_OK;
}

// Step 1 (networking.py:408): the frame goes up -- labels (int32), the thinning's mask (one byte per voxel, non-zero = skeleton) and the
// Frangi frame (float32) -- and skel = labels * mask is formed.  max_label (may be NULL) = the largest label.
extern "C" int nl_network_load(nl_ctx *c, const int32_t *labels, const uint8_t *skel_mask, const float *frangi, int ndim, int64_t *max_label,
                               char *err, size_t errlen) {
    NL_ENTER(c);
    NL_JOIN_SIDE(c);
    if (!labels || !skel_mask || !frangi) return nl_fail(err, errlen, NL_EINVAL, "nl_network_load: NULL labels, mask or frangi");
    if (int rc = nw_check(c, ndim, err, errlen)) return rc;
    if (int rc = nw_begin(c, err, errlen)) return rc;
    if (!c->nw_fr) NL_HIP(hipMalloc((void **)&c->nw_fr, (size_t)c->n * 4));
    if (!c->nw_mask) NL_HIP(hipMalloc((void **)&c->nw_mask, (size_t)c->n));
    c->nw_ndim = ndim;
    hipStream_t st = c->stream;
    NL_HIP(hipMemcpyAsync(c->nw_lab, labels, (size_t)c->n * 4, hipMemcpyHostToDevice, st));
    NL_HIP(hipMemcpyAsync(c->nw_mask, skel_mask, (size_t)c->n, hipMemcpyHostToDevice, st));
    NL_HIP(hipMemcpyAsync(c->nw_fr, frangi, (size_t)c->n * 4, hipMemcpyHostToDevice, st));
    int *d_stats = (int *)c->d_small + 8;
    NL_HIP(zero_small(d_stats, 8, st));
    nw_skel_kernel<<<grid1d(c->n, 256, 2048), 256, 0, st>>>(c->nw_lab, c->nw_mask, (int *)c->f[0], c->n, d_stats);
    NL_CHECK_LAUNCH();
    if (int rc = nw_labels_done(c, max_label, err, errlen)) return rc;
    c->nw_stage = 1;
    return NL_OK;
}

// Step 1 with the thinning on the device (networking.py:394-409): labels and the Frangi frame go up, the mask is the thinning of
// labels > 0 (thin.inc; 3-D frames only), then skel = labels * mask as above.  n_mask (may be NULL) = the mask's voxels.
extern "C" int nl_network_load_thin(nl_ctx *c, const int32_t *labels, const float *frangi, int ndim, int rounds_per_sync, int64_t *max_label,
                                    int64_t *n_mask, char *err, size_t errlen) {
    NL_ENTER(c);
    NL_JOIN_SIDE(c);
    if (!labels || !frangi) return nl_fail(err, errlen, NL_EINVAL, "nl_network_load_thin: NULL labels or frangi");
    if (ndim != 3) return nl_fail(err, errlen, NL_EINVAL, "the thinning on the device is the 3-D one: ndim = %d is not supported (thin 2-D frames on the host)", ndim);
    if (int rc = nw_check(c, ndim, err, errlen)) return rc;
    if (int rc = nw_begin(c, err, errlen)) return rc;
    if (!c->nw_fr) NL_HIP(hipMalloc((void **)&c->nw_fr, (size_t)c->n * 4));
    if (!c->nw_mask) NL_HIP(hipMalloc((void **)&c->nw_mask, (size_t)c->n));
    c->nw_ndim = ndim;
    hipStream_t st = c->stream;
    NL_HIP(hipMemcpyAsync(c->nw_lab, labels, (size_t)c->n * 4, hipMemcpyHostToDevice, st));
    NL_HIP(hipMemcpyAsync(c->nw_fr, frangi, (size_t)c->n * 4, hipMemcpyHostToDevice, st));
    if (int rc = thin_device(c, c->nw_lab, rounds_per_sync, err, errlen)) return rc;
    int *d_stats = (int *)c->d_small + 8;
    NL_HIP(zero_small(d_stats, 8, st));
    nw_skel_kernel<<<grid1d(c->n, 256, 2048), 256, 0, st>>>(c->nw_lab, c->nw_mask, (int *)c->f[0], c->n, d_stats);
    NL_CHECK_LAUNCH();
    if (int rc = nw_labels_done(c, max_label, err, errlen)) return rc;
    if (n_mask) *n_mask = c->thin_counts[1];
    c->nw_stage = 1;
    return NL_OK;
}

// Steps 2 and 3 (networking.py:261-296, :342-387).  n_removed: voxels the clean step zeroed; n_seeded: labels that got a voxel.
extern "C" int nl_network_clean_seed(nl_ctx *c, int64_t *n_removed, int64_t *n_seeded, char *err, size_t errlen) {
    NL_ENTER(c);
    if (c->nw_stage != 1) return nl_fail(err, errlen, NL_ESTATE, "nl_network_clean_seed needs nl_network_load first");
    hipStream_t st = c->stream;
    const NwGeom g = nw_geom(c);
    const unsigned grid = grid1d(c->n, 256, 8192);
    unsigned long long *d_cnt = (unsigned long long *)c->d_small;
    int *skel = (int *)c->f[3];
    NL_HIP(zero_small(d_cnt, 16, st));
    if (int rc = nw_t0(c, err, errlen)) return rc;
    nw_clean_kernel<<<grid, 256, 0, st>>>((const int *)c->f[0], skel, g, d_cnt);
    NL_CHECK_LAUNCH();
    if (int rc = nw_t1(c, 0, err, errlen)) return rc;
    const i64 nl = c->nw_max_label + 1;
    if (int rc = nw_t0(c, err, errlen)) return rc;
    if (c->nw_max_label > 0) {
        NL_HIP(hipMemsetAsync(nw_best(c), 0, (size_t)nl * 8, st));
        NL_HIP(hipMemsetAsync(nw_has(c), 0, (size_t)nl * 4, st));
        nw_has_kernel<<<grid, 256, 0, st>>>(skel, c->n, nw_has(c));
        nw_best_kernel<<<grid, 256, 0, st>>>(c->nw_lab, c->nw_fr, c->n, nw_has(c), nw_best(c));
        NL_CHECK_LAUNCH();
        nw_plant_kernel<<<(unsigned)((c->nw_max_label + 255) / 256), 256, 0, st>>>(nw_best(c), (int)c->nw_max_label, skel, d_cnt + 1);
        NL_CHECK_LAUNCH();
    }
    NL_HIP(hipMemcpyAsync(c->h_small, d_cnt, 16, hipMemcpyDeviceToHost, st));
    if (int rc = nw_t1(c, 1, err, errlen)) return rc;
    if (n_removed) *n_removed = (int64_t)((unsigned long long *)c->h_small)[0];
    if (n_seeded) *n_seeded = (int64_t)((unsigned long long *)c->h_small)[1];
    c->nw_stage = 2;
    return NL_OK;
}

// Step 4 (networking.py:839-847): the seeded skeleton carries its voxels' own labels, so it is skel_pre; classes and branch labels
// are nl_skel_pixel_class's and nl_skel_branch_labels' kernels on it, in place.
extern "C" int nl_network_classes(nl_ctx *c, int64_t *n_skel, int64_t *n_branches, char *err, size_t errlen) {
    NL_ENTER(c);
    if (c->nw_stage != 2) return nl_fail(err, errlen, NL_ESTATE, "nl_network_classes needs nl_network_clean_seed first");
    if (int rc = nw_t0(c, err, errlen)) return rc;
    if (int rc = nw_pixel_class_resident(c, nullptr, n_skel, err, errlen)) return rc;
    if (int rc = nl_skel_branch_labels(c, nullptr, nullptr, n_branches, err, errlen)) return rc;
    if (int rc = nw_t1(c, 2, err, errlen)) return rc;
    c->nw_has_classes = 1;
    c->nw_stage = 3;
    return NL_OK;
}

// Step 5 alone: labels and branch labels (int32, the frame's shape) go up and nl_network_relabel may follow.
extern "C" int nl_network_relabel_load(nl_ctx *c, const int32_t *labels, const int32_t *branch, int ndim, int64_t *max_label, char *err, size_t errlen) {
    NL_ENTER(c);
    NL_JOIN_SIDE(c);
    if (!labels || !branch) return nl_fail(err, errlen, NL_EINVAL, "nl_network_relabel_load: NULL labels or branch labels");
    if (int rc = nw_check(c, ndim, err, errlen)) return rc;
    if (int rc = nw_begin(c, err, errlen)) return rc;
    c->nw_ndim = ndim;
    hipStream_t st = c->stream;
    NL_HIP(hipMemcpyAsync(c->nw_lab, labels, (size_t)c->n * 4, hipMemcpyHostToDevice, st));
    NL_HIP(hipMemcpyAsync(c->f[3], branch, (size_t)c->n * 4, hipMemcpyHostToDevice, st));
    int *d_stats = (int *)c->d_small + 8;
    NL_HIP(zero_small(d_stats, 8, st));
    nw_minmax_kernel<<<grid1d(c->n, 256, 2048), 256, 0, st>>>(c->nw_lab, c->n, d_stats);
    NL_CHECK_LAUNCH();
    if (int rc = nw_labels_done(c, max_label, err, errlen)) return rc;
    c->nw_stage = 3;
    return NL_OK;
}

// Step 5 (networking.py:485-577).  spacing: ndim values, (Z, Y, X) or (Y, X).  scratch_voxels: box voxels one batch may hold (<= 0: half of
// the free HBM); never less than one frame, the largest box there is.  Objects are never split.  Outputs (may be NULL): objects with a
// seed, the sum of their box volumes, the batches run.
extern "C" int nl_network_relabel(nl_ctx *c, const double *spacing, int64_t scratch_voxels, int64_t *n_objects, int64_t *box_volume,
                                  int64_t *n_batches, char *err, size_t errlen) {
    NL_ENTER(c);
    if (c->nw_stage < 3) return nl_fail(err, errlen, NL_ESTATE, "nl_network_relabel needs nl_network_classes or nl_network_relabel_load first");
    if (!spacing) return nl_fail(err, errlen, NL_EINVAL, "spacing is NULL");
    NwGeom g = nw_geom(c);
    for (int a = 0; a < g.ndim; ++a) {
        const double s = spacing[a];
        if (!(s > 0.0) || !(s < 1e300)) return nl_fail(err, errlen, NL_EINVAL, "spacing must be positive and finite");
        g.s[3 - g.ndim + a] = s;
    }
    hipStream_t st = c->stream;
    const int *branch = (const int *)c->f[3];
    unsigned int *out = (unsigned int *)c->f[0];
    const i64 maxl = c->nw_max_label;
    if (n_objects) *n_objects = 0;
    if (box_volume) *box_volume = 0;
    if (n_batches) *n_batches = 0;
    c->nw_ms[3] = 0.f;
    if (int rc = nw_t0(c, err, errlen)) return rc;
    NL_HIP(hipMemsetAsync(out, 0, (size_t)c->n * 4, st));
    if (maxl == 0) { c->nw_stage = 4; return nw_t1(c, 3, err, errlen); }
    // boxes and seed flags per label
    const int wpr = (int)((c->nx + 63) / 64);
    nw_box_init_kernel<<<(unsigned)((maxl + 1 + 255) / 256), 256, 0, st>>>(nw_box(c), nw_seeded(c), (int)maxl);
    nw_box_kernel<<<grid1d((i64)g.nz * g.ny * wpr * 64, 256, (i64)1 << 20), 256, 0, st>>>(c->nw_lab, branch, g, wpr, nw_box(c), nw_seeded(c));
    NL_CHECK_LAUNCH();
    // Their sizes come to the host (28 bytes per label), which cuts the batches; the voxels stay where they are.
    std::vector<int> box((size_t)(maxl + 1) * 6), seeded((size_t)maxl + 1);
    NL_HIP(hipMemcpyAsync(box.data(), nw_box(c), box.size() * 4, hipMemcpyDeviceToHost, st));
    NL_HIP(hipMemcpyAsync(seeded.data(), nw_seeded(c), seeded.size() * 4, hipMemcpyDeviceToHost, st));
    NL_HIP(hipStreamSynchronize(st));
    i64 budget = scratch_voxels;
    if (budget <= 0) {
        size_t free_b = 0, total_b = 0;
        NL_HIP(hipMemGetInfo(&free_b, &total_b));
        budget = (i64)(free_b / 2 / 8) + c->nw_scr_cap;               // what the scratch already holds counts as free
    }
    budget = std::min(std::max(budget, c->n), NW_MAX_SCRATCH);
    std::vector<NwObj> objs;
    std::vector<i64> batch_first;                                    // index of each batch's first object, then objs.size()
    i64 used = 0, lines[3] = {0, 0, 0}, vol_sum = 0, largest = 0;
    for (i64 l = 1; l <= maxl; ++l) {
        const int *b = &box[(size_t)l * 6];
        if (!seeded[(size_t)l] || b[3] < 0) continue;
        NwObj o;
        o.label = (int)l; o.z0 = b[0]; o.y0 = b[1]; o.x0 = b[2];
        o.dz = b[3] - b[0] + 1; o.dy = b[4] - b[1] + 1; o.dx = b[5] - b[2] + 1; o.pad = 0;
        const i64 vol = (i64)o.dz * o.dy * o.dx;
        if (batch_first.empty() || used + vol > budget) {
            batch_first.push_back((i64)objs.size());
            largest = std::max(largest, used);
            used = 0; lines[0] = lines[1] = lines[2] = 0;
        }
        o.off = used;
        o.line0[0] = lines[0]; o.line0[1] = lines[1]; o.line0[2] = lines[2];
        used += vol; vol_sum += vol;
        lines[0] += (i64)o.dy * o.dx; lines[1] += (i64)o.dz * o.dx; lines[2] += (i64)o.dz * o.dy;
        objs.push_back(o);
    }
    largest = std::max(largest, used);
    if (!objs.empty()) {
        if (int rc = nw_grow(&c->nw_objs, &c->nw_objs_cap, (i64)objs.size(), sizeof(NwObj), st, err, errlen)) return rc;
        if (largest > c->nw_scr_cap) {
            NL_HIP(hipStreamSynchronize(st));
            if (c->nw_feat) { NL_HIP(hipFree(c->nw_feat)); c->nw_feat = nullptr; }
            if (c->nw_stk) { NL_HIP(hipFree(c->nw_stk)); c->nw_stk = nullptr; }
            c->nw_scr_cap = 0;
            NL_HIP(hipMalloc((void **)&c->nw_feat, (size_t)largest * 4));
            NL_HIP(hipMalloc((void **)&c->nw_stk, (size_t)largest * 4));
            c->nw_scr_cap = largest;
        }
        NL_HIP(hipMemcpyAsync(c->nw_objs, objs.data(), objs.size() * sizeof(NwObj), hipMemcpyHostToDevice, st));
        batch_first.push_back((i64)objs.size());
        for (size_t k = 0; k + 1 < batch_first.size(); ++k) {
            const NwObj *d = (const NwObj *)c->nw_objs + batch_first[k];
            const int nobj = (int)(batch_first[k + 1] - batch_first[k]);
            const NwObj &last = objs[(size_t)batch_first[k + 1] - 1];
            const i64 total = last.off + (i64)last.dz * last.dy * last.dx;
            const i64 nl0 = last.line0[0] + (i64)last.dy * last.dx, nl1 = last.line0[1] + (i64)last.dz * last.dx, nl2 = last.line0[2] + (i64)last.dz * last.dy;
            const auto blocks = [](i64 count) { return (unsigned)((count + 255) / 256); };
            nwr_init_kernel<<<blocks(total), 256, 0, st>>>(d, nobj, total, c->nw_lab, branch, g, c->nw_feat);
            if (g.ndim == 3) nwr_pass_kernel<0><<<blocks(nl0), 256, 0, st>>>(d, nobj, nl0, g, c->nw_feat, c->nw_stk);
            nwr_pass_kernel<1><<<blocks(nl1), 256, 0, st>>>(d, nobj, nl1, g, c->nw_feat, c->nw_stk);
            nwr_pass_kernel<2><<<blocks(nl2), 256, 0, st>>>(d, nobj, nl2, g, c->nw_feat, c->nw_stk);
            nwr_gather_kernel<<<blocks(total), 256, 0, st>>>(d, nobj, total, c->nw_lab, branch, g, c->nw_feat, out);
            NL_CHECK_LAUNCH();
        }
    }
    if (int rc = nw_t1(c, 3, err, errlen)) return rc;           // (waits for the stream: `objs` may go)
    if (n_objects) *n_objects = (int64_t)objs.size();
    if (box_volume) *box_volume = vol_sum;
    if (n_batches) *n_batches = objs.empty() ? 0 : (int64_t)batch_first.size() - 1;
    c->nw_stage = 4;
    return NL_OK;
}

// The products, each may be NULL: the branch skeleton labels (int32), the pixel classes (uint8; not after nl_network_relabel_load) and
// the relabelled volume (uint32; after nl_network_relabel).
extern "C" int nl_network_fetch(nl_ctx *c, int32_t *branch, uint8_t *pixel_class, uint32_t *relabelled, char *err, size_t errlen) {
    NL_ENTER(c);
    if (c->nw_stage < 3) return nl_fail(err, errlen, NL_ESTATE, "nl_network_fetch before the classes of this frame");
    if (pixel_class && !c->nw_has_classes) return nl_fail(err, errlen, NL_ESTATE, "no pixel classes on the device: the frame came through nl_network_relabel_load");
    if (relabelled && c->nw_stage < 4) return nl_fail(err, errlen, NL_ESTATE, "nl_network_fetch(relabelled) before nl_network_relabel");
    hipStream_t st = c->stream;
    if (branch) NL_HIP(hipMemcpyAsync(branch, c->f[3], (size_t)c->n * 4, hipMemcpyDeviceToHost, st));
    if (pixel_class) NL_HIP(hipMemcpyAsync(pixel_class, c->f[2], (size_t)c->n, hipMemcpyDeviceToHost, st));
    if (relabelled) NL_HIP(hipMemcpyAsync(relabelled, c->f[0], (size_t)c->n * 4, hipMemcpyDeviceToHost, st));
    NL_HIP(hipStreamSynchronize(st));
    return NL_OK;
}

// Device time (ms) of the steps of the current frame: ms[0] clean, [1] seed, [2] classes, [3] relabel; transfers excluded.
extern "C" int nl_network_kernel_ms(nl_ctx *c, float *ms, char *err, size_t errlen) {
    if (!c || !ms) return nl_fail(err, errlen, NL_EINVAL, "ctx or ms is NULL");
    for (int k = 0; k < 4; ++k) ms[k] = c->nw_ms[k];
    return NL_OK;
}
