// Part of libnellie_hip.so (gfx950): the Hessian walk of a scale on the host side -- the divisors and their proof, the launch plan
// (walk_plan.h) and its one launcher, the resolve kernel's launch and its deferral, and the entry points nl_hessian_stats,
// nl_vesselness_spec / _resolve / _count / _step.  The device chain (nellie_hip.hip) enqueues its walks through spec_enqueue and
// resolve_enqueue.  The one-voxel kernel and the resolve kernel are compiled here, with the library's default flags; the pair kernel and
// the wave-autonomous kernel behind nl_hv_launch (nellie_hv.hip).  C-ABI in include/nellie_amd.h.
#include "nl_host.h"

#include "walk_common.h"
#include "hessian.inc"
#include "resolve.inc"
#include "walk_plan.h"

// The walk's switches, read in this one place.  Once per process, but the two that tests switch inside one process.
static WalkSwitches walk_switches_env() {
    auto num = [](const char *name, long long unset) { const char *e = getenv(name); return e ? atoll(e) : unset; };
    static const WalkSwitches once = walk_switches(num("NELLIE_HV_RS", 8), 1, 0, num("NELLIE_HM_TY", 8), num("NELLIE_HV_ZCHUNK", 0), num("NELLIE_VQ_CAP", 0),
                                                   num("NELLIE_SPEC_MAX_GB", 64));
    WalkSwitches s = once;
    s.np = walk_switches(8, num("NELLIE_HV_NP", 1), 0, 8, 0, 0, 0).np;
    s.dpp = num("NELLIE_HV_DPP", 0) == 1;
    return s;
}
VqAlloc vq_alloc(int64_t nzl, int64_t ny, int64_t nx) { return vq_alloc(walk_switches_env(), nzl, ny, nx); }
int64_t vq_alloc_entries(int64_t nzl, int64_t ny, int64_t nx) { return vq_alloc(nzl, ny, nx).entries; }
WalkPlan walk_plan(const nl_ctx *c, int mode, int64_t z0, int64_t z1) {
    const WalkSwitches sw = walk_switches_env();
    return walk_plan(sw, vq_alloc(sw, c->nzl, c->ny, c->nx), mode, c->ny, c->nx, c->own_lo, c->own_hi, z0, z1, c->fast_div, c->fast_div2);
}

// Host only (no context, no device): the plan as thirteen integers -- family, tile rows, rs, np, division form, planes per workgroup, ntx,
// nty, Z chunks, grid, regions per launch, qcap, planes per launch.
extern "C" int nl_host_walk_plan(int mode, int64_t nzl, int64_t ny, int64_t nx, int64_t own_lo, int64_t own_hi, int64_t z0, int64_t z1, int fast_div,
                                 int fast_div2, const int64_t switches[7], int64_t plan[13], char *err, size_t errlen) {
    if (!switches || !plan) return nl_fail(err, errlen, NL_EINVAL, "switches or plan is NULL");
    if (mode < 0 || mode > 2 || nzl < 1 || ny < 1 || nx < 1) return nl_fail(err, errlen, NL_EINVAL, "bad mode or geometry");
    if (own_lo < 0 || own_hi > nzl || own_lo >= own_hi) return nl_fail(err, errlen, NL_EINVAL, "bad owned range [%lld,%lld)", (i64)own_lo, (i64)own_hi);
    if (mode == 0) { z0 = own_lo; z1 = own_hi; }
    if (z0 < 0 || z1 > nzl || z0 >= z1) return nl_fail(err, errlen, NL_EINVAL, "bad plane range [%lld,%lld)", (i64)z0, (i64)z1);
    const WalkSwitches sw = walk_switches(switches[0], switches[1], switches[2], switches[3], switches[4], switches[5], switches[6]);
    const WalkPlan p = walk_plan(sw, vq_alloc(sw, nzl, ny, nx), mode, ny, nx, own_lo, own_hi, z0, z1, fast_div, fast_div2);
    const int64_t v[13] = {p.family, p.ty, p.rs, p.np, p.fastv, p.zchunk, p.ntx, p.nty, p.nzc, p.grid, p.nregions, p.qcap, p.launch_planes};
    memcpy(plan, v, sizeof(v));
    return NL_OK;
}

// ---- the one launcher ------------------------------------------------------------------------------------------------------------
// The one-voxel kernel: MODE 0-2 x tile rows 8, 16 x {three-instruction division, float64 division}
template <int MODE, int TY, bool FAST>
static void launch_g(const HvLaunch &a, const HessDv<FAST> &hr) {
    hessian_g_kernel<MODE, TY, FAST><<<a.nblocks, HGCfg<TY>::NT, HGCfg<TY>::lds_bytes(), a.stream>>>(
        a.g, a.cmask, a.pmask, a.wpr, a.geom, hr, a.vp, a.vq, a.z0, a.z1, a.ntx, a.nty, a.res, a.d_cnt);
}
template <int MODE, int TY>
static void launch_g_div(const HvLaunch &a) {
    if (a.fastv) launch_g<MODE, TY, true>(a, hessdv_fast(a.hp)); else launch_g<MODE, TY, false>(a, hessdv_exact(a.hp));
}
template <int MODE>
static void launch_g_ty(const HvLaunch &a, int ty) {
    if (ty == 8) launch_g_div<MODE, 8>(a); else launch_g_div<MODE, 16>(a);
}
// The planes [za, zb) of a scale in `mode`, enqueued by the kernel family the plan names: statistics into res, the h_mask count of the decided
// voxels into *d_cnt, queue entries by the plan's regions (*nregions of them).  dev_lohi: spec_enqueue.
static int walk_launch(nl_ctx *c, const WalkPlan &p, int mode, VessP vp, const MaskSlots &ms, i64 za, i64 zb, unsigned int *res, unsigned long long *d_cnt,
                       const float *dev_lohi, unsigned *nregions, char *err, size_t errlen) {
    vp.qcap = p.qcap;
    if (mode == 2) vp.zchunk = p.zchunk;
    const unsigned grid = walk_grid(p, zb - za);
    const HvLaunch a{mode, p.rs, p.np, p.fastv, grid, c->stream, gauss_cur(c), ms.cm, ms.pm, ms.wpr, geom(c), hessp(c), vp,
                     mode ? VQueue{(float4 *)c->d_vq, c->d_vq_count} : VQueue{}, (int)za, (int)zb, p.ntx, p.nty, res, d_cnt, dev_lohi};
    if (p.family == WALK_WAVE)     // the strips OR their bits into the words (two strips share a word): the slot's planes start from zero
        NL_HIP(hipMemsetAsync(ms.cm + za * c->ny * ms.wpr, 0, (size_t)(zb - za) * c->ny * ms.wpr * 8, c->stream));
    if (p.family != WALK_ONE_VOXEL) NL_HIP(nl_hv_launch(a));
    else if (mode == 0) launch_g_ty<0>(a, p.ty);
    else if (mode == 1) launch_g_ty<1>(a, p.ty);
    else launch_g_ty<2>(a, p.ty);
    NL_CHECK_LAUNCH();
    if (nregions) *nregions = grid * (unsigned)p.regions_per_group;
    return NL_OK;
}

// grid of the queue kernels: NELLIE_RESOLVE_GRID caps it (waves then walk several regions each).  Measured at 512 x 1024 x 1024
// (ms/step of the resolve group): 1792 workgroups 2.77, 2048 2.69, 4096 2.67, 8192 2.79, 16384 (rounds 1-2) and more 3.16 --
// a wave that walks 8-16 regions amortises its start-up and evens out the regions' very different entry counts
static unsigned resolve_grid(unsigned blocks) {
    static long cap = -1;
    if (cap < 0) { const char *e = getenv("NELLIE_RESOLVE_GRID"); cap = e ? atol(e) : 8192; }
    return (cap > 0 && (unsigned)cap < blocks) ? (unsigned)cap : blocks;
}
// Exhaustive proof that the 3-instruction division is exact for the six divisors in use.
static int check_fast_div(nl_ctx *c, char *err, size_t errlen) {
    const float ds[6] = {c->hz, c->hy, c->hx, c->hz2, c->hy2, c->hx2};
    unsigned int *bad = (unsigned int *)c->d_small + 64;
    NL_HIP(zero_small(bad, 12 * 4, c->stream));
    for (int k = 0; k < 6; ++k) {
        divcheck_kernel<1><<<(1u << 23) / 256, 256, 0, c->stream>>>(dv_fast(ds[k]), ds[k], bad + k);
        divcheck_kernel<2><<<(1u << 23) / 256, 256, 0, c->stream>>>(dv_two(ds[k]), ds[k], bad + 6 + k);
    }
    NL_CHECK_LAUNCH();
    unsigned int *h = (unsigned int *)c->h_small + 64;
    NL_HIP(hipMemcpyAsync(h, bad, 12 * 4, hipMemcpyDeviceToHost, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    c->fast_div = 1; c->fast_div2 = 1;
    for (int k = 0; k < 6; ++k) {
        const bool normal = ds[k] > 1e-30f && ds[k] < 1e30f;
        if (h[k] || !normal) c->fast_div = 0;
        if (h[6 + k] || !normal) c->fast_div2 = 0;
    }
    // NELLIE_EXACT_DIV=1: the float64 path everywhere; =3: at most the three-instruction sequence (A/B of the two-instruction one)
    const char *e = getenv("NELLIE_EXACT_DIV");
    if (e && atoi(e) == 1) { c->fast_div = 0; c->fast_div2 = 0; }
    if (e && atoi(e) == 3) c->fast_div2 = 0;
    return NL_OK;
}

int set_spacing(nl_ctx *c, const double spacing[3], char *err, size_t errlen) {
    if (!spacing) return nl_fail(err, errlen, NL_EINVAL, "spacing is NULL");
    if ((!c->two_d && c->gnz < 2) || c->ny < 2 || c->nx < 2)
        return nl_fail(err, errlen, NL_EINVAL, "Shape of array too small to calculate a numerical gradient, at least (edge_order + 1) elements are required.");
    if (c->chk_spacing[0] != spacing[0] || c->chk_spacing[1] != spacing[1] || c->chk_spacing[2] != spacing[2]) c->fsq_cache_valid = 0;
    c->hz = (float)spacing[0]; c->hy = (float)spacing[1]; c->hx = (float)spacing[2];
    c->hz2 = (float)(2.0 * spacing[0]); c->hy2 = (float)(2.0 * spacing[1]); c->hx2 = (float)(2.0 * spacing[2]);
    if (!c->have_spacing || c->chk_spacing[0] != spacing[0] || c->chk_spacing[1] != spacing[1] || c->chk_spacing[2] != spacing[2]) {
        int rcx = check_fast_div(c, err, errlen);
        if (rcx) return rcx;
        c->chk_spacing[0] = spacing[0]; c->chk_spacing[1] = spacing[1]; c->chk_spacing[2] = spacing[2];
    }
    c->have_spacing = 1;
    return NL_OK;
}

extern "C" int nl_set_spacing(nl_ctx *c, const double spacing[3], char *err, size_t errlen) {
    NL_ENTER(c);
    return set_spacing(c, spacing, err, errlen);
}

extern "C" int nl_hessian_stats(nl_ctx *c, const double spacing[3], float *max_abs, float *max_frob_sq, int *any_inf,
                                char *err, size_t errlen) {
    NL_ENTER(c);
    { int rcs = set_spacing(c, spacing, err, errlen); if (rcs) return rcs; }
    c->spec_valid = 0;
    unsigned int *res = (unsigned int *)c->d_small;
    NL_HIP(zero_small(res, 16, c->stream));
    if (c->two_d) {
        int rc2 = hessian2d_stats_enqueue(c, res, err, errlen);
        if (rc2) return rc2;
    } else {
        ProfScope ps(c, "hessian_stats");
        int rcl = walk_launch(c, walk_plan(c, 0, c->own_lo, c->own_hi), 0, VessP{}, MaskSlots{nullptr, nullptr, 0}, c->own_lo, c->own_hi, res, nullptr, nullptr,
                              nullptr, err, errlen);
        if (rcl) return rcl;
    }
    unsigned int *h = (unsigned int *)c->h_small;
    NL_HIP(hipMemcpyAsync(h, res, 16, hipMemcpyDeviceToHost, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    if (max_abs) memcpy(max_abs, &h[0], 4);
    if (max_frob_sq) memcpy(max_frob_sq, &h[1], 4);
    if (any_inf) *any_inf = (int)h[2];
    return NL_OK;
}

extern "C" int nl_set_frob_norm(nl_ctx *c, float max_abs, float max_finite, char *err, size_t errlen) {
    if (!c) return nl_fail(err, errlen, NL_EINVAL, "ctx is NULL");
    c->frob_max_abs = max_abs; c->frob_max_finite = max_finite;
    return NL_OK;
}

// h_mask = sqrt(frob_sq)/max_abs > thr (or > 0).  sqrt and the division by a positive constant are monotone, so the
// mask is exactly {frob_sq >= x_min} for the smallest float32 x_min whose image passes the test; it is found by
// bisection over the (ordered) bit patterns of the non-negative floats, with the same two IEEE operations the
// volume op would do.  The kernel then needs one compare per voxel instead of a square root and a division.
float mask_threshold_on_fsq(float max_abs, int use_thr, float thr) {
    auto pred = [&](float x) -> bool {
        volatile float fr = sqrtf(x);
        fr = fr / max_abs;
        return use_thr ? (fr > thr) : (fr > 0.0f);
    };
    unsigned int lo = 0u, hi = 0x7f800000u;          // hi = +inf bits: "nothing finite passes"
    float fmaxv; { unsigned int b = 0x7f7fffffu; memcpy(&fmaxv, &b, 4); }
    if (!pred(fmaxv)) { float inf; memcpy(&inf, &hi, 4); return inf; }
    hi = 0x7f7fffffu;
    while (lo < hi) {                                 // smallest pattern with pred true
        const unsigned int mid = lo + (hi - lo) / 2;
        float x; memcpy(&x, &mid, 4);
        if (pred(x)) hi = mid; else lo = mid + 1;
    }
    float r; memcpy(&r, &lo, 4);
    return r;
}

static VessP make_vessp(nl_ctx *c, float gamma_sq, float alpha_sq, float beta_sq, int use_thr, float thr) {
    VessP vp{};
    vp.gamma_sq = gamma_sq; vp.alpha_sq = alpha_sq; vp.beta_sq = beta_sq; vp.use_thr = use_thr; vp.thr = thr;
    vp.max_abs = c->frob_max_abs; vp.max_finite = c->frob_max_finite;
    vp.cnt_lo = (int)c->own_lo; vp.cnt_hi = (int)c->own_hi;
    vp.first = c->mask_slots_used == 0 ? 1 : 0;
    vp.fsq_min = mask_threshold_on_fsq(c->frob_max_abs, use_thr, thr);
    vp.m_inf = use_thr ? (c->frob_max_finite > thr) : (c->frob_max_finite > 0.0f);
    vp.all_ones = (use_thr && thr == -INFINITY) ? 1 : 0;       // the host's way of saying mask=False (pipeline.py: thr_cmp = -inf)
    vp.nan_flag = (unsigned int *)((char *)c->d_small + NL_NAN_FLAG_OFF);
    c->last_fsq_min = vp.fsq_min;
    return vp;
}

// The walk of a scale in MODE 2, enqueued: statistics into res[0..3] (all "max": bit patterns of non-negative floats, flags),
// h_mask count of the decided voxels into *d_cnt (both zeroed by the caller).  dev_lohi != NULL: the bracket is read from device
// memory by the kernel (chain.inc) and fsq_lo / fsq_hi are ignored.
int spec_enqueue(nl_ctx *c, const double spacing[3], float fsq_lo, float fsq_hi, int64_t z0, int64_t z1, unsigned int *res,
                        unsigned long long *d_cnt, const float *dev_lohi, char *err, size_t errlen) {
    if (z0 < 0 && z1 < 0) { z0 = c->own_lo; z1 = c->own_hi; }
    if (z0 < 0 || z1 > c->nzl || z0 >= z1) return nl_fail(err, errlen, NL_EINVAL, "bad plane range [%lld,%lld)", (i64)z0, (i64)z1);
    if (z0 > c->own_lo || z1 < c->own_hi) return nl_fail(err, errlen, NL_EINVAL, "the plane range must cover the owned planes");
    NL_JOIN_SIDE(c);
    if (!c->spec_ok) return nl_fail(err, errlen, NL_ESTATE, "one-pass vesselness is not available for this context (queue too large)");
    if (!dev_lohi && !(fsq_lo <= fsq_hi)) return nl_fail(err, errlen, NL_EINVAL, "empty bracket [%g,%g]", (double)fsq_lo, (double)fsq_hi);
    { int rcs = set_spacing(c, spacing, err, errlen); if (rcs) return rcs; }
    VessP vp{};
    vp.cnt_lo = (int)c->own_lo; vp.cnt_hi = (int)c->own_hi;
    vp.have_prev = c->mask_slots_used > 0;
    vp.fsq_lo = fsq_lo; vp.fsq_hi = fsq_hi;
    {
        ProfScope ps(c, "vesselness");
        const WalkPlan p = walk_plan(c, 2, z0, z1);
        if (dev_lohi && p.family == WALK_ONE_VOXEL) return nl_fail(err, errlen, NL_ESTATE, "the device-resident chain needs the two-voxel walk");
        // (the scale's slot is committed by nl_vesselness_resolve)
        int rcl = walk_launch(c, p, 2, vp, mask_slots(c, c->mask_slots_used), z0, z1, res, d_cnt, dev_lohi, &c->spec_nregions, err, errlen);
        if (rcl) return rcl;
        c->spec_qcap = p.qcap;
    }
    // fused: max |H|, max frob_sq (bit patterns of non-negative floats), the inf and overflow flags -- all "max"; the count stays local
    if (fused(c)) { int rcr = reduce_u32_max(c, res, 4, err, errlen); if (rcr) return rcr; }
    c->spec_z0 = z0; c->spec_z1 = z1;
    return NL_OK;
}

// ---- one-pass vesselness (MODE 2 of the Hessian kernel + the resolve kernel), see hessian.inc ---------------
extern "C" int nl_vesselness_spec(nl_ctx *c, const double spacing[3], float fsq_lo, float fsq_hi, int64_t z0, int64_t z1,
                                  float *max_abs, float *max_frob_sq, int *any_inf, int *overflow, char *err, size_t errlen) {
    NL_ENTER(c);
    unsigned long long *d_cnt = (unsigned long long *)c->d_small;
    unsigned int *res = (unsigned int *)c->d_small + 16;
    NL_HIP(zero_small(c->d_small, 128, c->stream));
    { int rc = spec_enqueue(c, spacing, fsq_lo, fsq_hi, z0, z1, res, d_cnt, nullptr, err, errlen); if (rc) return rc; }
    unsigned int *h = (unsigned int *)c->h_small;
    NL_HIP(hipMemcpyAsync(h, c->d_small, 128, hipMemcpyDeviceToHost, c->stream));      // [0] count, [16..19] statistics
    NL_HIP(hipStreamSynchronize(c->stream));
    c->spec_count = *(unsigned long long *)c->h_small;       // d_small is scratch for the sampling calls in between
    h += 16;
    if (max_abs) memcpy(max_abs, &h[0], 4);
    if (max_frob_sq) memcpy(max_frob_sq, &h[1], 4);
    if (any_inf) *any_inf = (int)h[2];
    if (overflow) *overflow = (int)h[3];
    c->spec_lo = fsq_lo; c->spec_hi = fsq_hi;
    c->spec_valid = (h[2] == 0 && h[3] == 0) ? 1 : 0;
    c->last_spec_overflow = (int)h[3];
    return NL_OK;
}

// The resolve kernel runs on the MAIN stream by default (round 4): since the two-voxel walk and the cheaper resolve kernel,
// running it beside the next scale's Gaussian buys nothing (48.8 vs 49.0 ms/step at 1024^3: the Z pass slows from 1.77 to 2.55 ms
// per launch while it shares the GPU) -- and sending it to the side stream only to make the main stream wait for it cost two
// cross-queue dependencies of ~13 us per scale (0.13 ms of a 3.3 ms config-5 frame).  NELLIE_RESOLVE_OVERLAP=1: the side stream,
// beside the next cascade step (every entry point that needs its result joins it: NL_JOIN_SIDE).
static bool resolve_on_side() {
    static int overlap = -1;
    if (overlap < 0) { const char *e = getenv("NELLIE_RESOLVE_OVERLAP"); overlap = (e && atoi(e)) ? 1 : 0; }
    return overlap != 0;
}
// h_mask count of the scale completed by the last nl_vesselness_resolve hit (waits for its kernel).
extern "C" int nl_vesselness_count(nl_ctx *c, int64_t *mask_count, char *err, size_t errlen) {
    NL_ENTER(c);
    if (!mask_count) return nl_fail(err, errlen, NL_EINVAL, "mask_count is NULL");
    unsigned long long *d_cnt = (unsigned long long *)((char *)c->d_small + (48 << 10));
    unsigned long long *h_cnt = (unsigned long long *)((char *)c->h_small + (48 << 10));
    hipStream_t st = resolve_on_side() ? c->side : c->stream;        // the stream the resolve kernel ran on
    NL_HIP(hipMemcpyAsync(h_cnt, d_cnt, 8, hipMemcpyDeviceToHost, st));
    NL_HIP(hipStreamSynchronize(st));
    *mask_count = (int64_t)(*h_cnt + c->spec_count);
    return NL_OK;
}

// The resolve kernel of a scale, enqueued on the side stream (ordered after everything submitted to the main stream so far);
// commits the scale's mask slot.  dev_params != NULL: gamma_sq, fsq_min and m_inf are read from device memory (chain.inc).
int resolve_enqueue(nl_ctx *c, VessP vp, unsigned long long *d_cnt, const float *dev_params, char *err, size_t errlen, bool force_side) {
    const i64 plane = c->ny * c->nx, z0 = c->spec_z0, z1 = c->spec_z1;
    const bool side = force_side || resolve_on_side();
    hipStream_t st = side ? c->side : c->stream;
    if (side) {
        NL_HIP(hipEventRecord(c->ev_main, c->stream));
        NL_HIP(hipStreamWaitEvent(c->side, c->ev_main, 0));
    }
    vp.qcap = c->spec_qcap;
    vp.idx_lo = (c->own_lo - z0) * plane; vp.idx_hi = (c->own_hi - z0) * plane;
    {
        ProfScope ps(c, "vesselness_resolve", st);
        const int k_scale = c->mask_slots_used++;
        vp.have_prev = k_scale > 0;
        const MaskSlots ms = mask_slots(c, k_scale);
        if (vp.first && !vmax_is_zero(c, z0, z1))
            NL_HIP(hipMemsetAsync(c->f[c->i_vmax] + z0 * plane, 0, (size_t)(z1 - z0) * plane * 4, st));
        c->vmax_zero_hi = 0;
        vesselness_queue_kernel<true><<<resolve_grid((c->spec_nregions + 3) / 4), 256, 0, st>>>(
            (const float4 *)c->d_vq, c->d_vq_count, c->spec_nregions, c->f[c->i_vmax], z0 * plane, vp, ms.cm, ms.pm, ms.wpr, (int)c->ny, (int)c->nx, z0, d_cnt,
            dev_params);
        NL_CHECK_LAUNCH();
    }
    if (side) {
        NL_HIP(hipEventRecord(c->ev_side, c->side));
        c->side_pending = 1;
    }
    c->spec_valid = 0;
    return NL_OK;
}

// Device chain (round 5, second session): the resolve kernel of scale s needs nothing the cascade step of scale s+1 touches, and the ten
// threshold kernels of scale s+1 (one wave or a 10^6-point lattice each: ~0.15 ms of a nearly idle GPU) need nothing the resolve kernel
// writes.  So nl_chain_scale(s) only NOTES the resolve launch; nl_chain_scale(s+1) -- called after the host has enqueued cascade step
// s+1 -- starts it on the side stream behind that step, and the threshold kernels run beside it on the main stream; the walk of scale
// s+1 joins (spec_enqueue: NL_JOIN_SIDE).  Beside the cascade step itself the resolve kernel only costs (both are bound by the float64
// pipe: NELLIE_RESOLVE_OVERLAP, profiles/r05_walk_variants_1024cube.txt).  Single context, volumes of 2^26 voxels and more (below, the
// side stream carries the cascade step that runs ahead); NELLIE_RESOLVE_DEFER=0: off.
bool resolve_defer_ok(const nl_ctx *c) {
    const char *e = getenv("NELLIE_RESOLVE_DEFER");               // read per call: tests switch it (2: whatever the size, for the small volumes of the suite)
    const int on = e ? atoi(e) : 1;
    if (on == 2) return !c->comm && !resolve_on_side();
    return on && !c->comm && !c->ahead_pending && !resolve_on_side() && c->n >= ((i64)1 << 26);
}
int resolve_deferred_launch(nl_ctx *c, bool on_side, char *err, size_t errlen) {
    if (!c->def_resolve) return NL_OK;
    c->def_resolve = 0;
    NL_JOIN_SIDE(c);          // the exact round of that scale ran on the side stream: whatever the main stream does next comes after it
    VessP vp;
    static_assert(sizeof(VessP) <= sizeof(((nl_ctx *)nullptr)->def_vp), "nl_ctx::def_vp holds a VessP");
    memcpy(&vp, c->def_vp, sizeof(VessP));
    return resolve_enqueue(c, vp, c->def_cnt, c->def_params, err, errlen, on_side);
}

// *hit = 1: the exact threshold lies in the bracket of the pass, the scale is complete (mask_count as
// nl_vesselness_step reports it); *hit = 0: nothing was changed, run nl_vesselness_step.
extern "C" int nl_vesselness_resolve(nl_ctx *c, float gamma_sq, float alpha_sq, float beta_sq, int use_thr, float thr,
                                     int *hit, int64_t *mask_count, char *err, size_t errlen) {
    NL_ENTER(c);
    if (!hit) return nl_fail(err, errlen, NL_EINVAL, "hit is NULL");
    *hit = 0;
    if (!c->spec_valid) return NL_OK;
    VessP vp = make_vessp(c, gamma_sq, alpha_sq, beta_sq, use_thr, thr);
    if (!(vp.fsq_min >= c->spec_lo && vp.fsq_min <= c->spec_hi)) { c->spec_valid = 0; return NL_OK; }
    // The kernel's counter lives outside the sampling scratch.
    unsigned long long *d_cnt = (unsigned long long *)((char *)c->d_small + (48 << 10));
    if (resolve_on_side()) {
        NL_HIP(hipEventRecord(c->ev_main, c->stream));
        NL_HIP(hipStreamWaitEvent(c->side, c->ev_main, 0));
        NL_HIP(zero_small(d_cnt, 8, c->side));
    } else {
        NL_HIP(zero_small(d_cnt, 8, c->stream));
    }
    { int rc = resolve_enqueue(c, vp, d_cnt, nullptr, err, errlen); if (rc) return rc; }
    *hit = 1;
    if (mask_count) {        // asking for the count here waits for the kernel; nl_vesselness_count can be called later instead
        int rcc = nl_vesselness_count(c, mask_count, err, errlen);
        if (rcc) return rcc;
    }
    return NL_OK;
}

extern "C" int nl_vesselness_step(nl_ctx *c, float gamma_sq, float alpha_sq, float beta_sq, int use_thr, float thr,
                                  int64_t z0, int64_t z1, int64_t *mask_count, char *err, size_t errlen) {
    NL_ENTER(c);
    if (z0 < 0 && z1 < 0) { z0 = c->own_lo; z1 = c->own_hi; }
    if (z0 < 0 || z1 > c->nzl || z0 >= z1) return nl_fail(err, errlen, NL_EINVAL, "bad plane range [%lld,%lld)", (i64)z0, (i64)z1);
    if (!c->have_spacing) return nl_fail(err, errlen, NL_ESTATE, "nl_vesselness_step before nl_hessian_stats");
    NL_JOIN_SIDE(c);
    unsigned long long *d_cnt = (unsigned long long *)c->d_small;
    NL_HIP(zero_small(d_cnt, 8, c->stream));
    VessP vp = make_vessp(c, gamma_sq, alpha_sq, beta_sq, use_thr, thr);
    c->spec_valid = 0;
    if (c->two_d) {
        int rc2 = vesselness2d_enqueue(c, vp, d_cnt, nullptr, err, errlen);
        if (rc2) return rc2;
    } else {
        ProfScope ps(c, "vesselness");
        // cumulative h_mask (AND over the scales so far): scale k reads slot (k-1)&1 and writes slot k&1
        const int k_scale = c->mask_slots_used++;
        vp.have_prev = k_scale > 0;
        const MaskSlots ms = mask_slots(c, k_scale);
        const i64 plane = c->ny * c->nx;
        if (vp.first && !vmax_is_zero(c, z0, z1))      // vesselness = zeros (filtering.py:807); only voxels alive in every mask are ever read again
            NL_HIP(hipMemsetAsync(c->f[c->i_vmax] + z0 * plane, 0, (size_t)(z1 - z0) * plane * 4, c->stream));
        c->vmax_zero_hi = 0;
        // one launch covers as many Z chunks as the queue has regions for
        const WalkPlan p = walk_plan(c, 1, z0, z1);
        vp.qcap = p.qcap;
        for (i64 za = z0; za < z1; za += p.launch_planes) {
            const i64 zb = za + p.launch_planes < z1 ? za + p.launch_planes : z1;
            unsigned nregions = 0;
            int rcl = walk_launch(c, p, 1, vp, ms, za, zb, nullptr, d_cnt, nullptr, &nregions, err, errlen);
            if (rcl) return rcl;
            vesselness_queue_kernel<false><<<resolve_grid((nregions + 3) / 4), 256, 0, c->stream>>>((float4 *)c->d_vq, c->d_vq_count, nregions, c->f[c->i_vmax],
                                                                                      za * plane, vp, nullptr, nullptr, ms.wpr, (int)c->ny, (int)c->nx, za, nullptr, nullptr);
            NL_CHECK_LAUNCH();
        }
    }
    if (mask_count) {
        NL_HIP(hipMemcpyAsync(c->h_small, d_cnt, 8, hipMemcpyDeviceToHost, c->stream));
        NL_HIP(hipStreamSynchronize(c->stream));
        *mask_count = (int64_t)(*(unsigned long long *)c->h_small);
    }
    return NL_OK;
}

// debug / known-answer kernel: eigenvalues (sorted by |.|) and Frangi response of explicit Hessians
static __global__ void __launch_bounds__(256)
debug_eig_kernel(const float *__restrict__ h6, i64 n, int impl, float alpha_sq, float beta_sq, float gamma_sq,
                 float *__restrict__ out4) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float h[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) h[k] = h6[i * 6 + k];
    float l1, l2, l3;
    if (impl == 0) eig3_sorted_abs(h, l1, l2, l3); else eig3_sorted_abs_libm(h, l1, l2, l3);
    out4[i * 4 + 0] = l1; out4[i * 4 + 1] = l2; out4[i * 4 + 2] = l3;
    out4[i * 4 + 3] = frangi3(l1, l2, l3, alpha_sq, beta_sq, gamma_sq);
}
extern "C" int nl_debug_eig_frangi(nl_ctx *c, const float *h6, int64_t n, int impl, float alpha_sq, float beta_sq,
                                   float gamma_sq, float *out4, char *err, size_t errlen) {
    NL_ENTER(c);
    if (!h6 || !out4 || n < 1 || n * 6 > c->n) return nl_fail(err, errlen, NL_EINVAL, "bad debug batch (n=%lld)", (i64)n);
    float *d_in = c->f[(c->i_gauss + 1) % 3], *d_out = c->f[(c->i_gauss + 2) % 3];
    NL_HIP(hipMemcpyAsync(d_in, h6, (size_t)n * 24, hipMemcpyHostToDevice, c->stream));
    debug_eig_kernel<<<(unsigned)((n + 255) / 256), 256, 0, c->stream>>>(d_in, n, impl, alpha_sq, beta_sq, gamma_sq, d_out);
    NL_CHECK_LAUNCH();
    NL_HIP(hipMemcpyAsync(out4, d_out, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream));
    NL_HIP(hipStreamSynchronize(c->stream));
    return NL_OK;
}

