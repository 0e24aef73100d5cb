// Part of libnellie_hip.so (gfx950).  The launch plan of the Hessian walk: which of the three kernel families runs (the one-voxel kernel of
// hessian.inc, the pair kernel of hessian_pair.inc, the wave-autonomous kernel of hessian_dpp.inc), its tiles, its grid and how the eigen
// queue is shared out among its waves -- and the queue's allocation, which is the same geometry.  Every launch site of nellie_walk.hip, the
// resolve kernel's region count and nl_ctx_info("queue_entries") take these numbers from here.  Plain host arithmetic: no HIP call, no
// device, no environment (nl_host_walk_plan evaluates it on any machine; tests/test_walk_plan_cpu.py pins it).  After walk_common.h.
#pragma once
#include <stdint.h>
#include "hv_launch.h"       // NL_HV_VARIANTS

// strips of the wave-autonomous walk (hessian_dpp.inc): 4 rows x 60 columns per wave
#define HD_SR 4
#define HD_COLS 60

// The environment's say in the plan, as walk_switches() normalises it (nellie_walk.hip reads the variables).
struct WalkSwitches {
    int rs;                 // NELLIE_HV_RS: rows per wave pair of the pair kernel, 8 (or 16 in a NL_HV_VARIANTS build); 0: the one-voxel kernel
    int np;                 // NELLIE_HV_NP: 2 = four voxels per lane (NL_HV_VARIANTS builds, 16-row tiles, two-instruction division), else 1
    int dpp;                // NELLIE_HV_DPP=1: the wave-autonomous kernel for the one-pass walk
    int ty;                 // NELLIE_HM_TY: tile rows of the one-voxel kernel, 8 (512-thread workgroups) or 16 (1024)
    int zchunk;             // NELLIE_HV_ZCHUNK: planes per workgroup of the one-pass walk, 0 = by the frame's size
    int64_t vq_cap;         // NELLIE_VQ_CAP: queue entries one known-threshold launch may use (a test knob to force several launches)
    int64_t spec_max_bytes; // NELLIE_SPEC_MAX_GB << 30: the one-pass walk is offered while its queue fits this
};
static inline WalkSwitches walk_switches(int64_t rs, int64_t np, int64_t dpp, int64_t ty, int64_t zchunk, int64_t vq_cap, int64_t spec_max_gb) {
    WalkSwitches s;
    s.rs = (rs == 0 || rs == 8 || (NL_HV_VARIANTS && rs == 16)) ? (int)rs : 8;
    s.np = (NL_HV_VARIANTS && np == 2) ? 2 : 1;
    s.dpp = dpp == 1;
    s.ty = ty == 16 ? 16 : 8;
    s.zchunk = (int)zchunk;
    s.vq_cap = vq_cap > 0 ? vq_cap : ((int64_t)1 << 28);
    s.spec_max_bytes = spec_max_gb << 30;
    return s;
}

// Global eigen queue: every wave of the vesselness kernel owns HM_REGION entries (32 bytes each), so one launch
// needs (padded plane) x (Z chunks x HM_ZCHUNK) entries.  A launch covers as many Z chunks as fit 2^28 entries
// (8 GiB); smaller volumes go in one launch.
// One-pass (MODE 2) vesselness needs every region of the whole slab at once, HM_SPEC_CAP entries each; it is
// offered when that fits NELLIE_SPEC_MAX_GB (default 64) GiB.
struct VqAlloc {
    int64_t chunks;         // Z chunks one known-threshold (MODE 1) launch covers
    int64_t entries;        // 32-byte queue entries allocated
    int64_t regions;        // region counters allocated
    int spec_ok;            // the one-pass walk is offered
};
static inline int64_t vq_padded_plane(int64_t ny, int64_t nx) { return ((nx + HM_TX - 1) / HM_TX) * HM_TX * (((ny + 31) / 32) * 32); }
static inline int64_t vq_spec_regions(int64_t nzl, int64_t ny, int64_t nx) { return vq_padded_plane(ny, nx) / 64 * ((nzl + HM_ZCHUNK - 1) / HM_ZCHUNK); }
static inline VqAlloc vq_alloc(const WalkSwitches &sw, int64_t nzl, int64_t ny, int64_t nx) {
    const int64_t per_chunk = vq_padded_plane(ny, nx) * HM_ZCHUNK, need = (nzl + HM_ZCHUNK - 1) / HM_ZCHUNK;
    int64_t chunks = sw.vq_cap / per_chunk;
    if (chunks > need) chunks = need;
    if (chunks < 1) chunks = 1;
    const int64_t step = chunks * per_chunk;
    int64_t spec = vq_spec_regions(nzl, ny, nx) * HM_SPEC_CAP;
    if (spec * 32 > sw.spec_max_bytes) spec = 0;
    const int64_t step_regions = step / HM_REGION, spec_regions = spec ? vq_spec_regions(nzl, ny, nx) : 0;
    return VqAlloc{chunks, step > spec ? step : spec, step_regions > spec_regions ? step_regions : spec_regions, spec > 0};
}

enum { WALK_ONE_VOXEL = 0, WALK_PAIR = 1, WALK_WAVE = 2 };
struct WalkPlan {
    int family;             // WALK_*
    int ty;                 // tile rows: 8 / 16 (one voxel), 2 * rs (pair), HD_SR (wave-autonomous)
    int rs, np;             // HvLaunch's: rows per wave pair and pair-rows per lane; np = 0 with rs = HD_SR: the wave-autonomous kernel
    int fastv;              // division: 0 float64, 1 three instructions, 2 two instructions (the one-voxel kernel has 0 and 1)
    int zchunk;             // planes per workgroup (wave)
    int ntx, nty, nzc;      // tiles (strips) in X and Y, Z chunks of [z0, z1)
    int64_t launch_planes;  // planes one launch covers: all of [z0, z1) but in MODE 1, where the queue holds VqAlloc::chunks chunks at a time
    int regions_per_group;  // queue regions per unit of `grid`
    int qcap;               // queue entries per region
    unsigned grid;          // nblocks of a launch of launch_planes planes (at most): workgroups, or waves of the wave-autonomous kernel
    unsigned nregions;      // its queue regions
};
static inline unsigned walk_grid(const WalkPlan &p, int64_t planes) { return (unsigned)(p.ntx * p.nty * (int)((planes + p.zchunk - 1) / p.zchunk)); }

// mode: 0 statistics over the owned planes, 1 known threshold, 2 one pass with a bracket (hessian.inc); [z0, z1): the planes walked
// (modes 1 and 2; mode 0 walks [own_lo, own_hi)); fast_div / fast_div2: what check_fast_div proved for the context's divisors.
static inline WalkPlan walk_plan(const WalkSwitches &sw, const VqAlloc &vq, int mode, int64_t ny, int64_t nx, int64_t own_lo, int64_t own_hi,
                                 int64_t z0, int64_t z1, int fast_div, int fast_div2) {
    auto fits = [&](int z) { return (int64_t)(z + 4) * ny * nx * 4 < ((int64_t)1 << 32); };
    auto cdiv = [](int64_t a, int64_t b) { return (a + b - 1) / b; };
    if (mode == 0) { z0 = own_lo; z1 = own_hi; }
    const int64_t nz = z1 - z0;
    WalkPlan p{};
    // the pair kernel addresses the planes of a Z chunk through one buffer resource (32-bit byte offsets)
    p.rs = fits(HM_ZCHUNK) ? sw.rs : 0;
    p.family = p.rs ? WALK_PAIR : WALK_ONE_VOXEL;
    p.fastv = p.rs ? (fast_div2 ? 2 : (fast_div ? 1 : 0)) : (fast_div ? 1 : 0);
    p.np = (sw.np == 2 && p.rs == 8 && p.fastv == 2) ? 2 : 1;
    p.ty = p.rs ? 2 * p.rs : sw.ty;
    p.ntx = (int)cdiv(nx, HM_TX); p.nty = (int)cdiv(ny, p.ty);
    p.zchunk = HM_ZCHUNK;
    p.launch_planes = mode == 1 ? vq.chunks * HM_ZCHUNK : nz;
    p.regions_per_group = p.rs ? p.rs / p.np : p.ty;                // a wave owns one row segment, two or four
    p.qcap = mode == 0 ? 0 : (mode == 1 ? HM_REGION : HM_SPEC_CAP) * (p.rs ? 2 * p.np : 1);
    if (mode == 2 && p.rs) {
        // Planes per workgroup: 64, or 128 where that still leaves thousands of workgroups (a chunk's prologue -- four planes
        // staged, the first gradient tile -- is paid half as often: walk -3 % at 1024^3; a 128-plane frame would run on 256
        // workgroups and lose 30 %).  The queue was sized for 64-plane chunks: twice the planes, twice the entries per region,
        // half the regions -- the same memory when the chunk count halves exactly or rounds the same way.
        const int64_t c64 = cdiv(nz, HM_ZCHUNK), c128 = cdiv(nz, 2 * HM_ZCHUNK);
        if (2 * c128 <= c64 && fits(2 * HM_ZCHUNK) && (sw.zchunk == 2 * HM_ZCHUNK || (sw.zchunk == 0 && (int64_t)p.ntx * p.nty * c128 >= 4096))) {
            p.zchunk = 2 * HM_ZCHUNK;
            p.qcap *= 2;
        }
    }
    if (mode == 2 && p.rs && sw.dpp) {
        // Wave-autonomous walk: one region per strip and chunk; the queue's bytes are shared out evenly (0.47 entries per voxel of a strip
        // where the pair kernel has 0.5: its strips overhang the volume by up to 59 columns).  Planes per wave: 128 where that leaves several
        // rounds of waves (a chunk's prologue -- four planes loaded, the first derivatives of one -- is paid half as often), 32 on small
        // frames (a 128 x 512 x 512 frame has 1152 strips: 64-plane chunks would fill three quarters of the 3072 wave slots once), else 64.
        const int ntxd = (int)cdiv(nx, HD_COLS), ntyd = (int)cdiv(ny, HD_SR);
        const int64_t strips = (int64_t)ntxd * ntyd;
        int zd = 32;
        if (sw.zchunk > 0 && (sw.zchunk & 3) == 0 && fits(sw.zchunk)) zd = sw.zchunk;
        else if (fits(128) && strips * cdiv(nz, 128) >= 8192) zd = 128;
        else if (fits(64) && strips * cdiv(nz, 64) >= 4096) zd = 64;
        const int64_t nreg = strips * cdiv(nz, zd);
        int64_t cap = vq.entries / nreg;
        if (cap > (int64_t)HD_SR * 64 * zd) cap = (int64_t)HD_SR * 64 * zd;
        if (cap > (1 << 24) - 1) cap = (1 << 24) - 1;
        // (else the queue cannot be shared out -- too few entries per strip, or no room for the region counts + the strips' h_mask counts:
        // the pair kernel walks)
        if (cap >= 64 && 2 * nreg <= vq.regions) {
            p.family = WALK_WAVE;
            p.ty = p.rs = HD_SR; p.np = 0;
            p.ntx = ntxd; p.nty = ntyd; p.zchunk = zd;
            p.regions_per_group = 1;
            p.qcap = (int)cap;
        }
    }
    p.nzc = (int)cdiv(nz, p.zchunk);
    p.grid = walk_grid(p, p.launch_planes < nz ? p.launch_planes : nz);
    p.nregions = mode ? p.grid * (unsigned)p.regions_per_group : 0;       // (the statistics walk queues nothing)
    return p;
}
