// Part of libnellie_hip.so (gfx950): the resolve kernel of the eigen queue, included by nellie_walk.hip after walk_common.h.
// Dense eigen-solve + Frangi response over the queue regions (filtering.py:583-584, 744-766), then the running
// maximum over scales (filtering.py:846-848).  One wave per region; `base` = voxel offset of the launch's first plane.
// RESOLVE (after a MODE 2 pass): entries flagged undecided first take the exact h_mask test; those that pass are
// counted, AND-ed with the earlier scales' mask bit, recorded in this scale's mask word (atomicOr: the pass wrote
// the decided bits) and, if still alive and not excluded by their trace, solved like the others.
template <bool RESOLVE>
__global__ void __launch_bounds__(256)
vesselness_queue_kernel(const float4 *__restrict__ ent, const unsigned int *__restrict__ count, unsigned int nregions,
                        float *__restrict__ vmax, i64 base, VessP vp, unsigned long long *cmask64,
                        const unsigned long long *pmask64, int wpr, int ny, int nx, i64 zbase,
                        unsigned long long *__restrict__ mask_count, const float *__restrict__ dev_params) {
    // inside a device-resident threshold chain (chain.inc: the head of a ChainScale record): gamma_sq, fsq_min, m_inf were
    // decided by a kernel
    if (dev_params) { vp.gamma_sq = dev_params[2]; vp.fsq_min = dev_params[3]; vp.m_inf = __float_as_int(dev_params[4]); }
    // A wave walks several regions (the launcher caps the grid): with one short-lived wave per region the kernel took
    // the same 7.7 ms/step whether it solved the eigenproblems or not -- wave start-up and the dependent count -> entries
    // loads dominated; 16384 workgroups x 4 waves, 8 regions each at 1024^3, bring it to 5.3 ms.  The next region's
    // count is requested before this region's entries are worked on.
    unsigned int passed = 0;
    // The running-maximum store of an entry is issued at the top of the NEXT trip (round 4).  vmcnt counts loads and stores in
    // order, and the compiler has to wait for "everything" where the prefetched entry changes registers at the end of a trip: with
    // the store as the youngest operation that wait was the store's full round trip, once per trip, with nothing of this wave
    // behind it.  Issued before the next trip's loads, the store completes behind the eigen-solve like they do.
    bool st_pending = false;
    i64 st_at = 0;
    float st_val = 0.0f;
    const unsigned int rstep = gridDim.x * 4u;
    unsigned int r = blockIdx.x * 4u + (threadIdx.x >> 6);
    unsigned int n_next = r < nregions ? count[r] : 0u;
    for (; r < nregions; r += rstep) {
    unsigned int n = n_next;
    n_next = (r + rstep < nregions) ? count[r + rstep] : 0u;
    if (RESOLVE && n > (unsigned int)vp.qcap) n = (unsigned int)vp.qcap;
    const float4 *e = ent + (size_t)r * (size_t)vp.qcap * 2;
    // A lane's entries are 64 apart; the NEXT entry is requested before this one is worked on, and the running maximum of
    // this entry's voxel is requested before its eigen-solve (~500 float64 instructions) instead of after it: the kernel
    // waits (82 % of its wave cycles in round 2), it does not compute -- both latencies now pass behind the arithmetic.
    unsigned int i = threadIdx.x & 63u;
    float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
    if (i < n) qent_load(e, i, a, b);
    // The region's first entry is "used" here, so that the loop is entered with no load outstanding: the compiler merges the loop
    // header's wait over both ways in, and the first trip's pending loads put a vmcnt(0) right behind the store below on every trip.
    asm volatile("" :: "v"(a.x), "v"(b.x));
    for (; i < n; i += 64u) {
        if (st_pending) { vmax[st_at] = st_val; st_pending = false; }
        const float4 a0 = a, b0 = b;
        if (i + 64u < n) qent_load(e, i + 64u, a, b);
        const float h[6] = {a0.x, a0.y, a0.z, a0.w, b0.x, b0.y};
        if (vp.all_ones) {                      // uniform; see VessP::nan_flag
            if ((h[0] != h[0]) | (h[1] != h[1]) | (h[2] != h[2]) | (h[3] != h[3]) | (h[4] != h[4]) | (h[5] != h[5])) *vp.nan_flag = 1u;
        }
        unsigned int idx = __float_as_uint(b0.z);
        const bool undecided = RESOLVE && (idx & HM_UNDECIDED);
        idx &= ~HM_UNDECIDED;
        const i64 c = base + idx;
        // vesselness >= 0 everywhere and the volume is all zeros before the first scale: `val > cur` is the running maximum
        // AND the test that keeps zero responses (37 % of the entries) from being written
        const float cur = vp.first ? 0.0f : vmax[c];
        if (undecided) {
            const float fsq = frob_sq_of(h);
            if (!((fsq >= vp.fsq_min) && (fsq < __int_as_float(0x7f800000) || vp.m_inf))) continue;
            if ((i64)idx >= vp.idx_lo && (i64)idx < vp.idx_hi) ++passed;
            const i64 plane = (i64)ny * nx;
            const i64 zl = idx / plane;
            const int rem = (int)(idx - zl * plane);
            const int yy = rem / nx, xx = rem - yy * nx;
            const i64 word = ((zbase + zl) * ny + yy) * wpr + (xx >> 6);
            const unsigned long long bit = 1ull << (xx & 63);
            if (vp.have_prev && !(pmask64[word] & bit)) continue;
            atomicOr(&cmask64[word], bit);
            const float tr = h[0] + h[3] + h[5];
            if (!HM_TRACE_OK(tr, fsq)) continue;
        }
        float l1, l2, l3;
        eig3_sorted_abs(h, l1, l2, l3);
        const float val = frangi3(l1, l2, l3, vp.alpha_sq, vp.beta_sq, vp.gamma_sq);
        if (val > cur) { st_pending = true; st_at = c; st_val = val; }
    }
    }
    if (st_pending) vmax[st_at] = st_val;
    if (RESOLVE) {
        unsigned long long t = wave_sum_u64((unsigned long long)passed);
        if ((threadIdx.x & 63u) == 0 && t) atomicAdd(mask_count, t);
    }
}
