// Part of libnellie_hip.so (gfx950): included by nellie_hip.hip after thresholds.inc; the records it logs are filled by nellie_sample.hip.
// =================================================================================================
// Device-resident threshold chain of a scale (filtering.py:365-380, 421-444, 555-566, 839-851)
// =================================================================================================
// The reference decides four data-dependent scalars per scale between its full-volume passes: gamma (from a histogram of
// the Gaussian), max |H| and the Frobenius threshold (from a histogram of normalised Frobenius norms), and -- in this build --
// the bracket that lets ONE walk over the Hessian serve a threshold that is not known yet.  Round 2 took each of them to the
// host and back (~40 synchronous round trips per frame: a third of a 128 x 512 x 512 frame's time).  Here small kernels do
// the same arithmetic between the large ones, the large ones read their thresholds from device memory, and nothing waits:
//   range + edges + histogram (sampling.inc)  ->  chain_thr1_kernel : gamma, gamma_sq, bracket [fsq_lo, fsq_hi]
//   walk (MODE 2, statistics into the record) ->  chain_post_kernel : max_abs, max_frob, the normalised sample range
//   edges + exact histogram                   ->  chain_thr2_kernel : threshold, fsq_min, m_inf, bracket hit, empty scale
//   resolve kernel
// The frame ends with ONE synchronisation (nl_chain_finish).  Everything the kernels decided is logged -- the three
// histograms with their edges and every derived scalar -- and the host REPEATS the arithmetic with the host code the
// synchronous path uses (thresholds.inc, mask_threshold_on_fsq, libm) and compares bit for bit.  A difference, an unusual
// condition (no positive sample, degenerate triangle, +inf, queue overflow, bracket miss, empty scale, underflow of the
// normalised range) or a failed comparison sets `flags`, and the caller redoes the frame the synchronous way: the chain can
// make a frame faster, never different.
// The first line of that list needs the scale's Gaussian only, the rest joins the frame's masks: where three Gaussians can coexist the
// host runs the first line of up to three scales ahead and walks them in the order chain_thr1_kernel's forecast of the mask fraction
// suggests (nellie_hip.hip: nl_chain_sample / nl_chain_walk).  The records stay indexed by sigma.
#define NL_CHAIN_BINS 256
#define NL_CHAIN_MAX_SCALES 16

struct ChainHist {                        // the record the sampling rounds fill: hist_layout (nl_host.h) at NL_CHAIN_BINS
    unsigned long long counts[NL_CHAIN_BINS];
    float edges[NL_CHAIN_BINS + 1];
    float pad_[3];
    unsigned int res[8];                  // [0] min bits, [1] max bits, [2..3] count, [4] flag (0 none, 1 ok, 2 not finite)
};
static_assert(sizeof(ChainHist) == hist_layout(NL_CHAIN_BINS).bytes && offsetof(ChainHist, edges) == hist_layout(NL_CHAIN_BINS).off_edges &&
              offsetof(ChainHist, res) == hist_layout(NL_CHAIN_BINS).off_res, "ChainHist is hist_layout");

enum {
    NL_CF_GAUSS_HIST = 1, NL_CF_RAW_HIST = 2, NL_CF_TRIANGLE = 4, NL_CF_BRACKET = 8, NL_CF_INF = 16, NL_CF_OVERFLOW = 32,
    NL_CF_NORM_RANGE = 64, NL_CF_MISS = 128, NL_CF_EMPTY = 256, NL_CF_VERIFY = 512
};

struct ChainScale {
    // what the big kernels read (ScaleParamsDev view, at offset 0)
    float fsq_lo, fsq_hi;                 // bracket of the walk
    float gamma_sq, fsq_min;              // resolve kernel
    int m_inf, flags;
    float norm[2];                        // (max_abs, max_finite) of the exact normalisation, read by the sampling kernels
    // statistics of the walk (atomicMax / atomicOr / atomicAdd targets) and of the resolve kernel
    unsigned int stats[4];                // max |H| bits, max frob_sq bits, any inf, overflow
    unsigned long long cnt_walk, cnt_resolve;
    // derived scalars, logged
    float gamma, max_abs, max_frob, thr, thr_cmp, raw_mn, raw_mx, nmn, nmx;
    int status_gauss, status_raw, status_exact;
    double tri[3], otsu[3];
    ChainHist h_gauss, h_raw, h_exact;
    // appended (nothing above moves): the share of the scale's lattice points whose raw frob_sq reaches fsq_lo -- a forecast of its
    // h_mask fraction, < 0 when there is none.  It orders the walks of a frame (nl_chain_walk) and decides no value.
    float pred_frac;
    int pad_;
};

// ---- the two histogram thresholds on the device: hist_thresholds_host on one wave ----------------------------------------
// Element-wise steps (bin centres, probabilities, the variance and distance arrays, their argmax) run on all 64 lanes; numpy's
// cumulative sums are SEQUENTIAL additions -- a parallel scan would round differently -- so lane 0 does those four scans, in
// order.  pow(height, 2.0) of the host code is height * height here; the verification on the host settles whether libm ever
// disagrees.  (The first version ran everything on one lane: ~170 us per threshold, 2.5 ms per frame.)
// numpy's argmax over a[0..n): a NaN is the maximum, the first one wins; otherwise the first largest value.  All lanes call it.
__device__ inline int wave_argmax_f64(const double *a, int n) {
    const int lane = threadIdx.x & 63;
    double best = 0.0; int at = 0x7fffffff; int first_nan = 0x7fffffff;
    for (int i = lane; i < n; i += 64) {
        const double v = a[i];
        if (v != v) { if (i < first_nan) first_nan = i; }
        else if (at == 0x7fffffff || v > best) { best = v; at = i; }      // strictly larger: the lane keeps its first maximum
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int onan = __shfl_xor(first_nan, o, 64);
        first_nan = onan < first_nan ? onan : first_nan;
        const double ob = __shfl_xor(best, o, 64);
        const int oa = __shfl_xor(at, o, 64);
        if (oa != 0x7fffffff && (at == 0x7fffffff || ob > best || (ob == best && oa < at))) { best = ob; at = oa; }
    }
    return first_nan != 0x7fffffff ? first_nan : (at == 0x7fffffff ? 0 : at);
}

// scratch: 6 * nbins doubles of LDS; the calling workgroup is ONE wave; every lane returns the same values
__device__ inline void dev_hist_thresholds(const unsigned long long *counts, const float *edges, int nbins, double *scratch,
                                           double *triangle, double *otsu, int *status) {
    const int lane = threadIdx.x & 63;
    double *p = scratch, *pc = scratch + nbins, *w1 = scratch + 2 * nbins, *a1 = scratch + 3 * nbins, *w2 = scratch + 4 * nbins,
           *a2 = scratch + 5 * nbins;
    unsigned long long part = 0;
    for (int i = lane; i < nbins; i += 64) part += counts[i];
    const long long total = (long long)wave_sum_u64(part);
    for (int i = lane; i < nbins; i += 64) {
        const float centre = (edges[i] + edges[i + 1]) / 2.0f;
        const double pi = (double)(long long)counts[i] / (double)total;
        p[i] = pi;
        pc[i] = pi * (double)centre;
    }
    __syncthreads();
    if (nbins == 4 * 64) {
        // The four cumulative sums, in numpy's order of additions, in registers: lane l holds elements 4l .. 4l+3; the lanes
        // take turns (a wave-uniform loop), each continues the running sums its predecessor broadcast with v_readlane.  256
        // dependent additions per sum either way, but none of them waits for LDS (one lane scanning LDS: 4 x 15 us).
        double pv[4], qv[4], o1[4], o2[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { pv[j] = p[4 * lane + j]; qv[j] = pc[4 * lane + j]; }
        auto bcast = [](double v, int src) -> double {
            const unsigned long long b = (unsigned long long)__double_as_longlong(v);
            const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)b, src);
            const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(b >> 32), src);
            return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
        };
        double acc = 0.0, accm = 0.0;
        for (int src = 0; src < 64; ++src) {                       // forward
            double a = acc, m = accm;
            if (lane == src) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { a += pv[j]; m += qv[j]; o1[j] = a; o2[j] = m; }
            }
            acc = bcast(a, src); accm = bcast(m, src);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { w1[4 * lane + j] = o1[j]; a1[4 * lane + j] = o2[j]; }
        acc = 0.0; accm = 0.0;
        for (int src = 63; src >= 0; --src) {                      // backward
            double a = acc, m = accm;
            if (lane == src) {
#pragma unroll
                for (int j = 3; j >= 0; --j) { a += pv[j]; m += qv[j]; o1[j] = a; o2[j] = m; }
            }
            acc = bcast(a, src); accm = bcast(m, src);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { w2[4 * lane + j] = o1[j]; a2[4 * lane + j] = o2[j]; }
    } else if (lane == 0) {
        double acc = 0.0, accm = 0.0;
        for (int i = 0; i < nbins; ++i) { acc += p[i]; accm += pc[i]; w1[i] = acc; a1[i] = accm; }
        acc = 0.0; accm = 0.0;
        for (int i = nbins - 1; i >= 0; --i) { acc += p[i]; accm += pc[i]; w2[i] = acc; a2[i] = accm; }
    }
    __syncthreads();
    // Otsu: var[i] = (w1[i] w2[i+1]) (m1[i] - m2[i+1])^2 with m = (cumulative p * centre) / (cumulative p); var over pc's space
    if (nbins < 2) *otsu = (double)((edges[0] + edges[1]) / 2.0f);
    else {
        double *var = pc;                                  // pc is dead from here on (a1, a2 hold its sums)
        for (int i = lane; i + 1 < nbins; i += 64) {
            const double m1 = a1[i] / w1[i], m2 = a2[i + 1] / w2[i + 1];
            const double d = m1 - m2;
            var[i] = (w1[i] * w2[i + 1]) * (d * d);
        }
        __syncthreads();
        const int at = wave_argmax_f64(var, nbins - 1);
        *otsu = (double)((edges[at] + edges[at + 1]) / 2.0f);
    }
    __syncthreads();
    // triangle
    *status = 0;
    int peak = wave_argmax_f64(p, nbins);
    const double height = p[peak];
    int lo = 0x7fffffff, hi = -1;
    for (int i = lane; i < nbins; i += 64)
        if (p[i] != 0.0) { if (i < lo) lo = i; if (i > hi) hi = i; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int ol = __shfl_xor(lo, o, 64), oh = __shfl_xor(hi, o, 64);
        lo = ol < lo ? ol : lo; hi = oh > hi ? oh : hi;
    }
    if (lo == 0x7fffffff) lo = -1;
    const bool mirrored = (peak - lo) < (hi - peak);
    if (mirrored) { lo = nbins - hi - 1; peak = nbins - peak - 1; }
    const int span = peak - lo;
    if (span <= 0 || lo < 0) { *status = 1; *triangle = 0.0; return; }
    const double norm = sqrt(height * height + (double)((long long)span * (long long)span));
    const double hn = height / norm, sn = (double)span / norm;
    double *dist = w1;                                     // the cumulative sums are dead
    __syncthreads();
    for (int k = lane; k < span; k += 64) {
        const int bin = mirrored ? nbins - 1 - (k + lo) : k + lo;
        dist[k] = hn * (double)k - sn * p[bin];
    }
    __syncthreads();
    int level = wave_argmax_f64(dist, span) + lo;
    if (mirrored) level = nbins - level - 1;
    *triangle = (double)((edges[level] + edges[level + 1]) / 2.0f);
}

__device__ inline bool dev_finite_f(float x) { return fabsf(x) <= 3.402823466e38f; }

// gamma and the bracket (pipeline.py: compute_vesselness / _fsq_bracket).  division, margin, test_scale: python floats.
// Two workgroups of one wave: block 0 the Gaussian samples (gamma), block 1 the raw Frobenius samples (the bracket) -- the two
// thresholds need nothing from each other.  Every lane computes the same scalars (the element-wise parts of the thresholds
// are spread over the lanes), lane 0 records them.
__global__ void __launch_bounds__(64)
chain_thr1_kernel(ChainScale *cs, double division, double margin, double test_scale, double n_lattice) {
    __shared__ double scratch[6 * NL_CHAIN_BINS];
    int flags = 0;
    if (blockIdx.x == 0) {
        // ---- gamma = min(triangle, otsu) of the positive Gaussian samples; <= 0 or none -> float32 eps (filtering.py:365-380)
        float gamma = 1.1920929e-07f;
        double tri0 = 0.0, otsu0 = 0.0;
        int st0 = 0;
        const ChainHist &h = cs->h_gauss;
        const unsigned long long cnt = *(const unsigned long long *)(h.res + 2);
        if (cnt == 0ull || h.res[4] != 1u) flags |= NL_CF_GAUSS_HIST;
        else {
            dev_hist_thresholds(h.counts, h.edges, NL_CHAIN_BINS, scratch, &tri0, &otsu0, &st0);
            if (st0) flags |= NL_CF_TRIANGLE;
            const float g = fminf((float)tri0, (float)otsu0);      // min() of two float32 values
            if (g > 0.0f) gamma = g;
        }
        const double g64 = (double)gamma;
        const float gamma_sq = (float)(2.0 * (g64 * g64));           // 2.0 * float(gamma) ** 2, then ctypes' c_float
        if (threadIdx.x == 0) {
            cs->gamma = gamma; cs->gamma_sq = gamma_sq;
            cs->tri[0] = tri0; cs->otsu[0] = otsu0; cs->status_gauss = st0;
            if (flags) atomicOr(&cs->flags, flags);
        }
        return;
    }
    // ---- bracket of the un-normalised frob_sq threshold: the reference's threshold code with max_abs := 1
    float lo = __int_as_float(0x7f800000), hi = __int_as_float(0x7f800000);     // flagged: nothing decided by the walk
    double tri1 = 0.0, otsu1 = 0.0;
    int st1 = 0;
    const ChainHist &h = cs->h_raw;
    const float raw_mn = __uint_as_float(h.res[0]), raw_mx = __uint_as_float(h.res[1]);
    const unsigned long long cnt = *(const unsigned long long *)(h.res + 2);
    if (cnt == 0ull || h.res[4] != 1u || !dev_finite_f(raw_mx)) flags |= NL_CF_RAW_HIST;
    else {
        dev_hist_thresholds(h.counts, h.edges, NL_CHAIN_BINS, scratch, &tri1, &otsu1, &st1);
        if (st1) flags |= NL_CF_TRIANGLE;
        const float tf = fminf((float)tri1, (float)otsu1);
        const double t = (double)tf * test_scale / division;
        const float l = (float)(t * t * (1.0 - margin)), u = (float)(t * t * (1.0 + margin));
        if (!(dev_finite_f(l) && dev_finite_f(u) && u > 0.0f) || !(l <= u)) flags |= NL_CF_BRACKET;
        else { lo = l; hi = u; }
    }
    // the forecast: the samples of the bins whose centre reaches the bracket's lower end, over all lattice points
    float pred = -1.0f;
    if (!flags && n_lattice > 0.0) {
        unsigned long long part = 0;
        for (int i = threadIdx.x; i < NL_CHAIN_BINS; i += 64) {
            const float centre = (h.edges[i] + h.edges[i + 1]) / 2.0f;
            if (centre * centre >= lo) part += h.counts[i];
        }
        pred = (float)((double)wave_sum_u64(part) / n_lattice);
    }
    if (threadIdx.x == 0) {
        cs->pred_frac = pred;
        cs->tri[1] = tri1; cs->otsu[1] = otsu1; cs->status_raw = st1;
        cs->raw_mn = raw_mn; cs->raw_mx = raw_mx;
        cs->fsq_lo = lo; cs->fsq_hi = hi;
        if (flags) atomicOr(&cs->flags, flags);
    }
}

// after the walk: max |H|, max frob, the normalisation of the exact round and its sample range (pipeline.py: _normalised_range)
__global__ void __launch_bounds__(64)
chain_post_kernel(ChainScale *cs) {
    if (threadIdx.x != 0) return;
    int flags = 0;
    const float max_abs32 = __uint_as_float(cs->stats[0]), max_fsq32 = __uint_as_float(cs->stats[1]);
    if (cs->stats[2]) flags |= NL_CF_INF;
    if (cs->stats[3]) flags |= NL_CF_OVERFLOW;
    const float max_abs = (max_abs32 <= 0.0f) ? 1.0f : max_abs32;
    cs->max_abs = max_abs;
    cs->max_frob = sqrtf(max_fsq32) / max_abs;
    cs->norm[0] = max_abs; cs->norm[1] = 0.0f;                  // (an inf sends the frame to the synchronous path anyway)
    const float mn = cs->raw_mn / max_abs, mx = cs->raw_mx / max_abs;
    cs->nmn = mn; cs->nmx = mx;
    unsigned int *res = cs->h_exact.res;
    res[0] = __float_as_uint(mn); res[1] = __float_as_uint(mx); res[2] = 1u; res[3] = 0u; res[4] = 0u;
    if (!(mn > 0.0f && dev_finite_f(mx)) || (cs->flags & NL_CF_RAW_HIST)) { flags |= NL_CF_NORM_RANGE; res[2] = 0u; }
    cs->flags |= flags;
}

// mask_threshold_on_fsq on the device: smallest float32 x with sqrt(x) / max_abs > thr (bisection over the bit patterns)
__device__ inline float dev_mask_threshold_on_fsq(float max_abs, float thr) {
    auto pred = [&](float x) -> bool { float fr = sqrtf(x); fr = fr / max_abs; return fr > thr; };
    unsigned int lo = 0u, hi = 0x7f7fffffu;
    if (!pred(__uint_as_float(hi))) return __int_as_float(0x7f800000);
    while (lo < hi) {
        const unsigned int mid = lo + (hi - lo) / 2;
        if (pred(__uint_as_float(mid))) hi = mid; else lo = mid + 1;
    }
    return __uint_as_float(lo);
}

// the exact threshold, the mask test on frob_sq, the bracket check (pipeline.py: compute_vesselness; make_vessp)
__global__ void __launch_bounds__(64)
chain_thr2_kernel(ChainScale *cs, double division) {
    __shared__ double scratch[6 * NL_CHAIN_BINS];
    int flags = 0, st = 0, m_inf = 0;
    double tri = 0.0, otsu = 0.0;
    float thr = 0.0f, thr_cmp = 0.0f, fsq_min = __int_as_float(0x7f800000);
    const ChainHist &h = cs->h_exact;
    if (h.res[4] != 1u || (cs->flags & NL_CF_NORM_RANGE)) flags |= NL_CF_NORM_RANGE;
    else {
        dev_hist_thresholds(h.counts, h.edges, NL_CHAIN_BINS, scratch, &tri, &otsu, &st);
        if (st) flags |= NL_CF_TRIANGLE;
        thr = fminf((float)tri, (float)otsu);
        thr_cmp = (float)((double)thr / division);
        if (!(cs->max_frob > thr_cmp)) flags |= NL_CF_EMPTY;
        fsq_min = dev_mask_threshold_on_fsq(cs->max_abs, thr_cmp);
        m_inf = (0.0f > thr_cmp) ? 1 : 0;                      // max_finite = 0 on this path
        if (!(fsq_min >= cs->fsq_lo && fsq_min <= cs->fsq_hi)) flags |= NL_CF_MISS;
    }
    if (threadIdx.x == 0) {
        cs->tri[2] = tri; cs->otsu[2] = otsu; cs->status_exact = st;
        cs->thr = thr; cs->thr_cmp = thr_cmp; cs->fsq_min = fsq_min; cs->m_inf = m_inf;
        cs->flags |= flags;
    }
}

// every record of a frame starts from the same state (one launch per frame instead of a memset and an upload per histogram)
__global__ void __launch_bounds__(256)
chain_init_kernel(ChainScale *cs, int n) {
    const size_t words = sizeof(ChainScale) / 4 * (size_t)n;
    unsigned int *w = (unsigned int *)cs;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (size_t)gridDim.x * blockDim.x) w[i] = 0u;
    __syncthreads();
    // (the min slots of the range records are set by a second launch: a grid-wide ordering is needed between the two)
}
__global__ void __launch_bounds__(64)
chain_init2_kernel(ChainScale *cs, int n) {
    const int k = threadIdx.x;
    if (k < n) { cs[k].h_gauss.res[0] = 0xffffffffu; cs[k].h_raw.res[0] = 0xffffffffu; }
}
