// Part of libnellie_hip.so (gfx950): included by nellie_sample.hip (and by no other unit), see include/nellie_amd.h for the C-ABI.
// =================================================================================================
// kernels: lattice sampling (strided subsample for the thresholds)
// =================================================================================================
struct Lattice {
    i64 sz, sy, sx;      // strides (global lattice)
    i64 cz, cy, cx;      // lattice extent on the owned planes
    i64 zfirst;          // local z of the first owned lattice plane
};

struct FieldSrc {
    const float *p;      // gauss (GAUSS/FROB) or frangi
    int field;
    HessP hp;
    float max_abs, max_finite;
    int two_d;           // (Y, X) image: the Hessian has three components
    const unsigned long long *bits;   // NL_FIELD_VESSELNESS: cumulative mask (1 bit/voxel), row pitch `wpr` words
    int wpr;
    const float *fsq_cache;           // NL_FIELD_FROB: frob_sq of every lattice point (filled once per scale), or NULL
    const float *norm_dev;            // NL_FIELD_FROB: (max_abs, max_finite) in device memory (chain.inc), or NULL: the two above
};

// raw frob_sq at a voxel (the part of NL_FIELD_FROB that does not depend on the normalisation)
__device__ __forceinline__ float frob_sq_at(const FieldSrc &fs, const VolGeom &v, i64 z, i64 y, i64 x) {
    if (fs.two_d) {
        float h[3];
        hessian2d_at(fs.p, v, fs.hp, y, x, h);
        return frob_sq2_of(h);
    }
    float h[6];
    hessian_at(fs.p, v, fs.hp, z, y, x, h);
    return frob_sq_of(h);
}

// lattice point i -> (ix, iy, iz).  Lattices are <= ~10^6 points: 32-bit divisions (a 64-bit division by a run-time
// divisor costs ~100 instructions on this part, three of them dominated the sampling kernels)
__device__ __forceinline__ void lattice_split(const Lattice &L, i64 i, i64 &ix, i64 &iy, i64 &iz) {
    if (L.cz * L.cy * L.cx <= 0x7fffffffLL) {                     // uniform
        const unsigned int u = (unsigned int)i, cx = (unsigned int)L.cx, cy = (unsigned int)L.cy;
        const unsigned int q = u / cx;
        ix = u - q * cx;
        const unsigned int q2 = q / cy;
        iy = q - q2 * cy;
        iz = q2;
    } else {
        ix = i % L.cx; iy = (i / L.cx) % L.cy; iz = i / (L.cx * L.cy);
    }
}

// `i` = linear index of the lattice point (for the per-scale cache of NL_FIELD_FROB)
__device__ __forceinline__ float field_value(const FieldSrc &fs, const VolGeom &v, i64 i, i64 z, i64 y, i64 x) {
    if (fs.field == NL_FIELD_FROB && fs.fsq_cache)
        return fs.norm_dev ? frob_norm(fs.fsq_cache[i], fs.norm_dev[0], fs.norm_dev[1]) : frob_norm(fs.fsq_cache[i], fs.max_abs, fs.max_finite);
    if (fs.field == NL_FIELD_FROB) {
        if (fs.two_d) {
            float h[3];
            hessian2d_at(fs.p, v, fs.hp, y, x, h);
            return frob_norm(frob_sq2_of(h), fs.max_abs, fs.max_finite);
        }
        float h[6];
        hessian_at(fs.p, v, fs.hp, z, y, x, h);
        return frob_norm(frob_sq_of(h), fs.max_abs, fs.max_finite);
    }
    if (fs.field == NL_FIELD_VESSELNESS) {          // vesselness * masks without materialising it
        const bool keep = (fs.bits[(z * v.ny + y) * fs.wpr + (x >> 6)] >> (x & 63)) & 1ull;
        return keep ? fs.p[(z * v.ny + y) * v.nx + x] : 0.0f;
    }
    return fs.p[(z * v.ny + y) * v.nx + x];
}

__global__ void __launch_bounds__(256)
sample_gather_kernel(FieldSrc fs, VolGeom v, Lattice L, float *__restrict__ out) {
    const i64 total = L.cz * L.cy * L.cx;
    i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    i64 ix, iy, iz; lattice_split(L, i, ix, iy, iz);
    out[i] = field_value(fs, v, i, L.zfirst + iz * L.sz, iy * L.sy, ix * L.sx);
}

// fills the per-scale cache: frob_sq at every lattice point
__global__ void __launch_bounds__(256)
sample_fsq_kernel(FieldSrc fs, VolGeom v, Lattice L, float *__restrict__ out) {
    const i64 total = L.cz * L.cy * L.cx;
    i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    i64 ix, iy, iz; lattice_split(L, i, ix, iy, iz);
    out[i] = frob_sq_at(fs, v, L.zfirst + iz * L.sz, iy * L.sy, ix * L.sx);
}

// results: [0] = min bits (uint), [1] = max bits (uint), [2..3] = count (u64).  Grid-stride, one set of
// atomics per workgroup (per-wave atomics on three shared words cost ~0.5 ms at 1e6 samples).
struct RangeAcc {
    float mn, mx;
    unsigned long long cnt;
    __device__ __forceinline__ void init() { mn = __int_as_float(0x7f800000); mx = 0.0f; cnt = 0; }
    __device__ __forceinline__ void add(float val) { if (val > 0.0f) { mn = fminf(mn, val); mx = fmaxf(mx, val); cnt++; } }
};
// s_mn, s_mx, s_c: four entries each (one per wave of the 256-thread workgroup)
__device__ __forceinline__ void range_commit(RangeAcc a, float *s_mn, float *s_mx, unsigned long long *s_c, unsigned int *__restrict__ res) {
    float mn = wave_min_f(a.mn), mx = wave_max_f(a.mx);
    unsigned long long cnt = wave_sum_u64(a.cnt);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { s_mn[w] = mn; s_mx[w] = mx; s_c[w] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) { mn = fminf(mn, s_mn[k]); mx = fmaxf(mx, s_mx[k]); cnt += s_c[k]; }
        if (cnt) {
            // positive floats order like their bit patterns
            atomicMin(&res[0], __float_as_uint(mn));
            atomicMax(&res[1], __float_as_uint(mx));
            atomicAdd((unsigned long long *)(res + 2), cnt);
        }
    }
}

__global__ void __launch_bounds__(256)
sample_minmax_kernel(FieldSrc fs, VolGeom v, Lattice L, unsigned int *__restrict__ res) {
    __shared__ float s_mn[4], s_mx[4];
    __shared__ unsigned long long s_c[4];
    const i64 total = L.cz * L.cy * L.cx;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    RangeAcc a; a.init();
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        i64 ix, iy, iz; lattice_split(L, i, ix, iy, iz);
        a.add(field_value(fs, v, i, L.zfirst + iz * L.sz, iy * L.sy, ix * L.sx));
    }
    range_commit(a, s_mn, s_mx, s_c, res);
}

// One pass over the lattice for a scale's two sample sets (filtering.py:365-380 the Gaussian, 421-444 the Frobenius norm):
// the Gaussian value and frob_sq of every lattice point, the latter kept in `cache` for the later passes of the scale
// (sample_fsq_kernel + 2 x sample_minmax_kernel in one launch).  fsF: NL_FIELD_FROB without a cache attached.
__global__ void __launch_bounds__(256)
sample_minmax2_kernel(FieldSrc fsG, FieldSrc fsF, VolGeom v, Lattice L, unsigned int *__restrict__ resG, unsigned int *__restrict__ resF,
                      float *__restrict__ cache) {
    __shared__ float s_mn[8], s_mx[8];
    __shared__ unsigned long long s_c[8];
    const i64 total = L.cz * L.cy * L.cx;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    RangeAcc g, f; g.init(); f.init();
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        i64 ix, iy, iz; lattice_split(L, i, ix, iy, iz);
        const i64 z = L.zfirst + iz * L.sz, y = iy * L.sy, x = ix * L.sx;
        g.add(fsG.p[(z * v.ny + y) * v.nx + x]);
        const float fsq = frob_sq_at(fsF, v, z, y, x);
        cache[i] = fsq;
        f.add(frob_norm(fsq, fsF.max_abs, fsF.max_finite));
    }
    range_commit(g, s_mn, s_mx, s_c, resG);
    __syncthreads();
    range_commit(f, s_mn + 4, s_mx + 4, s_c + 4, resF);
}

// numpy's bin edges for float32 data on the device (numpy/lib/_histograms_impl.py `_get_outer_edges`, `_get_bin_edges`
// -> np.linspace in float32: arange * step + start, last edge = stop; an empty range widens by +-0.5), from the
// min / max a preceding sample_minmax_kernel left in `res`.  flag: 0 no positive sample, 1 edges valid, 2 range not
// finite.  One wave.  Lets the range pass and the histogram pass run back to back without a host round trip.
__device__ __forceinline__ void build_edges(const unsigned int *__restrict__ res, int nbins, float *__restrict__ edges, unsigned int *__restrict__ flag) {
    const unsigned long long cnt = *(const unsigned long long *)(res + 2);
    float first = __uint_as_float(res[0]), last = __uint_as_float(res[1]);
    unsigned int f = 1u;
    if (cnt == 0ull) f = 0u;
    else if (!(fabsf(first) <= 3.402823466e38f) || !(fabsf(last) <= 3.402823466e38f)) f = 2u;
    if (threadIdx.x == 0) *flag = f;
    if (f != 1u) return;
    if (first == last) { first = first - 0.5f; last = last + 0.5f; }
    const float delta = last - first;
    const float div = (float)nbins;
    const float step = delta / div;
    for (int i = threadIdx.x; i <= nbins; i += 64) {
        float y = (float)i;
        if (step == 0.0f) { y = y / div; y = y * delta; } else y = y * step;
        y = y + first;
        edges[i] = (i == nbins) ? last : y;
    }
}
__global__ void __launch_bounds__(64)
sample_edges_kernel(const unsigned int *__restrict__ res, int nbins, float *__restrict__ edges, unsigned int *__restrict__ flag) {
    build_edges(res, nbins, edges, flag);
}
// two records, one workgroup each
__global__ void __launch_bounds__(64)
sample_edges2_kernel(const unsigned int *__restrict__ resA, float *__restrict__ edgesA, unsigned int *__restrict__ flagA,
                     const unsigned int *__restrict__ resB, float *__restrict__ edgesB, unsigned int *__restrict__ flagB, int nbins) {
    if (blockIdx.x == 0) build_edges(resA, nbins, edgesA, flagA);
    else build_edges(resB, nbins, edgesB, flagB);
}

// numpy histogram fast path, float32 (numpy/lib/_histograms_impl.py): see include/nellie_amd.h
__device__ __forceinline__ void hist_add(float a, const float *s_edges, unsigned int *s_cnt, float first, float last, float denom, int nbins) {
    if (a > 0.0f && a >= first && a <= last) {
        const float fi = ((a - first) / denom) * (float)nbins;
        int idx = (int)fi;
        if (idx == nbins) idx -= 1;
        if (a < s_edges[idx]) idx -= 1;
        if (a >= s_edges[idx + 1] && idx != nbins - 1) idx += 1;
        atomicAdd(&s_cnt[idx], 1u);
    }
}

__global__ void __launch_bounds__(256)
sample_hist_kernel(FieldSrc fs, VolGeom v, Lattice L, const float *__restrict__ edges, int nbins,
                   unsigned long long *__restrict__ counts, const unsigned int *__restrict__ flag) {
    if (flag && *flag != 1u) return;                         // uniform: nothing to bin
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *s_edges = (float *)smem;                          // nbins+1
    unsigned int *s_cnt = (unsigned int *)(s_edges + nbins + 1 + ((nbins + 1) & 1));   // nbins
    for (int k = threadIdx.x; k <= nbins; k += blockDim.x) s_edges[k] = edges[k];
    for (int k = threadIdx.x; k < nbins; k += blockDim.x) s_cnt[k] = 0;
    __syncthreads();
    const float first = s_edges[0], last = s_edges[nbins];
    const float denom = last - first;
    const i64 total = L.cz * L.cy * L.cx;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        i64 ix, iy, iz; lattice_split(L, i, ix, iy, iz);
        hist_add(field_value(fs, v, i, L.zfirst + iz * L.sz, iy * L.sy, ix * L.sx), s_edges, s_cnt, first, last, denom, nbins);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nbins; k += blockDim.x)
        if (s_cnt[k]) atomicAdd(&counts[k], (unsigned long long)s_cnt[k]);
}

// Both histograms of a scale's first round in one pass (the Gaussian samples and the cached frob_sq under fsF's normalisation).
// Dynamic LDS: 2 x the layout of sample_hist_kernel.
__global__ void __launch_bounds__(256)
sample_hist2_kernel(FieldSrc fsG, FieldSrc fsF, VolGeom v, Lattice L, int nbins,
                    const float *__restrict__ edgesG, unsigned long long *__restrict__ countsG, const unsigned int *__restrict__ flagG,
                    const float *__restrict__ edgesF, unsigned long long *__restrict__ countsF, const unsigned int *__restrict__ flagF) {
    const bool doG = *flagG == 1u, doF = *flagF == 1u;       // uniform
    if (!doG && !doF) return;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int ne = nbins + 1 + ((nbins + 1) & 1);
    float *s_eG = (float *)smem;
    unsigned int *s_cG = (unsigned int *)(s_eG + ne);
    float *s_eF = (float *)(s_cG + nbins);
    unsigned int *s_cF = (unsigned int *)(s_eF + ne);
    for (int k = threadIdx.x; k <= nbins; k += blockDim.x) { s_eG[k] = doG ? edgesG[k] : 0.0f; s_eF[k] = doF ? edgesF[k] : 0.0f; }
    for (int k = threadIdx.x; k < nbins; k += blockDim.x) { s_cG[k] = 0; s_cF[k] = 0; }
    __syncthreads();
    const float firstG = s_eG[0], lastG = s_eG[nbins], denomG = lastG - firstG;
    const float firstF = s_eF[0], lastF = s_eF[nbins], denomF = lastF - firstF;
    const i64 total = L.cz * L.cy * L.cx;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        i64 ix, iy, iz; lattice_split(L, i, ix, iy, iz);
        if (doG) hist_add(fsG.p[((L.zfirst + iz * L.sz) * v.ny + iy * L.sy) * v.nx + ix * L.sx], s_eG, s_cG, firstG, lastG, denomG, nbins);
        if (doF) hist_add(field_value(fsF, v, i, 0, 0, 0), s_eF, s_cF, firstF, lastF, denomF, nbins);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < nbins; k += blockDim.x) {
        if (s_cG[k]) atomicAdd(&countsG[k], (unsigned long long)s_cG[k]);
        if (s_cF[k]) atomicAdd(&countsF[k], (unsigned long long)s_cF[k]);
    }
}

__global__ void __launch_bounds__(256)
flat_gather_kernel(const float *__restrict__ p, i64 base, i64 offset, i64 step, i64 count, float *__restrict__ out) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = p[base + offset + i * step];
}

// Positive samples only, compacted (order unspecified: the consumers -- percentile, min/max, histogram -- do not
// depend on it).  One atomic per wave.
__device__ __forceinline__ void append_positive(float val, bool in_range, float *__restrict__ out, unsigned int *__restrict__ counter) {
    const bool pos = in_range && val > 0.0f;
    const unsigned long long bal = __ballot(pos);
    if (!bal) return;
    const int lane = threadIdx.x & 63;
    const int leader = __builtin_ctzll(bal);
    unsigned int base = 0;
    if (lane == leader) base = atomicAdd(counter, (unsigned int)__builtin_popcountll(bal));
    base = __shfl(base, leader, 64);
    if (pos) out[base + __builtin_amdgcn_mbcnt_hi((unsigned int)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)bal, 0u))] = val;
}

__global__ void __launch_bounds__(256)
sample_gather_pos_kernel(FieldSrc fs, VolGeom v, Lattice L, float *__restrict__ out, unsigned int *__restrict__ counter) {
    const i64 total = L.cz * L.cy * L.cx;
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    float val = 0.0f;
    if (i < total) {
        i64 ix, iy, iz; lattice_split(L, i, ix, iy, iz);
        val = field_value(fs, v, i, L.zfirst + iz * L.sz, iy * L.sy, ix * L.sx);
    }
    append_positive(val, i < total, out, counter);
}

__global__ void __launch_bounds__(256)
flat_gather_pos_kernel(const float *__restrict__ p, i64 base, i64 offset, i64 step, i64 count, float *__restrict__ out,
                       unsigned int *__restrict__ counter) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    const float val = (i < count) ? p[base + offset + i * step] : 0.0f;
    append_positive(val, i < count, out, counter);
}
