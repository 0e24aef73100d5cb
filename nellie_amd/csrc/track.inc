// Hu-moment marker tracking (nellie/tracking/hu_tracking.py, dense ROI path): per-frame features and frame-pair matching.
// Included by nellie_hip_track.hip only.  DESIGN.md "Tracking" states the arithmetic each kernel reproduces.
#pragma once

#define TRK_CHUNK 4096         // voxels per workgroup of the ordered marker compaction (16 per lane)
#define TRK_NH_MAX 18          // log-Hu features per marker (3-D: three projections x 6)
#define TRK_NF_MAX (1 + 4 + TRK_NH_MAX)

// ---- float16 helpers (host and device): numpy's float64 -> float16 cast and the float32 pairwise sum of np.nansum ---------
__host__ __device__ inline uint16_t trk_f64_to_f16(double x) {
    uint64_t b;
    memcpy(&b, &x, 8);
    const uint16_t sign = (uint16_t)((b >> 48) & 0x8000u);
    const uint64_t ab = b & 0x7fffffffffffffffull;
    if (ab >= 0x7ff0000000000000ull) return sign | (ab > 0x7ff0000000000000ull ? 0x7e00u : 0x7c00u);
    const int e = (int)(ab >> 52) - 1023;
    if (e < -25) return sign;                                    // below half the smallest subnormal (ties to even: 0)
    if (e > 15) return sign | 0x7c00u;
    const uint64_t m = (ab & 0xfffffffffffffull) | (1ull << 52);
    const int shift = e >= -14 ? 42 : 28 - e;                    // normal: 10 mantissa bits; subnormal: units of 2^-24
    uint64_t r = m >> shift;
    const uint64_t rem = m & ((1ull << shift) - 1), half = 1ull << (shift - 1);
    if (rem > half || (rem == half && (r & 1))) ++r;
    uint32_t bits = e >= -14 ? (uint32_t)(((e + 15 - 1) << 10) + r) : (uint32_t)r;   // a mantissa carry moves into the exponent
    if (bits >= 0x7c00u) bits = 0x7c00u;
    return sign | (uint16_t)bits;
}

__host__ __device__ inline float trk_f16_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    const uint32_t e = (h >> 10) & 0x1f, m = h & 0x3ffu;
    uint32_t bits;
    if (e == 0x1f) bits = sign | 0x7f800000u | (m << 13);
    else if (e) bits = sign | ((e + 112) << 23) | (m << 13);
    else if (!m) bits = sign;
    else {                                                        // subnormal half -> normal float
        int k = 0;
        uint32_t mm = m;
        while (!(mm & 0x400u)) { mm <<= 1; ++k; }
        bits = sign | ((uint32_t)(113 - k) << 23) | ((mm & 0x3ffu) << 13);
    }
    float f;
    memcpy(&f, &bits, 4);
    return f;
}

// float32 -> float16, round to nearest even (numpy's npy_float_to_half)
__host__ __device__ inline uint16_t trk_f32_to_f16(float f) { return trk_f64_to_f16((double)f); }   // exact: a float32 is a double,
                                                                                                      // rounding it once is the same

// np.nansum over k float16 values: NaN -> 0, float32 pairwise sum (8 accumulators below 128 items), rounded to half
__host__ __device__ inline uint16_t trk_half_nansum(const uint16_t *h, int k) {
    float a[TRK_NF_MAX];
    for (int i = 0; i < k; ++i) {
        const float v = trk_f16_to_f32(h[i]);
        a[i] = v != v ? 0.0f : v;
    }
    float res;
    if (k < 8) {
        res = 0.0f;
        for (int i = 0; i < k; ++i) res = res + a[i];
    } else {
        float r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        for (int i = 8; i < k - k % 8; i += 8)
            for (int j = 0; j < 8; ++j) r[j] = r[j] + a[i + j];
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (int i = k - k % 8; i < k; ++i) res = res + a[i];
    }
    return trk_f32_to_f16(res);
}

// ---- numpy's float32 np.sum of a flat array (the float stats, DESIGN.md "Tracking"): the array is cut into 8192-item blocks
// (the ufunc buffer), whose sums are added in order into a float32 accumulator starting at 0.  A block is numpy's
// pairwise_sum: below 8 items in sequence, up to 128 items 8 strided accumulators, above that split at n/2 - (n/2) % 8.
// The split tree of a block has at most 65 leaves (64..128 items each, or one leaf when the block has <= 128 items) and
// depth <= 7; a leaf is packed as offset | length << 13 | depth << 21.
#define TRK_PW_BLOCK 8192
#define TRK_PW_MAXLEAF 72

__host__ __device__ inline int trk_pw_leaves(int L, unsigned int *leaf) {
    int so[16], sl[16], sd[16], sp = 0, nl = 0;
    so[0] = 0; sl[0] = L; sd[0] = 0; sp = 1;
    while (sp > 0) {
        --sp;
        const int o = so[sp], l = sl[sp], d = sd[sp];
        if (l <= 128) { leaf[nl++] = (unsigned int)o | ((unsigned int)l << 13) | ((unsigned int)d << 21); continue; }
        int n2 = l / 2;
        n2 -= n2 % 8;
        so[sp] = o + n2; sl[sp] = l - n2; sd[sp] = d + 1; ++sp;   // right pushed first: leaves come out left to right
        so[sp] = o; sl[sp] = n2; sd[sp] = d + 1; ++sp;
    }
    return nl;
}

// one leaf of pairwise_sum (n <= 128 items)
__host__ __device__ inline float trk_pw_leaf(const float *a, int n) {
    if (n < 8) {
        float res = 0.0f;
        for (int i = 0; i < n; ++i) res = res + a[i];
        return res;
    }
    float r[8];
    for (int j = 0; j < 8; ++j) r[j] = a[j];
    for (int i = 8; i < n - n % 8; i += 8)
        for (int j = 0; j < 8; ++j) r[j] = r[j] + a[i + j];
    float res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (int i = n - n % 8; i < n; ++i) res = res + a[i];
    return res;
}

// the block's sum from its leaf sums (left to right): a completed subtree is added to the stack's top while both have one depth
__host__ __device__ inline float trk_pw_combine(const float *ls, const unsigned int *leaf, int nl) {
    float v[16];
    int d[16], sp = 0;
    for (int k = 0; k < nl; ++k) {
        float x = ls[k];
        int e = (int)(leaf[k] >> 21);
        while (sp > 0 && d[sp - 1] == e) { x = v[--sp] + x; --e; }
        v[sp] = x; d[sp] = e; ++sp;
    }
    return v[0];
}

__host__ __device__ inline float trk_np_sum_f32(const float *a, i64 n) {
    unsigned int leaf[TRK_PW_MAXLEAF];
    float ls[TRK_PW_MAXLEAF];
    float acc = 0.0f;
    int nl = 0, Lp = -1;
    for (i64 b = 0; b < n; b += TRK_PW_BLOCK) {
        const int L = (int)(n - b < TRK_PW_BLOCK ? n - b : TRK_PW_BLOCK);
        if (L != Lp) { nl = trk_pw_leaves(L, leaf); Lp = L; }
        for (int k = 0; k < nl; ++k) ls[k] = trk_pw_leaf(a + b + (leaf[k] & 0x1fffu), (int)((leaf[k] >> 13) & 0xffu));
        acc = acc + trk_pw_combine(ls, leaf, nl);
    }
    return acc;
}

// np.mean(row) of a float64 row of k <= 18 items: the same pairwise order in float64, then / k
__device__ inline double trk_mean_f64(const double *a, int k) {
    double res;
    if (k < 8) {
        res = 0.0;
        for (int i = 0; i < k; ++i) res = res + a[i];
    } else {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        for (int i = 8; i < k - k % 8; i += 8)
            for (int j = 0; j < 8; ++j) r[j] = r[j] + a[i + j];
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (int i = k - k % 8; i < k; ++i) res = res + a[i];
    }
    return res / (double)k;
}

// order-preserving key of a float32 (ascending keys = ascending values); -0 == +0, NaN lowest (numpy's argmin returns the first NaN)
__device__ inline unsigned int trk_fkey(float f) {
    if (f != f) return 0u;
    if (f == 0.0f) f = 0.0f;
    const unsigned int u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ inline float trk_fkey_inv(unsigned int k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// ---- Frangi normalisation (hu_tracking.py:594-602): positives -> log10, then negatives minus their minimum ----------------
__global__ void trk_frangi_log_kernel(float *__restrict__ fr, i64 n, unsigned int *__restrict__ minkey) {
    __shared__ unsigned int s_min;
    if (threadIdx.x == 0) s_min = 0xffffffffu;
    __syncthreads();
    unsigned int mk = 0xffffffffu;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
        float v = fr[i];
        if (v > 0.0f) { v = (float)log10((double)v); fr[i] = v; }
        if (v < 0.0f) { const unsigned int k = trk_fkey(v); mk = k < mk ? k : mk; }
    }
    atomicMin(&s_min, mk);
    __syncthreads();
    if (threadIdx.x == 0 && s_min != 0xffffffffu) atomicMin(minkey, s_min);
}

__global__ void trk_frangi_shift_kernel(float *__restrict__ fr, i64 n, const unsigned int *__restrict__ minkey) {
    const unsigned int k = *minkey;
    if (k == 0xffffffffu) return;                                 // no negative value
    const float mn = trk_fkey_inv(k);
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
        const float v = fr[i];
        if (v < 0.0f) fr[i] = v - mn;
    }
}

// ---- markers in np.argwhere (raster) order: per-chunk counts, one-workgroup exclusive scan, ordered write -----------------
__global__ __launch_bounds__(256) void trk_mark_count_kernel(const uint8_t *__restrict__ mk, i64 n, unsigned int *__restrict__ blk) {
    __shared__ unsigned int s;
    if (threadIdx.x == 0) s = 0;
    __syncthreads();
    const i64 base = (i64)blockIdx.x * TRK_CHUNK;
    unsigned int c = 0;
    for (int it = 0; it < TRK_CHUNK / 256; ++it) {
        const i64 i = base + it * 256 + threadIdx.x;
        c += (i < n && mk[i] != 0) ? 1u : 0u;
    }
    atomicAdd(&s, c);
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = s;
}

// exclusive scan of nblk counts in place, total in *total (one workgroup of 1024 lanes, each a contiguous segment)
__global__ __launch_bounds__(1024) void trk_scan_kernel(unsigned int *__restrict__ blk, i64 nblk, unsigned int *__restrict__ total) {
    __shared__ unsigned int part[1024];
    const i64 seg = (nblk + 1023) / 1024;
    const i64 a = threadIdx.x * seg, b = a + seg < nblk ? a + seg : nblk;
    unsigned int s = 0;
    for (i64 i = a; i < b; ++i) s += blk[i];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int run = 0;
        for (int t = 0; t < 1024; ++t) { const unsigned int v = part[t]; part[t] = run; run += v; }
        *total = run;
    }
    __syncthreads();
    unsigned int run = part[threadIdx.x];
    for (i64 i = a; i < b; ++i) { const unsigned int v = blk[i]; blk[i] = run; run += v; }
}

__global__ __launch_bounds__(256) void trk_mark_write_kernel(const uint8_t *__restrict__ mk, i64 n, const unsigned int *__restrict__ blk,
                                                             int *__restrict__ coord, int ny, int nx) {
    __shared__ unsigned int wtot[4];
    const i64 base = (i64)blockIdx.x * TRK_CHUNK;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned int run = blk[blockIdx.x];
    for (int it = 0; it < TRK_CHUNK / 256; ++it) {
        const i64 i = base + it * 256 + threadIdx.x;
        const bool f = i < n && mk[i] != 0;
        const unsigned long long bal = __ballot(f);
        const unsigned int before = (unsigned int)__popcll(bal & ((1ull << lane) - 1ull));
        if (lane == 0) wtot[w] = (unsigned int)__popcll(bal);
        __syncthreads();
        unsigned int off = run;
        for (int k = 0; k < w; ++k) off += wtot[k];
        if (f) {
            const unsigned int o = off + before;
            const i64 x = i % nx, yz = i / nx;
            coord[3 * (i64)o + 0] = (int)(yz / ny);
            coord[3 * (i64)o + 1] = (int)(yz % ny);
            coord[3 * (i64)o + 2] = (int)x;
        }
        run += wtot[0] + wtot[1] + wtot[2] + wtot[3];
        __syncthreads();
    }
}

// ---- radii: ceil(2 * max3x3x3(distance)) at the markers (size-3 maximum filter, faces clamped = scipy's 'reflect') ----------
__global__ void trk_radius_kernel(const int *__restrict__ coord, int n, const float *__restrict__ dist, int nz, int ny, int nx,
                                  const double *__restrict__ scale, double *__restrict__ phys, int *__restrict__ rad,
                                  int *__restrict__ rmax) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const int z = coord[3 * k], y = coord[3 * k + 1], x = coord[3 * k + 2];
    float m = -INFINITY;
    for (int dz = -1; dz <= 1; ++dz) {
        const int zz = min(max(z + dz, 0), nz - 1);
        for (int dy = -1; dy <= 1; ++dy) {
            const int yy = min(max(y + dy, 0), ny - 1);
            for (int dx = -1; dx <= 1; ++dx) {
                const int xx = min(max(x + dx, 0), nx - 1);
                m = fmaxf(m, dist[((i64)zz * ny + yy) * nx + xx]);
            }
        }
    }
    const float r = ceilf(m * 2.0f);
    const int ri = r > 1e6f ? 1000000 : (r < 0.0f ? 0 : (int)r);
    rad[k] = ri;
    atomicMax(rmax, ri);
    phys[3 * k + 0] = (double)z * scale[0];
    phys[3 * k + 1] = (double)y * scale[1];
    phys[3 * k + 2] = (double)x * scale[2];
}

// ---- per-marker features: one workgroup per marker ------------------------------------------------------------------------
template <typename T> struct TrkAcc { typedef double S; };
template <> struct TrkAcc<uint8_t> { typedef unsigned long long S; };
template <> struct TrkAcc<uint16_t> { typedef unsigned long long S; };

// block sums of NV values (fixed order: wave butterfly, then the four waves in order) -- deterministic
template <typename S, int NV>
__device__ inline void trk_block_sum(S (&v)[NV], S *lds /* 4 * NV */) {
    for (int j = 0; j < NV; ++j)
        for (int o = 32; o > 0; o >>= 1) v[j] = v[j] + __shfl_xor(v[j], o);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0)
        for (int j = 0; j < NV; ++j) lds[w * NV + j] = v[j];
    __syncthreads();
    for (int j = 0; j < NV; ++j) v[j] = ((lds[j] + lds[NV + j]) + lds[2 * NV + j]) + lds[3 * NV + j];
    __syncthreads();
}

// [mean, variance] with the reference's dtypes.  Integer inputs wrap their squares in the input dtype, sum in uint64 and square
// the sum in uint64 (modular: exact in any order).  Float32 inputs take the float32 sums of trk_np_sums_roi and square the
// sum in float32, as numpy does.
__device__ inline void trk_stats_store_int(unsigned long long cnt, unsigned long long s, unsigned long long sq, float *out) {
    if (cnt == 0) { out[0] = 0.0f; out[1] = 0.0f; return; }
    const double c = (double)cnt;
    const unsigned long long s2 = s * s;
    out[0] = (float)((double)s / c);
    out[1] = (float)(((double)sq - (double)s2 / c) / c);
}

__device__ inline void trk_stats_store_f32(unsigned long long cnt, float s, float sq, float *out) {
    if (cnt == 0) { out[0] = 0.0f; out[1] = 0.0f; return; }
    const double c = (double)cnt;
    out[0] = (float)((double)s / c);
    out[1] = (float)(((double)sq - (double)(s * s) / c) / c);
}

struct TrkPwLds {
    unsigned int leaf[TRK_PW_MAXLEAF];
    float ls[2][TRK_PW_MAXLEAF];
    int nl;
};

// trk_np_sum_f32 of get(e) and of get(e) * get(e) over e < n, by the whole workgroup (uniform n); the sums land in thread 0.
// A leaf is summed by a group of 8 lanes, lane j holding accumulator j, and the lanes' butterfly is numpy's
// ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)) (float addition commutes; only the grouping matters).
template <typename G>
__device__ inline void trk_np_sums_roi(i64 n, G get, TrkPwLds &P, float &s, float &sq) {
    const int j = threadIdx.x & 7, g = threadIdx.x >> 3, ng = blockDim.x >> 3;
    float acc0 = 0.0f, acc1 = 0.0f;
    int Lp = -1;
    for (i64 b = 0; b < n; b += TRK_PW_BLOCK) {
        const int L = (int)(n - b < TRK_PW_BLOCK ? n - b : TRK_PW_BLOCK);
        if (L != Lp) {
            if (threadIdx.x == 0) P.nl = trk_pw_leaves(L, P.leaf);
            __syncthreads();
            Lp = L;
        }
        const int nl = P.nl;
        for (int k = g; k < nl; k += ng) {
            const unsigned int lf = P.leaf[k];
            const i64 o = b + (lf & 0x1fffu);
            const int l = (int)((lf >> 13) & 0xffu), e8 = l - l % 8;
            float r0 = 0.0f, r1 = 0.0f;
            if (l >= 8) {
                r0 = get(o + j);
                r1 = r0 * r0;
                for (int i = 8 + j; i < e8; i += 8) { const float v = get(o + i); r0 = r0 + v; r1 = r1 + v * v; }
                for (int m = 1; m < 8; m <<= 1) { r0 = r0 + __shfl_xor(r0, m); r1 = r1 + __shfl_xor(r1, m); }
            }
            if (j == 0) {
                for (int i = e8; i < l; ++i) { const float v = get(o + i); r0 = r0 + v; r1 = r1 + v * v; }
                P.ls[0][k] = r0;
                P.ls[1][k] = r1;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            acc0 = acc0 + trk_pw_combine(P.ls[0], P.leaf, nl);
            acc1 = acc1 + trk_pw_combine(P.ls[1], P.leaf, nl);
        }
        __syncthreads();                                          // leaf sums (and leaves) are rewritten by the next block
    }
    s = acc0;
    sq = acc1;
}

template <typename T> __device__ inline unsigned long long trk_sq(T v) {
    return (unsigned long long)(T)(v * v);                        // wraps in the input dtype like numpy's ** 2
}

__device__ inline void trk_hu(const double (&eta)[4][4], double *lh) {
    const double e20 = eta[2][0], e02 = eta[0][2], e11 = eta[1][1], e30 = eta[3][0], e12 = eta[1][2], e21 = eta[2][1], e03 = eta[0][3];
    const double a = e30 + e12, b = e21 + e03, c = e30 - 3 * e12, d = 3 * e21 - e03, f = e20 - e02;
    double hu[6];
    hu[0] = e20 + e02;
    hu[1] = f * f + 4 * (e11 * e11);
    hu[2] = c * c + d * d;
    hu[3] = a * a + b * b;
    hu[4] = (c * a) * (a * a - 3 * (b * b)) + (d * b) * (3 * (a * a) - b * b);
    hu[5] = f * (a * a - b * b) + ((4 * e11) * a) * b;
    for (int k = 0; k < 6; ++k) {
        const double m = fmax(fabs(hu[k]), 2.2250738585072014e-308);
        const double sg = hu[k] > 0 ? 1.0 : (hu[k] < 0 ? -1.0 : 0.0);
        const double l = -sg * log10(m);
        lh[k] = isfinite(l) ? l : 0.0;
    }
}

// moments of the image in `tile` (h rows = y, w columns = x; zero outside) -> six log-Hu values
template <typename T>
__device__ void trk_tile_hu(const float *tile, int h, int w, double *lds, double *out) {
    typedef typename TrkAcc<T>::S S;
    S m[16];
    for (int j = 0; j < 16; ++j) m[j] = 0;
    for (int i = threadIdx.x; i < h * w; i += blockDim.x) {
        const int y = i / w, x = i % w;
        const float v = tile[i];
        if constexpr (std::is_same<S, double>::value) {
            const double xp[4] = {1.0, (double)x, (double)(x * x), (double)(x * x * x)};
            const double yp[4] = {1.0, (double)y, (double)(y * y), (double)(y * y * y)};
            for (int p = 0; p < 4; ++p)
                for (int q = 0; q < 4; ++q) m[p * 4 + q] += ((double)v * xp[p]) * yp[q];
        } else {
            const unsigned long long iv = (unsigned long long)(long long)v;
            const unsigned long long xp[4] = {1ull, (unsigned long long)x, (unsigned long long)(x * x), (unsigned long long)x * x * x};
            const unsigned long long yp[4] = {1ull, (unsigned long long)y, (unsigned long long)(y * y), (unsigned long long)y * y * y};
            for (int p = 0; p < 4; ++p)
                for (int q = 0; q < 4; ++q) m[p * 4 + q] += (iv * xp[p]) * yp[q];    // int64 with wrapping, as numpy
        }
    }
    trk_block_sum<S, 16>(m, (S *)lds);
    double M[16];
    for (int j = 0; j < 16; ++j) {
        if constexpr (std::is_same<S, double>::value) M[j] = m[j];
        else M[j] = (double)(long long)m[j];
    }
    const double xb = M[4] / (M[0] + 1e-12), yb = M[1] / (M[0] + 1e-12);
    double mu[16];
    for (int j = 0; j < 16; ++j) mu[j] = 0.0;
    for (int i = threadIdx.x; i < h * w; i += blockDim.x) {
        const double v = (double)tile[i];
        if (v == 0.0) continue;
        const double dx = (double)(i % w) - xb, dy = (double)(i / w) - yb;
        const double xp[4] = {1.0, dx, dx * dx, dx * dx * dx}, yp[4] = {1.0, dy, dy * dy, dy * dy * dy};
        for (int p = 0; p < 4; ++p)
            for (int q = 0; q < 4; ++q) mu[p * 4 + q] += (v * xp[p]) * yp[q];
    }
    trk_block_sum<double, 16>(mu, lds);
    if (threadIdx.x == 0) {
        double eta[4][4];
        for (int p = 0; p < 4; ++p)
            for (int q = 0; q < 4; ++q) eta[p][q] = mu[p * 4 + q] / (pow(M[0], (p + q + 2) / 2.0) + 1e-12);
        trk_hu(eta, out);
    }
    __syncthreads();
}

struct TrkFrame {
    int nz, ny, nx, two_d, R;
    const float *fr;
    const int *coord, *rad;
    float *stats;       // (n, 4)
    double *hu;         // (n, 6 | 18)
};

template <typename T>
__global__ __launch_bounds__(256) void trk_features_kernel(const T *__restrict__ im, TrkFrame F) {
    extern __shared__ float tile[];                              // R * R floats
    __shared__ double lds[4 * 16];
    __shared__ TrkPwLds pw;
    const int k = blockIdx.x;
    const int r = F.rad[k];
    const int c[3] = {F.coord[3 * k], F.coord[3 * k + 1], F.coord[3 * k + 2]};
    const int dims[3] = {F.nz, F.ny, F.nx};
    int lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        if (F.two_d && a == 0) { lo[0] = 0; hi[0] = 1; continue; }
        lo[a] = max(c[a] - r, 0);
        hi[a] = min(c[a] + r + 1, dims[a]);
    }
    const int ez = hi[0] - lo[0], ey = hi[1] - lo[1], ex = hi[2] - lo[2];
    auto at = [&](int z, int y, int x) -> i64 { return ((i64)(lo[0] + z) * F.ny + (lo[1] + y)) * F.nx + (lo[2] + x); };

    // integer stats, non-zero counts and the Z projection (or the 2-D ROI itself): lane owns a (y, x) column
    unsigned long long si = 0, sqi = 0, ci = 0, cf = 0;
    const bool padz = ez < F.R;
    for (int i = threadIdx.x; i < F.R * F.R; i += blockDim.x) {
        const int y = i / F.R, x = i % F.R;
        float pm = 0.0f;
        if (y < ey && x < ex) {
            float mx = -INFINITY;
            for (int z = 0; z < ez; ++z) {
                const i64 o = at(z, y, x);
                const T v = im[o];
                if (v != (T)0) {
                    ++ci;
                    if constexpr (!std::is_same<T, float>::value) { si += (unsigned long long)v; sqi += trk_sq<T>(v); }
                }
                if (F.fr[o] != 0.0f) ++cf;
                mx = fmaxf(mx, (float)v);
            }
            pm = (padz && !F.two_d) ? fmaxf(mx, 0.0f) : mx;       // the dense path's zero padding joins the maximum
        }
        tile[i] = pm;
    }
    {
        unsigned long long v[4] = {si, sqi, ci, cf};
        trk_block_sum<unsigned long long, 4>(v, (unsigned long long *)lds);
        ci = v[2];
        cf = v[3];
        if (threadIdx.x == 0 && !std::is_same<T, float>::value) trk_stats_store_int(ci, v[0], v[1], F.stats + 4 * (i64)k);
    }
    // float32 stats: numpy's float32 sums over the ROI zero-padded to R^d and flattened (e = (z * R + y) * R + x)
    {
        const int R = F.R;
        const i64 nroi = F.two_d ? (i64)R * R : (i64)R * R * R;
        auto roi = [&](const auto *src, i64 e) -> float {
            const int z = (int)(e / ((i64)R * R)), yx = (int)(e - (i64)z * R * R), y = yx / R, x = yx - y * R;
            if (z >= ez || y >= ey || x >= ex) return 0.0f;
            const float v = (float)src[at(z, y, x)];
            return v != 0.0f ? v : 0.0f;
        };
        float s, sq;
        if constexpr (std::is_same<T, float>::value) {
            trk_np_sums_roi(nroi, [&](i64 e) { return roi(im, e); }, pw, s, sq);
            if (threadIdx.x == 0) trk_stats_store_f32(ci, s, sq, F.stats + 4 * (i64)k);
        }
        trk_np_sums_roi(nroi, [&](i64 e) { return roi(F.fr, e); }, pw, s, sq);
        if (threadIdx.x == 0) trk_stats_store_f32(cf, s, sq, F.stats + 4 * (i64)k + 2);
    }
    __syncthreads();
    const int nh = F.two_d ? 6 : 18;
    double *out = F.hu + (i64)nh * k;
    trk_tile_hu<T>(tile, F.R, F.R, lds, out);
    if (F.two_d) return;
    // Y projection: image (z rows, x columns); X projection: image (z rows, y columns)
    for (int pass = 0; pass < 2; ++pass) {
        const int el = pass == 0 ? ey : ex;                      // the axis the maximum runs over
        for (int i = threadIdx.x; i < F.R * F.R; i += blockDim.x) {
            const int z = i / F.R, u = i % F.R;
            float pm = 0.0f;
            if (z < ez && u < (pass == 0 ? ex : ey)) {
                float mx = -INFINITY;
                for (int t = 0; t < el; ++t) mx = fmaxf(mx, (float)im[pass == 0 ? at(z, t, u) : at(z, u, t)]);
                pm = el < F.R ? fmaxf(mx, 0.0f) : mx;
            }
            tile[i] = pm;
        }
        __syncthreads();
        trk_tile_hu<T>(tile, F.R, F.R, lds, out + 6 * (pass + 1));
    }
}

// ---- matching ---------------------------------------------------------------------------------------------------------------
// features as the matcher reads them: nf = 1 + 4 + nh doubles per marker are not stored; stats (float32) and log-Hu (float64)
// are read where the feature kernel left them.
struct TrkPair {
    int n_post, n_pre, ndim, nh;
    const double *phys_post, *phys_pre;
    const float *st_post, *st_pre;
    const double *hu_post, *hu_pre;
    double maxd;
};

__device__ inline double trk_dist(const TrkPair &P, int i, int j) {
    double s = 0.0;
    for (int a = 3 - P.ndim; a < 3; ++a) {
        const double d = P.phys_post[3 * (i64)i + a] - P.phys_pre[3 * (i64)j + a];
        s = s + d * d;
    }
    return s;
}

// feature f of pair (i, j): 0 = distance / maxd, 1..4 = |d stats| (float64 of float32), 5.. = |d log-Hu| (float64)
__device__ inline double trk_feat(const TrkPair &P, int i, int j, int f, double dn) {
    if (f == 0) return dn;
    if (f < 5) return fabs((double)P.st_post[4 * (i64)i + f - 1] - (double)P.st_pre[4 * (i64)j + f - 1]);
    return fabs(P.hu_post[(i64)P.nh * i + f - 5] - P.hu_pre[(i64)P.nh * j + f - 5]);
}

// dense pass (a) / (b): per post row, sums over the masked pairs in j order of the features (a) or of their squared deviations
// from the means (b); row partials [n_post][1 + nf] (count first)
__global__ void trk_dense_rowsum_kernel(TrkPair P, const double *__restrict__ mean, double *__restrict__ part) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n_post) return;
    const int nf = 5 + P.nh;
    double acc[TRK_NF_MAX];
    for (int f = 0; f < nf; ++f) acc[f] = 0.0;
    double cnt = 0.0;
    for (int j = 0; j < P.n_pre; ++j) {
        const double d = sqrt(trk_dist(P, i, j));
        if (!(d < P.maxd)) continue;
        cnt += 1.0;
        const double dn = d / P.maxd;
        for (int f = 0; f < nf; ++f) {
            const double m = trk_feat(P, i, j, f, dn);
            if (mean) { const double e = m - mean[f]; acc[f] += e * e; }
            else acc[f] += m;
        }
    }
    double *o = part + (i64)(1 + nf) * i;
    o[0] = cnt;
    for (int f = 0; f < nf; ++f) o[1 + f] = acc[f];
}

// rows -> totals in row order, one lane per column of the partials; out[f] = total_f / count (the mean), or with stdev set
// sqrt(total_f / count) + 1e-8 (the std of _zscore_normalize)
__global__ void trk_colsum_kernel(const double *__restrict__ part, int nrows, int ncol, int stdev, double *__restrict__ out) {
    const int f = threadIdx.x;
    if (f >= ncol) return;
    double s = 0.0, c = 0.0;
    for (int i = 0; i < nrows; ++i) { s += part[(i64)(1 + ncol) * i + 1 + f]; c += part[(i64)(1 + ncol) * i]; }
    const double v = c > 0 ? s / c : 0.0;
    out[f] = stdev ? sqrt(v) + 1e-8 : v;
}

// half cost of one masked pair (hu_tracking.py:866-891)
__device__ inline uint16_t trk_dense_cost(const TrkPair &P, int i, int j, double d, const double *mean, const double *stdv) {
    const int nf = 5 + P.nh;
    uint16_t h[TRK_NF_MAX];
    const double dn = d / P.maxd;
    for (int f = 0; f < nf; ++f) {
        double z = (trk_feat(P, i, j, f, dn) - mean[f]) / stdv[f];
        if (f >= 1 && f < 5) z = z / 4.0;
        else if (f >= 5) z = z / (double)P.nh;
        h[f] = trk_f64_to_f16(z);
    }
    return trk_half_nansum(h, nf);
}

// dense pass (c): row minima (lane per post row) or column minima (lane per pre column), numpy's argmin rule (first index on ties,
// NaN first); masked-out pairs cost +inf.  full != NULL also stores the whole half matrix (tests).
__global__ void trk_dense_min_kernel(TrkPair P, const double *__restrict__ mean, const double *__restrict__ stdv, int by_col,
                                     int *__restrict__ idx_out, float *__restrict__ val_out, uint16_t *__restrict__ full) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    const int na = by_col ? P.n_pre : P.n_post, nb = by_col ? P.n_post : P.n_pre;
    if (a >= na) return;
    unsigned int best = 0xffffffffu;
    int bi = 0;
    const unsigned int kinf = trk_fkey(INFINITY);
    for (int b = 0; b < nb; ++b) {
        const int i = by_col ? b : a, j = by_col ? a : b;
        const double d = sqrt(trk_dist(P, i, j));
        unsigned int key = kinf;
        uint16_t hc = 0x7c00u;
        if (d < P.maxd) {
            hc = trk_dense_cost(P, i, j, d, mean, stdv);
            key = trk_fkey(trk_f16_to_f32(hc));
        }
        if (full && !by_col) full[(i64)i * P.n_pre + j] = hc;
        if (key < best) { best = key; bi = b; }
    }
    idx_out[a] = bi;
    val_out[a] = best == 0u ? NAN : trk_fkey_inv(best);
}

// ---- sparse matching (hu_tracking.py:947-1095): candidates are the pairs with squared distance <= maxd^2 (cKDTree's
// query_ball_point), visited in ascending index order like its sorted lists
__device__ inline void trk_sparse_feats(const TrkPair &P, int i, int j, double *m) {
    m[0] = sqrt(trk_dist(P, i, j)) / P.maxd;
    for (int f = 0; f < 4; ++f) m[1 + f] = (double)fabsf(P.st_post[4 * (i64)i + f] - P.st_pre[4 * (i64)j + f]);
    for (int f = 0; f < P.nh; ++f) m[5 + f] = (double)fabsf((float)P.hu_post[(i64)P.nh * i + f] - (float)P.hu_pre[(i64)P.nh * j + f]);
}

// per post row: [count, sum_f, sum of squares_f] over its candidates (squares of the float32 differences in float32)
__global__ void trk_sparse_rowsum_kernel(TrkPair P, double *__restrict__ part) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P.n_post) return;
    const int nf = 5 + P.nh;
    const double r2 = P.maxd * P.maxd;
    double s[TRK_NF_MAX], q[TRK_NF_MAX], m[TRK_NF_MAX];
    for (int f = 0; f < nf; ++f) { s[f] = 0.0; q[f] = 0.0; }
    double cnt = 0.0;
    for (int j = 0; j < P.n_pre; ++j) {
        if (!(trk_dist(P, i, j) <= r2)) continue;
        cnt += 1.0;
        trk_sparse_feats(P, i, j, m);
        s[0] += m[0]; q[0] += m[0] * m[0];
        for (int f = 1; f < nf; ++f) { s[f] += m[f]; const float v = (float)m[f]; q[f] += (double)(v * v); }
    }
    double *o = part + (i64)(1 + 2 * nf) * i;
    o[0] = cnt;
    for (int f = 0; f < nf; ++f) { o[1 + f] = s[f]; o[1 + nf + f] = q[f]; }
}

// totals in row order -> mean and std (E[x^2] - mean^2, clamped at 0, + 1e-8) per feature: ms[0..nf) means, ms[nf..2nf) stds
__global__ void trk_sparse_moments_kernel(const double *__restrict__ part, int nrows, int nf, double *__restrict__ ms) {
    const int f = threadIdx.x;
    if (f >= nf) return;
    double s = 0.0, q = 0.0, c = 0.0;
    for (int i = 0; i < nrows; ++i) {
        const double *o = part + (i64)(1 + 2 * nf) * i;
        c += o[0]; s += o[1 + f]; q += o[1 + nf + f];
    }
    const double mean = c > 0 ? s / c : 0.0;
    const double var = c > 0 ? fmax(q / c - mean * mean, 0.0) : 0.0;
    ms[f] = mean;
    ms[nf + f] = sqrt(var) + 1e-8;
}

__device__ inline double trk_sparse_cost(const TrkPair &P, int i, int j, const double *ms) {
    const int nf = 5 + P.nh;
    double m[TRK_NF_MAX], zs[4], zh[TRK_NH_MAX];
    trk_sparse_feats(P, i, j, m);
    const double zd = (m[0] - ms[0]) / ms[nf];
    for (int f = 0; f < 4; ++f) zs[f] = (m[1 + f] - ms[1 + f]) / ms[nf + 1 + f];
    for (int f = 0; f < P.nh; ++f) zh[f] = (m[5 + f] - ms[5 + f]) / ms[nf + 5 + f];
    return (zd + trk_mean_f64(zs, 4)) + trk_mean_f64(zh, P.nh);
}

// row pass: argmin over the candidates with cost <= 1 (first index on ties), stored as float32;
// column pass: candidates in ascending post index, `c < stored float32 minimum` replaces it (hu_tracking.py:1071-1075)
__global__ void trk_sparse_min_kernel(TrkPair P, const double *__restrict__ ms, int by_col, int *__restrict__ idx_out, float *__restrict__ val_out) {
    const int a = blockIdx.x * blockDim.x + threadIdx.x;
    const int na = by_col ? P.n_pre : P.n_post, nb = by_col ? P.n_post : P.n_pre;
    if (a >= na) return;
    const double r2 = P.maxd * P.maxd;
    int bi = -1;
    double best = INFINITY;
    float bestf = INFINITY;
    for (int b = 0; b < nb; ++b) {
        const int i = by_col ? b : a, j = by_col ? a : b;
        if (!(trk_dist(P, i, j) <= r2)) continue;
        const double c = trk_sparse_cost(P, i, j, ms);
        if (!(c <= 1.0)) continue;
        if (by_col) {
            if (c < (double)bestf) { bestf = (float)c; bi = b; }
        } else if (c < best) { best = c; bi = b; }
    }
    idx_out[a] = bi;
    val_out[a] = by_col ? bestf : (float)best;
}
