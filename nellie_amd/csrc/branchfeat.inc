// Branch-level features (Branches of nellie/feature_extraction/hierarchical.py) -- kernels of nellie_hip_branchfeat.hip
// (DESIGN.md section 16).
//
// Everything that touches voxels: the skeleton list (the voxels with skeleton label > 0, compacted in raster order by the mask,
// scan and rank of rank_scan.inc), the distinct labels (a presence bit per label value in [0, max label], ranked by the same scan,
// so every per-label array is dense: one row per label present, whatever the values), per skeleton voxel its degree (same-label
// neighbours) and its radius (nf_nearest_sq of nodefeat.inc over the border bits), per label the same-label pairs per "positive"
// offset, the sorted list of 2 * radius and its median, and over the full branch-label volume the exact integer sums of every
// region and the most frequent reassigned label.  The organelle level (DESIGN.md section 18) takes the same sums over the
// component-label volume per run of equal labels along X.
//
// Per-label lists are one sorted array: keys (label rank, value) go through a bitonic sort of the whole array, padded with keys
// above all others to a power of two, after which label b's values lie sorted at [off[b], off[b + 1]).  A group may have any size.
//
// Every count and sum is an integer atomic; nothing depends on the order in which lanes finish: two runs give the same bits.
#pragma once
#include "nodefeat.inc"

#define BF_NOFF3 13                   // "positive" offsets of the 26-neighbourhood: the first non-zero component is +1
#define BF_NOFF2 4                    // and of the 8-neighbourhood

// ---- labels ----------------------------------------------------------------------------------------------------------------------
// element i of an integer array as int64 (the host refuses float dtypes); a uint64 above 2^63 - 1 reads as negative: no label
__device__ __forceinline__ i64 bf_int(const void *__restrict__ p, int dtype, i64 i) {
    switch (dtype) {
        case NL_U8: return ((const uint8_t *)p)[i];
        case NL_I8: return ((const int8_t *)p)[i];
        case NL_U16: return ((const uint16_t *)p)[i];
        case NL_I16: return ((const int16_t *)p)[i];
        case NL_U32: return ((const uint32_t *)p)[i];
        case NL_I32: return ((const int32_t *)p)[i];
        case NL_U64: return (i64)((const uint64_t *)p)[i];
        default: return ((const int64_t *)p)[i];
    }
}

struct BfPositive {                   // rank_mask_kernel's predicate: label > 0
    const void *src;
    int dtype;
    __device__ bool operator()(i64 i) const { return bf_int(src, dtype, i) > 0; }
};

struct BfLabels {                     // the labels of a frame's voxels list[0 .. n), or (list == NULL) of all its voxels
    const void *src;
    int dtype;
    const i64 *list;
    __device__ i64 operator()(i64 k) const { return bf_int(src, dtype, list ? list[k] : k); }
};

struct BfDegreeIs {                   // rank_mask_kernel's predicate over the skeleton list: degree == want
    const uint8_t *deg;
    int want;
    __device__ bool operator()(i64 k) const { return deg[k] == want; }
};

// One lane per element: top[0] = the largest label > 0 (the host zeroes it).
static __global__ __launch_bounds__(256) void bf_max_kernel(BfLabels lab, i64 n, u64 *__restrict__ top) {
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    i64 v = k < n ? lab(k) : 0;
    v = v > 0 ? v : 0;
    for (int w = 32; w > 0; w >>= 1) {
        const i64 o = __shfl_xor(v, w);
        v = o > v ? o : v;
    }
    if ((threadIdx.x & 63) == 0 && v > 0) atomicMax(top, (u64)v);
}

// One lane per element: the presence bit of every label > 0 (the host zeroes the words; every label is at most the maximum
// bf_max_kernel found over the same elements, which sized them).
static __global__ __launch_bounds__(256) void bf_present_kernel(BfLabels lab, i64 n, u64 *pres) {
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const i64 l = lab(k);
    if (l <= 0) return;
    const u64 bit = 1ull << (l & 63);
    if (!(pres[l >> 6] & bit)) atomicOr(&pres[l >> 6], bit);
}

static __global__ __launch_bounds__(256) void bf_popc_kernel(const u64 *__restrict__ pres, i64 words, int *__restrict__ wcount) {
    const i64 w = (i64)blockIdx.x * 256 + threadIdx.x;
    if (w < words) wcount[w] = __popcll(pres[w]);
}

// One lane per label value in [0, values): a present one writes itself at its rank -- the distinct labels, ascending.
static __global__ __launch_bounds__(256) void bf_uniq_kernel(const u64 *__restrict__ pres, const int *__restrict__ pre, i64 values, i64 *__restrict__ uniq) {
    const i64 l = (i64)blockIdx.x * 256 + threadIdx.x;
    if (l >= values) return;
    if ((pres[l >> 6] >> (l & 63)) & 1ull) uniq[ra_rank(pres, pre, l)] = l;
}

// ---- skeleton list ---------------------------------------------------------------------------------------------------------------
// One lane per skeleton voxel k (raster order): its label, the label's rank, the label's voxel count and its first voxel (the
// smallest k; the host sets first[] to all ones and zeroes count[]).
static __global__ __launch_bounds__(256) void bf_list_kernel(BfLabels lab, i64 m, const u64 *__restrict__ pres, const int *__restrict__ pre,
                                                            i64 *__restrict__ label, int *__restrict__ rank, int *__restrict__ count, u64 *__restrict__ first) {
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    if (k >= m) return;
    const i64 l = lab(k);                                              // > 0: the list holds the voxels of the mask label > 0
    const int r = ra_rank(pres, pre, l);
    label[k] = l;
    rank[k] = r;
    atomicAdd(&count[r], 1);
    atomicMin(&first[r], (u64)k);
}

// One lane per label: the linear index of its first voxel.
static __global__ __launch_bounds__(256) void bf_first_voxel_kernel(const u64 *__restrict__ first, const i64 *__restrict__ vox, i64 labels, i64 *__restrict__ out) {
    const i64 b = (i64)blockIdx.x * 256 + threadIdx.x;
    if (b < labels) out[b] = vox[first[b]];
}

// ---- degree and edge counts ------------------------------------------------------------------------------------------------------
// One lane per skeleton voxel: deg = its neighbours (26 in 3-D, 8 in 2-D) inside the frame that carry its label; for every positive
// offset, in the order dz, dy, dx each over -1, 0, 1, the pair (voxel, voxel + offset) is counted once in edges[rank * NOFF + j].
template <int D>
__global__ __launch_bounds__(256) void bf_degree_kernel(const void *__restrict__ skel, int dtype, const i64 *__restrict__ vox, const int *__restrict__ rank,
                                                        i64 m, NfGeom g, uint8_t *__restrict__ deg, unsigned int *__restrict__ edges) {
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    if (k >= m) return;
    const int NOFF = D == 3 ? BF_NOFF3 : BF_NOFF2;
    const i64 i = vox[k];
    const i64 l = bf_int(skel, dtype, i);
    const i64 z = i / (g.nx * g.ny), y = (i / g.nx) % g.ny, x = i % g.nx;
    unsigned int *row = edges + (i64)rank[k] * NOFF;
    int d = 0, j = 0;
    for (int dz = D == 3 ? -1 : 0; dz <= (D == 3 ? 1 : 0); ++dz)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if (dz == 0 && dy == 0 && dx == 0) continue;
                const bool positive = dz > 0 || (dz == 0 && dy > 0) || (dz == 0 && dy == 0 && dx > 0);
                const i64 zz = z + dz, yy = y + dy, xx = x + dx;
                const bool inside = zz >= 0 && zz < g.nz && yy >= 0 && yy < g.ny && xx >= 0 && xx < g.nx;
                if (inside && bf_int(skel, dtype, (zz * g.ny + yy) * g.nx + xx) == l) {
                    ++d;
                    if (positive) atomicAdd(&row[j], 1u);
                }
                j += positive;
            }
    deg[k] = (uint8_t)d;
}

// ---- radii -----------------------------------------------------------------------------------------------------------------------
// One wave per skeleton voxel: the distance in um to the nearest border voxel, NaN when the frame has none (*any_border == 0).
static __global__ __launch_bounds__(64) void bf_radius_kernel(const i64 *__restrict__ vox, i64 m, NfGeom g, const u64 *__restrict__ border,
                                                              const int *__restrict__ any_border, double *__restrict__ radius) {
    const i64 k = blockIdx.x;
    if (k >= m) return;
    if (*any_border == 0) {
        if (threadIdx.x == 0) radius[k] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    const double best = nf_nearest_sq(vox[k], g, border);
    if (threadIdx.x == 0) radius[k] = sqrt(best);
}

// One lane per rank of a compacted list: the positions k of the set bits of a mask over [0, m), in order.
static __global__ __launch_bounds__(256) void bf_positions_kernel(i64 m, const u64 *__restrict__ bits, const int *__restrict__ pre, i64 *__restrict__ out) {
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    if (k >= m) return;
    if ((bits[k >> 6] >> (k & 63)) & 1ull) out[ra_rank(bits, pre, k)] = k;
}

// ---- the sort --------------------------------------------------------------------------------------------------------------------
struct BfKey2 {                       // (label rank, the bits of a float64 >= +0.0, which order as the values do)
    u64 hi, lo;
};
__device__ __forceinline__ bool bf_less(const BfKey2 &a, const BfKey2 &b) { return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo); }
__device__ __forceinline__ bool bf_less(u64 a, u64 b) { return a < b; }

// One step of the bitonic network over P = 2^q keys: element i and its partner i ^ j, ascending where (i & kk) == 0.
template <typename K> __global__ __launch_bounds__(256) void bf_bitonic_kernel(K *__restrict__ a, i64 P, i64 j, i64 kk) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    const i64 p = i ^ j;
    if (p <= i) return;                                                // p < P: both are below the power of two P
    const K x = a[i], y = a[p];
    if ((i & kk) == 0 ? bf_less(y, x) : bf_less(x, y)) {
        a[i] = y;
        a[p] = x;
    }
}

// One lane per key slot of P: (rank, bits of 2 * radius) of skeleton voxel k, and above every key past the m-th.
static __global__ __launch_bounds__(256) void bf_median_keys_kernel(const int *__restrict__ rank, const double *__restrict__ radius, i64 m, i64 P,
                                                                    BfKey2 *__restrict__ keys) {
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    if (k >= P) return;
    BfKey2 key{~0ull, ~0ull};
    if (k < m) {
        key.hi = (u64)rank[k];
        key.lo = (u64)__double_as_longlong(radius[k] * 2.0);
    }
    keys[k] = key;
}

// One lane per label: np.median of its sorted values at [off[b], off[b] + count[b]) -- the middle one, or the mean of the two.
static __global__ __launch_bounds__(256) void bf_median_kernel(const BfKey2 *__restrict__ keys, const int *__restrict__ off, const int *__restrict__ count,
                                                               i64 labels, double *__restrict__ median) {
    const i64 b = (i64)blockIdx.x * 256 + threadIdx.x;
    if (b >= labels) return;
    const i64 a = off[b], k = count[b];
    const double lo = __longlong_as_double((long long)keys[a + (k - 1) / 2].lo), hi = __longlong_as_double((long long)keys[a + k / 2].lo);
    median[b] = k % 2 ? lo : (lo + hi) / 2.0;
}

// ---- region sums -----------------------------------------------------------------------------------------------------------------
// One lane per voxel of the branch-label volume: its region r (the rank of its label > 0) gets, in acc[field * R + r], field 0 the
// voxel count n, then per axis the smallest coordinate (the host sets these to all ones), the largest, S_a = sum c_a, and
// Q_ab = sum c_a * c_b for a <= b in row order.  All exact: coordinates < 2^15 and n < 2^31 (the host checks both) keep Q < 2^61.
template <int D>
__global__ __launch_bounds__(256) void bf_region_kernel(BfLabels lab, i64 n, NfGeom g, const u64 *__restrict__ pres, const int *__restrict__ pre, i64 R,
                                                        u64 *__restrict__ acc) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const i64 l = lab(i);
    if (l <= 0) return;
    const i64 r = ra_rank(pres, pre, l);
    u64 c[D];
    if (D == 3) c[0] = (u64)(i / (g.nx * g.ny));
    c[D - 2] = (u64)((i / g.nx) % g.ny);
    c[D - 1] = (u64)(i % g.nx);
    atomicAdd(&acc[r], 1ull);
    int f = 1;
    for (int a = 0; a < D; ++a) atomicMin(&acc[(f++) * R + r], c[a]);
    for (int a = 0; a < D; ++a) atomicMax(&acc[(f++) * R + r], c[a]);
    for (int a = 0; a < D; ++a) atomicAdd(&acc[(f++) * R + r], c[a]);
    for (int a = 0; a < D; ++a)
        for (int b = a; b < D; ++b) atomicAdd(&acc[(f++) * R + r], c[a] * c[b]);
}

// One lane per voxel: a region voxel appends the key (region rank << 32 | reassigned label) at the cursor (any order: the sort
// follows); flag[0] = 1 when a reassigned label is negative or above 2^31 - 1.  The host has sized keys for every region voxel.
static __global__ __launch_bounds__(256) void bf_mode_keys_kernel(BfLabels lab, BfLabels value, i64 n, const u64 *__restrict__ pres, const int *__restrict__ pre,
                                                                  u64 *__restrict__ keys, i64 cap, u64 *__restrict__ cursor, int *__restrict__ flag) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const i64 l = lab(i);
    if (l <= 0) return;
    const i64 v = value(i);
    if (v < 0 || v > 0x7fffffffll) {
        atomicOr(flag, 1);
        return;
    }
    const u64 at = atomicAdd(cursor, 1ull);
    if ((i64)at < cap) keys[at] = ((u64)ra_rank(pres, pre, l) << 32) | (u64)v;
}

// One lane per sorted key: the first of a run of equal keys finds the run's end by bisection and offers (length << 32 | ~label)
// to its region's maximum: the longest run wins, among equals the smallest label -- argmax(bincount).  A key whose region is not
// below R (the padding) is passed over.
static __global__ __launch_bounds__(256) void bf_mode_kernel(const u64 *__restrict__ keys, i64 total, i64 R, u64 *__restrict__ best) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const u64 key = keys[i];
    if ((key >> 32) >= (u64)R) return;
    if (i > 0 && keys[i - 1] == key) return;
    i64 lo = i, hi = total;                                            // keys[lo] == key, keys[hi] > key or hi == total
    while (hi - lo > 1) {
        const i64 mid = lo + (hi - lo) / 2;
        if (keys[mid] == key) lo = mid; else hi = mid;
    }
    const u64 len = (u64)(hi - i);
    atomicMax(&best[key >> 32], (len << 32) | (0xffffffffull - (key & 0xffffffffull)));
}

// ---- region sums by row runs -----------------------------------------------------------------------------------------------------
#define BF_ROWS_BAND 16               // consecutive rows (one plane) of a workgroup: four per wave

// field f of the layout of bf_region_kernel: 0 and the fields past the extrema add, 1 .. D take the minimum, D + 1 .. 2 D the maximum
template <int D> __device__ __forceinline__ void bf_field_apply(u64 *cell, int f, u64 v) {
    if (f >= 1 && f <= D) atomicMin(cell, v);
    else if (f > D && f <= 2 * D) atomicMax(cell, v);
    else atomicAdd(cell, v);
}

// The sums of bf_region_kernel, bit for bit (integer add, min and max only: no order matters), taken per run of equal labels along
// X instead of per voxel.  A workgroup owns a band of BF_ROWS_BAND consecutive rows (z, y) of one plane, a wave whole rows of it,
// which it walks in chunks of 64 voxels.  One ballot marks the lanes whose label differs from the lane before (lane 0 always: a run
// never continues from a chunk, let alone from a row, into the next -- it becomes two runs, and the sums are additive); the head
// lane of a run of label > 0 takes the run's length [x0, x0 + len) from the next set bit and adds closed forms, one global atomic
// per field and run:
//     n += len;  min / max: x0 and x0 + len - 1 for x, z and y themselves;  S_x += len x0 + len (len - 1) / 2,  S_a += c_a len;
//     Q_xx += len x0^2 + x0 len (len - 1) + (len - 1) len (2 len - 1) / 6,  Q_ax += c_a S_x(run),  Q_ab += c_a c_b len.
// len <= 64 here (a chunk) and coordinates < 2^15 (the host checks) keep every term below 2^15 * 2^15 * 2^15 = 2^45 < 2^47; the
// totals keep bf_region_kernel's bound Q < 2^61.  acc starts as for bf_region_kernel.  (A per-workgroup LDS table that combined the
// runs of a band before they reached global memory was measured and left out: DESIGN.md section 18.)
template <int D>
__global__ __launch_bounds__(256) void bf_region_rows_kernel(BfLabels lab, NfGeom g, i64 bands, const u64 *__restrict__ pres, const int *__restrict__ pre,
                                                             i64 R, u64 *__restrict__ acc) {
    constexpr int F = 1 + 3 * D + D * (D + 1) / 2;
    static_assert(F <= 16, "the host allocates sixteen fields per region");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const i64 z = (i64)blockIdx.x / bands, y0 = ((i64)blockIdx.x % bands) * BF_ROWS_BAND;
    const i64 y1 = y0 + BF_ROWS_BAND < g.ny ? y0 + BF_ROWS_BAND : g.ny;
    for (i64 y = y0 + wave; y < y1; y += 4) {
        const i64 row = (z * g.ny + y) * g.nx;
        for (i64 xc = 0; xc < g.nx; xc += 64) {                        // uniform over the wave: ballot and shuffle see all 64 lanes
            const i64 x = xc + lane;
            i64 l = x < g.nx ? lab(row + x) : 0;                       // past the row's end: background, which ends a run at nx
            l = l > 0 ? l : 0;
            const i64 before = __shfl_up(l, 1);
            const u64 heads = __ballot(lane == 0 || l != before);
            if (l == 0 || !((heads >> lane) & 1ull)) continue;         // the loop's bounds are uniform: the wave is whole again at its head
            const u64 rest = lane == 63 ? 0ull : heads >> (lane + 1);  // the heads after this one
            const u64 len = rest ? (u64)__ffsll((long long)rest) : (u64)(64 - lane);       // <= 64, and x + len <= nx
            const i64 r = ra_rank(pres, pre, l);
            const u64 ux = (u64)x;
            const u64 sx = len * ux + len * (len - 1) / 2;                                 // sum of x over the run
            const u64 qxx = len * ux * ux + ux * len * (len - 1) + (len - 1) * len * (2 * len - 1) / 6;
            u64 c[D], v[F];
            if (D == 3) c[0] = (u64)z;
            c[D - 2] = (u64)y;
            c[D - 1] = ux;
            int f = 0;
            v[f++] = len;
            for (int a = 0; a < D; ++a) v[f++] = c[a];
            for (int a = 0; a < D - 1; ++a) v[f++] = c[a];
            v[f++] = ux + len - 1;
            for (int a = 0; a < D - 1; ++a) v[f++] = c[a] * len;
            v[f++] = sx;
            for (int a = 0; a < D; ++a)
                for (int b = a; b < D; ++b) v[f++] = b < D - 1 ? c[a] * c[b] * len : a < D - 1 ? c[a] * sx : qxx;
#pragma unroll
            for (int j = 0; j < F; ++j) bf_field_apply<D>(&acc[(i64)j * R + r], j, v[j]);
        }
    }
}
