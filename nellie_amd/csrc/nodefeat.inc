// Node-level features (Nodes and aggregate_stats_for_class of nellie/feature_extraction/hierarchical.py) -- kernels of
// nellie_hip_nodefeat.hip (DESIGN.md section 15).
//
// Nodes are the voxels with pixel class > 0, compacted in raster order by the mask, scan and rank of rank_scan.inc.  The border
// is one bit per voxel; a wave searches a growing box of it around its node for the nearest set bit.  Groups of values (a node's
// voxels; later a branch's nodes) are CSR lists of indices; one wave reduces one group, or one buffer block of a wide group (the
// image's one group per frame, DESIGN.md section 19).  Every sum is numpy's sum of a row of L
// elements, the group's k values followed by L - k zeros: blocks of 8192 elements added in order, each summed as a pairwise tree
// whose shape comes from the block's length, the work from k (nf_tree_sum).
//
// All arithmetic is float64 in numpy's operation order; compiled with -ffp-contract=off.  Nothing here depends on the order in
// which waves or lanes finish: two runs give the same bits.
#pragma once
#include "rank_scan.inc"

struct NfGeom {
    i64 nz, ny, nx, n;
    double s[3];                      // spacing of the D axes, in axis order ((Z,) Y, X)
    double s3[3];                     // spacing of (Z, Y, X); a 2-D frame is one plane and its Z spacing is Y's
};

#define NF_STACK 72                   // entries of a tree walk's stack: two per level, and a tree over 2^31 elements has 26 levels
#define NF_LEAF 128                   // numpy's PW_BLOCKSIZE: at most that many elements are summed without splitting
#define NF_BLOCK 8192                 // numpy's ufunc buffer in elements (np.getbufsize()): a row is reduced in such pieces, as TRK_PW_BLOCK

// ---- element access ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double nf_value(const void *__restrict__ p, int dtype, i64 i) {
    switch (dtype) {
        case NL_U8: return (double)((const uint8_t *)p)[i];
        case NL_I8: return (double)((const int8_t *)p)[i];
        case NL_U16: return (double)((const uint16_t *)p)[i];
        case NL_I16: return (double)((const int16_t *)p)[i];
        case NL_U32: return (double)((const uint32_t *)p)[i];
        case NL_I32: return (double)((const int32_t *)p)[i];
        case NL_F32: return (double)((const float *)p)[i];
        default: return ((const double *)p)[i];
    }
}

__device__ __forceinline__ bool nf_is_set(const void *__restrict__ p, int dtype, i64 i, bool positive) {
    switch (dtype) {
        case NL_U8: return ((const uint8_t *)p)[i] != 0;
        case NL_I8: return positive ? ((const int8_t *)p)[i] > 0 : ((const int8_t *)p)[i] != 0;
        case NL_U16: return ((const uint16_t *)p)[i] != 0;
        case NL_I16: return positive ? ((const int16_t *)p)[i] > 0 : ((const int16_t *)p)[i] != 0;
        case NL_U32: return ((const uint32_t *)p)[i] != 0;
        case NL_I32: return positive ? ((const int32_t *)p)[i] > 0 : ((const int32_t *)p)[i] != 0;
        case NL_F32: return positive ? ((const float *)p)[i] > 0.f : ((const float *)p)[i] != 0.f;
        case NL_F64: return positive ? ((const double *)p)[i] > 0.0 : ((const double *)p)[i] != 0.0;
        case NL_U64: return ((const uint64_t *)p)[i] != 0;
        default: return positive ? ((const int64_t *)p)[i] > 0 : ((const int64_t *)p)[i] != 0;
    }
}

struct NfSet {                        // rank_mask_kernel's predicate: > 0 (nodes) or != 0 (border, as np.argwhere takes it)
    const void *src;
    int dtype;
    bool positive;
    __device__ bool operator()(i64 i) const { return nf_is_set(src, dtype, i, positive); }
};

// ---- node list -----------------------------------------------------------------------------------------------------------------
// One lane per voxel: a node writes its linear index at its rank.
static __global__ __launch_bounds__(256) void nf_compact_kernel(i64 n, const u64 *__restrict__ bits, const int *__restrict__ pre, i64 *__restrict__ node_vox) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (!((bits[i >> 6] >> (i & 63)) & 1ull)) return;
    node_vox[ra_rank(bits, pre, i)] = i;
}

// One lane per node: the frame's value at the node, `size` bytes wide.
static __global__ __launch_bounds__(256) void nf_gather_kernel(const void *__restrict__ frame, int size, const i64 *__restrict__ node_vox, i64 m,
                                                               void *__restrict__ out) {
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    if (k >= m) return;
    const i64 i = node_vox[k];
    switch (size) {
        case 1: ((uint8_t *)out)[k] = ((const uint8_t *)frame)[i]; break;
        case 2: ((uint16_t *)out)[k] = ((const uint16_t *)frame)[i]; break;
        case 4: ((uint32_t *)out)[k] = ((const uint32_t *)frame)[i]; break;
        default: ((uint64_t *)out)[k] = ((const uint64_t *)frame)[i]; break;
    }
}

// One lane per node: its coordinates as int64 (m, D).
static __global__ __launch_bounds__(256) void nf_coords_kernel(const i64 *__restrict__ node_vox, i64 m, NfGeom g, int D, i64 *__restrict__ coords) {
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    if (k >= m) return;
    const i64 i = node_vox[k];
    if (D == 3) coords[k * 3] = i / (g.nx * g.ny);
    coords[k * D + D - 2] = (i / g.nx) % g.ny;
    coords[k * D + D - 1] = i % g.nx;
}

// One lane per voxel, one wave per mask word: the border as bits, any[0] = 1 when a voxel is set (the host zeroes it).
static __global__ __launch_bounds__(256) void nf_border_kernel(NfSet on, i64 n, u64 *__restrict__ bits, int *__restrict__ any) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    const u64 b = __ballot(i < n && on(i));
    if ((threadIdx.x & 63) == 0) {
        bits[i >> 6] = b;
        if (b) atomicOr(any, 1);
    }
}

// ---- wave reductions -------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double nf_wave_min(double v) {
    for (int w = 32; w > 0; w >>= 1) {
        const double o = __shfl_xor(v, w);
        v = o < v ? o : v;
    }
    return v;
}

__device__ __forceinline__ i64 nf_wave_sum(i64 v) {
    for (int w = 32; w > 0; w >>= 1) v += __shfl_xor(v, w);
    return v;
}

// ---- node thickness --------------------------------------------------------------------------------------------------------------
// nf_nearest_sq: the squared distance (um^2) from voxel v to the nearest set bit of `border`, which has one; called by all 64 lanes
// of a one-wave workgroup, every lane returns it.  Shared with branchfeat.inc (the radii of the skeleton voxels).
//
// A box of half-widths floor(R / s_a) voxels holds every voxel within R: one outside it is at least floor(R / s_a) + 1 > R / s_a
// voxels away along some axis (a quotient rounded to float64 is never below an integer the exact one reaches).  Its squared
// distance as computed here, from products and a difference that are each off by at most 2^-53 of a coordinate in um, stays above
// R * R * (1 - 2^-16) for frames below 2^34 voxels per axis, R being at least one voxel.  So when the box's best squared
// distance is at or below that, it is the frame's.  Otherwise R doubles, until the box is the frame.
// The lanes take the (row, mask word) pairs of the box; a row's bits may start and end inside a word.
__device__ __forceinline__ double nf_nearest_sq(i64 v, const NfGeom &g, const u64 *__restrict__ border) {
    const int lane = threadIdx.x;
    const i64 c[3] = {v / (g.nx * g.ny), (v / g.nx) % g.ny, v % g.nx};
    const i64 dim[3] = {g.nz, g.ny, g.nx};
    const double *s = g.s3;
    const double p[3] = {(double)c[0] * s[0], (double)c[1] * s[1], (double)c[2] * s[2]};
    double R = s[0] > s[1] ? s[0] : s[1];
    R = 2.0 * (R > s[2] ? R : s[2]);
    const double inf = __longlong_as_double(0x7ff0000000000000ll);
    double best = inf;
    for (;;) {
        i64 lo[3], hi[3];
        bool whole = true;
        for (int a = 0; a < 3; ++a) {
            const double q = floor(R / s[a]);
            const i64 half = q < 4.0e18 ? (i64)q : (i64)4e18;
            lo[a] = half > c[a] ? 0 : c[a] - half;
            hi[a] = half >= dim[a] - 1 - c[a] ? dim[a] - 1 : c[a] + half;
            whole = whole && lo[a] == 0 && hi[a] == dim[a] - 1;
        }
        const i64 rows_y = hi[1] - lo[1] + 1, rows = (hi[0] - lo[0] + 1) * rows_y;
        const i64 wpr = (hi[2] - lo[2]) / 64 + 2;                      // mask words a row of the box can touch
        best = inf;
        for (i64 item = lane; item < rows * wpr; item += 64) {
            const i64 row = item / wpr, wi = item % wpr;
            const i64 z = lo[0] + row / rows_y, y = lo[1] + row % rows_y;
            const i64 first = (z * g.ny + y) * g.nx + lo[2], last = first + (hi[2] - lo[2]);      // the row's voxels, both inside the frame
            const i64 w = (first >> 6) + wi;
            if (w > (last >> 6)) continue;
            u64 b = border[w];
            if (w == (first >> 6)) b &= ~0ull << (first & 63);
            if (w == (last >> 6)) b &= ~0ull >> (63 - (last & 63));
            const double dz = p[0] - (double)z * s[0], dy = p[1] - (double)y * s[1];
            const double dzy = dz * dz + dy * dy;                      // 2-D: z = 0 and dz * dz = +0.0 leave dy * dy as it is
            while (b) {
                const int bit = __ffsll((long long)b) - 1;
                b &= b - 1;
                const i64 x = (w << 6) + bit - (first - lo[2]);
                const double dx = p[2] - (double)x * s[2];
                const double d2 = dzy + dx * dx;
                best = d2 < best ? d2 : best;
            }
        }
        best = nf_wave_min(best);
        if (whole || best <= R * R * (1.0 - 0x1p-16)) break;
        R = R + R;
    }
    return best;
}

// One wave per node: 2 * the distance in um to the nearest border voxel, NaN when the frame has none (*any_border == 0).
static __global__ __launch_bounds__(64) void nf_thickness_kernel(const i64 *__restrict__ node_vox, i64 m, NfGeom g, const u64 *__restrict__ border,
                                                                 const int *__restrict__ any_border, double *__restrict__ thickness) {
    const i64 node = blockIdx.x;
    if (node >= m) return;
    const int lane = threadIdx.x;
    if (*any_border == 0) {
        if (lane == 0) thickness[node] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    const double best = nf_nearest_sq(node_vox[node], g, border);
    if (lane == 0) thickness[node] = sqrt(best) * 2.0;
}

// ---- numpy's sum over padded rows ------------------------------------------------------------------------------------------------
// nf_block_tree: numpy's pairwise sum of one block of a row: n elements, the first k of which are elem(base .. base + k) and the
// rest +0.0 (0 < k <= n <= NF_BLOCK).  Called by all 64 lanes of a one-wave workgroup with the same arguments; every lane returns
// the sum.  scratch: at most 129 doubles of the wave's own, k / 64 + 2 suffice.
//
// The tree splits n > 128 elements at n / 2 rounded down to a multiple of 8 and sums n <= 128 as a leaf: eight accumulators over
// the largest multiple of 8, combined pairwise, then the remainder in order (below 8 elements: one running sum).  A subtree or a
// tail made of padding only adds +0.0, which changes nothing but the sign of a zero, and the 0.0 that nf_tree_sum starts from
// settles that sign whatever the tree gave; so padding is skipped and the work is O(k + log n).  Eight lanes share a leaf, one
// accumulator each; the leaf sums go through `scratch` and are combined by a second walk of the tree.
template <typename F> __device__ double nf_block_tree(F elem, int base, int k, int n_block, double *__restrict__ scratch) {
    const int team = threadIdx.x >> 3, j = threadIdx.x & 7;
    int slo[NF_STACK], sn[NF_STACK];
    int top = 1, leaf = 0;
    slo[0] = 0;
    sn[0] = n_block;
    for (;;) {
        int mylo = 0, myn = 0, mine = -1, got = 0;                     // the next eight leaves, one per team
        while (top > 0 && got < 8) {
            --top;
            const int lo = slo[top], n = sn[top];
            if (lo >= k) continue;
            if (n > NF_LEAF) {
                int n2 = n / 2;
                n2 -= n2 % 8;
                slo[top] = lo + n2; sn[top] = n - n2; ++top;
                slo[top] = lo; sn[top] = n2; ++top;
                continue;
            }
            if (got == team) { mylo = lo; myn = n; mine = leaf; }
            ++got;
            ++leaf;
        }
        if (got == 0) break;
        const int kk = mine < 0 ? 0 : (k - mylo < myn ? k - mylo : myn);      // the leaf's elements that are not padding
        const int at = base + mylo;
        double r = 0.0;
        if (n_block < 8) {                                             // one leaf, a running sum
            for (int i = 0; i < kk; ++i) r = r + elem(at + i);
        } else {
            const int m8 = myn - myn % 8, stop = kk < m8 ? kk : m8;
            if (j < stop) r = elem(at + j);
            for (int i = j + 8; i < stop; i += 8) r = r + elem(at + i);
            r = r + __shfl_xor(r, 1);
            r = r + __shfl_xor(r, 2);
            r = r + __shfl_xor(r, 4);
            for (int i = m8; i < kk; ++i) r = r + elem(at + i);
        }
        if (mine >= 0 && j == 0) scratch[mine] = r;
    }
    __syncthreads();
    // the second walk: a stack of pending subtrees (n < 0: both halves are summed, add them) and one of their sums
    double val[NF_STACK / 2 + 2];
    int vt = 0;
    top = 1;
    leaf = 0;
    slo[0] = 0;
    sn[0] = n_block;
    while (top > 0) {
        --top;
        const int lo = slo[top], n = sn[top];
        if (n < 0) {
            const double b = val[--vt], a = val[--vt];
            val[vt++] = a + b;
            continue;
        }
        if (n <= NF_LEAF) {
            val[vt++] = scratch[leaf++];
            continue;
        }
        int n2 = n / 2;
        n2 -= n2 % 8;
        if (lo + n2 < k) {                                             // the right half holds values too
            slo[top] = lo; sn[top] = -1; ++top;
            slo[top] = lo + n2; sn[top] = n - n2; ++top;
        }
        slo[top] = lo; sn[top] = n2; ++top;
    }
    const double sum = val[0];
    __syncthreads();                                                   // the scratch may be written again
    return sum;
}

// What np.sum gives for a row of a matrix padded to L columns, the first k of which are elem(0 .. k) and the rest +0.0 (k <= L),
// and with L = k for a vector.  numpy runs a reduction's inner loop in pieces of its ufunc buffer, NF_BLOCK elements, restarting
// at every row: the sum is 0.0, then for every block b of the row `sum + pairwise tree of the block`, the block's length being
// min(NF_BLOCK, L - NF_BLOCK * b).  A block of padding adds +0.0 to a sum that began as 0.0 + ..., never -0.0, and changes nothing:
// only the blocks that start below k are visited.  For L <= NF_BLOCK this is 0.0 + one tree over L.  Called by all 64 lanes of a
// one-wave workgroup with the same k, L and scratch; every lane returns the sum.  scratch: k / 64 + 2 doubles of the wave's own
// (one block at a time: a leaf of a split tree has at least 64 elements, so at most 129 leaves hold values).
template <typename F> __device__ double nf_tree_sum(F elem, int k, int L, double *__restrict__ scratch) {
    double sum = 0.0;
    for (i64 b = 0; b < k; b += NF_BLOCK) {                            // i64: the step past a k near 2^31 must not wrap
        const int base = (int)b, n_block = L - base < NF_BLOCK ? L - base : NF_BLOCK;
        sum = sum + nf_block_tree(elem, base, k - base < n_block ? k - base : n_block, n_block, scratch);
    }
    return sum;
}

// ---- aggregation -----------------------------------------------------------------------------------------------------------------
// A group's values as float64; an index outside [0, nval) (the host has refused those) reads as NaN.
struct NfGroupValues {
    const void *values;
    int dtype;
    i64 nval;
    const i64 *idx;                   // the group's indices
    __device__ double operator()(int i) const {
        const i64 q = idx[i];
        return q >= 0 && q < nval ? nf_value(values, dtype, q) : __longlong_as_double(0x7ff8000000000000ll);
    }
};

struct NfZeroNan {                    // the values with NaN as +0.0: nansum's operand
    NfGroupValues v;
    __device__ double operator()(int i) const {
        const double x = v(i);
        return x == x ? x : 0.0;
    }
};

struct NfSquaredDeviation {           // (v - mean)^2 with NaN entries as +0.0: _nanvar's operand
    NfGroupValues v;
    double mean;
    __device__ double operator()(int i) const {
        const double x = v(i);
        const double d = x - mean;
        return x == x ? d * d : 0.0;
    }
};

// The smallest and the largest value with their positions in the group, at = -1 for none.  Among equal extremes (+0.0 and -0.0)
// the one latest in the group is taken, as numpy's fmin / fmax reductions do; positions are distinct, so merging is order-free.
struct NfExtremes {
    double lo, hi;
    int lo_at, hi_at;
    __device__ void take(double x, int at) {                           // positions ascending
        if (lo_at < 0 || x <= lo) { lo = x; lo_at = at; }
        if (hi_at < 0 || x >= hi) { hi = x; hi_at = at; }
    }
    __device__ void merge(double ol, int ol_at, double oh, int oh_at) {
        if (ol_at >= 0 && (lo_at < 0 || ol < lo || (ol == lo && ol_at > lo_at))) { lo = ol; lo_at = ol_at; }
        if (oh_at >= 0 && (hi_at < 0 || oh > hi || (oh == hi && oh_at > hi_at))) { hi = oh; hi_at = oh_at; }
    }
    __device__ void wave() {                                           // every lane ends with the wave's
        for (int w = 32; w > 0; w >>= 1) merge(__shfl_xor(lo, w), __shfl_xor(lo_at, w), __shfl_xor(hi, w), __shfl_xor(hi_at, w));
    }
};

// One wave per group: out[key * groups + group] for key = mean, std_dev, min, max, sum, over the group's values as a row padded
// to L columns.  A group of at least wide_from values (wide_from > 0) is left to the block kernels below.
static __global__ __launch_bounds__(64) void nf_aggregate_kernel(const void *__restrict__ values, int dtype, i64 nval, const i64 *__restrict__ off,
                                                                 const i64 *__restrict__ idx, i64 groups, int L, i64 wide_from,
                                                                 double *__restrict__ scratch, double *__restrict__ out) {
    const i64 grp = blockIdx.x;
    if (grp >= groups) return;
    const int lane = threadIdx.x;
    const i64 a = off[grp];
    const int k = (int)(off[grp + 1] - a);
    if (wide_from > 0 && k > 0 && k >= wide_from) return;
    const NfGroupValues v{values, dtype, nval, idx + a};
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    NfExtremes e{nan, nan, -1, -1};
    i64 count = 0;
    for (int i = lane; i < k; i += 64) {
        const double x = v(i);
        if (x != x) continue;
        ++count;
        e.take(x, i);
    }
    e.wave();
    const double lo = e.lo, hi = e.hi;
    count = nf_wave_sum(count);
    double *sc = scratch + (a / 64 + 2 * grp);
    const double sum = nf_tree_sum(NfZeroNan{v}, k, L, sc);
    const double mean = sum / (double)count;
    const double var = nf_tree_sum(NfSquaredDeviation{v, mean}, k, L, sc) / (double)count;
    if (lane == 0) {
        out[grp] = mean;
        out[groups + grp] = sqrt(var);
        out[2 * groups + grp] = lo;
        out[3 * groups + grp] = hi;
        out[4 * groups + grp] = sum;
    }
}

// ---- aggregation of wide groups, one wave per buffer block -----------------------------------------------------------------------
// A row's blocks of NF_BLOCK elements are independent trees; only the chain `sum = sum + tree(block b)`, b ascending, is ordered
// (nf_tree_sum).  So a wide group is cut into items (group, block): one wave sums one block exactly as nf_tree_sum would
// (nf_wide_block_kernel), then one wave per group adds the blocks' sums in that order (nf_wide_chain_kernel).  Twice: the values,
// which gives the mean, then the squared deviations from it.  The same additions in the same order as nf_aggregate_kernel: the
// same bits.  No atomics; every item and every group has its own slots.
struct NfWide {
    const i64 *items;                 // (n_items, 2): the row of `wide` and the block
    const i64 *wide;                  // (n_wide, 2): the group and its first item; its items follow one another, blocks ascending
    double *sum;                      // per item: the block's sum
    i64 *count;                       // per item: the block's values that are not NaN
    double *lo, *hi;                  // per item: the block's extremes and their positions in the group (NfExtremes)
    int *lo_at, *hi_at;
    double *mean;                     // per wide group
    i64 *total;                       // per wide group: its values that are not NaN
};

// One wave per item.  DEV = false: the block's sum of the values (NaN as +0.0), count and extremes.  DEV = true: its sum of the
// squared deviations from the group's mean.  The leaf sums of nf_block_tree go through LDS: 129 doubles at most.
template <bool DEV>
__global__ __launch_bounds__(64) void nf_wide_block_kernel(const void *__restrict__ values, int dtype, i64 nval, const i64 *__restrict__ off,
                                                           const i64 *__restrict__ idx, int L, NfWide W, i64 n_items) {
    __shared__ double sc[NF_LEAF + 4];
    const i64 item = blockIdx.x;
    if (item >= n_items) return;
    const int lane = threadIdx.x;
    const i64 w = W.items[2 * item], b = W.items[2 * item + 1], grp = W.wide[2 * w];
    const i64 a = off[grp];
    const int k = (int)(off[grp + 1] - a);
    const int base = (int)(b * NF_BLOCK), n_block = L - base < NF_BLOCK ? L - base : NF_BLOCK;
    const int kb = k - base < n_block ? k - base : n_block;           // the block's elements that are not padding
    if (kb <= 0) return;                                               // never: the host lists the blocks that start below k
    const NfGroupValues v{values, dtype, nval, idx + a};
    if (DEV) {
        const double sum = nf_block_tree(NfSquaredDeviation{v, W.mean[w]}, base, kb, n_block, sc);
        if (lane == 0) W.sum[item] = sum;
        return;
    }
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    NfExtremes e{nan, nan, -1, -1};
    i64 count = 0;
    for (int i = base + lane; i < base + kb; i += 64) {
        const double x = v(i);
        if (x != x) continue;
        ++count;
        e.take(x, i);
    }
    e.wave();
    count = nf_wave_sum(count);
    const double sum = nf_block_tree(NfZeroNan{v}, base, kb, n_block, sc);
    if (lane == 0) {
        W.sum[item] = sum;
        W.count[item] = count;
        W.lo[item] = e.lo; W.lo_at[item] = e.lo_at;
        W.hi[item] = e.hi; W.hi_at[item] = e.hi_at;
    }
}

// One wave per wide group: 0.0, then + the sum of every block, blocks ascending; the lanes fetch 64 sums at a time and every lane
// adds them in order.  DEV = false: mean, min, max and sum of the group into `out`, the mean and the count kept for the second
// pass.  DEV = true: std_dev.
template <bool DEV>
__global__ __launch_bounds__(64) void nf_wide_chain_kernel(const i64 *__restrict__ off, i64 groups, NfWide W, i64 n_wide, double *__restrict__ out) {
    const i64 w = blockIdx.x;
    if (w >= n_wide) return;
    const int lane = threadIdx.x;
    const i64 grp = W.wide[2 * w], first = W.wide[2 * w + 1];
    const i64 k = off[grp + 1] - off[grp];
    const int nb = (int)((k + NF_BLOCK - 1) / NF_BLOCK);
    double sum = 0.0;
    for (int b0 = 0; b0 < nb; b0 += 64) {
        const int m = nb - b0 < 64 ? nb - b0 : 64;
        const double p = lane < m ? W.sum[first + b0 + lane] : 0.0;
        for (int j = 0; j < m; ++j) sum = sum + __shfl(p, j);
    }
    if (DEV) {
        const double var = sum / (double)W.total[w];
        if (lane == 0) out[groups + grp] = sqrt(var);
        return;
    }
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    NfExtremes e{nan, nan, -1, -1};
    i64 count = 0;
    for (int b = lane; b < nb; b += 64) {
        count += W.count[first + b];
        e.merge(W.lo[first + b], W.lo_at[first + b], W.hi[first + b], W.hi_at[first + b]);
    }
    e.wave();
    count = nf_wave_sum(count);
    const double mean = sum / (double)count;
    if (lane == 0) {
        W.mean[w] = mean;
        W.total[w] = count;
        out[grp] = mean;
        out[2 * groups + grp] = e.lo;
        out[3 * groups + grp] = e.hi;
        out[4 * groups + grp] = sum;
    }
}

// ---- node statistics -------------------------------------------------------------------------------------------------------------
// sum over the axes of sign * vec * dir at the i-th voxel of a node's list, NaN as +0.0; dir = (voxel - node) / its norm in
// voxels, NaN where the norm is 0.  vec == NULL: every vector is NaN.
template <int D> struct NfDot {
    const i64 *coords;                // (n_vox, D) voxel coordinates
    const float *vec;                 // (n_vox, D) or NULL
    const i64 *idx;
    i64 nvox;
    i64 node[D];
    bool negate;
    __device__ double raw(int i) const {
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        const i64 q = idx[i];
        if (!vec || q < 0 || q >= nvox) return nan;
        double d[D];
        double sq = 0.0;
        for (int a = 0; a < D; ++a) {
            d[a] = (double)(coords[q * D + a] - node[a]);
            sq = sq + d[a] * d[a];
        }
        const double norm = sqrt(sq);
        double sum = 0.0;
        for (int a = 0; a < D; ++a) {
            const double dir = norm != 0.0 ? d[a] / norm : nan;
            const double f = (double)vec[q * D + a];
            sum = sum + (negate ? -f : f) * dir;
        }
        return sum;
    }
    __device__ double operator()(int i) const {
        const double x = raw(i);
        return x == x ? x : 0.0;
    }
};

template <int D> __device__ double nf_nanmean_dot(const NfDot<D> &e, int k, double *sc) {
    i64 count = 0;
    for (int i = threadIdx.x; i < k; i += 64) {
        const double x = e.raw(i);
        count += x == x;
    }
    count = nf_wave_sum(count);
    const double sum = nf_tree_sum(e, k, k, sc);
    return sum / (double)count;
}

// One wave per node: out[j * m + node] for j = z, y, x, divergence, convergence, vergere.  The node's voxels are its group of the
// CSR (off, idx); z, y, x are the mean voxel coordinate (exact integer sum / count) times the spacing, z NaN in 2-D.
template <int D>
__global__ __launch_bounds__(64) void nf_node_stats_kernel(const i64 *__restrict__ node_vox, i64 m, NfGeom g, const i64 *__restrict__ coords, i64 nvox,
                                                           const float *__restrict__ vec01, const float *__restrict__ vec12,
                                                           const i64 *__restrict__ off, const i64 *__restrict__ idx, double *__restrict__ scratch,
                                                           double *__restrict__ out) {
    const i64 node = blockIdx.x;
    if (node >= m) return;
    const int lane = threadIdx.x;
    const i64 a = off[node];
    const int k = (int)(off[node + 1] - a);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    if (k == 0) {
        if (lane < 6) out[(i64)lane * m + node] = nan;
        return;
    }
    i64 tot[D];
    for (int ax = 0; ax < D; ++ax) tot[ax] = 0;
    for (int i = lane; i < k; i += 64) {
        const i64 q = idx[a + i];
        if (q < 0 || q >= nvox) continue;
        for (int ax = 0; ax < D; ++ax) tot[ax] += coords[q * D + ax];
    }
    double pos[3] = {nan, nan, nan};
    for (int ax = 0; ax < D; ++ax) pos[3 - D + ax] = (double)nf_wave_sum(tot[ax]) / (double)k * g.s[ax];
    const i64 v = node_vox[node];
    NfDot<D> e{coords, vec01, idx + a, nvox, {}, true};
    if (D == 3) e.node[0] = v / (g.nx * g.ny);
    e.node[D - 2] = (v / g.nx) % g.ny;
    e.node[D - 1] = v % g.nx;
    double *sc = scratch + (a / 64 + 2 * node);
    const double conv = -nf_nanmean_dot<D>(e, k, sc);
    e.vec = vec12;
    e.negate = false;
    const double div = nf_nanmean_dot<D>(e, k, sc);
    if (lane == 0) {
        out[node] = pos[0];
        out[m + node] = pos[1];
        out[2 * m + node] = pos[2];
        out[3 * m + node] = div;
        out[4 * m + node] = conv;
        out[5 * m + node] = conv + div;
    }
}
