// The analysis overlay (nellie_napari/nellie_analysis.py:955-1218): a column of a feature table painted onto the labelled voxels of a
// frame -- kernels of nellie_hip_overlay.hip (DESIGN.md section 24).
//
// The labelled voxels of a frame are its rows, in raster order: the 1-bit mask `label > 0` with the scanned word populations
// (rank_scan.inc) gives every set voxel its row.  A row's value is the mean of attr[g] over its distinct groups g whose attr[g] is
// not NaN; a row has one group (branch, organelle; -1: none) or a run of a CSR (nodes), which the lane walks by repeated selection
// of the smallest group above the last one taken -- distinct groups in ascending order whatever the stored order, without a sort.
// The reference sums a dense float64 column of n_attr entries in which every other entry is +0.0, with np.sum: row by row when its
// matrix is C-ordered, as pairwise trees over pieces of 8192 entries when the column is contiguous (DESIGN.md section 24.2).
// Adding +0.0 is exact, so the lane visits its own groups only and follows the tree by their positions.
//
// The paint is one streaming pass: a lane takes 16 bytes of the output (two float64 or uint64, four float32), the mask word they
// lie in and its prefix, derives the rows of the set voxels by popcount, gathers their values and stores NaN (0 for labels)
// elsewhere.  The frame is painted as a linear array, so the 16-byte stores are aligned for every width; a tail of fewer than 16
// bytes is stored element by element.  The label frame is not read again.
//
// Block sizes: 256 lanes everywhere.  No atomics.  Compiled with -ffp-contract=off: every add of a sum is a float64 add of its own.
#pragma once

#include "rank_scan.inc"

typedef double ov_v2d __attribute__((ext_vector_type(2)));
typedef float ov_v4f __attribute__((ext_vector_type(4)));
typedef u64 ov_v2u __attribute__((ext_vector_type(2)));

#define OV_NO_GROUP 0x7fffffff        // above every group index (the host refuses an index that large)

struct OvLabelled {                   // rank_mask_kernel's predicate over an int32 label frame
    const int *lab;
    __device__ bool operator()(i64 i) const { return lab[i] > 0; }
};

__device__ __forceinline__ double ov_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

// a row's mean: numpy's sum starts from +0.0, so a zero sum is +0.0 whatever the signs of its terms
__device__ __forceinline__ double ov_mean(double acc, int cnt) { return cnt == 0 ? ov_nan() : (acc + 0.0) / (double)cnt; }

// One lane per row: its single group
__global__ __launch_bounds__(256) void ov_values_single_kernel(const int *__restrict__ group, i64 V, const double *__restrict__ attr, i64 n_attr,
                                                               double *__restrict__ val) {
    const i64 r = (i64)blockIdx.x * 256 + threadIdx.x;
    if (r >= V) return;
    const int g = group[r];
    double acc = 0.0;
    int cnt = 0;
    if (g >= 0 && (i64)g < n_attr) {
        const double v = attr[g];
        if (v == v) { acc = v; cnt = 1; }
    }
    val[r] = ov_mean(acc, cnt);
}

// A row's run of the CSR, walked in ascending order of its distinct groups: `cur` is the smallest group not yet taken
// (OV_NO_GROUP: none is left); a group at or beyond n_attr (the host has refused those) ends the walk.
struct OvRun {
    const int *__restrict__ idx;
    i64 a, b;
    const double *__restrict__ attr;
    i64 n_attr;
    int cur, cnt;
    __device__ void seek(int last) {
        int best = OV_NO_GROUP;
        for (i64 j = a; j < b; ++j) {
            const int g = idx[j];
            if (g > last && g < best) best = g;
        }
        cur = (i64)best < n_attr ? best : OV_NO_GROUP;
    }
    // the value of `cur` as nanmean's sum sees it (NaN: +0.0, not counted), and on to the next group
    __device__ double take() {
        const double v = attr[cur];
        seek(cur);
        if (v != v) return 0.0;
        ++cnt;
        return v;
    }
};

#define OV_LEAF 128                   // numpy's PW_BLOCKSIZE
#define OV_BLOCK 8192                 // numpy's ufunc buffer in elements: a contiguous column is reduced in such pieces

// numpy's pairwise sum of the n <= OV_LEAF column entries from `lo` on, the run's groups among them with their values and +0.0
// everywhere else: below 8 entries one running sum; else eight accumulators over the largest multiple of 8, combined as a tree,
// then the remainder in order.  An absent entry adds +0.0, which is exact, so only the run's groups are visited.
__device__ double ov_leaf_sum(OvRun &run, i64 lo, int n) {
    const i64 end = lo + n;
    double res = 0.0;
    if (n >= 8) {
        const i64 m8 = lo + (n - n % 8);
        double r[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        while ((i64)run.cur < m8) {
            const int j = (int)((run.cur - lo) & 7);
            const double v = run.take();
#pragma unroll
            for (int q = 0; q < 8; ++q) r[q] = q == j ? r[q] + v : r[q];
        }
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    }
    while ((i64)run.cur < end) res = res + run.take();
    return res;
}

// numpy's pairwise sum of one buffer block of the column, entries [base, base + nb), nb <= OV_BLOCK: more than OV_LEAF entries are
// split at half their number rounded down to a multiple of 8.  Post-order over an explicit stack (a block has at most 7 levels);
// a subtree without a group of the run is +0.0.
__device__ double ov_block_sum(OvRun &run, i64 base, int nb) {
    int slo[16], sn[16], top = 1, vt = 0;
    double val[10];
    slo[0] = 0;
    sn[0] = nb;
    while (top > 0) {
        --top;
        const int lo = slo[top], n = sn[top];
        if (n < 0) {
            const double y = val[--vt], x = val[--vt];
            val[vt++] = x + y;
        } else if ((i64)run.cur >= base + lo + n) {
            val[vt++] = 0.0;
        } else if (n <= OV_LEAF) {
            val[vt++] = ov_leaf_sum(run, base + lo, n);
        } else {
            int n2 = n / 2;
            n2 -= n2 % 8;
            slo[top] = lo; sn[top] = -1; ++top;
            slo[top] = lo + n2; sn[top] = n - n2; ++top;
            slo[top] = lo; sn[top] = n2; ++top;
        }
    }
    return val[0];
}

// One lane per row: its run idx[off[r] .. off[r + 1]).  The sum is numpy's over the dense column of n_attr entries: pairwise = 0:
// one add per entry in ascending order (the reference's matrix is C-ordered: it was padded); else in pieces of OV_BLOCK entries,
// each a pairwise tree (the matrix is F-ordered, or one column wide).
__global__ __launch_bounds__(256) void ov_values_csr_kernel(const i64 *__restrict__ off, const int *__restrict__ idx, i64 V,
                                                            const double *__restrict__ attr, i64 n_attr, int pairwise, double *__restrict__ val) {
    const i64 r = (i64)blockIdx.x * 256 + threadIdx.x;
    if (r >= V) return;
    OvRun run{idx, off[r], off[r + 1], attr, n_attr, OV_NO_GROUP, 0};
    run.seek(-1);
    double acc = 0.0;
    if (!pairwise) {
        while (run.cur != OV_NO_GROUP) acc = acc + run.take();
    } else {
        while (run.cur != OV_NO_GROUP) {
            const i64 base = ((i64)run.cur / OV_BLOCK) * OV_BLOCK;
            const i64 left = n_attr - base;
            acc = acc + ov_block_sum(run, base, (int)(left < OV_BLOCK ? left : OV_BLOCK));
        }
    }
    val[r] = ov_mean(acc, run.cnt);
}

// what a voxel shows: the row's value, rounded once to float32, or as a label (0 where the value is NaN, negative, infinite or
// 2^64 and above, else truncated)
template <typename T> struct OvOut;
template <> struct OvOut<double> {
    typedef ov_v2d Vec;
    static __device__ __forceinline__ double of(double v) { return v; }
    static __device__ __forceinline__ double none() { return ov_nan(); }
};
template <> struct OvOut<float> {
    typedef ov_v4f Vec;
    static __device__ __forceinline__ float of(double v) { return (float)v; }
    static __device__ __forceinline__ float none() { return __int_as_float(0x7fc00000); }
};
template <> struct OvOut<u64> {
    typedef ov_v2u Vec;
    static __device__ __forceinline__ u64 of(double v) { return (v >= 1.0 && v < 18446744073709551616.0) ? (u64)v : 0ull; }
    static __device__ __forceinline__ u64 none() { return 0ull; }
};

// One lane per 16 bytes of the output: K = 16 / sizeof(T) voxels of one mask word (K divides 64).
template <typename T>
__global__ __launch_bounds__(256) void ov_paint_kernel(const u64 *__restrict__ bits, const int *__restrict__ wpre, const double *__restrict__ val,
                                                       i64 n, T *__restrict__ out) {
    constexpr int K = 16 / (int)sizeof(T);
    const i64 i = ((i64)blockIdx.x * 256 + threadIdx.x) * K;
    if (i >= n) return;
    const int sh = (int)(i & 63);
    const u64 word = bits[i >> 6];
    i64 row = (i64)wpre[i >> 6] + __popcll(word & ((1ull << sh) - 1ull));
    T v[K];
    for (int k = 0; k < K; ++k) {
        const bool on = (word >> (sh + k)) & 1ull;      // a voxel at or beyond n has no bit
        v[k] = on ? OvOut<T>::of(val[row]) : OvOut<T>::none();
        row += on ? 1 : 0;
    }
    if (i + K <= n) {
        typename OvOut<T>::Vec q;
        for (int k = 0; k < K; ++k) q[k] = v[k];
        __builtin_nontemporal_store(q, reinterpret_cast<typename OvOut<T>::Vec *>(out + i));
    } else {
        for (int k = 0; k < K && i + k < n; ++k) out[i + k] = v[k];
    }
}
