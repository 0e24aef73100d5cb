// Kernels of nellie_hip_adjacency.hip: the edge lists of the hierarchy's adjacency maps (_save_adjacency_maps of
// nellie/feature_extraction/hierarchical.py).  Every list is a stable compaction that writes one (row, column) int64 pair per edge:
// the selected rows are ranked with the mask, word populations and exclusive scan of rank_scan.inc, and every selected lane stores
// its pair at its rank as one 16-byte vector store (a wave's selected lanes have consecutive ranks: its stores are contiguous).
#pragma once
#include "rank_scan.inc"

// a label array of int32 or int64 elements
struct AdjLabels {
    const void *p;
    int wide;                         // 1: int64, 0: int32
    __device__ __forceinline__ i64 operator[](i64 i) const { return wide ? ((const i64 *)p)[i] : (i64)((const int *)p)[i]; }
};

// pairs: the rows with a label above 0
struct AdjPositive {
    AdjLabels lab;
    __device__ __forceinline__ bool operator()(i64 i) const { return lab[i] > 0; }
};

// rows (i, lab[i] - bias) of the rows with lab[i] > 0, at their ranks.  The ballot is taken again from the label the lane has
// loaded for its pair anyway: the same bits as the mask's word, without reading it.
static __global__ __launch_bounds__(256) void adj_pairs_write_kernel(AdjLabels lab, i64 n, i64 bias, const int *__restrict__ pre,
                                                                     longlong2 *__restrict__ out) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    const i64 v = i < n ? lab[i] : 0;
    const u64 b = __ballot(v > 0);
    if (v > 0) out[pre[i >> 6] + __popcll(b & ((1ull << (i & 63)) - 1ull))] = make_longlong2(i, v - bias);
}

// expand: one lane per edge e of a CSR; its row is the last r with off[r] <= e (off[0] = 0 <= e < off[rows]: rows without edges,
// wherever they stand, share their offset with the next row that has some and are passed over)
static __global__ __launch_bounds__(256) void adj_expand_kernel(const i64 *__restrict__ off, i64 rows, const i64 *__restrict__ val, i64 E,
                                                                longlong2 *__restrict__ out) {
    const i64 e = (i64)blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    i64 lo = 0, hi = rows;
    while (hi - lo > 1) {
        const i64 mid = lo + ((hi - lo) >> 1);
        if (off[mid] <= e) lo = mid;
        else hi = mid;
    }
    out[e] = make_longlong2(lo, val[e]);
}

// lookup: table[parent[j]] = the last j with that label (the table holds -1 elsewhere; every parent[j] is in [0, table size))
static __global__ __launch_bounds__(256) void adj_table_kernel(const i64 *__restrict__ parent, i64 p, i64 *__restrict__ table) {
    const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
    if (j < p) atomicMax(&table[parent[j]], j);
}

// the children whose label is in the table; a child above the table's last label leaves the smallest such row in *bad (children are >= 0)
struct AdjListed {
    const i64 *child, *table;
    i64 max_label;
    i64 *bad;
    __device__ __forceinline__ bool operator()(i64 i) const {
        const i64 c = child[i];
        if (c > max_label) {
            atomicMin(bad, i);
            return false;
        }
        return table[c] >= 0;
    }
};

// rows (i, table[child[i]]) of the listed children, at their ranks (no child is above max_label any more)
static __global__ __launch_bounds__(256) void adj_lookup_write_kernel(const i64 *__restrict__ child, i64 n, const i64 *__restrict__ table,
                                                                      const int *__restrict__ pre, longlong2 *__restrict__ out) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    const i64 idx = i < n ? table[child[i]] : -1;
    const u64 b = __ballot(idx >= 0);
    if (idx >= 0) out[pre[i >> 6] + __popcll(b & ((1ull << (i & 63)) - 1ull))] = make_longlong2(i, idx);
}
