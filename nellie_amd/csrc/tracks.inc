// Voxel tracks of a label stack (nellie/tracking/all_tracks_for_label.py over flow_interpolation.py:317-426) -- kernels of
// nellie_hip_tracks.hip (DESIGN.md section 23).
//
// The seeds are the voxels of one frame's predicate mask whose rank is a multiple of `skip`, as float64 coordinates.  A step
// moves every coordinate by its interpolated flow vector (lost once the vector row is all NaN, for good), ballots the kept ones
// and, behind a scan of the word counts, appends one row [id, frame, (z,) y, x] per kept coordinate -- two, interleaved, at the
// first frame of a direction.  A track's rows are emitted in step order and a coordinate that is kept at a step was kept at every
// step before it, so the ordinal of a row within its track is the same for every row of a step: the backward rows reach their
// defined order (id, then frame ascending) through a count per id and a scan, without a sort.  The final filter tests the 1-bit
// mask of the row's frame at the coordinates rounded half to even.
//
// Block sizes: every kernel runs 256 lanes, one per voxel, coordinate or row, and ballots 64 wide; the scans cover
// RA_SCAN_CHUNK = 4096 counts per workgroup.  No floating-point atomics, no atomics at all: every position is computed.
// A 2-D frame is the 3-D case with one plane.  Compiled with -ffp-contract=off: a step is one float64 add or subtract.
#pragma once

#include "rank_scan.inc"

struct TkGeom { i64 nz, ny, nx, n; };

// rank_mask_kernel's predicates over an int32 label frame
struct TkLabelled {
    const int *lab;
    __device__ bool operator()(i64 i) const { return lab[i] > 0; }
};
struct TkIsLabel {
    const int *lab;
    int want;
    __device__ bool operator()(i64 i) const { return lab[i] == want; }
};

// One lane per mask word: its population (the seeds of a mask that is already on the device)
__global__ __launch_bounds__(256) void tk_popcount_kernel(const u64 *__restrict__ bits, i64 words, int *__restrict__ wcount) {
    const i64 w = (i64)blockIdx.x * 256 + threadIdx.x;
    if (w < words) wcount[w] = __popcll(bits[w]);
}

// One lane per voxel: a set voxel whose rank is a multiple of `skip` writes its coordinates as seed rank / skip.
template <int D>
__global__ __launch_bounds__(256) void tk_seed_kernel(const u64 *__restrict__ bits, const int *__restrict__ pre, TkGeom g, int skip,
                                                      double *__restrict__ seed) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= g.n) return;
    if (!((bits[i >> 6] >> (i & 63)) & 1ull)) return;
    const int rank = ra_rank(bits, pre, i);
    if (rank % skip) return;
    const i64 k = rank / skip;
    if (D == 3) seed[k * 3] = (double)(i / (g.nx * g.ny));
    seed[k * D + D - 2] = (double)((i / g.nx) % g.ny);
    seed[k * D + D - 1] = (double)(i % g.nx);
}

// One lane per coordinate: lost (the vector row is all NaN: the coordinate becomes NaN) or kept (coordinate +- vector).  The kept
// bits of 64 coordinates are one word with its count; `first`: the coordinate before the step is put aside for its start row;
// per_id != NULL: the rows this id has emitted so far (the backward order's counts).
template <int D>
__global__ __launch_bounds__(256) void tk_update_kernel(double *__restrict__ cur, const double *__restrict__ vec, i64 n, double sign, int first,
                                                        double *__restrict__ old, int *__restrict__ per_id, u64 *__restrict__ keep,
                                                        int *__restrict__ wcount) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    bool kept = false;
    if (i < n) {
        double v[D], c[D];
        bool lost = true;
        for (int a = 0; a < D; ++a) {
            v[a] = vec[i * D + a];
            c[a] = cur[i * D + a];
            lost = lost && v[a] != v[a];
        }
        kept = !lost;
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        for (int a = 0; a < D; ++a) {
            if (kept && first) old[i * D + a] = c[a];
            cur[i * D + a] = lost ? nan : (sign > 0.0 ? c[a] + v[a] : c[a] - v[a]);
        }
        if (kept && per_id) per_id[i] += first ? 2 : 1;
    }
    const u64 b = __ballot(kept);
    if ((threadIdx.x & 63) == 0) {      // keep / wcount hold a word for every wave of the grid
        keep[i >> 6] = b;
        wcount[i >> 6] = __popcll(b);
    }
}

// One lane per coordinate: the kept ones append their row(s) at `begin` in coordinate order.  W = 2 + D doubles per row.
template <int D>
__global__ __launch_bounds__(256) void tk_emit_kernel(const double *__restrict__ cur, const double *__restrict__ old, i64 n,
                                                      const u64 *__restrict__ keep, const int *__restrict__ pre, i64 begin, int first,
                                                      double id0, double frame_from, double frame_to, double *__restrict__ rows) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (!((keep[i >> 6] >> (i & 63)) & 1ull)) return;
    const i64 k = ra_rank(keep, pre, i);
    const int W = 2 + D;
    double *r = rows + (begin + (first ? 2 * k : k)) * W;
    const double id = id0 + (double)i;
    if (first) {
        r[0] = id;
        r[1] = frame_from;
        for (int a = 0; a < D; ++a) r[2 + a] = old[i * D + a];
        r += W;
    }
    r[0] = id;
    r[1] = frame_to;
    for (int a = 0; a < D; ++a) r[2 + a] = cur[i * D + a];
}

// One lane per row of a step's range [begin, end), for the rows of one frame (a first step holds two): whether the row stays --
// every coordinate, rounded half to even, inside the frame (tested in double, so that NaN, infinities and far values never reach
// an integer) and on a set bit of the frame's mask; bits = NULL: the frame lies outside the stack -- and where it goes in the
// defined order.  Forward rows stay where they are; a backward row of id k, the ord-th of its track (the start row of a first
// step ord, its next row ord + 1), goes to start[k] + per_id[k] - 1 - ord.
template <int D>
__global__ __launch_bounds__(256) void tk_filter_kernel(const double *__restrict__ rows, i64 begin, i64 end, double frame, TkGeom g,
                                                        const u64 *__restrict__ bits, int backward, int first, int ord, double id0,
                                                        const int *__restrict__ start, const int *__restrict__ per_id,
                                                        int *__restrict__ src, int *__restrict__ flag) {
    const i64 j = (i64)blockIdx.x * 256 + threadIdx.x;
    const i64 i = begin + j;
    if (i >= end) return;
    const int W = 2 + D;
    const double *r = rows + i * W;
    if (r[1] != frame) return;
    bool on = bits != nullptr;
    const double lim[3] = {(double)g.nz, (double)g.ny, (double)g.nx};
    i64 p[3] = {0, 0, 0};
    for (int a = 0; a < D; ++a) {
        const double c = rint(r[2 + a]);
        if (!(c >= 0.0 && c < lim[3 - D + a])) on = false;      // -0.0 is inside, NaN is not
        else p[3 - D + a] = (i64)c;
    }
    if (on) {
        const i64 m = (p[0] * g.ny + p[1]) * g.nx + p[2];
        on = (bits[m >> 6] >> (m & 63)) & 1ull;
    }
    i64 dest = i;
    if (backward) {
        const i64 k = (i64)(r[0] - id0);
        dest = (i64)start[k] + per_id[k] - 1 - (ord + (first ? (int)(j & 1) : 0));
    }
    src[dest] = (int)i;
    flag[dest] = on ? 1 : 0;
}

// One lane per position of the defined order: a row that stays is copied to its rank among them.
template <int D>
__global__ __launch_bounds__(256) void tk_compact_kernel(const double *__restrict__ rows, i64 n, const int *__restrict__ src,
                                                         const int *__restrict__ flag, const int *__restrict__ pre, double *__restrict__ out) {
    const i64 d = (i64)blockIdx.x * 256 + threadIdx.x;
    if (d >= n || !flag[d]) return;
    const int W = 2 + D;
    const double *r = rows + (i64)src[d] * W;
    double *o = out + (i64)pre[d] * W;
    for (int a = 0; a < W; ++a) o[a] = r[a];
}
