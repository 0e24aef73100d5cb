// Shared by nellie_hip_reassign.hip, nellie_hip_voxfeat.hip, nellie_hip_nodefeat.hip, nellie_hip_branchfeat.hip, nellie_hip_adjacency.hip, nellie_hip_tracks.hip, nellie_hip_overlay.hip and nellie_hip_transitions.hip: a frame's 1-bit-per-voxel mask with its word populations, the
// exclusive scan of int counts (workgroup sums, one workgroup over the sums, write) with its host driver, the rank of a set bit
// of such a mask and the voxels' coordinates as flow queries.  The kernels are static: every translation unit that includes this
// file has its own copy.
#pragma once

#define RA_SCAN_CHUNK 4096            // counts per workgroup of the exclusive scan (256 lanes x 16)

typedef unsigned long long u64;

// One lane per voxel, one wave per mask word: bits[w] and the word's population count.  on(i): voxel i belongs to the mask.
template <typename Pred>
__global__ __launch_bounds__(256) void rank_mask_kernel(Pred on, i64 n, u64 *__restrict__ bits, int *__restrict__ wcount) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    const u64 b = __ballot(i < n && on(i));
    if ((threadIdx.x & 63) == 0) {
        bits[i >> 6] = b;
        wcount[i >> 6] = __popcll(b);
    }
}

static __global__ __launch_bounds__(256) void ra_scan_sums_kernel(const int *__restrict__ cnt, i64 m, i64 *__restrict__ bsum) {
    __shared__ i64 red[256];
    const i64 base = (i64)blockIdx.x * RA_SCAN_CHUNK + (i64)threadIdx.x * 16;
    i64 sum = 0;
    for (int k = 0; k < 16; ++k)
        if (base + k < m) sum += cnt[base + k];
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) bsum[blockIdx.x] = red[0];
}

// One workgroup: exclusive scan of the nb workgroup sums in place, total[0] = their sum.
static __global__ __launch_bounds__(1024) void ra_scan_top_kernel(i64 *__restrict__ bsum, i64 nb, i64 *__restrict__ total) {
    __shared__ i64 part[1024];
    const i64 per = (nb + 1023) / 1024;
    const i64 a = (i64)threadIdx.x * per, b = a + per < nb ? a + per : nb;
    i64 sum = 0;
    for (i64 c = a; c < b; ++c) sum += bsum[c];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int w = 1; w < 1024; w <<= 1) {
        const i64 add = (int)threadIdx.x >= w ? part[threadIdx.x - w] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    i64 run = part[threadIdx.x] - sum;
    for (i64 c = a; c < b; ++c) {
        const i64 k = bsum[c];
        bsum[c] = run;
        run += k;
    }
    if (threadIdx.x == 1023) total[0] = part[1023];
}

// pre[i] = the sum of cnt[0 .. i) (the host has checked that the total fits an int)
static __global__ __launch_bounds__(256) void ra_scan_write_kernel(const int *__restrict__ cnt, i64 m, const i64 *__restrict__ bsum, int *__restrict__ pre) {
    __shared__ int part[256];
    const i64 base = (i64)blockIdx.x * RA_SCAN_CHUNK + (i64)threadIdx.x * 16;
    int v[16];
    int sum = 0;
    for (int k = 0; k < 16; ++k) {
        v[k] = base + k < m ? cnt[base + k] : 0;
        sum += v[k];
    }
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int w = 1; w < 256; w <<= 1) {
        const int add = (int)threadIdx.x >= w ? part[threadIdx.x - w] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    int run = (int)bsum[blockIdx.x] + part[threadIdx.x] - sum;
    for (int k = 0; k < 16; ++k) {
        if (base + k < m) pre[base + k] = run;
        run += v[k];
    }
}

// rank of voxel i among the labelled voxels (its bit is set)
__device__ __forceinline__ int ra_rank(const u64 *__restrict__ bits, const int *__restrict__ pre, i64 i) {
    const u64 b = bits[i >> 6];
    return pre[i >> 6] + __popcll(b & ((1ull << (i & 63)) - 1ull));
}

// The voxels vox[0 .. n) (linear indices of a frame with rows of nx and planes of ny rows) as float64 query rows (n, D) of the
// flow interpolation: (z, y, x), or (y, x) of a one-plane frame.
static __global__ __launch_bounds__(256) void rank_coords_kernel(const i64 *__restrict__ vox, i64 n, i64 ny, i64 nx, int D, double *__restrict__ q) {
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const i64 i = vox[k];
    if (D == 3) q[k * 3] = (double)(i / (nx * ny));
    q[k * D + D - 2] = (double)((i / nx) % ny);
    q[k * D + D - 1] = (double)(i % nx);
}

// ---- host: the scan's driver ---------------------------------------------------------------------------------------------------
struct RankScan {
    i64 *d_bsum = nullptr;            // rank_scan_sums(longest scan) workgroup sums
    i64 *d_total = nullptr, *h_total = nullptr;      // one word, and its pinned landing place
};
static inline i64 rank_scan_sums(i64 longest) { return (longest + RA_SCAN_CHUNK - 1) / RA_SCAN_CHUNK + 1; }

// Exclusive scan of cnt[0 .. m) into pre, the total into *total (an error above `limit`).  Synchronises the stream.
static int rank_scan(const RankScan &s, hipStream_t st, const int *cnt, i64 m, int *pre, i64 limit, const char *what, i64 *total,
                     char *err, size_t errlen) {
    *total = 0;
    if (m <= 0) return NL_OK;
    const i64 nb = (m + RA_SCAN_CHUNK - 1) / RA_SCAN_CHUNK;
    ra_scan_sums_kernel<<<(unsigned)nb, 256, 0, st>>>(cnt, m, s.d_bsum);
    NL_CHECK_LAUNCH();
    ra_scan_top_kernel<<<1, 1024, 0, st>>>(s.d_bsum, nb, s.d_total);
    NL_CHECK_LAUNCH();
    NL_HIP(hipMemcpyAsync(s.h_total, s.d_total, 8, hipMemcpyDeviceToHost, st));
    NL_HIP(hipStreamSynchronize(st));
    *total = *s.h_total;
    if (*total > limit) return nl_fail(err, errlen, NL_EINVAL, "more than %lld %s", (long long)limit, what);
    ra_scan_write_kernel<<<(unsigned)nb, 256, 0, st>>>(cnt, m, s.d_bsum, pre);
    NL_CHECK_LAUNCH();
    return NL_OK;
}
