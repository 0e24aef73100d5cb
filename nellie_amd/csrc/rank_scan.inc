// Shared by nellie_hip_reassign.hip and nellie_hip_voxfeat.hip: the exclusive scan of int counts (workgroup sums, one workgroup
// over the sums, write) and the rank of a set bit of a 1-bit-per-voxel mask with word ranks.  The kernels are static: every
// translation unit that includes this file has its own copy.
#pragma once

#define RA_SCAN_CHUNK 4096            // counts per workgroup of the exclusive scan (256 lanes x 16)

typedef unsigned long long u64;

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
