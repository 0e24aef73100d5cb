// Voxel-level features (Voxels of nellie/feature_extraction/hierarchical.py) -- kernels of nellie_hip_voxfeat.hip (DESIGN.md
// section 13).
//
// A frame is its mask (component label > 0) as one bit per voxel with the number of set bits before every 64-bit word, and the
// labelled voxels compacted in raster order (linear index, the two labels, intensity and structure value in their own dtypes).
// The pivot of a branch label is found by two atomic minima, first on the bits of the norm, then on the voxel index among the
// voxels that hold that norm; one lane per voxel then computes the motility features in float64, in numpy's operation order.
// A node walks its box over the mask bits in raster order; counting and placing give both CSR lists, and the per-voxel lists are
// sorted afterwards.  The atomics only take minima, count and place: every result has a fixed order, two runs give the same bits.
//
// A 2-D frame is a 3-D one with one plane.  Compiled with -ffp-contract=off: never a fused multiply-add where numpy multiplies
// and adds.
#pragma once
#include "rank_scan.inc"

struct VfGeom {
    i64 nz, ny, nx, n;
    double s[3];                      // spacing of the D axes, in axis order ((Z,) Y, X)
    double dt;
};

#define VF_NO_PIVOT 0x7f7f7f7f        // a pivot table entry no voxel has claimed (the table is filled with the byte 0x7f)

// ---- frame: mask, compaction -----------------------------------------------------------------------------------------------
__device__ __forceinline__ bool vf_positive(const void *__restrict__ p, int dtype, i64 i) {
    switch (dtype) {
        case NL_U8: return ((const uint8_t *)p)[i] > 0;
        case NL_I8: return ((const int8_t *)p)[i] > 0;
        case NL_U16: return ((const uint16_t *)p)[i] > 0;
        case NL_I16: return ((const int16_t *)p)[i] > 0;
        case NL_U32: return ((const uint32_t *)p)[i] > 0;
        case NL_I32: return ((const int32_t *)p)[i] > 0;
        case NL_F32: return ((const float *)p)[i] > 0.f;
        case NL_F64: return ((const double *)p)[i] > 0.0;
        case NL_U64: return ((const uint64_t *)p)[i] > 0;
        default: return ((const int64_t *)p)[i] > 0;
    }
}

struct VfPositive {                   // rank_mask_kernel's predicate: positive in dtype `dtype`
    const void *src;
    int dtype;
    __device__ bool operator()(i64 i) const { return vf_positive(src, dtype, i); }
};

__device__ __forceinline__ void vf_copy_elem(const void *__restrict__ src, i64 i, void *__restrict__ dst, i64 k, int size) {
    switch (size) {
        case 1: ((uint8_t *)dst)[k] = ((const uint8_t *)src)[i]; break;
        case 2: ((uint16_t *)dst)[k] = ((const uint16_t *)src)[i]; break;
        case 4: ((uint32_t *)dst)[k] = ((const uint32_t *)src)[i]; break;
        default: ((uint64_t *)dst)[k] = ((const uint64_t *)src)[i]; break;
    }
}

// One lane per voxel: the labelled ones write their row; max_branch[0] = the largest branch label among them.
__global__ __launch_bounds__(256) void vf_compact_kernel(const int *__restrict__ comp, const int *__restrict__ branch, const void *__restrict__ raw,
                                                         int raw_size, const void *__restrict__ st, int st_size, i64 n,
                                                         const u64 *__restrict__ bits, const int *__restrict__ pre, i64 *__restrict__ vox,
                                                         int *__restrict__ lab_c, int *__restrict__ lab_b, void *__restrict__ raw_c,
                                                         void *__restrict__ st_c, int *__restrict__ max_branch) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (!((bits[i >> 6] >> (i & 63)) & 1ull)) return;
    const int k = ra_rank(bits, pre, i);
    const int b = branch[i];
    vox[k] = i;
    lab_c[k] = comp[i];
    lab_b[k] = b;
    vf_copy_elem(raw, i, raw_c, k, raw_size);
    vf_copy_elem(st, i, st_c, k, st_size);
    if (b > 0) atomicMax(max_branch, b);
}

// ---- flow queries, pivots --------------------------------------------------------------------------------------------------
__device__ __forceinline__ void vf_position(i64 i, const VfGeom &g, int D, double *p) {
    if (D == 3) {
        p[0] = (double)(i / (g.nx * g.ny));
        p[1] = (double)((i / g.nx) % g.ny);
        p[2] = (double)(i % g.nx);
    } else {
        p[0] = (double)(i / g.nx);
        p[1] = (double)(i % g.nx);
    }
}

// sqrt of the squares added in axis order
template <int D> __device__ __forceinline__ double vf_norm(const double *x) {
    double sum = x[0] * x[0];
    for (int a = 1; a < D; ++a) sum = sum + x[a] * x[a];
    return sqrt(sum);
}

// |vector * spacing| of a voxel's flow vector; false when a component is NaN
template <int D> __device__ __forceinline__ bool vf_vec_norm(const double *__restrict__ vpx, i64 k, const VfGeom &g, double *norm) {
    double v[D];
    bool ok = true;
    for (int a = 0; a < D; ++a) {
        v[a] = vpx[k * D + a] * g.s[a];
        ok = ok && v[a] == v[a];
    }
    *norm = vf_norm<D>(v);
    return ok;
}

// Pass 1: best[label] = the smallest norm of the label, as the bits of a non-negative double (their order is the order of the values).
template <int D>
__global__ __launch_bounds__(256) void vf_pivot_norm_kernel(const double *__restrict__ vpx, i64 n, VfGeom g, const int *__restrict__ lab_b,
                                                            int nlab, u64 *__restrict__ best) {
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int l = lab_b[k];
    double norm;
    if (l < 0 || l >= nlab || !vf_vec_norm<D>(vpx, k, g, &norm)) return;
    atomicMin(&best[l], (u64)__double_as_longlong(norm));
}

// Pass 2: pivot[label] = the lowest voxel index among the voxels whose norm is the label's smallest.
template <int D>
__global__ __launch_bounds__(256) void vf_pivot_index_kernel(const double *__restrict__ vpx, i64 n, VfGeom g, const int *__restrict__ lab_b,
                                                             int nlab, const u64 *__restrict__ best, int *__restrict__ pivot) {
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int l = lab_b[k];
    double norm;
    if (l < 0 || l >= nlab || !vf_vec_norm<D>(vpx, k, g, &norm)) return;
    if ((u64)__double_as_longlong(norm) == best[l]) atomicMin(&pivot[l], (int)k);
}

// ---- motility --------------------------------------------------------------------------------------------------------------
// numpy's float remainder for a positive divisor
__device__ __forceinline__ double vf_pymod(double a, double b) {
    double m = fmod(a, b);
    if (m != 0.0) {
        if (m < 0.0) m = m + b;
    } else {
        m = 0.0;
    }
    return m;
}

// (rb - ra) / dt and its norm
template <int D> __device__ __forceinline__ double vf_linear(const double *ra, const double *rb, double dt, double *vel) {
    for (int a = 0; a < D; ++a) vel[a] = (rb[a] - ra[a]) / dt;
    return vf_norm<D>(vel);
}

// Angular velocity of ra -> rb about the origin.  2-D: the wrapped angle difference / dt (vel[0]), magnitude its absolute
// value.  3-D: ra x rb / (|ra| |rb|) / dt, NaN where |ra| |rb| == 0, magnitude its norm.
template <int D> __device__ __forceinline__ double vf_angular(const double *ra, const double *rb, double dt, double *vel) {
    if constexpr (D == 2) {
        const double ta = atan2(ra[1], ra[0]), tb = atan2(rb[1], rb[0]);
        double delta = tb - ta;
        delta = vf_pymod(delta + M_PI, 2.0 * M_PI) - M_PI;
        vel[0] = delta / dt;
        return fabs(vel[0]);
    } else {
        double c[3];
        c[0] = ra[1] * rb[2] - ra[2] * rb[1];
        c[1] = ra[2] * rb[0] - ra[0] * rb[2];
        c[2] = ra[0] * rb[1] - ra[1] * rb[0];
        const double norm = vf_norm<3>(ra) * vf_norm<3>(rb);
        for (int a = 0; a < 3; ++a) vel[a] = (norm == 0.0 ? NAN : c[a] / norm) / dt;
        return vf_norm<3>(vel);
    }
}

// One direction of one voxel: positions a -> b (um), its vector (um, for the NaN pattern) and the pivot's positions.
template <int D> struct VfPair {
    double lin[D], ang[3], rel_lin[D], rel_ang[3], rel_a[D], rel_b[D];
    double lin_mag, ang_mag, rel_lin_mag, rel_ang_mag;
    __device__ __forceinline__ void run(const double *ca, const double *cb, const double *vec, const double *pa, const double *pb, double dt) {
        lin_mag = vf_linear<D>(ca, cb, dt, lin);
        ang_mag = vf_angular<D>(ca, cb, dt, ang);
        for (int a = 0; a < D; ++a) {
            const bool gone = vec[a] != vec[a];
            rel_a[a] = ca[a] - (gone ? NAN : pa[a]);
            rel_b[a] = cb[a] - (gone ? NAN : pb[a]);
        }
        rel_lin_mag = vf_linear<D>(rel_a, rel_b, dt, rel_lin);
        rel_ang_mag = vf_angular<D>(rel_a, rel_b, dt, rel_ang);
    }
};

// Block offsets of the float32 outputs, in units of n floats: vec01 (D), vec12 (D), linear_vel_vector (D), linear_vel,
// angular_vel_vector (A = 1 in 2-D, 3 in 3-D), angular_vel, linear_acc, angular_acc, rel_linear_vel, rel_angular_vel,
// rel_linear_acc, rel_angular_acc, rel_directionality.
#define VF_OUT_BLOCKS 13
__host__ __device__ inline void vf_out_layout(int D, int *off) {
    const int A = D == 3 ? 3 : 1;
    const int width[VF_OUT_BLOCKS] = {D, D, D, 1, A, 1, 1, 1, 1, 1, 1, 1, 1};
    off[0] = 0;
    for (int j = 0; j < VF_OUT_BLOCKS; ++j) off[j + 1] = off[j] + width[j];
}

// One lane per voxel.  v01 / v12: the interpolated flow vectors in voxels (n, D), NaN rows where there is none.
template <int D>
__global__ __launch_bounds__(256) void vf_motility_kernel(const i64 *__restrict__ vox, i64 n, VfGeom g, const int *__restrict__ lab_b, int nlab,
                                                          const double *__restrict__ v01, const double *__restrict__ v12,
                                                          const int *__restrict__ pivot01, const int *__restrict__ pivot12,
                                                          float *__restrict__ out) {
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    constexpr int A = D == 3 ? 3 : 1;
    int off[VF_OUT_BLOCKS + 1];
    vf_out_layout(D, off);
    const double dt = g.dt;
    double px[3], c0[D], c1[D], c2[D], vec01[D], vec12[D];
    vf_position(vox[k], g, D, px);
    for (int a = 0; a < D; ++a) {
        const double a01 = v01[k * D + a], a12 = v12[k * D + a];
        vec01[a] = a01 * g.s[a];
        vec12[a] = a12 * g.s[a];
        c1[a] = px[a] * g.s[a];
        c0[a] = (px[a] - a01) * g.s[a];
        c2[a] = (px[a] + a12) * g.s[a];
    }
    // the pivots' positions: before and at t (direction 01), at t and after (direction 12); NaN without a pivot
    double p0[D], p1a[D], p1b[D], p2[D];
    const int l = lab_b[k];
    const int q01 = l >= 0 && l < nlab ? pivot01[l] : VF_NO_PIVOT, q12 = l >= 0 && l < nlab ? pivot12[l] : VF_NO_PIVOT;
    for (int a = 0; a < D; ++a) p0[a] = p1a[a] = p1b[a] = p2[a] = NAN;
    if (q01 < n) {
        double qx[3];
        vf_position(vox[q01], g, D, qx);
        for (int a = 0; a < D; ++a) {
            p0[a] = (qx[a] - v01[(i64)q01 * D + a]) * g.s[a];
            p1a[a] = qx[a] * g.s[a];
        }
    }
    if (q12 < n) {
        double qx[3];
        vf_position(vox[q12], g, D, qx);
        for (int a = 0; a < D; ++a) {
            p1b[a] = qx[a] * g.s[a];
            p2[a] = (qx[a] + v12[(i64)q12 * D + a]) * g.s[a];
        }
    }
    VfPair<D> a, b;
    a.run(c0, c1, vec01, p0, p1a, dt);
    b.run(c1, c2, vec12, p1b, p2, dt);
    const double r1 = vf_norm<D>(b.rel_a), r2 = vf_norm<D>(b.rel_b), denom = r2 + r1;
    const double direct = denom != 0.0 ? fabs(r2 - r1) / denom : NAN;
    double d_lin[D], d_rel[D], d_ang[3], d_rang[3];
    for (int x = 0; x < D; ++x) {
        d_lin[x] = (b.lin[x] - a.lin[x]) / dt;
        d_rel[x] = (b.rel_lin[x] - a.rel_lin[x]) / dt;
    }
    for (int x = 0; x < A; ++x) {
        d_ang[x] = (b.ang[x] - a.ang[x]) / dt;
        d_rang[x] = (b.rel_ang[x] - a.rel_ang[x]) / dt;
    }
    const double lin_acc = vf_norm<D>(d_lin), rel_lin_acc = vf_norm<D>(d_rel);
    const double ang_acc = D == 2 ? fabs(d_ang[0]) : vf_norm<A>(d_ang), rel_ang_acc = D == 2 ? fabs(d_rang[0]) : vf_norm<A>(d_rang);
    for (int x = 0; x < D; ++x) {
        out[off[0] * n + k * D + x] = (float)vec01[x];
        out[off[1] * n + k * D + x] = (float)vec12[x];
        out[off[2] * n + k * D + x] = (float)b.lin[x];
    }
    out[off[3] * n + k] = (float)b.lin_mag;
    for (int x = 0; x < A; ++x) out[off[4] * n + k * A + x] = (float)b.ang[x];
    out[off[5] * n + k] = (float)b.ang_mag;
    out[off[6] * n + k] = (float)lin_acc;
    out[off[7] * n + k] = (float)ang_acc;
    out[off[8] * n + k] = (float)b.rel_lin_mag;
    out[off[9] * n + k] = (float)b.rel_ang_mag;
    out[off[10] * n + k] = (float)rel_lin_acc;
    out[off[11] * n + k] = (float)rel_ang_acc;
    out[off[12] * n + k] = (float)direct;
}

// ---- nodes -----------------------------------------------------------------------------------------------------------------
// One lane per voxel: the ones with pixel class > 0 write their linear index and radius.
__global__ __launch_bounds__(256) void vf_node_compact_kernel(const void *__restrict__ dist, int dist_dtype, i64 n, const u64 *__restrict__ bits,
                                                              const int *__restrict__ pre, i64 *__restrict__ node_vox, double *__restrict__ radius) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (!((bits[i >> 6] >> (i & 63)) & 1ull)) return;
    const int k = ra_rank(bits, pre, i);
    node_vox[k] = i;
    radius[k] = dist_dtype == NL_F32 ? (double)((const float *)dist)[i] : ((const double *)dist)[i];
}

// numpy's float64 -> int64 cast: truncation toward zero; what does not fit becomes the smallest int64 (the clamp to 0 follows)
__device__ __forceinline__ i64 vf_trunc(double v) {
    if (!(v > -9.2e18 && v < 9.2e18)) return (i64)0x8000000000000000ull;
    return (i64)v;
}

// Box limits per node and axis: lims[(a * m + k) * 2 + {0, 1}] = trunc(radius * -1 + index), trunc(radius * 1 + index) + 1, clamped
// to [0, size of the axis].
__global__ __launch_bounds__(256) void vf_node_lims_kernel(const i64 *__restrict__ node_vox, const double *__restrict__ radius, i64 m, VfGeom g,
                                                           int D, i64 *__restrict__ lims) {
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    if (k >= m) return;
    double p[3];
    vf_position(node_vox[k], g, D, p);
    const i64 size[3] = {D == 3 ? g.nz : g.ny, D == 3 ? g.ny : g.nx, g.nx};
    const double r = radius[k];
    for (int a = 0; a < D; ++a) {
        i64 lo = vf_trunc(r * -1.0 + p[a]), hi = vf_trunc(r * 1.0 + p[a]) + 1;
        lo = lo < 0 ? 0 : (lo > size[a] ? size[a] : lo);
        hi = hi < 0 ? 0 : (hi > size[a] ? size[a] : hi);
        lims[(a * m + k) * 2] = lo;
        lims[(a * m + k) * 2 + 1] = hi;
    }
}

// The walk of one node's box over the mask bits in raster order: f(rank) for every labelled voxel inside, both ends of the
// limits included (an upper limit equal to the axis size ends at the last voxel).
template <typename F>
__device__ __forceinline__ void vf_walk_box(const i64 *__restrict__ lims, i64 m, i64 k, const VfGeom &g, int D, const u64 *__restrict__ bits,
                                            const int *__restrict__ pre, F f) {
    i64 lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    const i64 size[3] = {g.nz, g.ny, g.nx};
    for (int a = 0; a < D; ++a) {
        const int b = 3 - D + a;
        lo[b] = lims[(a * m + k) * 2];
        hi[b] = lims[(a * m + k) * 2 + 1];
        if (hi[b] > size[b] - 1) hi[b] = size[b] - 1;
    }
    if (lo[2] > hi[2]) return;
    for (i64 z = lo[0]; z <= hi[0]; ++z)
        for (i64 y = lo[1]; y <= hi[1]; ++y) {
            const i64 first = (z * g.ny + y) * g.nx + lo[2], last = (z * g.ny + y) * g.nx + hi[2];
            for (i64 w = first >> 6; w <= last >> 6; ++w) {
                u64 b = bits[w];
                if (w == first >> 6) b &= ~0ull << (first & 63);
                if (w == last >> 6) b &= ~0ull >> (63 - (last & 63));
                if (!b) continue;
                const u64 word = bits[w];
                const int base = pre[w];
                while (b) {
                    const int bit = __ffsll((long long)b) - 1;
                    b &= b - 1;
                    f(base + __popcll(word & ((1ull << bit) - 1ull)));
                }
            }
        }
}

// One lane per node: the number of voxels in its box, and one count per (voxel, node) pair at the voxel.
__global__ __launch_bounds__(256) void vf_node_count_kernel(const i64 *__restrict__ lims, i64 m, VfGeom g, int D, const u64 *__restrict__ bits,
                                                            const int *__restrict__ pre, int *__restrict__ ncount, int *__restrict__ vcount) {
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    if (k >= m) return;
    int count = 0;
    vf_walk_box(lims, m, k, g, D, bits, pre, [&](int rank) {
        ++count;
        atomicAdd(&vcount[rank], 1);
    });
    ncount[k] = count;
}

// One lane per node: its voxels in raster order into node_val[nstart ..), itself into every one of its voxels' lists.
__global__ __launch_bounds__(256) void vf_node_place_kernel(const i64 *__restrict__ lims, i64 m, VfGeom g, int D, const u64 *__restrict__ bits,
                                                            const int *__restrict__ pre, const int *__restrict__ nstart, int *__restrict__ node_val,
                                                            int *__restrict__ cursor, int *__restrict__ vox_val) {
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    if (k >= m) return;
    int at = nstart[k];
    vf_walk_box(lims, m, k, g, D, bits, pre, [&](int rank) {
        node_val[at++] = rank;
        vox_val[atomicAdd(&cursor[rank], 1)] = (int)k;
    });
}

// One lane per voxel: its short list of nodes into ascending order.
__global__ __launch_bounds__(256) void vf_sort_lists_kernel(i64 n, const int *__restrict__ start, const int *__restrict__ count, int *__restrict__ val) {
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int a = start[k], b = a + count[k];
    for (int p = a + 1; p < b; ++p) {
        const int c = val[p];
        int q = p - 1;
        while (q >= a && val[q] > c) {
            val[q + 1] = val[q];
            --q;
        }
        val[q + 1] = c;
    }
}
