// Voxel reassignment (nellie/tracking/voxel_reassignment.py) -- kernels of nellie_hip_reassign.hip (DESIGN.md section 12).
//
// A frame is its union mask (branch > 0 | obj > 0) as one bit per voxel, the number of set bits before every 64-bit word, and
// the labelled voxels compacted in raster order (linear index, the two labels, the two reassigned labels).  The nearest labelled
// voxel to a predicted centroid is found by walking a table of lattice offsets, sorted by scaled length, from the rounded
// centroid and testing mask bits.  Candidates are grouped per target by a counting sort; one lane per target then orders its
// short list and votes.  The atomics only count and place: every result has a fixed order, two runs give the same bits.
//
// A 2-D frame runs as a 3-D one with one plane: 0 + dy*dy + dx*dx is dy*dy + dx*dx bit for bit.
// Compiled with -ffp-contract=off: the distances are products and sums, never a fused multiply-add.
#pragma once

#include "rank_scan.inc"            // mask, exclusive scan, ra_rank, query coordinates, u64

struct RaGeom {
    i64 nz, ny, nx, n;
    double s[3];                      // spacing (z, y, x); z is 1 for a 2-D frame (its differences are 0)
};

struct RaOffset {                     // 24 bytes
    int dz, dy, dx;
    int pad;
    double len;                       // |offset * spacing|
};

// ---- mask, scan, compaction ---------------------------------------------------------------------------------------------
struct RaLabelled {                   // rank_mask_kernel's predicate: the union mask
    const int *branch, *obj;
    __device__ bool operator()(i64 i) const { return branch[i] > 0 || obj[i] > 0; }
};

// One lane per voxel: the labelled ones write their row.  seed: reassigned = the labels themselves (frame 0), else 0.
__global__ __launch_bounds__(256) void ra_compact_kernel(const int *__restrict__ branch, const int *__restrict__ obj, i64 n,
                                                         const u64 *__restrict__ bits, const int *__restrict__ pre, int seed,
                                                         i64 *__restrict__ vox, int *__restrict__ lab_b, int *__restrict__ lab_o,
                                                         int *__restrict__ re_b, int *__restrict__ re_o) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if (!((bits[i >> 6] >> (i & 63)) & 1ull)) return;
    const int k = ra_rank(bits, pre, i);
    const int b = branch[i], o = obj[i];
    vox[k] = i;
    lab_b[k] = b;
    lab_o[k] = o;
    re_b[k] = seed && b > 0 ? b : 0;
    re_o[k] = seed && o > 0 ? o : 0;
}

// ---- search -------------------------------------------------------------------------------------------------------------
// One lane per query voxel: c = voxel + sign * vector; the nearest labelled voxel m of the other frame under
// d2 = sum_axes (float64(float32(c)) * s - m * s)^2, the lowest linear index on a tie; d = float32(|float32(c - m) * s|).
// match[k] = the rank of m when float64(d) < r, else -1 (a NaN vector included).
//
// The table holds every lattice offset of scaled length <= r + one voxel diagonal, by ascending length.  The centroid is
// within half a diagonal of the lattice point it rounds to, so the voxel at offset o is at least len(o) - half_diag away:
// the walk ends once that exceeds the best distance so far (a hair of slack covers the rounding of the bound itself).
// Nothing outside the table is within r + half a diagonal, and a nearest voxel farther than r is dropped by the test on d.
template <int D>
__global__ __launch_bounds__(256) void ra_search_kernel(const i64 *__restrict__ vox, i64 n, const double *__restrict__ vec, double sign,
                                                        RaGeom g, const u64 *__restrict__ bits, const int *__restrict__ pre,
                                                        const RaOffset *__restrict__ table, int ntab, double half_diag, double r,
                                                        int *__restrict__ match, float *__restrict__ dist) {
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    int found = -1;
    float d_out = 0.f;
    double v[3] = {0.0, 0.0, 0.0};
    for (int a = 0; a < D; ++a) v[3 - D + a] = vec[k * D + a];
    const bool ok = v[0] == v[0] && v[1] == v[1] && v[2] == v[2];
    const i64 i = vox[k];
    const double p[3] = {(double)(i / (g.nx * g.ny)), (double)((i / g.nx) % g.ny), (double)(i % g.nx)};
    double c[3], qs[3];
    i64 rc[3];
    bool reach = ok;
    for (int a = 0; a < 3; ++a) {
        c[a] = sign > 0.0 ? p[a] + v[a] : p[a] - v[a];
        const float cf = (float)c[a];
        qs[a] = (double)cf * g.s[a];
        const double rn = rint((double)cf);
        if (!(rn > -1e9 && rn < 1e9)) reach = false;       // infinite or absurdly far: no voxel is within r
        rc[a] = reach ? (i64)rn : 0;
    }
    if (reach) {
        double best2 = INFINITY, bestd = INFINITY;
        i64 besti = -1;
        for (int j = 0; j < ntab; ++j) {
            const RaOffset o = table[j];
            if (o.len - half_diag > bestd * (1.0 + 1e-12)) break;
            const i64 z = rc[0] + o.dz, y = rc[1] + o.dy, x = rc[2] + o.dx;
            if (z < 0 || z >= g.nz || y < 0 || y >= g.ny || x < 0 || x >= g.nx) continue;
            const i64 m = (z * g.ny + y) * g.nx + x;
            if (!((bits[m >> 6] >> (m & 63)) & 1ull)) continue;
            const double ez = qs[0] - (double)z * g.s[0], ey = qs[1] - (double)y * g.s[1], ex = qs[2] - (double)x * g.s[2];
            double d2 = ez * ez;
            d2 = d2 + ey * ey;
            d2 = d2 + ex * ex;
            if (d2 < best2 || (d2 == best2 && m < besti)) {
                best2 = d2;
                bestd = sqrt(d2);
                besti = m;
            }
        }
        if (besti >= 0) {
            const i64 mz = besti / (g.nx * g.ny), my = (besti / g.nx) % g.ny, mx = besti % g.nx;
            const double ez = (double)(float)(c[0] - (double)mz) * g.s[0];
            const double ey = (double)(float)(c[1] - (double)my) * g.s[1];
            const double ex = (double)(float)(c[2] - (double)mx) * g.s[2];
            double e2 = ez * ez;
            e2 = e2 + ey * ey;
            e2 = e2 + ex * ex;
            const float d = (float)sqrt(e2);
            if ((double)d < r) {
                found = ra_rank(bits, pre, besti);
                d_out = d;
            }
        }
    }
    match[k] = found;
    dist[k] = d_out;
}

// ---- candidates per target ----------------------------------------------------------------------------------------------
// Candidate ids: forward candidate of prev voxel i is i (target fw_match[i]); backward candidate of next voxel j is n0 + j
// (target j, source bw_match[j]): ascending id is the reference's candidate order.
__global__ __launch_bounds__(256) void ra_count_kernel(const int *__restrict__ fw_match, i64 n0, const int *__restrict__ bw_match, i64 n1,
                                                       int *__restrict__ cnt) {
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    if (k < n0) {
        const int t = fw_match[k];
        if (t >= 0) atomicAdd(&cnt[t], 1);
    } else if (k < n0 + n1) {
        const i64 j = k - n0;
        if (bw_match[j] >= 0) atomicAdd(&cnt[j], 1);
    }
}

__global__ __launch_bounds__(256) void ra_place_kernel(const int *__restrict__ fw_match, i64 n0, const int *__restrict__ bw_match, i64 n1,
                                                       int *__restrict__ cursor, int *__restrict__ ent) {
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    if (k < n0) {
        const int t = fw_match[k];
        if (t >= 0) ent[atomicAdd(&cursor[t], 1)] = (int)k;
    } else if (k < n0 + n1) {
        const i64 j = k - n0;
        if (bw_match[j] >= 0) ent[atomicAdd(&cursor[j], 1)] = (int)k;
    }
}

struct RaCand {
    const int *fw_match, *bw_match;
    const float *fw_d, *bw_d;
    int n0;
    __device__ __forceinline__ int src(int c) const { return c < n0 ? c : bw_match[c - n0]; }
    __device__ __forceinline__ float d(int c) const { return c < n0 ? fw_d[c] : bw_d[c - n0]; }
};

// The vote of one target for one label type: its list ent[a .. b) is put into (source label, -weight, candidate) order
// (candidates whose source has no reassigned label go last), the weights 1 / (d + 1e-6) of a label are summed one after the
// other, the largest sum wins and a tie stays with the smaller label.  0 when nothing votes.
__device__ int ra_vote(const RaCand &cd, const int *__restrict__ re_prev, int *__restrict__ ent, int a, int b) {
    for (int p = a + 1; p < b; ++p) {
        const int c = ent[p];
        const int l0 = re_prev[cd.src(c)];
        const int lc = l0 > 0 ? l0 : 0x7fffffff;
        const double wc = -(1.0 / ((double)cd.d(c) + 1e-6));
        int q = p - 1;
        while (q >= a) {
            const int e = ent[q];
            const int l1 = re_prev[cd.src(e)];
            const int le = l1 > 0 ? l1 : 0x7fffffff;
            const double we = -(1.0 / ((double)cd.d(e) + 1e-6));
            const bool after = le > lc || (le == lc && (we > wc || (we == wc && e > c)));
            if (!after) break;
            ent[q + 1] = e;
            --q;
        }
        ent[q + 1] = c;
    }
    int win = 0, cur = 0;
    double win_sum = 0.0, sum = 0.0;
    for (int p = a; p < b; ++p) {
        const int c = ent[p];
        const int l = re_prev[cd.src(c)];
        if (l <= 0) break;
        const double w = 1.0 / ((double)cd.d(c) + 1e-6);
        if (l != cur) {
            if (cur > 0 && sum > win_sum) { win = cur; win_sum = sum; }
            cur = l;
            sum = w;
        } else {
            sum = sum + w;
        }
    }
    if (cur > 0 && sum > win_sum) win = cur;
    return win;
}

// One lane per target (next voxel): the best pair (smallest d, then the earlier candidate) and the two votes.
__global__ __launch_bounds__(256) void ra_vote_kernel(i64 n1, RaCand cd, const int *__restrict__ start, const int *__restrict__ cnt,
                                                      int *__restrict__ ent, const int *__restrict__ re_b_prev, const int *__restrict__ re_o_prev,
                                                      const int *__restrict__ lab_b, const int *__restrict__ lab_o,
                                                      int *__restrict__ re_b, int *__restrict__ re_o, int *__restrict__ best_src) {
    const i64 t = (i64)blockIdx.x * 256 + threadIdx.x;
    if (t >= n1) return;
    const int a = start[t], b = a + cnt[t];
    int best = -1;
    float best_d = 0.f;
    for (int p = a; p < b; ++p) {
        const int c = ent[p];
        const float d = cd.d(c);
        if (best < 0 || d < best_d || (d == best_d && c < best)) {
            best = c;
            best_d = d;
        }
    }
    best_src[t] = best < 0 ? -1 : cd.src(best);
    re_b[t] = lab_b[t] > 0 && b > a ? ra_vote(cd, re_b_prev, ent, a, b) : 0;
    re_o[t] = lab_o[t] > 0 && b > a ? ra_vote(cd, re_o_prev, ent, a, b) : 0;
}
