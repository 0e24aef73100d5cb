// Solidity (DESIGN.md section 25) -- kernels of nellie_hip_branchfeat.hip: per region of a label frame, the exact number of
// lattice points in the closed convex hull of its voxels' diamonds (skimage's area_convex / pixel volume).  Three steps:
//   1. candidates: per row (z, y) of a region's bounding box the smallest and the largest x of the region (only the ends of a run
//      along X can be hull vertices), then per (region, plane) the rows that are vertices of the plane's 2-D hull;
//   2. the hull itself, on the host in exact integers (convex_hull.h), which returns per region a list of facets N . p <= d in
//      doubled box-relative coordinates;
//   3. the count: one lane per box row cuts [0, extent_x) by every facet and adds the length of what is left.
// Everything is an integer; the counts do not depend on the order in which lanes finish.
#pragma once
#include "branchfeat.inc"

#define CV_WG 256                     // lanes, and box rows, per workgroup of the count kernel
#define CV_CHUNK 64                   // facets staged in LDS at a time (2 KiB)
#define CV_MAX_GRID 1024              // workgroups of one count launch: the rest of the row blocks are reached by striding
#define CV_NO_MIN 0x7f7f7f7f          // xmin of a row without a candidate (memset 0x7f); xmax is then -1 (memset 0xff)

struct CvBox { int lo[3], ext[3]; };  // a region's bounding box: smallest (z, y, x) and extents; z: 0 and 1 in 2-D

// ---- step 1: candidates ----------------------------------------------------------------------------------------------------------
// One lane per voxel: a voxel whose label differs from its left neighbour's offers its x to the row's minimum, one whose label
// differs from its right neighbour's to the row's maximum.  Rows: rowoff[r] + (z - lo_z) * ext_y + (y - lo_y), inside the table as
// the box is the region's own.
static __global__ __launch_bounds__(256) void cv_extremes_kernel(BfLabels lab, i64 n, NfGeom g, const u64 *__restrict__ pres, const int *__restrict__ pre,
                                                                 const CvBox *__restrict__ box, const i64 *__restrict__ rowoff, int *__restrict__ xmin,
                                                                 int *__restrict__ xmax) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const i64 l = lab(i);
    if (l <= 0) return;
    const i64 x = i % g.nx;
    const bool first = x == 0 || lab(i - 1) != l, last = x == g.nx - 1 || lab(i + 1) != l;
    if (!first && !last) return;
    const i64 z = i / (g.nx * g.ny), y = (i / g.nx) % g.ny;
    const int r = ra_rank(pres, pre, l);
    const CvBox b = box[r];
    const i64 row = rowoff[r] + (z - b.lo[0]) * b.ext[1] + (y - b.lo[1]);
    if (first) atomicMin(&xmin[row], (int)x);
    if (last) atomicMax(&xmax[row], (int)x);
}

// One lane per (region, plane), found by bisection of planeoff (planes before every region, R + 1 entries).  The rows of a plane
// arrive sorted by y; a monotone chain keeps the rows whose (y, xmin) is a vertex of the plane's hull on the low-x side, another
// the rows whose (y, xmax) is one on the high-x side.  The chains' stacks lie in keep_lo / keep_hi over the plane's own rows (a
// stack never holds more rows than have been read).  A row off a chain loses that end: xmin = CV_NO_MIN, xmax = -1.  A vertex of
// the region's 3-D hull is a vertex of its plane's 2-D hull, so none is lost; in 2-D this already is the hull.
static __global__ __launch_bounds__(256) void cv_plane_kernel(i64 planes, i64 R, const i64 *__restrict__ planeoff, const CvBox *__restrict__ box,
                                                              const i64 *__restrict__ rowoff, int *__restrict__ xmin, int *__restrict__ xmax,
                                                              int *__restrict__ keep_lo, int *__restrict__ keep_hi) {
    const i64 k = (i64)blockIdx.x * 256 + threadIdx.x;
    if (k >= planes) return;
    i64 a = 0, b = R;                                                  // planeoff[a] <= k < planeoff[b]
    while (b - a > 1) {
        const i64 mid = a + (b - a) / 2;
        if (planeoff[mid] <= k) a = mid; else b = mid;
    }
    const int ny = box[a].ext[1];
    const i64 base = rowoff[a] + (k - planeoff[a]) * ny;
    int *mn = xmin + base, *mx = xmax + base, *slo = keep_lo + base, *shi = keep_hi + base;
    int nlo = 0, nhi = 0;
    for (int y = 0; y < ny; ++y) {
        if (mn[y] > mx[y]) continue;                                   // no voxel of the region in this row
        while (nlo >= 2) {                                             // the middle one stays when it lies strictly on the low-x side
            const i64 ya = slo[nlo - 2], yb = slo[nlo - 1];
            if ((i64)(mn[yb] - mn[ya]) * (y - ya) < (i64)(mn[y] - mn[ya]) * (yb - ya)) break;
            --nlo;
        }
        slo[nlo++] = y;
        while (nhi >= 2) {
            const i64 ya = shi[nhi - 2], yb = shi[nhi - 1];
            if ((i64)(mx[yb] - mx[ya]) * (y - ya) > (i64)(mx[y] - mx[ya]) * (yb - ya)) break;
            --nhi;
        }
        shi[nhi++] = y;
    }
    int plo = 0, phi = 0;
    for (int y = 0; y < ny; ++y) {
        if (plo < nlo && slo[plo] == y) ++plo; else mn[y] = CV_NO_MIN;
        if (phi < nhi && shi[phi] == y) ++phi; else mx[y] = -1;
    }
}

// ---- step 3: the count -----------------------------------------------------------------------------------------------------------
// floor(a / b) for b > 0, clamped: a result outside (-2^17, 2^17) comes back as some value beyond the same end, which is all an
// interval inside [0, 2^15) needs, whichever sign it is used with.  The quotient is estimated in float64 (relative error 2^-51: below one for |q| < 2^17) and
// set right by one exact multiply: |q| * b stays below 2^18 * 2^36.
__device__ __forceinline__ i64 cv_floor_div(i64 a, i64 b) {
    double e = floor((double)a / (double)b);
    e = e < -131071.0 ? -131071.0 : e > 131071.0 ? 131071.0 : e;
    i64 q = (i64)e;
    if (q * b > a) --q;
    else if ((q + 1) * b <= a) ++q;
    return q;
}

struct CvTask { int region, row0; };  // a block of up to CV_WG box rows of one region

// One workgroup per task (striding over them), one lane per box row (z, y) of the task's region.  The region's facets
// facets[4 f .. 4 f + 3] = (N_z, N_y, N_x, d), f in [facetoff[r], facetoff[r + 1]), pass through LDS in chunks of CV_CHUNK; each
// lane cuts its interval [lo, hi] of x in [0, ext_x) by N_x 2 x <= d - N_z 2 z - N_y 2 y: a floor for N_x > 0, a ceiling for
// N_x < 0, all or nothing for N_x = 0.  max(0, hi - lo + 1) is summed over the wave and added once to count[r].  |d|, |N . p|
// < 2^54 and |N_x| < 2^35 (convex_hull.h).
static __global__ __launch_bounds__(CV_WG) void cv_count_kernel(const CvTask *__restrict__ tasks, i64 ntasks, const CvBox *__restrict__ box,
                                                                const i64 *__restrict__ facetoff, const i64 *__restrict__ facets, u64 *__restrict__ count) {
    __shared__ i64 stage[CV_CHUNK * 4];
    for (i64 t = blockIdx.x; t < ntasks; t += gridDim.x) {             // uniform over the workgroup, as are the chunk bounds
        const CvTask task = tasks[t];
        const CvBox b = box[task.region];
        const i64 rows = (i64)b.ext[0] * b.ext[1], row = (i64)task.row0 + threadIdx.x;
        const bool live = row < rows;
        const i64 Z = 2 * (row / b.ext[1]), Y = 2 * (row % b.ext[1]);
        const i64 f0 = facetoff[task.region], f1 = facetoff[task.region + 1];
        i64 lo = 0, hi = live && f1 > f0 ? b.ext[2] - 1 : -1;            // no facets: no hull, nothing inside
        for (i64 c = f0; c < f1; c += CV_CHUNK) {
            const int m = (int)(f1 - c < CV_CHUNK ? f1 - c : CV_CHUNK);
            __syncthreads();                                           // the chunk before has been read by every lane
            for (int j = threadIdx.x; j < m * 4; j += CV_WG) stage[j] = facets[c * 4 + j];
            __syncthreads();
            if (lo > hi) continue;
            for (int j = 0; j < m; ++j) {
                const i64 nx = stage[4 * j + 2];
                const i64 rhs = stage[4 * j + 3] - stage[4 * j] * Z - stage[4 * j + 1] * Y;
                if (nx == 0) {
                    if (rhs < 0) hi = -1;
                } else if (nx > 0) {
                    const i64 q = cv_floor_div(rhs, 2 * nx);
                    hi = q < hi ? q : hi;
                } else {
                    const i64 q = -cv_floor_div(rhs, -2 * nx);         // ceil(rhs / (2 nx)) = -floor(rhs / (-2 nx))
                    lo = q > lo ? q : lo;
                }
            }
        }
        u64 sum = hi >= lo ? (u64)(hi - lo + 1) : 0ull;
        for (int w = 32; w > 0; w >>= 1) sum += __shfl_xor(sum, w);
        if ((threadIdx.x & 63) == 0 && sum > 0) atomicAdd(&count[task.region], sum);
    }
}
