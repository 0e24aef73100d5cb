// Flow-vector interpolation (nellie/tracking/flow_interpolation.py:141-256) -- kernels of nellie_hip_flow.hip.
//
// The flow rows of one time point ("check" rows: scaled position, vector, cost) are binned into a uniform grid whose cells
// are at least FLOW_CELL_SLACK * r wide, sorted by (cell, row index).  A query (one per lane) visits the 3^D cells around
// its own in cell order and the rows of a cell in row order, three times: zero test and minimum, sum, vector.  Nothing is
// stored per query, and every sum has a fixed order: two runs give the same bits.
//
// A 2-D field runs as a 3-D one with a leading axis of constant 0: 0 + dy*dy + dx*dx is dy*dy + dx*dx bit for bit.
// Compiled with -ffp-contract=off: d2 is products and sums, never a fused multiply-add.
#pragma once

#define FLOW_CELL_SLACK (1.0 + 1.0 / 1048576.0)   // cells a hair wider than r: a row within r is in a neighbouring cell whatever
                                                   // the rounding of the two cell indices (their error is below 1e-11 cells)
#define FLOW_MAX_CELLS (1 << 18)
#define FLOW_MIN_CELLS (1 << 12)

struct FlowRow {        // 64 bytes: one row is one aligned half cache line
    double c[3];        // check coordinate * spacing
    double v[3];        // flow vector (voxels)
    double cost;
    double pad;
};

struct FlowGrid {
    double mn[3];       // lower corner of the rows' bounding box (scaled)
    double inv[3];      // 1 / cell edge per axis
    int dims[3];
    int ncell;
};

struct FlowSpacing { double s[3]; };

// floor((x - mn) * inv) kept in double, so that a far or non-finite coordinate never reaches an integer conversion
__device__ __forceinline__ double flow_cell_pos(double x, double mn, double inv) { return floor((x - mn) * inv); }

__device__ __forceinline__ int flow_row_cell(const FlowGrid &g, const double *cs) {
    int idx = 0;
    for (int a = 0; a < 3; ++a) {
        double f = flow_cell_pos(cs[a], g.mn[a], g.inv[a]);
        int k = 0;
        if (f >= 1.0) k = f >= (double)(g.dims[a] - 1) ? g.dims[a] - 1 : (int)f;   // NaN, negative and zero give 0
        idx = idx * g.dims[a] + k;
    }
    return idx;
}

// scaled check coordinates of row i (coords / vectors are (n, D) row-major; D = 2 maps to axes 1, 2)
__device__ __forceinline__ void flow_scaled(const double *coords, int D, i64 i, const FlowSpacing &sp, double *cs) {
    cs[0] = 0.0;
    for (int a = 0; a < D; ++a) cs[3 - D + a] = coords[i * D + a] * sp.s[3 - D + a];
}

// One workgroup: the bounding box of the scaled rows, then the grid -- cells of edge FLOW_CELL_SLACK * r, doubled along the
// longest axis (in cells) until at most max_cells are left -- and zeroes its counters.
__global__ __launch_bounds__(1024) void flow_grid_kernel(const double *__restrict__ coords, int D, int n, FlowSpacing sp, double r, int max_cells,
                                                         FlowGrid *__restrict__ grid, int *__restrict__ start) {
    __shared__ double red[1024];
    __shared__ double box[6];
    __shared__ int s_ncell;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = threadIdx.x; i < n; i += 1024) {
        double cs[3];
        flow_scaled(coords, D, i, sp, cs);
        for (int a = 0; a < 3; ++a) {
            lo[a] = cs[a] < lo[a] ? cs[a] : lo[a];
            hi[a] = cs[a] > hi[a] ? cs[a] : hi[a];
        }
    }
    for (int q = 0; q < 6; ++q) {
        const bool is_min = q < 3;
        red[threadIdx.x] = is_min ? lo[q] : hi[q - 3];
        __syncthreads();
        for (int w = 512; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) {
                const double a = red[threadIdx.x], b = red[threadIdx.x + w];
                red[threadIdx.x] = is_min ? (b < a ? b : a) : (b > a ? b : a);
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) box[q] = red[0];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double h = r * FLOW_CELL_SLACK;
        FlowGrid g;
        double full[3];
        int mult[3] = {1, 1, 1};
        for (int a = 0; a < 3; ++a) {
            double ext = box[3 + a] - box[a];
            if (!(ext >= 0.0) || !(ext < 1e300)) ext = 0.0;             // no finite rows on this axis: one cell
            double f = floor(ext / h) + 1.0;
            full[a] = f < 1e15 ? f : 1e15;
            g.mn[a] = box[a] == box[a] && fabs(box[a]) < 1e300 ? box[a] : 0.0;
        }
        for (;;) {
            double cells = 1.0;
            int longest = 0;
            double dims[3];
            for (int a = 0; a < 3; ++a) {
                dims[a] = ceil(full[a] / (double)mult[a]);
                cells *= dims[a];
                if (dims[a] > dims[longest]) longest = a;
            }
            if (cells <= (double)max_cells || mult[longest] >= (1 << 30)) {
                for (int a = 0; a < 3; ++a) {
                    g.dims[a] = (int)dims[a];
                    g.inv[a] = 1.0 / (h * (double)mult[a]);
                }
                g.ncell = (int)cells;
                if (!(cells <= (double)max_cells)) {                 // an extent no grid of this size resolves: one cell, every query scans it
                    g.ncell = 1;
                    for (int a = 0; a < 3; ++a) { g.dims[a] = 1; g.inv[a] = 0.0; }
                }
                break;
            }
            mult[longest] *= 2;
        }
        *grid = g;
        s_ncell = g.ncell;
    }
    __syncthreads();
    for (int c = threadIdx.x; c <= s_ncell; c += 1024) start[c] = 0;
}

__global__ __launch_bounds__(256) void flow_count_kernel(const double *__restrict__ coords, int D, int n, FlowSpacing sp,
                                                         const FlowGrid *__restrict__ grid, int *__restrict__ start, int *__restrict__ cell_of) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const FlowGrid g = *grid;
    double cs[3];
    flow_scaled(coords, D, i, sp, cs);
    const int c = flow_row_cell(g, cs);
    cell_of[i] = c;
    atomicAdd(&start[c], 1);
}

// One workgroup: exclusive scan of the cell counts in place (start[ncell] = n), and a copy as the placement cursors.
__global__ __launch_bounds__(1024) void flow_scan_kernel(const FlowGrid *__restrict__ grid, int *__restrict__ start, int *__restrict__ cursor) {
    __shared__ int part[1024];
    const int ncell = grid->ncell;
    const int per = (ncell + 1023) / 1024;
    const int a = threadIdx.x * per, b = a + per < ncell ? a + per : ncell;
    int sum = 0;
    for (int c = a; c < b; ++c) sum += start[c];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int w = 1; w < 1024; w <<= 1) {
        const int add = (int)threadIdx.x >= w ? part[threadIdx.x - w] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    int run = part[threadIdx.x] - sum;
    for (int c = a; c < b; ++c) {
        const int k = start[c];
        start[c] = run;
        cursor[c] = run;
        run += k;
    }
    if (threadIdx.x == 1023) start[ncell] = part[1023];
}

__global__ __launch_bounds__(256) void flow_place_kernel(int n, const int *__restrict__ cell_of, int *__restrict__ cursor, int *__restrict__ perm) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    perm[atomicAdd(&cursor[cell_of[i]], 1)] = i;
}

// One lane per cell: puts the cell's rows into ascending row index (the placement order above is whatever the atomics gave)
// and writes them out.  A cell holds a handful of rows; an insertion sort is enough.
__global__ __launch_bounds__(256) void flow_sort_write_kernel(const double *__restrict__ coords, const double *__restrict__ vectors,
                                                              const double *__restrict__ costs, int D, FlowSpacing sp,
                                                              const FlowGrid *__restrict__ grid, const int *__restrict__ start,
                                                              int *__restrict__ perm, FlowRow *__restrict__ rows) {
    const int ncell = grid->ncell;
    for (int c = blockIdx.x * 256 + threadIdx.x; c < ncell; c += gridDim.x * 256) {
        const int a = start[c], b = start[c + 1];
        for (int p = a + 1; p < b; ++p) {
            const int key = perm[p];
            int q = p - 1;
            while (q >= a && perm[q] > key) {
                perm[q + 1] = perm[q];
                --q;
            }
            perm[q + 1] = key;
        }
        for (int p = a; p < b; ++p) {
            const i64 i = perm[p];
            FlowRow R;
            flow_scaled(coords, D, i, sp, R.c);
            R.v[0] = 0.0;
            for (int k = 0; k < D; ++k) R.v[3 - D + k] = vectors[i * D + k];
            R.cost = costs[i];
            R.pad = 0.0;
            rows[p] = R;
        }
    }
}

// The rows of the up to 27 cells around the query, in cell order: z, y outer, the x neighbours of one (z, y) are one run of `start`.
#define FLOW_FOR_NEIGHBOURS(...)                                                               \
    for (int cz = lo[0]; cz <= hi[0]; ++cz)                                                    \
        for (int cy = lo[1]; cy <= hi[1]; ++cy) {                                              \
            const int base_ = (cz * g.dims[1] + cy) * g.dims[2];                               \
            const int a_ = start[base_ + lo[2]], b_ = start[base_ + hi[2] + 1];                \
            for (int j = a_; j < b_; ++j) {                                                    \
                const FlowRow *R = rows + j;                                                   \
                const double dz_ = qs[0] - R->c[0], dy_ = qs[1] - R->c[1], dx_ = qs[2] - R->c[2]; \
                double d2 = dz_ * dz_;                                                         \
                d2 = d2 + dy_ * dy_;                                                           \
                d2 = d2 + dx_ * dx_;                                                           \
                if (d2 <= r2) { __VA_ARGS__ }                                                  \
            }                                                                                  \
        }

// the reference's distance weight of one neighbour: (d == 0) * 1.0 when any neighbour sits on the query, else 1 / d
__device__ __forceinline__ double flow_raw_weight(double d2, double cost, bool any_zero) {
    const double dw = any_zero ? (d2 == 0.0 ? 1.0 : 0.0) : 1.0 / sqrt(d2);
    return (-cost) * dw;
}

template <int D>
__global__ __launch_bounds__(256) void flow_interp_kernel(const double *__restrict__ q, i64 n, const FlowRow *__restrict__ rows,
                                                          const int *__restrict__ start, const FlowGrid *__restrict__ grid, FlowSpacing sp,
                                                          double r2, double *__restrict__ out, unsigned long long *__restrict__ found) {
    const i64 i = (i64)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const FlowGrid g = *grid;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double qs[3] = {0.0, 0.0, 0.0};
    for (int a = 0; a < D; ++a) qs[3 - D + a] = q[i * D + a] * sp.s[3 - D + a];
    int lo[3], hi[3];
    bool reach = true;
    for (int a = 0; a < 3; ++a) {
        const double f = flow_cell_pos(qs[a], g.mn[a], g.inv[a]);
        if (!(f >= -1.0 && f <= (double)g.dims[a])) {       // NaN, infinite or more than a cell outside the rows' box
            reach = false;
            lo[a] = 0;
            hi[a] = -1;
        } else {
            const int k = (int)f;
            lo[a] = k - 1 < 0 ? 0 : k - 1;
            hi[a] = k + 1 > g.dims[a] - 1 ? g.dims[a] - 1 : k + 1;
        }
    }
    int k = 0;
    if (reach) {
        // sweep 1: neighbour count, any d == 0, and the minimum raw weight in both forms
        bool any_zero = false, any_far = false;
        double min_zero = INFINITY, min_inv = INFINITY;
        FLOW_FOR_NEIGHBOURS({
            ++k;
            if (d2 == 0.0) {
                any_zero = true;
                const double w = flow_raw_weight(d2, R->cost, true);
                min_zero = w < min_zero ? w : min_zero;
            } else {
                any_far = true;
                const double w = flow_raw_weight(d2, R->cost, false);
                min_inv = w < min_inv ? w : min_inv;
            }
        })
        if (k > 0) {
            double wmin = min_inv;
            if (any_zero) {
                wmin = min_zero;
                if (any_far && !(wmin < 0.0)) wmin = 0.0;       // the neighbours off the query weigh -cost * 0.0
            }
            const double shift = wmin - 1.0;
            // sweep 2: the sum of the shifted weights
            double sum = 0.0;
            FLOW_FOR_NEIGHBOURS({
                double w = flow_raw_weight(d2, R->cost, any_zero);
                w = w - shift;
                sum = sum + w;
            })
            // sweep 3: the vector
            double v[3] = {0.0, 0.0, 0.0};
            FLOW_FOR_NEIGHBOURS({
                double w = flow_raw_weight(d2, R->cost, any_zero);
                w = w - shift;
                w = w / sum;
                v[0] = v[0] + R->v[0] * w;
                v[1] = v[1] + R->v[1] * w;
                v[2] = v[2] + R->v[2] * w;
            })
            for (int a = 0; a < D; ++a) out[i * D + a] = v[3 - D + a];
            atomicAdd(found, 1ull);
        }
    }
    if (k == 0)
        for (int a = 0; a < D; ++a) out[i * D + a] = nan;
}
