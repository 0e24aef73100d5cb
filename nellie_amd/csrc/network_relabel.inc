// Network stage, everything behind the thinning but the classes (nellie/segmentation/networking.py:828-851):
//   skel    = labels * thinning mask                                                   (:408)
//   clean   : skeleton voxels whose 3x3x3 (2-D: 3x3) neighbourhood holds two labels    (:261-296)
//   seed    : one skeleton voxel, at the Frangi maximum, for every label without one   (:342-387)
//   relabel : per object, in its bounding box, the feature transform of the object's own branch voxels (:485-577) -- scipy's
//             separable Voronoi transform (ni_morphology.c, _VoronoiFT), one thread per line, all lines of all boxes of a batch
//             per launch.  float64, scipy's operation order; the unit is built with -ffp-contract=off.
// A feature is the frame-linear index of a seed (int32; -1: none), so a frame has fewer than 2^31 voxels here.

struct NwGeom { int nz, ny, nx, ndim; double s[3]; };

// One object of a batch: its label, its box, the first slot of the box in the scratch buffers and its first line in each pass.
struct NwObj { int label, z0, y0, x0, dz, dy, dx, pad; i64 off, line0[3]; };

#define NW_BOX_EMPTY 0x7fffffff

// stats[0] = max(stats[0], mx), stats[1] = min(stats[1], mn) over a 256-thread workgroup: one atomic pair per workgroup (atomics on one
// word are served one after another, about 10 ns each: per wave they cost more than the pass over the frame)
__device__ __forceinline__ void nw_block_minmax(int mx, int mn, int *__restrict__ stats) {
    __shared__ int s_mx[4], s_mn[4];
    for (int o = 32; o > 0; o >>= 1) {
        const int a = __shfl_xor(mx, o), b = __shfl_xor(mn, o);
        mx = a > mx ? a : mx;
        mn = b < mn ? b : mn;
    }
    if ((threadIdx.x & 63) == 0) { s_mx[threadIdx.x >> 6] = mx; s_mn[threadIdx.x >> 6] = mn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) { mx = s_mx[w] > mx ? s_mx[w] : mx; mn = s_mn[w] < mn ? s_mn[w] : mn; }
        if (mx > 0) atomicMax(stats, mx);
        if (mn < 0) atomicMin(stats + 1, mn);
    }
}

// ---- skel = labels * mask; the largest label ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
nw_skel_kernel(const int *__restrict__ lab, const uint8_t *__restrict__ mask, int *__restrict__ skel, i64 n, int *__restrict__ stats) {
    int mx = 0, mn = 0;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
        const int l = lab[i];
        skel[i] = mask[i] ? l : 0;
        mx = l > mx ? l : mx;
        mn = l < mn ? l : mn;
    }
    nw_block_minmax(mx, mn, stats);
}

__global__ void __launch_bounds__(256)
nw_minmax_kernel(const int *__restrict__ lab, i64 n, int *__restrict__ stats) {
    int mx = 0, mn = 0;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
        const int l = lab[i];
        mx = l > mx ? l : mx;
        mn = l < mn ? l : mn;
    }
    nw_block_minmax(mx, mn, stats);
}

// ---- clean (:261-296) -----------------------------------------------------------------------------------------------------------------
// in -> out (two volumes: a voxel's verdict reads its neighbours' ORIGINAL labels).  Voxels on a face are copied; an interior voxel has
// its whole neighbourhood inside the frame.
__global__ void __launch_bounds__(256)
nw_clean_kernel(const int *__restrict__ in, int *__restrict__ out, NwGeom g, unsigned long long *__restrict__ n_removed) {
    const i64 n = (i64)g.nz * g.ny * g.nx;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
        int v = in[i];
        if (v > 0) {
            const int x = (int)(i % g.nx), y = (int)((i / g.nx) % g.ny), z = (int)(i / ((i64)g.nx * g.ny));
            const bool three = g.ndim == 3;
            const bool inner = x > 0 && x < g.nx - 1 && y > 0 && y < g.ny - 1 && (!three || (z > 0 && z < g.nz - 1));
            if (inner) {
                int mn = v, mx = v;
                const int dz0 = three ? -1 : 0, dz1 = three ? 1 : 0;
                for (int dz = dz0; dz <= dz1; ++dz)
                    for (int dy = -1; dy <= 1; ++dy) {
                        const int *r = in + ((i64)(z + dz) * g.ny + (y + dy)) * g.nx + x;
                        for (int dx = -1; dx <= 1; ++dx) {
                            const int w = r[dx];
                            if (w > 0) { mn = w < mn ? w : mn; mx = w > mx ? w : mx; }
                        }
                    }
                if (mn != mx) { v = 0; atomicAdd(n_removed, 1ull); }
            }
        }
        out[i] = v;
    }
}

// ---- seed (:342-387) ------------------------------------------------------------------------------------------------------------------
// has[L] = 1 where label L has a voxel in the cleaned skeleton (every writer stores the same value)
__global__ void __launch_bounds__(256)
nw_has_kernel(const int *__restrict__ skel, i64 n, int *__restrict__ has) {
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
        const int s = skel[i];
        if (s > 0) has[s] = 1;
    }
}

// best[L] = max over the voxels of a label without skeleton of (rank of the Frangi value, lowest index first): NaN ranks above every
// number, -0.0 equals 0.0.  0 = no voxel: a key is never 0 (an index is below 2^31).
__global__ void __launch_bounds__(256)
nw_best_kernel(const int *__restrict__ lab, const float *__restrict__ fr, i64 n, const int *__restrict__ has,
               unsigned long long *__restrict__ best) {
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) {
        const int l = lab[i];
        if (l <= 0 || has[l]) continue;
        const float f = fr[i];
        unsigned int u;
        if (f != f) u = 0xffffffffu;
        else {
            u = __float_as_uint(f == 0.0f ? 0.0f : f);
            u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
        }
        atomicMax(best + l, ((unsigned long long)u << 32) | (unsigned long long)(0xffffffffu - (unsigned int)i));
    }
}

__global__ void __launch_bounds__(256)
nw_plant_kernel(const unsigned long long *__restrict__ best, int max_label, int *__restrict__ skel, unsigned long long *__restrict__ n_seeded) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x + 1;
    if (l > max_label) return;
    const unsigned long long b = best[l];
    if (!b) return;
    skel[0xffffffffu - (unsigned int)(b & 0xffffffffull)] = l;
    atomicAdd(n_seeded, 1ull);
}

// ---- relabel: boxes ----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
nw_box_init_kernel(int *__restrict__ box, int *__restrict__ seeded, int max_label) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l > max_label) return;
    int *b = box + (i64)l * 6;
    b[0] = b[1] = b[2] = NW_BOX_EMPTY;
    b[3] = b[4] = b[5] = -1;
    seeded[l] = 0;
}

// One wave per 64 voxels of a row: the lanes that hold one label share (z, y), their x range comes from the ballot, and one lane
// sends the six updates, and only those that move a bound.
__global__ void __launch_bounds__(256)
nw_box_kernel(const int *__restrict__ lab, const int *__restrict__ branch, NwGeom g, int wpr, int *__restrict__ box, int *__restrict__ seeded) {
    const i64 nw = (i64)g.nz * g.ny * wpr;
    const i64 wstride = ((i64)gridDim.x * blockDim.x) >> 6;
    const int lane = threadIdx.x & 63;
    for (i64 w = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6; w < nw; w += wstride) {
        const i64 row = w / wpr;
        const int x0 = (int)(w % wpr) * 64, x = x0 + lane;
        int l = 0;
        bool sd = false;
        if (x < g.nx) {
            l = lab[row * g.nx + x];
            sd = l > 0 && branch[row * g.nx + x] > 0;
        }
        unsigned long long todo = __ballot(l > 0);
        const int y = (int)(row % g.ny), z = (int)(row / g.ny);
        while (todo) {
            const int lead = __builtin_ctzll(todo);
            const int ll = __shfl(l, lead);
            const unsigned long long same = __ballot(l == ll);
            const unsigned long long sds = __ballot(l == ll && sd);
            if (lane == lead) {
                int *b = box + (i64)ll * 6;
                const int xa = x0 + __builtin_ctzll(same), xb = x0 + 63 - __builtin_clzll(same);
                // the box as L2 holds it (a plain load may be answered by this CU's L1 for ever): a box only grows, so a bound that
                // already covers this chunk needs no atomic, and after its first planes an object sends almost none
                int cur[6];
#pragma unroll
                for (int k = 0; k < 6; ++k) cur[k] = __hip_atomic_load(b + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (cur[0] > z) atomicMin(b + 0, z);
                if (cur[1] > y) atomicMin(b + 1, y);
                if (cur[2] > xa) atomicMin(b + 2, xa);
                if (cur[3] < z) atomicMax(b + 3, z);
                if (cur[4] < y) atomicMax(b + 4, y);
                if (cur[5] < xb) atomicMax(b + 5, xb);
                if (sds) seeded[ll] = 1;
            }
            todo &= ~same;
        }
    }
}

// ---- relabel: the batch ----------------------------------------------------------------------------------------------------------------
// the last object whose first slot (FIELD 3: first line of pass 0..2) is <= key
template <int FIELD> __device__ __forceinline__ int nw_find(const NwObj *__restrict__ objs, int nobj, i64 key) {
    int lo = 0, hi = nobj - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const i64 start = FIELD == 3 ? objs[mid].off : objs[mid].line0[FIELD];
        if (start <= key) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// feat[slot] = the voxel itself where it is a seed of the box's object, else none
__global__ void __launch_bounds__(256)
nwr_init_kernel(const NwObj *__restrict__ objs, int nobj, i64 total, const int *__restrict__ lab, const int *__restrict__ branch, NwGeom g,
                int *__restrict__ feat) {
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const NwObj o = objs[nw_find<3>(objs, nobj, t)];
    const i64 r = t - o.off;
    const int x = (int)(r % o.dx), y = (int)((r / o.dx) % o.dy), z = (int)(r / ((i64)o.dx * o.dy));
    const i64 gi = ((i64)(o.z0 + z) * g.ny + (o.y0 + y)) * g.nx + (o.x0 + x);
    feat[t] = (lab[gi] == o.label && branch[gi] > 0) ? (int)gi : -1;
}

struct NwPt { int c[3]; };
__device__ __forceinline__ NwPt nw_point(int f, const NwGeom &g) {
    NwPt p;
    const unsigned int u = (unsigned int)f, plane = (unsigned int)g.ny * (unsigned int)g.nx;
    p.c[0] = (int)(u / plane);
    const unsigned int r = u - (unsigned int)p.c[0] * plane;
    p.c[1] = (int)(r / (unsigned int)g.nx);
    p.c[2] = (int)(r - (unsigned int)p.c[1] * (unsigned int)g.nx);
    return p;
}

// sum over the axes other than D, in axis order, of ((p - c) * s)^2
template <int D> __device__ __forceinline__ double nw_off_axis(const NwPt &p, const int *c, const NwGeom &g) {
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        if (j == D) continue;
        const double t = (double)(p.c[j] - c[j]) * g.s[j];
        acc += t * t;
    }
    return acc;
}

// squared distance, over all axes in order, from the line position `pos` (coordinate along D) to p
template <int D> __device__ __forceinline__ double nw_dist(const NwPt &p, const int *c, int pos, const NwGeom &g) {
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double t = (double)(p.c[j] - (j == D ? pos : c[j])) * g.s[j];
        acc += t * t;
    }
    return acc;
}

// One pass of the transform along axis D (0 = Z, 1 = Y, 2 = X): one thread per line.  Lines are numbered with X fastest (D = 2: Y
// fastest), so in the passes along Z and Y adjacent lanes walk adjacent X; along X adjacent lanes are one box row apart.  The line's
// stack holds features, not positions: the query pass overwrites the line it reads.
// A 2-D frame runs D = 1, 2 with nz = 1: the Z terms are +0.0 and change no sum.
template <int D> __global__ void __launch_bounds__(256)
nwr_pass_kernel(const NwObj *__restrict__ objs, int nobj, i64 nlines, NwGeom g, int *__restrict__ feat, int *__restrict__ stk) {
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nlines) return;
    const NwObj o = objs[nw_find<D>(objs, nobj, t)];
    const i64 r = t - o.line0[D];
    int c[3] = {o.z0, o.y0, o.x0};       // the line's frame coordinates; c[D] = its first voxel
    i64 base, stride;
    int len;
    if (D == 0) {
        const int x = (int)(r % o.dx), y = (int)(r / o.dx);
        c[1] += y; c[2] += x;
        base = (i64)y * o.dx + x; stride = (i64)o.dy * o.dx; len = o.dz;
    } else if (D == 1) {
        const int x = (int)(r % o.dx), z = (int)(r / o.dx);
        c[0] += z; c[2] += x;
        base = (i64)z * o.dy * o.dx + x; stride = o.dx; len = o.dy;
    } else {
        const int y = (int)(r % o.dy), z = (int)(r / o.dy);
        c[0] += z; c[1] += y;
        base = ((i64)z * o.dy + y) * o.dx; stride = 1; len = o.dx;
    }
    int *F = feat + o.off + base, *S = stk + o.off + base;
    const double sd = g.s[D];
    // build: the features of the line whose Voronoi cells meet it, in order
    int top = -1;
    for (int i = 0; i < len; ++i) {
        const int fi = F[(i64)i * stride];
        if (fi < 0) continue;
        const NwPt pw = nw_point(fi, g);
        const double fd = (double)pw.c[D];
        const double wR = nw_off_axis<D>(pw, c, g);
        while (top >= 1) {
            const NwPt pv = nw_point(S[(i64)top * stride], g), pu = nw_point(S[(i64)(top - 1) * stride], g);
            const double f1 = (double)pv.c[D];
            double a = f1 - (double)pu.c[D], b = fd - f1;
            a *= sd;
            b *= sd;
            const double cc = a + b;
            const double uR = nw_off_axis<D>(pu, c, g), vR = nw_off_axis<D>(pv, c, g);
            if (cc * vR - b * uR - a * wR - a * b * cc <= 0.0) break;
            --top;
        }
        ++top;
        S[(i64)top * stride] = fi;
    }
    if (top < 0) return;
    // query: every voxel of the line takes the nearest of them, the earlier one on a tie
    int l = 0;
    int cur = S[0];
    NwPt pc = nw_point(cur, g);
    int nxt = top > 0 ? S[stride] : -1;
    NwPt pn = nw_point(nxt < 0 ? 0 : nxt, g);
    for (int i = 0; i < len; ++i) {
        double d1 = nw_dist<D>(pc, c, c[D] + i, g);
        while (l < top) {
            const double d2 = nw_dist<D>(pn, c, c[D] + i, g);
            if (d1 <= d2) break;
            d1 = d2;
            ++l;
            cur = nxt; pc = pn;
            nxt = l < top ? S[(i64)(l + 1) * stride] : -1;
            pn = nw_point(nxt < 0 ? 0 : nxt, g);
        }
        F[(i64)i * stride] = cur;
    }
}

// out = branch[feature] at the object's own voxels
__global__ void __launch_bounds__(256)
nwr_gather_kernel(const NwObj *__restrict__ objs, int nobj, i64 total, const int *__restrict__ lab, const int *__restrict__ branch, NwGeom g,
                  const int *__restrict__ feat, unsigned int *__restrict__ out) {
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total) return;
    const NwObj o = objs[nw_find<3>(objs, nobj, t)];
    const i64 r = t - o.off;
    const int x = (int)(r % o.dx), y = (int)((r / o.dx) % o.dy), z = (int)(r / ((i64)o.dx * o.dy));
    const i64 gi = ((i64)(o.z0 + z) * g.ny + (o.y0 + y)) * g.nx + (o.x0 + x);
    if (lab[gi] != o.label) return;
    const int f = feat[t];
    out[gi] = f >= 0 ? (unsigned int)branch[f] : 0u;
}
