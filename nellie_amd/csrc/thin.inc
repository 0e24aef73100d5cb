// The 3-D thinning of Lee, Kashyap & Chu (1994) as skimage.morphology.skeletonize runs it on a volume (networking.py:394-409), in the
// round-parallel form that tests/thinning_restatement.py states and holds against skimage voxel for voxel.
//
// Axes are (z, y, x); outside the frame is background.  A voxel's 3x3x3 neighbourhood is a 27-bit word, bit (dz+1)*9 + (dy+1)*3 + (dx+1),
// bit 13 the voxel itself.  A sub-iteration of direction d:
//   (1) candidates: set voxels whose neighbour at d is background, that are no endpoint, Euler-invariant and simple -- all judged on
//       the image as the sub-iteration finds it (thin_candidates_kernel: one independent decision per voxel);
//   (2) re-check, sequential in raster order in skimage: a candidate is deleted when it is simple on the image as the earlier
//       deletions of the list left it.  The verdict reads the 26 neighbours only, so a candidate is READY when none of the 13
//       neighbours that precede it in raster order is an undecided candidate; two ready candidates are never neighbours and nothing a
//       ready candidate reads is written in the same round, so all ready candidates decide at once (thin_round_kernel, one launch per
//       round).  Readiness is judged on the voxel's linear index, so the order of the work lists does not matter.
// State volume `st` (int32 per voxel, zeroed once per frame): -1 = undecided candidate, r > 0 = decided in the launch of serial r.  The
// serial grows by one with every launch of the two kernels, so "decided in this very launch" (== serial) still reads as undecided
// whatever the timing, and marks of earlier sub-iterations read as decided without any clearing.
// Work lists hold distinct voxel indices (int32: frames below 2^31 voxels) and live in volumes of one int per voxel: none can overflow.
// Counters: the list read by the launch of serial s has its length in cnt[s % 3]; that launch fills cnt[(s + 1) % 3] and zeroes
// cnt[(s + 2) % 3], which the launch of serial s - 1 read.  Launches of one stream run one after another.
#pragma once

#ifndef __HIPCC__                          // the decision functions and the planning also compile as plain C++ (host-side checks)
#define __host__
#define __device__
#define __forceinline__ inline
#endif

#define THIN_CENTRE 13
#define THIN_NEIGHBOURS 0x7ffdfffu        // all 27 bits but the centre

struct ThinTables {
    unsigned int adj[27];                 // 26-adjacency inside the block, centre left out
    unsigned char oct[8][7];              // the seven neighbours (bit numbers) of each octant: index a*4 + b*2 + c - 1 <-> offset (a sz, b sy, c sx)
    signed char euler[128];               // 8 x the octant's share of the change of the Euler characteristic when the centre cube is added
};

// Generated from the definitions (tests/thinning_restatement.py states the same and test_thinning_cpu.py compares them word by word).
// Euler characteristic: vertices - edges + faces - cubes of the union of the set voxels as closed unit cubes.  Adding the centre cube
// adds the cube (-1) and every cell of its boundary that no set neighbour already has; a boundary cell at offset o belongs to the
// neighbours at o with some components zeroed.  Of an octant (sz, sy, sx) the vertex at its corner is wholly its own (weight 8), each
// of its three edges is shared with one other octant (4), each face with three (2), the cube with all eight (1): the eight table values
// sum to 8 x the change.
constexpr ThinTables thin_make_tables() {
    ThinTables t{};
    for (int k = 0; k < 27; ++k) {
        unsigned int m = 0;
        for (int j = 0; j < 27; ++j) {
            if (j == k || j == THIN_CENTRE || k == THIN_CENTRE) continue;
            const int dz = k / 9 - j / 9, dy = (k / 3) % 3 - (j / 3) % 3, dx = k % 3 - j % 3;
            if (dz >= -1 && dz <= 1 && dy >= -1 && dy <= 1 && dx >= -1 && dx <= 1) m |= 1u << j;
        }
        t.adj[k] = m;
    }
    for (int o = 0; o < 8; ++o) {
        const int sz = (o & 4) ? 1 : -1, sy = (o & 2) ? 1 : -1, sx = (o & 1) ? 1 : -1;
        for (int i = 1; i < 8; ++i) {
            const int dz = (i & 4) ? sz : 0, dy = (i & 2) ? sy : 0, dx = (i & 1) ? sx : 0;
            t.oct[o][i - 1] = (unsigned char)((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1));
        }
    }
    for (int cfg = 0; cfg < 128; ++cfg) {
        // bit i - 1 of cfg: the neighbour whose offset has the components i selects (4: z, 2: y, 1: x)
        int v = -1;
        for (int cell = 1; cell < 8; ++cell) {             // the cell at the offset `cell` selects
            bool taken = false;
            for (int i = 1; i < 8; ++i)
                if ((i & cell) == i && (cfg >> (i - 1) & 1)) taken = true;
            if (taken) continue;
            const int dims = ((cell >> 2) & 1) + ((cell >> 1) & 1) + (cell & 1);
            v += dims == 3 ? 8 : dims == 2 ? -4 : 2;       // vertex +, edge -, face +
        }
        t.euler[cfg] = (signed char)v;
    }
    return t;
}

static constexpr ThinTables THIN_HOST_TABLES = thin_make_tables();
#ifdef __HIPCC__
__constant__ ThinTables thin_dev_tables = thin_make_tables();
#endif

__host__ __device__ __forceinline__ const ThinTables &thin_tables() {
#ifdef __HIP_DEVICE_COMPILE__
    return thin_dev_tables;
#else
    return THIN_HOST_TABLES;
#endif
}

__host__ __device__ __forceinline__ int thin_popcount(unsigned int w) {
#ifdef __HIP_DEVICE_COMPILE__
    return __popc(w);
#else
    return __builtin_popcount(w);
#endif
}
__host__ __device__ __forceinline__ int thin_lowest(unsigned int w) {
#ifdef __HIP_DEVICE_COMPILE__
    return __ffs((int)w) - 1;
#else
    return __builtin_ctz(w);
#endif
}

// the centre and exactly one neighbour
__host__ __device__ __forceinline__ bool thin_is_endpoint(unsigned int word) { return thin_popcount(word) == 2; }

__host__ __device__ __forceinline__ bool thin_euler_invariant(unsigned int word) {
    const ThinTables &t = thin_tables();
    int sum = 0;
#pragma unroll
    for (int o = 0; o < 8; ++o) {
        unsigned int cfg = 0;
#pragma unroll
        for (int i = 0; i < 7; ++i) cfg |= ((word >> t.oct[o][i]) & 1u) << i;
        sum += t.euler[cfg];
    }
    return sum == 0;
}

// The set neighbours form at most one 26-connected component inside the block (none: simple).  Flood from the lowest set bit.
__host__ __device__ __forceinline__ bool thin_is_simple(unsigned int word) {
    const ThinTables &t = thin_tables();
    const unsigned int mask = word & THIN_NEIGHBOURS;
    if (!mask) return true;
    unsigned int reached = mask & (0u - mask), frontier = reached;
    while (frontier) {
        const int b = thin_lowest(frontier);
        frontier &= frontier - 1u;
        const unsigned int fresh = t.adj[b] & mask & ~reached;
        reached |= fresh;
        frontier |= fresh;
    }
    return reached == mask;
}

// bit 0 endpoint, bit 1 Euler-invariant, bit 2 simple
__host__ __device__ __forceinline__ unsigned char thin_decide(unsigned int word) {
    return (unsigned char)((thin_is_endpoint(word) ? 1 : 0) | (thin_euler_invariant(word) ? 2 : 0) | (thin_is_simple(word) ? 4 : 0));
}

// ---- host: batch planning ----------------------------------------------------------------------------------------------------------
#define THIN_ROUNDS_PER_SYNC 8            // rounds launched blind between two read-backs of the counters (<= 0 selects this)
#define THIN_MAX_GRID 1024                // workgroups of a launch over a list: the kernels stride

static inline int thin_batch(int rounds_per_sync) { return rounds_per_sync > 0 ? (rounds_per_sync > 4096 ? 4096 : rounds_per_sync) : THIN_ROUNDS_PER_SYNC; }
// workgroups for a list of at most `bound` entries (the true length is on the device)
static inline unsigned int thin_grid(long long bound) {
    long long g = (bound + 255) / 256;
    if (g > THIN_MAX_GRID) g = THIN_MAX_GRID;
    if (g < 1) g = 1;
    return (unsigned int)g;
}
// skimage treats a frame of one plane as an image: the four in-plane directions only
static inline int thin_ndirs(long long nz) { return nz == 1 ? 4 : 6; }

#ifdef __HIPCC__
// ---- device ------------------------------------------------------------------------------------------------------------------------
struct ThinGeom { int nz, ny, nx; };

// Counters of one thinning, in the context's small scratch.
struct ThinCnt {
    unsigned int cnt[3];                  // lengths of the undecided lists (see the head of this file)
    unsigned int n_fg;                    // foreground voxels = length of the voxel list
    unsigned int sub_removed[6];          // voxels deleted per direction of the current outer iteration
    unsigned int pad[2];
    unsigned long long rounds, candidates, removed;
};

// (dz, dy, dx) of direction k: y-1, y+1, x+1, x-1, z+1, z-1
__device__ __forceinline__ void thin_dir(int k, int &dz, int &dy, int &dx) {
    dz = k == 4 ? 1 : k == 5 ? -1 : 0;
    dy = k == 0 ? -1 : k == 1 ? 1 : 0;
    dx = k == 2 ? 1 : k == 3 ? -1 : 0;
}

__device__ __forceinline__ unsigned int thin_word(const uint8_t *__restrict__ img, const ThinGeom &g, int z, int y, int x) {
    unsigned int w = 0;
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz) {
        const int zz = z + dz;
        if (zz < 0 || zz >= g.nz) continue;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            const int yy = y + dy;
            if (yy < 0 || yy >= g.ny) continue;
            const uint8_t *r = img + ((i64)zz * g.ny + yy) * g.nx;
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int xx = x + dx;
                if (xx < 0 || xx >= g.nx) continue;
                if (r[xx]) w |= 1u << ((dz + 1) * 9 + (dy + 1) * 3 + (dx + 1));
            }
        }
    }
    return w;
}

// img = lab > 0 (one byte per voxel)
static __global__ void __launch_bounds__(256) thin_from_labels_kernel(const int *__restrict__ lab, uint8_t *__restrict__ img, i64 n) {
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) img[i] = lab[i] > 0;
}
// img = img != 0 in place (the stand-alone call takes any non-zero byte as foreground)
static __global__ void __launch_bounds__(256) thin_normalise_kernel(uint8_t *__restrict__ img, i64 n) {
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (i64)gridDim.x * blockDim.x) img[i] = img[i] != 0;
}

// The workgroup's threads with `take` append `value` to list[0 .. *count): one atomic per workgroup.  Every thread of the workgroup
// calls it.  The list has room for every voxel of the frame and a voxel is appended once, so the slot is always inside it.
__device__ __forceinline__ void thin_append(bool take, int value, int *__restrict__ list, unsigned int *__restrict__ count) {
    __shared__ unsigned int s_wave[4], s_base;
    const unsigned long long b = __ballot(take);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) s_wave[wave] = (unsigned int)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned int total = s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        s_base = total ? atomicAdd(count, total) : 0u;
    }
    __syncthreads();
    if (take) {
        unsigned int off = s_base;
        for (int w = 0; w < wave; ++w) off += s_wave[w];
        list[off + (unsigned int)__popcll(b & ((1ull << lane) - 1ull))] = value;
    }
    __syncthreads();                      // s_wave and s_base are written again by the caller's next trip
}

// The foreground voxels of the frame into vox[0 .. n_fg).
static __global__ void __launch_bounds__(256) thin_compact_kernel(const uint8_t *__restrict__ img, i64 n, int *__restrict__ vox, ThinCnt *__restrict__ tc) {
    const i64 stride = (i64)gridDim.x * blockDim.x;
    const i64 trips = (n + stride - 1) / stride;                    // the same for every thread: thin_append synchronises the workgroup
    for (i64 t = 0; t < trips; ++t) {
        const i64 i = t * stride + (i64)blockIdx.x * blockDim.x + threadIdx.x;
        thin_append(i < n && img[i], (int)i, vox, &tc->n_fg);
    }
}

// Step (1) of the sub-iteration of direction `dir`, launch serial `serial`: over the voxel list, the candidates into `out` and marked
// undecided in st.
static __global__ void __launch_bounds__(256)
thin_candidates_kernel(const uint8_t *__restrict__ img, ThinGeom g, const int *__restrict__ vox, int dir, unsigned int serial, int *__restrict__ st,
                       int *__restrict__ out, ThinCnt *__restrict__ tc) {
    if (blockIdx.x == 0 && threadIdx.x == 0) tc->cnt[(serial + 2u) % 3u] = 0u;
    const unsigned int n = tc->n_fg;
    unsigned int *cnt = &tc->cnt[(serial + 1u) % 3u];
    int ddz, ddy, ddx;
    thin_dir(dir, ddz, ddy, ddx);
    const unsigned int stride = gridDim.x * blockDim.x;
    const unsigned int trips = (n + stride - 1u) / stride;
    unsigned int mine = 0;
    for (unsigned int t = 0; t < trips; ++t) {
        const unsigned int k = t * stride + blockIdx.x * blockDim.x + threadIdx.x;
        bool cand = false;
        int v = 0;
        if (k < n) {
            v = vox[k];
            if (img[v]) {
                const int x = v % g.nx, y = (v / g.nx) % g.ny, z = v / (g.nx * g.ny);
                const int zz = z + ddz, yy = y + ddy, xx = x + ddx;
                const bool inside = zz >= 0 && zz < g.nz && yy >= 0 && yy < g.ny && xx >= 0 && xx < g.nx;
                if (!inside || !img[((i64)zz * g.ny + yy) * g.nx + xx]) {
                    const unsigned int w = thin_word(img, g, z, y, x);
                    cand = !thin_is_endpoint(w) && thin_euler_invariant(w) && thin_is_simple(w);
                }
            }
        }
        if (cand) { st[v] = -1; ++mine; }
        thin_append(cand, v, out, cnt);
    }
    if (mine) atomicAdd(&tc->candidates, (unsigned long long)mine);
}

// One round of step (2), launch serial `serial`: over the undecided list `in`, the ready candidates decide and the others go to `out`.
static __global__ void __launch_bounds__(256)
thin_round_kernel(uint8_t *__restrict__ img, ThinGeom g, const int *__restrict__ in, int dir, unsigned int serial, int *__restrict__ st,
                  int *__restrict__ out, ThinCnt *__restrict__ tc) {
    if (blockIdx.x == 0 && threadIdx.x == 0) tc->cnt[(serial + 2u) % 3u] = 0u;
    const unsigned int n = tc->cnt[serial % 3u];
    if (n == 0u) return;                                            // launched blind behind the sub-iteration's last round
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&tc->rounds, 1ull);
    unsigned int *cnt = &tc->cnt[(serial + 1u) % 3u];
    const unsigned int stride = gridDim.x * blockDim.x;
    const unsigned int trips = (n + stride - 1u) / stride;
    unsigned int gone = 0;
    for (unsigned int t = 0; t < trips; ++t) {
        const unsigned int k = t * stride + blockIdx.x * blockDim.x + threadIdx.x;
        bool wait = false;
        int v = 0;
        if (k < n) {
            v = in[k];
            const int x = v % g.nx, y = (v / g.nx) % g.ny, z = v / (g.nx * g.ny);
            // the 13 neighbours before v in raster order: the plane below, the row before in this plane, the voxel before in this row
#pragma unroll
            for (int j = 0; j < 13; ++j) {
                const int dz = j / 9 - 1, dy = (j / 3) % 3 - 1, dx = j % 3 - 1;
                const int zz = z + dz, yy = y + dy, xx = x + dx;
                if (zz < 0 || zz >= g.nz || yy < 0 || yy >= g.ny || xx < 0 || xx >= g.nx) continue;
                const int s = st[((i64)zz * g.ny + yy) * g.nx + xx];
                if (s < 0 || s == (int)serial) wait = true;
            }
            if (!wait) {
                if (thin_is_simple(thin_word(img, g, z, y, x))) { img[v] = 0; ++gone; }
                st[v] = (int)serial;
            }
        }
        thin_append(wait, v, out, cnt);
    }
    if (gone) {
        atomicAdd(&tc->sub_removed[dir], gone);
        atomicAdd(&tc->removed, (unsigned long long)gone);
    }
}
#endif
