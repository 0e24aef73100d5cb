// Label on X-RUNS instead of voxels (labelling.py:467-509), included by nellie_hip.hip.
//
// The thresholded Frangi image is ~98 % background.  The masks are bit-packed (one 64-bit word per
// 64 x-voxels of a row, 1 bit/voxel = N/8 bytes, resident in L2 / Infinity Cache), every row is
// decomposed into maximal runs of set bits, and hole filling plus both 26-connected labellings run as a
// lock-free union-find over RUNS (~10^6..10^7 nodes instead of 10^9 voxels).  Runs are numbered in
// raster order (row major, then x), and the union-find always keeps the smaller index as the root, so a
// component's root is the run holding its first voxel in raster order: ranking the roots reproduces
// scipy.ndimage.label's numbering exactly.
//
//   rl_threshold_pack    mask = frangi > thr                           labelling.py:478
//   rl_count / rl_emit   run extraction (foreground, or background for the hole fill)
//   rl_union<CONN>       unions with the overlapping runs of the raster-preceding rows
//   rl_border / rl_fill  binary_fill_holes: background components that reach no face -> set  :486
//   rl_area / rl_keep    bincount + keep >= min_area                    :495-501
//   majority_bits        uniform_filter(3) > 0.5 as a bit-sliced 27-input popcount           :503-505
//   rl_paint             int32 label volume                             :507

struct RunRec { int row; unsigned int x; };   // x = xs | (xe << 16), run = [xs, xe)
// The number of runs as a kernel sees it (round 4): from the host (h >= 0: the launcher waited for it) or read where the scan left
// it (p: row_off[nrows]) -- then no launch of a labelling waits for the host, kernels walk the runs grid-stride, and a run set
// beyond the scratch capacity `cap` turns every kernel into a no-op (rl_emit_kernel raises the flag the host reads at the end).
struct RunN { const unsigned int *p; i64 h; i64 cap; };
__device__ __forceinline__ i64 run_n(const RunN &r) { const i64 n = r.p ? (i64)*r.p : r.h; return n > r.cap ? 0 : n; }

__device__ __forceinline__ unsigned long long rl_word(const unsigned long long *__restrict__ bits, i64 row, int w, int wpr,
                                                      int nx, bool invert) {
    unsigned long long v = bits[row * wpr + w];
    if (invert) v = ~v;
    const int rem = nx - w * 64;
    if (rem < 64) v &= (rem <= 0) ? 0ull : ((1ull << rem) - 1ull);
    return v;
}

// mask = has_thr && frangi > thr, packed.  One wave per row, four 64-voxel words (four independent coalesced
// loads per lane) per iteration.  `support` (may be NULL): a bit mask outside which the frame is known to be <= 0
// (thr >= 0 then fails there) -- only words with support bits are read from the float volume.
__global__ void __launch_bounds__(256)
rl_threshold_pack_kernel(const float *__restrict__ f, const unsigned long long *__restrict__ support, unsigned long long *__restrict__ bits,
                         int has_thr, float thr_host, int nx, i64 nrows, int wpr, const float *__restrict__ thr_dev = nullptr) {
    const float thr = thr_dev ? *thr_dev : thr_host;        // decided by a kernel (nl_mask_volume_dev) or by the host
    const i64 wstride = ((i64)gridDim.x * blockDim.x) >> 6;
    const int lane = threadIdx.x & 63;
    // the row's support words in one coalesced load (lane l holds word l); a row without support is all zeros; the next row's
    // words are requested before this row is worked on
    const bool row_words = support && wpr <= 64;
    const i64 first = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    unsigned long long mine_next = (row_words && first < nrows && lane < wpr) ? support[first * wpr + lane] : 0ull;
    unsigned long long st_res = 0ull;          // this row's result words leave at the top of the next trip, before its loads
    i64 st_row = -1;                           // (see pack_masked_kernel)
    for (i64 row = first; row < nrows; row += wstride) {
        const float *fr = f + row * nx;
        unsigned long long *br = bits + row * wpr;
        if (row_words) {
            if (st_row >= 0 && lane < wpr) bits[st_row * wpr + lane] = st_res;
            // only the words with support are visited, eight (eight independent loads per lane) per trip; the row's result words
            // leave in one store (lane l holds word l) -- see pack_masked_kernel
            const unsigned long long mine = mine_next;
            mine_next = (row + wstride < nrows && lane < wpr) ? support[(row + wstride) * wpr + lane] : 0ull;
            unsigned long long nz = __ballot(mine != 0ull), res = 0ull;
            while (nz) {                                            // uniform
                int wi[8];
                float v[8];
                bool on[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    wi[k] = nz ? (int)__builtin_ctzll(nz) : -1;
                    nz &= nz - 1ull;
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const unsigned long long a = wi[k] >= 0 ? wave_read_u64(mine, wi[k]) : 0ull;
                    const int x = wi[k] * 64 + lane;
                    on[k] = ((a >> lane) & 1ull) && x < nx;
                    v[k] = on[k] ? fr[x] : -1.0f;
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    if (wi[k] < 0) break;                           // uniform
                    const unsigned long long b = __ballot(has_thr && on[k] && v[k] > thr);
                    if (lane == wi[k]) res = b;
                }
            }
            st_res = res; st_row = row;
            continue;
        }
        for (int w0 = 0; w0 < wpr; w0 += 4) {
            unsigned long long sm[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                sm[k] = (support && w0 + k < wpr) ? support[row * wpr + w0 + k] : ~0ull;      // (no support mask, or rows of > 64 words)
            }
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int x = (w0 + k) * 64 + lane;
                v[k] = (x < nx && ((sm[k] >> lane) & 1ull)) ? fr[x] : -1.0f;
            }
            unsigned long long b[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int x = (w0 + k) * 64 + lane;
                b[k] = __ballot(has_thr && x < nx && ((sm[k] >> lane) & 1ull) && v[k] > thr);
            }
            if (lane < 4 && w0 + lane < wpr) br[w0 + lane] = lane == 0 ? b[0] : (lane == 1 ? b[1] : (lane == 2 ? b[2] : b[3]));
        }
    }
    if (st_row >= 0 && lane < wpr) bits[st_row * wpr + lane] = st_res;
}

// number of runs per row
__global__ void __launch_bounds__(256)
rl_count_kernel(const unsigned long long *__restrict__ bits, int invert, unsigned int *__restrict__ counts, i64 nrows, int wpr, int nx) {
    const i64 row = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= nrows) return;
    unsigned long long carry = 0;
    unsigned int cnt = 0;
    for (int w = 0; w < wpr; ++w) {
        const unsigned long long v = rl_word(bits, row, w, wpr, nx, invert != 0);
        cnt += (unsigned int)__builtin_popcountll(v & ~((v << 1) | carry));
        carry = v >> 63;
    }
    counts[row] = cnt;
}

// ---- counting with one WAVE per row (rows of up to 64 words = 4096 voxels): lane l holds word l, so a row is one
// coalesced load instead of `wpr` dependent ones per thread.  (The same layout brought nothing for rl_emit_kernel.)
__device__ __forceinline__ unsigned long long rl_row_word(const unsigned long long *__restrict__ bits, i64 row, int lane, int wpr,
                                                          int nx, bool invert) {
    return lane < wpr ? rl_word(bits, row, lane, wpr, nx, invert) : 0ull;
}
__device__ __forceinline__ unsigned long long rl_run_starts(unsigned long long v, int lane) {
    unsigned long long prev = __shfl_up(v, 1, 64);
    if (lane == 0) prev = 0ull;
    return v & ~((v << 1) | (prev >> 63));                      // set bits whose left neighbour (also across words) is clear
}

// P = smallest power of two >= wpr: a wave covers 64 / P rows at once (lane = row-in-group * P + word), and walks several
// such groups (the launcher caps the grid: with one 16-lane-wide wave per 1024-voxel row the pass ran at 0.9 TB/s).
__global__ void __launch_bounds__(256)
rl_count_wave_kernel(const unsigned long long *__restrict__ bits, int invert, unsigned int *__restrict__ counts, i64 nrows, int wpr, int nx,
                     int P) {
    const int lane = threadIdx.x & 63;
    const int rpw = 64 / P;
    const int sub = lane / P, word = lane - sub * P;
    const i64 ngroups = (nrows + rpw - 1) / rpw;
    const i64 wstride = ((i64)gridDim.x * blockDim.x) >> 6;
    for (i64 grp = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6; grp < ngroups; grp += wstride) {
        const i64 row = grp * rpw + sub;
        const bool ok = row < nrows && word < wpr;
        const unsigned long long v = ok ? rl_word(bits, row, word, wpr, nx, invert != 0) : 0ull;
        unsigned long long prev = __shfl_up(v, 1, 64);
        if (word == 0) prev = 0ull;
        unsigned int c = (unsigned int)__builtin_popcountll(v & ~((v << 1) | (prev >> 63)));
        for (int o = P >> 1; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if (word == 0 && row < nrows) counts[row] = c;
    }
}

// generic exclusive scan of u32 counts: chunk sums -> blk_scan_kernel -> per-chunk scan
__global__ void __launch_bounds__(256)
chunk_sum_kernel(const unsigned int *__restrict__ in, i64 n, unsigned int *__restrict__ blk) {
    const i64 base = (i64)blockIdx.x * SCAN_CHUNK;
    unsigned long long s = 0;
    for (int k = threadIdx.x; k < SCAN_CHUNK; k += 256) { const i64 i = base + k; if (i < n) s += in[i]; }
    __shared__ unsigned int sh[4];
    s = wave_sum_u64(s);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = (unsigned int)s;
    __syncthreads();
    if (threadIdx.x == 0) blk[blockIdx.x] = sh[0] + sh[1] + sh[2] + sh[3];
}
__global__ void __launch_bounds__(256)
chunk_scan_kernel(const unsigned int *__restrict__ in, unsigned int *__restrict__ out, i64 n, const unsigned int *__restrict__ blk) {
    const i64 base = (i64)blockIdx.x * SCAN_CHUNK;
    __shared__ unsigned int s_w[4];
    __shared__ unsigned int s_run;
    if (threadIdx.x == 0) s_run = blk[blockIdx.x];
    __syncthreads();
    for (int k0 = 0; k0 < SCAN_CHUNK; k0 += 256) {
        const i64 i = base + k0 + threadIdx.x;
        const unsigned int val = (i < n) ? in[i] : 0u;
        unsigned int inc = val;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const unsigned int t = __shfl_up(inc, o, 64); if ((threadIdx.x & 63) >= o) inc += t; }
        const int w = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 63) s_w[w] = inc;
        __syncthreads();
        unsigned int woff = 0;
        for (int q = 0; q < w; ++q) woff += s_w[q];
        const unsigned int run = s_run;
        if (i < n) out[i] = run + woff + inc - val;
        __syncthreads();
        if (threadIdx.x == 0) s_run = run + s_w[0] + s_w[1] + s_w[2] + s_w[3];
        __syncthreads();
    }
}

// write the runs of every row (raster order) and initialise the union-find.  STAGED: the 256 rows of a workgroup are one
// contiguous stretch of mask words; they are read coalesced into LDS (row pitch wpr + 1 words against bank conflicts)
// and every thread then walks its own row there -- walking it in global memory makes each lane touch its own cache
// line on every step (0.22 ms for a 134 MB mask).
template <bool STAGED>
__global__ void __launch_bounds__(256)
rl_emit_kernel(const unsigned long long *__restrict__ bits, int invert, const unsigned int *__restrict__ row_off,
               RunRec *__restrict__ runs, int *__restrict__ parent, i64 nrows, int wpr, int nx, int *__restrict__ link, i64 cap,
               unsigned int *__restrict__ overflow) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned long long *sw = (unsigned long long *)smem;
    const i64 row = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (STAGED) {
        const i64 w0 = (i64)blockIdx.x * blockDim.x * wpr;
        const i64 wend = nrows * (i64)wpr;
        for (int k = threadIdx.x; k < 256 * wpr; k += 256) {
            const i64 gw = w0 + k;
            const int rr = k / wpr, ww = k - rr * wpr;
            sw[rr * (wpr + 1) + ww] = gw < wend ? bits[gw] : 0ull;
        }
        __syncthreads();
    }
    if (row >= nrows) return;
    if ((i64)row_off[nrows] > cap) {                         // more runs than the scratch volumes hold: nothing is written
        if (row == 0) *overflow = 1u;
        return;
    }
    auto word = [&](int w) -> unsigned long long {
        if (!STAGED) return rl_word(bits, row, w, wpr, nx, invert != 0);
        unsigned long long t = sw[threadIdx.x * (wpr + 1) + w];
        if (invert) t = ~t;
        const int rem = nx - w * 64;
        if (rem < 64) t &= (rem <= 0) ? 0ull : ((1ull << rem) - 1ull);
        return t;
    };
    unsigned int o = row_off[row];
    bool in_run = false;
    int xs_open = 0;
    auto emit = [&](int xs, int xe) {
        runs[o].row = (int)row;
        runs[o].x = (unsigned int)xs | ((unsigned int)xe << 16);
        parent[o] = (int)o;
        if (link) link[o] = -1;                              // (the pair filter's slots: was a fill of its own sized by the host)
        ++o;
    };
    for (int w = 0; w < wpr; ++w) {
        unsigned long long t = word(w);
        if (in_run) {
            const unsigned long long inv = ~t;
            if (inv == 0ull) continue;                        // the open run swallows the whole word
            const int e = __builtin_ctzll(inv);
            emit(xs_open, w * 64 + e);
            in_run = false;
            t &= ~((1ull << e) - 1ull);                       // e < 64 here
        }
        while (t) {
            const int s = __builtin_ctzll(t);
            const unsigned long long rest = ~(t >> s);
            const int len = rest ? __builtin_ctzll(rest) : 64;    // ones from bit s (bits above 63-s read as 0)
            if (s + len >= 64) { in_run = true; xs_open = w * 64 + s; break; }
            emit(w * 64 + s, w * 64 + s + len);
            t &= ~(((1ull << len) - 1ull) << s);
        }
    }
    if (in_run) emit(xs_open, nx);
}

// unions of run i with the overlapping runs of the raster-preceding neighbour rows
//   CONN 26: rows (z-1,y-1) (z-1,y) (z-1,y+1) (z,y-1), x ranges may touch diagonally (xs' <= xe && xe' >= xs)
//   CONN 6 : rows (z-1,y) (z,y-1), x ranges must overlap          (xs' <  xe && xe' >  xs)
// skip != 0 (hole filling, CONN 6): two runs that BOTH touch a face of the volume (planes zf_lo / zf_hi of the run set -- -1
// where a Z slab has no true face --, rows 0 / ny-1, columns 0 / skip_nx) are not
// joined -- each is "outside" on its own account (rl_border_kernel flags its root), and every path from an enclosed
// run to the outside ends at the first such run, so the answer of binary_fill_holes is unchanged while the one
// giant background component (and the contention on its root) never forms.
template <int CONN>
__global__ void __launch_bounds__(256)
rl_union_kernel(const RunRec *__restrict__ runs, const unsigned int *__restrict__ row_off, int *__restrict__ parent, RunN rn, int ny,
                int skip, int zf_lo, int zf_hi, int skip_nx) {
  const i64 nruns = run_n(rn);
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < nruns; i += (i64)gridDim.x * blockDim.x) {
    const RunRec r = runs[i];
    const int xs = (int)(r.x & 0xffffu), xe = (int)(r.x >> 16);
    const int z = r.row / ny, y = r.row % ny;
    auto on_face = [&](int zz, int yy, int a, int b) -> bool {
        return zz == zf_lo || zz == zf_hi || yy == 0 || yy == ny - 1 || a == 0 || b == skip_nx;
    };
    const bool mine = skip != 0 && on_face(z, y, xs, xe);
    auto row = [&](int zz, int yy) {
        if (zz < 0 || yy < 0 || yy >= ny) return;
        const i64 rr = (i64)zz * ny + yy;
        unsigned int lo = row_off[rr], hi = row_off[rr + 1];
        if (lo == hi) return;
        // first run whose end reaches us: xe' >= xs (26) / xe' > xs (6); ends increase along the row
        const int need = (CONN == 26) ? xs : xs + 1;
        unsigned int a = lo, b = hi;
        while (a < b) {
            const unsigned int m = (a + b) >> 1;
            if ((int)(runs[m].x >> 16) < need) a = m + 1; else b = m;
        }
        for (unsigned int j = a; j < hi; ++j) {
            const unsigned int xj = runs[j].x;
            const int xs2 = (int)(xj & 0xffffu);
            if ((CONN == 26) ? (xs2 > xe) : (xs2 >= xe)) break;
            if (mine && on_face(zz, yy, xs2, (int)(xj >> 16))) continue;
            uf_union(parent, (int)i, (int)j);
        }
    };
    if (CONN == 6) {
        row(z - 1, y);
        row(z, y - 1);
    } else {
        row(z - 1, y - 1);
        row(z - 1, y);
        row(z - 1, y + 1);
        row(z, y - 1);
    }
  }
}

// ---- two-level union-find --------------------------------------------------------------------------------------
// The neighbour search of rl_union_kernel is free (0.01 ms per pass without the unions); its cost is the unions: ~10^7
// of them, each two finds on chains that run across the planes.  Most are redundant: a component's cross-section in
// plane z meets the cross-section of the same component in plane z-1 through dozens of run pairs.  So:
//  (1) rl_union_plane_kernel: one workgroup per Z plane joins the plane's runs (neighbour row y-1) in an LDS parent
//      array and records every run's in-plane root (`proot`, also the initial `parent`);
//  (2) rl_union_cross_kernel: a run pair (i in plane z, j in plane z-1) stands for the pair of in-plane components
//      (A, B) = (proot[i], proot[j]); the first thread to claim A's link slot for B performs union(A, B), every later
//      pair with the same (A, B) is dropped after one atomic.  A second, different B for the same A is simply united
//      (rare).  Unions are idempotent and commutative, so the partition is the one the single-level pass builds, and
//      the smaller run index still ends up as the root (scipy's numbering).
// Segments with more runs than the LDS array keep proot[i] = i; the cross pass then also handles their row y-1.
#define RL_PLANE_CAP 15360
// A plane is cut into `nseg` SEGMENTS of 2^seg_shift rows, one workgroup each (round 4): with one workgroup per plane a
// 136-plane slab of 2048 x 2048 occupied half of the CUs with twice the runs per workgroup, and the in-LDS chains of a
// 2048-row object were twice as long (0.24 ms per pass against 0.14 at 1024^3).  A segment's components are what the cross
// pass pairs up; it then also joins row y-1 for the first row of every segment (and for segments beyond the LDS array).
template <int CONN>
__global__ void __launch_bounds__(256)
rl_union_plane_kernel(const RunRec *__restrict__ runs, const unsigned int *__restrict__ row_off, int *__restrict__ parent,
                      int *__restrict__ proot, int ny, int skip, int zf_lo, int zf_hi, int skip_nx, uint8_t *__restrict__ seg_done,
                      int seg_shift, int nseg, RunN rn) {
    __shared__ int sp[RL_PLANE_CAP];
    if (rn.p && (i64)*rn.p > rn.cap) return;                 // run set beyond the scratch volumes: no-op (uniform)
    const int z = blockIdx.x / nseg, sg = blockIdx.x - z * nseg;
    const int y0 = sg << seg_shift;
    const int y1 = (y0 + (1 << seg_shift)) < ny ? (y0 + (1 << seg_shift)) : ny;
    const unsigned int r0 = row_off[(i64)z * ny + y0], r1 = row_off[(i64)z * ny + y1];
    const unsigned int np = r1 - r0;
    if (np > RL_PLANE_CAP) {                                                          // uniform
        if (threadIdx.x == 0) seg_done[blockIdx.x] = 0;
        for (unsigned int k = threadIdx.x; k < np; k += blockDim.x) proot[r0 + k] = (int)(r0 + k);
        return;
    }
    if (threadIdx.x == 0) seg_done[blockIdx.x] = 1;
    if (np == 0) return;
    for (unsigned int k = threadIdx.x; k < np; k += blockDim.x) sp[k] = (int)k;
    __syncthreads();
    auto ld = [&](int i) -> int { return __hip_atomic_load(&sp[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
    auto find_halve = [&](int i) -> int {
        int p = ld(i);
        while (p != i) {
            const int g = ld(p);
            if (g != p) atomicMin(&sp[i], g);
            i = p; p = g;
        }
        return i;
    };
    auto unite = [&](int a, int b) {
        while (true) {
            a = find_halve(a); b = find_halve(b);
            if (a == b) return;
            if (a < b) { const int t = a; a = b; b = t; }
            const int old = atomicMin(&sp[a], b);
            if (old == a) return;
            a = old;
        }
    };
    auto on_face = [&](int zz, int yy, int a, int b) -> bool {
        return zz == zf_lo || zz == zf_hi || yy == 0 || yy == ny - 1 || a == 0 || b == skip_nx;
    };
    for (unsigned int k = threadIdx.x; k < np; k += blockDim.x) {
        const RunRec r = runs[r0 + k];
        const int y = r.row - z * ny;
        if (y == y0) continue;                              // the segment's first row: its predecessor belongs to the cross pass
        const int xs = (int)(r.x & 0xffffu), xe = (int)(r.x >> 16);
        const bool mine = skip != 0 && on_face(z, y, xs, xe);
        const i64 rr = (i64)z * ny + (y - 1);
        const unsigned int lo = row_off[rr], hi = row_off[rr + 1];
        if (lo == hi) continue;
        const int need = (CONN == 26) ? xs : xs + 1;
        unsigned int a = lo, b = hi;
        while (a < b) {
            const unsigned int m = (a + b) >> 1;
            if ((int)(runs[m].x >> 16) < need) a = m + 1; else b = m;
        }
        for (unsigned int j = a; j < hi; ++j) {
            const unsigned int xj = runs[j].x;
            const int xs2 = (int)(xj & 0xffffu);
            if ((CONN == 26) ? (xs2 > xe) : (xs2 >= xe)) break;
            if (mine && on_face(z, y - 1, xs2, (int)(xj >> 16))) continue;
            unite((int)k, (int)(j - r0));
        }
    }
    __syncthreads();
    for (unsigned int k = threadIdx.x; k < np; k += blockDim.x) {
        int i = (int)k, pp = sp[i];
        while (pp != i) { i = pp; pp = sp[i]; }
        parent[r0 + k] = (int)r0 + i;
        proot[r0 + k] = (int)r0 + i;
    }
}

template <int CONN>
__global__ void __launch_bounds__(256)
rl_union_cross_kernel(const RunRec *__restrict__ runs, const unsigned int *__restrict__ row_off, int *__restrict__ parent,
                      const int *__restrict__ proot, int *__restrict__ link, RunN rn, int ny, int skip, int zf_lo, int zf_hi, int skip_nx,
                      const uint8_t *__restrict__ seg_done, int seg_shift, int nseg) {
  const i64 nruns = run_n(rn);
  for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < nruns; i += (i64)gridDim.x * blockDim.x) {
    const RunRec r = runs[i];
    const int xs = (int)(r.x & 0xffffu), xe = (int)(r.x >> 16);
    const int z = r.row / ny, y = r.row % ny;
    auto on_face = [&](int zz, int yy, int a, int b) -> bool {
        return zz == zf_lo || zz == zf_hi || yy == 0 || yy == ny - 1 || a == 0 || b == skip_nx;
    };
    const bool mine = skip != 0 && on_face(z, y, xs, xe);
    const int A = proot[i];
    int lastB = -1;                                  // consecutive neighbours mostly belong to one component
    auto row = [&](int zz, int yy) {
        if (zz < 0 || yy < 0 || yy >= ny) return;
        const i64 rr = (i64)zz * ny + yy;
        unsigned int lo = row_off[rr], hi = row_off[rr + 1];
        if (lo == hi) return;
        const int need = (CONN == 26) ? xs : xs + 1;
        unsigned int a = lo, b = hi;
        while (a < b) {
            const unsigned int m = (a + b) >> 1;
            if ((int)(runs[m].x >> 16) < need) a = m + 1; else b = m;
        }
        for (unsigned int j = a; j < hi; ++j) {
            const unsigned int xj = runs[j].x;
            const int xs2 = (int)(xj & 0xffffu);
            if ((CONN == 26) ? (xs2 > xe) : (xs2 >= xe)) break;
            if (mine && on_face(zz, yy, xs2, (int)(xj >> 16))) continue;
            const int B = proot[j];
            if (A == B || B == lastB) continue;
            lastB = B;
            // a plain read first: atomics on one address retire ~10 ns apart, and the thousands of run pairs of a long object's
            // cross-section all ask about the same (A, B) -- after the first claim they see it here and leave
            if (__hip_atomic_load(&link[A], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == B) continue;
            const int old = atomicCAS(&link[A], -1, B);
            if (old == B) continue;                                  // this component pair is already being joined
            uf_union(parent, A, B);
        }
    };
    const bool in_plane = !seg_done[z * nseg + (y >> seg_shift)] || (y & ((1 << seg_shift) - 1)) == 0;
    if (CONN == 6) {
        row(z - 1, y);
        if (in_plane) row(z, y - 1);
    } else {
        row(z - 1, y - 1);
        row(z - 1, y);
        row(z - 1, y + 1);
        if (in_plane) row(z, y - 1);
    }
  }
}

// background components that touch a face of the GLOBAL volume
__global__ void __launch_bounds__(256)
rl_border_kernel(const RunRec *__restrict__ runs, const int *__restrict__ parent, uint8_t *__restrict__ flag, RunN rn, VolGeom v) {
    const i64 nruns = run_n(rn);
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < nruns; i += (i64)gridDim.x * blockDim.x) {
        const RunRec r = runs[i];
        const int xs = (int)(r.x & 0xffffu), xe = (int)(r.x >> 16);
        const i64 z = r.row / v.ny, y = r.row % v.ny;
        const i64 gz = v.gz0 + z;
        if (gz == 0 || gz == v.gnz - 1 || y == 0 || y == v.ny - 1 || xs == 0 || xe == (int)v.nx) flag[parent[i]] = 1;
    }
}
// a[i] = value for the runs' scratch arrays (the host does not know how many runs there are)
__global__ void __launch_bounds__(256)
rl_fill_u32_kernel(unsigned int *__restrict__ a, unsigned int value, RunN rn) {
    const i64 nruns = run_n(rn);
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < nruns; i += (i64)gridDim.x * blockDim.x) a[i] = value;
}
__global__ void __launch_bounds__(256)
rl_fill_u8_kernel(uint8_t *__restrict__ a, RunN rn) {
    const i64 nruns = run_n(rn);
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < nruns; i += (i64)gridDim.x * blockDim.x) a[i] = 0;
}

__device__ __forceinline__ void rl_set_bits(unsigned long long *__restrict__ bits, i64 row, int wpr, int xs, int xe) {
    for (int w = xs >> 6; w <= (xe - 1) >> 6; ++w) {
        const int lo = xs > w * 64 ? xs - w * 64 : 0;
        const int hi = xe < (w + 1) * 64 ? xe - w * 64 : 64;      // bits [lo, hi)
        const unsigned long long m = ((hi == 64) ? ~0ull : ((1ull << hi) - 1ull)) & ~((1ull << lo) - 1ull);
        atomicOr(&bits[row * wpr + w], m);
    }
}

// enclosed background -> foreground
__global__ void __launch_bounds__(256)
rl_fill_kernel(const RunRec *__restrict__ runs, const int *__restrict__ parent, const uint8_t *__restrict__ flag,
               unsigned long long *__restrict__ bits, RunN rn, int wpr) {
    const i64 nruns = run_n(rn);
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < nruns; i += (i64)gridDim.x * blockDim.x) {
        if (flag[parent[i]]) continue;
        const RunRec r = runs[i];
        rl_set_bits(bits, r.row, wpr, (int)(r.x & 0xffffu), (int)(r.x >> 16));
    }
}

// area[root] += run length; a workgroup first merges its 4096 consecutive runs in an LDS hash table so a huge
// object costs one global atomic per workgroup, not one per run
#define RL_HT 256
#define RL_CHUNK 4096
__global__ void __launch_bounds__(256)
rl_area_kernel(const RunRec *__restrict__ runs, const int *__restrict__ parent, int *__restrict__ area, RunN rn) {
    __shared__ int keys[RL_HT];
    __shared__ int vals[RL_HT];
    const i64 nruns = run_n(rn);
    const i64 nchunk = (nruns + RL_CHUNK - 1) / RL_CHUNK;
  for (i64 chunk = blockIdx.x; chunk < nchunk; chunk += gridDim.x) {          // uniform per workgroup
    __syncthreads();
    for (int k = threadIdx.x; k < RL_HT; k += 256) { keys[k] = -1; vals[k] = 0; }
    __syncthreads();
    const i64 base = chunk * RL_CHUNK;
    for (int k = threadIdx.x; k < RL_CHUNK; k += 256) {
        const i64 i = base + k;
        if (i >= nruns) break;
        const int root = parent[i];
        const int len = (int)(runs[i].x >> 16) - (int)(runs[i].x & 0xffffu);
        unsigned int h = ((unsigned int)root * 2654435761u) >> 24;
        bool done = false;
        for (int probe = 0; probe < 8 && !done; ++probe) {
            const int old = atomicCAS(&keys[h], -1, root);
            if (old == -1 || old == root) { atomicAdd(&vals[h], len); done = true; }
            else h = (h + 1) & (RL_HT - 1);
        }
        if (!done) atomicAdd(&area[root], len);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < RL_HT; k += 256)
        if (keys[k] >= 0 && vals[k]) atomicAdd(&area[keys[k]], vals[k]);
  }
}

// keep the runs of objects with >= min_area voxels
__global__ void __launch_bounds__(256)
rl_keep_kernel(const RunRec *__restrict__ runs, const int *__restrict__ parent, const int *__restrict__ area, int min_area,
               unsigned long long *__restrict__ bits, RunN rn, int wpr) {
    const i64 nruns = run_n(rn);
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < nruns; i += (i64)gridDim.x * blockDim.x) {
        if (area[parent[i]] < min_area) continue;
        const RunRec r = runs[i];
        rl_set_bits(bits, r.row, wpr, (int)(r.x & 0xffffu), (int)(r.x >> 16));
    }
}

// uniform_filter(float32 mask, size 3, mode='reflect') > 0.5  ==  at least 14 of the 27 clamped neighbours set.
// One thread per 64-voxel word: the 27 one-bit inputs (9 neighbour rows x {x-1, x, x+1}) are summed with a
// bit-sliced 5-bit counter, then compared with 14, all in 64-bit lanes.
__global__ void __launch_bounds__(256)
majority_bits_kernel(const unsigned long long *__restrict__ in, unsigned long long *__restrict__ out, VolGeom v, int wpr, i64 z_lo, i64 z_hi) {
    // planes [z_lo, z_hi) of the bit volume are produced (a Z slab: its owned planes; their neighbours are real ghost planes).
    // 32-bit index arithmetic: a bit volume has N / 64 < 2^25 words.
    const unsigned int ny = (unsigned int)v.ny, uw = (unsigned int)wpr;
    const unsigned int nw = (unsigned int)(z_hi - z_lo) * ny * uw;
    const unsigned int t0 = blockIdx.x * blockDim.x + threadIdx.x;
    if (t0 >= nw) return;
    const unsigned int w = t0 % uw, row0 = t0 / uw;
    const int y = (int)(row0 % ny), z = (int)(row0 / ny) + (int)z_lo;
    const i64 t = ((i64)z * ny + y) * wpr + w;
    const bool last = (w == uw - 1u);                               // the word holding x = nx-1
    const unsigned long long top = 1ull << (((int)v.nx - 1) & 63);   // ... at this bit
    const unsigned long long valid = (top << 1) - 1ull;             // bits of the last word that are voxels (all 64: top << 1 wraps to 0)
    unsigned long long c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0;
    auto add = [&](unsigned long long b) {
        unsigned long long t0_ = c0 & b; c0 ^= b; b = t0_;
        t0_ = c1 & b; c1 ^= b; b = t0_;
        t0_ = c2 & b; c2 ^= b; b = t0_;
        t0_ = c3 & b; c3 ^= b; b = t0_;
        c4 ^= b;
    };
    // the nine words of this column first: if they are all empty no voxel of the word can reach 14 (a bit then only has
    // its x-1 or its x+1 neighbours in the adjacent word, at most 9 of them) -- true for 97 % of the words of a frame
    unsigned long long cw[9];
    i64 rws[9];
    unsigned long long any = 0ull;
#pragma unroll
    for (int dz = -1; dz <= 1; ++dz) {
        int zz = z + dz;
        const i64 gg = v.gz0 + zz;
        if (gg < 0 || gg >= v.gnz) zz = z;                         // reflect == clamp for a 3-window
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
            int yy = y + dy;
            yy = yy < 0 ? 0 : (yy >= (int)ny ? (int)ny - 1 : yy);
            const int k = (dz + 1) * 3 + (dy + 1);
            rws[k] = ((i64)zz * ny + yy) * wpr;
            cw[k] = in[rws[k] + w];
            any |= cw[k];
        }
    }
    if (any == 0ull) { out[t] = 0ull; return; }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const unsigned long long cur = cw[k];
        // x-1: shift up; bit 0 comes from the previous word's bit 63, or (x = 0) from bit 0 itself
        const unsigned long long prev = (w > 0u) ? in[rws[k] + w - 1] : 0ull;
        const unsigned long long left = (cur << 1) | ((w > 0u) ? (prev >> 63) : (cur & 1ull));
        // x+1: shift down; the top bit comes from the next word's bit 0, or (x = nx-1) is its own neighbour
        const unsigned long long next = last ? 0ull : in[rws[k] + w + 1];
        const unsigned long long right = (cur >> 1) | (last ? (cur & top) : (next << 63));
        add(left); add(cur); add(right);
    }
    // count >= 14  <=>  c4 | (c3 & c2 & c1)   (14 = 0b01110; 16+ has c4; 14,15 have c3&c2&c1)
    unsigned long long res = c4 | (c3 & c2 & c1);
    if (last) res &= valid;
    out[t] = res;
}

// ids in raster order of the roots were written to newid[]; paint the int32 volume.  One wave per row.
// (Round 4, measured at 1024^3 / on a 128 x 2048 x 2048 slab: this form 0.98 / 0.43 ms; four rows per wave, their offsets in one load
// and the zero stores back to back 1.12 / 0.51; the volume cleared by a fill (6.4 TB/s) and only rows with runs touched 0.66 + 0.40 /
// 0.32 + 0.16; the same with a wave looking at 64 rows and painting those with runs in turn 0.66 + 0.39 / 0.32 + 0.31 -- most rows of
// these frames hold runs, and a 4 B/voxel write stream wants many short waves.)
// SPARSE: `out` is already all zero on these rows (a fill beside the last scale's walk: nl_gauss_step) -- only the voxels inside the
// runs are stored, a row without runs costs its two offsets.
template <bool SPARSE>
__global__ void __launch_bounds__(256)
rl_paint_kernel(const unsigned long long *__restrict__ bits, const unsigned int *__restrict__ row_off, const int *__restrict__ parent,
                const int *__restrict__ newid, int *__restrict__ out, i64 row0, i64 row1, int wpr, int nx) {
    // rows [row0, row1) of the mask are painted; out[0] is the first voxel of row0
    const i64 wstride = ((i64)gridDim.x * blockDim.x) >> 6;
    const int lane = threadIdx.x & 63;
    for (i64 row = row0 + (((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6); row < row1; row += wstride) {
        const unsigned int seen0 = row_off[row], nr = row_off[row + 1] - seen0;
        unsigned int seen = seen0;               // runs of this row that started before the current word
        // the labels of the row's first 64 runs, fetched side by side (two dependent random reads each): doing
        // them voxel by voxel inside the word loop would expose that latency once per non-empty word
        int *orow = out + (row - row0) * nx;
        const bool vec = ((nx & 3) == 0) && ((reinterpret_cast<size_t>(orow) & 15) == 0);
        if (SPARSE && nr == 0u) continue;
        if (nr == 0u && vec) {                  // a row without runs (most rows): zeros, without looking at the mask
            for (int q = lane; q < nx / 4; q += 64) reinterpret_cast<int4 *>(orow)[q] = make_int4(0, 0, 0, 0);
            continue;
        }
        const int lab_mine = ((unsigned int)lane < nr) ? newid[parent[seen0 + lane]] : 0;
        if (vec) {
            // a row with runs: zeros first, in four wide stores like an empty row, then only the words that hold voxels are
            // visited -- a row has a handful of runs, not 16 words' worth
            if (!SPARSE) {
            for (int q = lane; q < nx / 4; q += 64) reinterpret_cast<int4 *>(orow)[q] = make_int4(0, 0, 0, 0);
            // the label stores below hit addresses the zero stores also wrote, from other lanes: wait until the zeros have been
            // acknowledged instead of relying on the order in which two stores of one wave reach L2 (the lookups of this row's
            // labels above are in flight meanwhile, other waves fill the time)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            unsigned long long carry = 0;
            int prev_w = -2;                     // last visited word: a run continues from it only if it is the word before
            for (int wb = 0; wb < wpr; wb += 64) {
                const unsigned long long mine = (wb + lane < wpr) ? rl_word(bits, row, wb + lane, wpr, nx, false) : 0ull;
                unsigned long long todo = __ballot(mine != 0ull);
                while (todo) {
                    const int wl = __builtin_ctzll(todo);
                    todo &= todo - 1;
                    const int w = wb + wl;
                    const unsigned long long v = __shfl(mine, wl, 64);
                    if (w != prev_w + 1) carry = 0ull;
                    const unsigned long long starts = v & ~((v << 1) | carry);
                    const int x = w * 64 + lane;
                    const bool set = (v >> lane) & 1ull;
                    const unsigned long long below = starts & ((lane == 63) ? ~0ull : ((1ull << (lane + 1)) - 1ull));
                    const unsigned int rl = set ? (seen - seen0) + (unsigned int)__builtin_popcountll(below) - 1u : 0u;
                    int lab = __shfl(lab_mine, (int)(rl & 63u), 64);
                    if (set && rl >= 64u) lab = newid[parent[seen0 + rl]];
                    if (set && x < nx) orow[x] = lab;
                    seen += (unsigned int)__builtin_popcountll(starts);
                    carry = v >> 63;
                    prev_w = w;
                }
            }
            continue;
        }
        unsigned long long carry = 0;
        for (int wb = 0; wb < wpr; wb += 64) {
            const unsigned long long mine = (wb + lane < wpr) ? rl_word(bits, row, wb + lane, wpr, nx, false) : 0ull;
            const int wend = wpr - wb < 64 ? wpr - wb : 64;
            for (int wl = 0; wl < wend; ++wl) {
                const int w = wb + wl;
                const unsigned long long v = __shfl(mine, wl, 64);
                const unsigned long long starts = v & ~((v << 1) | carry);
                const int x = w * 64 + lane;
                // index of my run = runs started before this word + starts at or below my bit - 1
                // (every lane takes part in the shuffle: a lane beyond nx may hold the label another lane needs)
                const bool set = (v >> lane) & 1ull;
                const unsigned long long below = starts & ((lane == 63) ? ~0ull : ((1ull << (lane + 1)) - 1ull));
                const unsigned int rl = set ? (seen - seen0) + (unsigned int)__builtin_popcountll(below) - 1u : 0u;
                int lab = __shfl(lab_mine, (int)(rl & 63u), 64);
                if (set && rl >= 64u) lab = newid[parent[seen0 + rl]];
                if (x < nx && (set || !SPARSE)) orow[x] = set ? lab : 0;
                seen += (unsigned int)__builtin_popcountll(starts);
                carry = v >> 63;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------
// Z-slab Label without replication (nellie_amd/sharded.py): every rank labels its own planes plus ONE ghost plane per
// interior side.  A component that crosses an interface appears on both ranks as a tree that contains runs of the two
// planes both ranks see (the neighbour's boundary plane = my ghost plane, bit for bit the same runs), so the k-th run of
// such a plane names the same voxels on both sides: the host joins the trees of neighbouring ranks through these
// tables and hands back what each phase needs (see the phases below).  The kernels here only add what the
// single-volume pipeline lacks: per-tree quantities restricted to the OWNED planes, the tables, and the patches.
#define SL_FILL 0      // aux = 1 if the background tree touches a face of the global volume (binary_fill_holes)
#define SL_AREA 1      // aux = voxels of the tree on the owned planes (the small-object filter)
#define SL_NUMBER 2    // aux = index of the tree's first run on the owned planes, INT_MAX if it has none (label numbering)

// aux[root] = min run index over the tree's runs on rows [row_lo, row_hi).  A root is the smallest index of its tree, so a
// tree rooted on the owned rows answers for itself; only trees rooted in the low ghost plane (runs below `own_first`) need
// the minimum over their owned runs -- taken with a read before the atomic: runs are visited in roughly increasing order,
// so after the first few almost every thread sees a smaller value already there and leaves (atomics on one address
// retire ~10 ns apart: one per run of a component that crosses the whole slab cost milliseconds).
__global__ void __launch_bounds__(256)
sl_first_own_kernel(const RunRec *__restrict__ runs, const int *__restrict__ parent, int *__restrict__ aux, i64 nruns, int row_lo, int row_hi,
                    const unsigned int *__restrict__ own_first_ptr) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nruns) return;
    const int own_first = (int)*own_first_ptr;              // first run of the first owned plane: row_off[row_lo], read where it lies
    const int row = runs[i].row;
    if (row < row_lo || row >= row_hi) return;
    const int r = parent[i];
    if (r >= own_first) { if (r == (int)i) aux[i] = (int)i; return; }
    if ((int)i < __hip_atomic_load(&aux[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&aux[r], (int)i);
}
// area[root] += run length, runs on rows [row_lo, row_hi) only (cf. rl_area_kernel)
__global__ void __launch_bounds__(256)
sl_area_kernel(const RunRec *__restrict__ runs, const int *__restrict__ parent, int *__restrict__ area, i64 nruns, int row_lo, int row_hi) {
    __shared__ int keys[RL_HT];
    __shared__ int vals[RL_HT];
    for (int k = threadIdx.x; k < RL_HT; k += 256) { keys[k] = -1; vals[k] = 0; }
    __syncthreads();
    const i64 base = (i64)blockIdx.x * RL_CHUNK;
    for (int k = threadIdx.x; k < RL_CHUNK; k += 256) {
        const i64 i = base + k;
        if (i >= nruns) break;
        const RunRec r = runs[i];
        if (r.row < row_lo || r.row >= row_hi) continue;
        const int root = parent[i];
        const int len = (int)(r.x >> 16) - (int)(r.x & 0xffffu);
        unsigned int h = ((unsigned int)root * 2654435761u) >> 24;
        bool done = false;
        for (int probe = 0; probe < 8 && !done; ++probe) {
            const int old = atomicCAS(&keys[h], -1, root);
            if (old == -1 || old == root) { atomicAdd(&vals[h], len); done = true; }
            else h = (h + 1) & (RL_HT - 1);
        }
        if (!done) atomicAdd(&area[root], len);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < RL_HT; k += 256)
        if (keys[k] >= 0 && vals[k]) atomicAdd(&area[keys[k]], vals[k]);
}
// ---- the tables the ranks exchange (round 4: compact, and built without a host round trip) ---------------------------------
// One ENTRY per segment component of a shared plane (a run whose in-plane root -- `proot`, written by rl_union_plane_kernel --
// is the run itself), in raster order.  Both ranks that see a plane hold the same bits of it, hence the same runs, the same
// segments and the same in-plane components: the k-th entry of a shared plane names the same voxels on both sides, and a tree
// contains whole segment components, so entry pairs join the trees of neighbouring ranks exactly as run pairs did -- with a
// few hundred entries per plane instead of thousands of runs.  proot == NULL (one-level union-find): every run is an entry.
//   bidx[p * capE + k] = run index of the k-th entry of plane p (0 ghost-low, 1 own-first, 2 own-last, 3 ghost-high)
//   hdr[p]             = entries of plane p (may exceed capE: sl_table2_kernel flags the overflow)
struct SlabPlanes { int row[4]; };          // first row of each of the four planes in the run set, -1: the slab has no such plane
__global__ void __launch_bounds__(1024)
sl_boundary_kernel(const unsigned int *__restrict__ row_off, const int *__restrict__ proot, SlabPlanes pl, int ny, int capE,
                   int *__restrict__ bidx, int *__restrict__ hdr) {
    __shared__ unsigned int s_w[16];
    __shared__ unsigned int s_base;
    const int p = blockIdx.x;
    if (pl.row[p] < 0) { if (threadIdx.x == 0) hdr[p] = 0; return; }
    const unsigned int r0 = row_off[pl.row[p]], r1 = row_off[pl.row[p] + ny];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_base = 0;
    __syncthreads();
    for (unsigned int c0 = r0; c0 < r1; c0 += 1024) {
        const unsigned int i = c0 + threadIdx.x;
        const bool f = i < r1 && (!proot || proot[i] == (int)i);
        const unsigned long long b = __ballot(f);
        const unsigned int below = (unsigned int)__builtin_popcountll(b & ((1ull << lane) - 1ull));
        if (lane == 0) s_w[w] = (unsigned int)__builtin_popcountll(b);
        __syncthreads();
        unsigned int off = s_base;
        for (int q = 0; q < w; ++q) off += s_w[q];
        if (f && off + below < (unsigned int)capE) bidx[(size_t)p * capE + off + below] = (int)i;
        __syncthreads();
        if (threadIdx.x == 0) { unsigned int t = 0; for (int q = 0; q < 16; ++q) t += s_w[q]; s_base += t; }
        __syncthreads();
    }
    if (threadIdx.x == 0) hdr[p] = (int)s_base;
}
// blob = [n0 n1 n2 n3 | total ints | overflow | runs | 0] [roots of plane 0..3] [values of plane 0..3]   (int32)
__global__ void __launch_bounds__(256)
sl_table2_kernel(const int *__restrict__ parent, const int *__restrict__ aux, const uint8_t *__restrict__ flag, const int *__restrict__ bidx,
                 int capE, const int *__restrict__ hdr, int *__restrict__ blob, const unsigned int *__restrict__ nruns_ptr) {
    const int p = blockIdx.x;
    int cnt[4], total = 0, off = 8, over = 0;
    for (int q = 0; q < 4; ++q) {
        const int h = hdr[q];
        cnt[q] = h < capE ? h : capE; over |= h > capE;
        if (q < p) off += cnt[q];
        total += cnt[q];
    }
    for (int e = threadIdx.x; e < cnt[p]; e += blockDim.x) {
        const int r = parent[bidx[(size_t)p * capE + e]];
        blob[off + e] = r;
        blob[total + off + e] = flag ? (int)flag[r] : aux[r];
    }
    if (p == 0 && threadIdx.x < 8) {
        const int t = threadIdx.x;
        blob[t] = t < 4 ? cnt[t] : (t == 4 ? 8 + 2 * total : (t == 5 ? over : (t == 6 ? (int)*nruns_ptr : 0)));
    }
}
__global__ void __launch_bounds__(256)
sl_patch_kernel(int *__restrict__ aux, uint8_t *__restrict__ flag, const int *__restrict__ idx, const int *__restrict__ val, int n) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    if (flag) flag[idx[k]] = (uint8_t)(val[k] != 0); else aux[idx[k]] = val[k];
}
__global__ void __launch_bounds__(256)
sl_gather_kernel(const unsigned int *__restrict__ src, const int *__restrict__ idx, int *__restrict__ out, int n, int add) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = (int)src[idx[k]] + add;
}
// enclosed background -> foreground / kept runs -> bits, runs on rows [row_lo, row_hi) only
__global__ void __launch_bounds__(256)
sl_fill_kernel(const RunRec *__restrict__ runs, const int *__restrict__ parent, const uint8_t *__restrict__ flag,
               unsigned long long *__restrict__ bits, i64 nruns, int wpr, int row_lo, int row_hi) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nruns) return;
    const RunRec r = runs[i];
    if (r.row < row_lo || r.row >= row_hi || flag[parent[i]]) return;
    rl_set_bits(bits, r.row, wpr, (int)(r.x & 0xffffu), (int)(r.x >> 16));
}
__global__ void __launch_bounds__(256)
sl_keep_kernel(const RunRec *__restrict__ runs, const int *__restrict__ parent, const int *__restrict__ area, int min_area,
               unsigned long long *__restrict__ bits, i64 nruns, int wpr, int row_lo, int row_hi) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nruns) return;
    const RunRec r = runs[i];
    if (r.row < row_lo || r.row >= row_hi || area[parent[i]] < min_area) return;
    rl_set_bits(bits, r.row, wpr, (int)(r.x & 0xffffu), (int)(r.x >> 16));
}
// sel[i] = 1 for a tree root on the owned rows: the runs whose raster rank numbers this rank's labels (the host then
// clears the roots of trees that continue on other ranks and re-selects the ones this rank owns)
__global__ void __launch_bounds__(256)
sl_select_kernel(const RunRec *__restrict__ runs, const int *__restrict__ parent, unsigned int *__restrict__ sel, i64 nruns, int row_lo, int row_hi) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nruns) return;
    const int row = runs[i].row;
    sel[i] = (parent[i] == (int)i && row >= row_lo && row < row_hi) ? 1u : 0u;
}
__global__ void __launch_bounds__(256)
sl_set_u32_kernel(unsigned int *__restrict__ a, const int *__restrict__ idx, int n, unsigned int v) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) a[idx[k]] = v;
}
// newid[i] = global label of the tree rooted at run i: base + local rank for a selected root, 0 otherwise
__global__ void __launch_bounds__(256)
sl_ids_kernel(const unsigned int *__restrict__ sel, const unsigned int *__restrict__ scan, int base, int *__restrict__ newid, i64 nruns) {
    const i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nruns) newid[i] = sel[i] ? base + (int)scan[i] + 1 : 0;
}
