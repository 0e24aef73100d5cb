// Part of libnellie_hip.so (gfx950): the kernels of the Frangi epilogue on the mask bit planes, included by nellie_hip.hip.
// vesselness * masks (filtering.py:926); counts voxels > 0 on the owned planes.
// The cumulative mask is a bit mask: one 64-bit word per 64 consecutive x of a row (row pitch `wpr` words).
__global__ void __launch_bounds__(256)
finish_kernel(float *__restrict__ vmax, const unsigned long long *__restrict__ cmask64, int nslots, i64 slot_words, int wpr,
              VolGeom v, i64 z0, i64 z1, i64 cnt_lo, i64 cnt_hi, unsigned long long *__restrict__ npos) {
    // one thread = 4 consecutive x of one row (they share a mask word); rows are padded to a multiple of 4 here
    const i64 qpr = (v.nx + 3) / 4;                                    // quads per row
    const i64 total = (z1 - z0) * v.ny * qpr;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    const bool vec = (v.nx & 3) == 0;
    unsigned long long cnt = 0;
    for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const i64 row = t / qpr;
        const i64 x0 = (t % qpr) * 4;
        const i64 zloc = z0 + row / v.ny;
        const bool counted = zloc >= cnt_lo && zloc < cnt_hi;
        unsigned long long bits = ~0ull;
        for (int k = 0; k < nslots; ++k) bits &= cmask64[k * slot_words + (z0 * v.ny + row) * wpr + (x0 >> 6)];
        const unsigned int b4 = (unsigned int)(bits >> (x0 & 63)) & 0xFu;
        float *p = vmax + (z0 * v.ny + row) * v.nx + x0;
        if (vec) {
            float4 val = *reinterpret_cast<float4 *>(p);
            if (b4 != 0xFu) {
                if (!(b4 & 1u)) val.x = 0.0f;
                if (!(b4 & 2u)) val.y = 0.0f;
                if (!(b4 & 4u)) val.z = 0.0f;
                if (!(b4 & 8u)) val.w = 0.0f;
                *reinterpret_cast<float4 *>(p) = val;
            }
            if (counted) cnt += (val.x > 0.0f) + (val.y > 0.0f) + (val.z > 0.0f) + (val.w > 0.0f);
        } else {
            for (int q = 0; q < 4 && x0 + q < v.nx; ++q) {
                float val = p[q];
                if (!((b4 >> q) & 1u)) { val = 0.0f; p[q] = 0.0f; }
                if (counted && val > 0.0f) cnt++;
            }
        }
    }
    block_add_u64(wave_sum_u64(cnt), npos);
}

// filtering.py:964-966: mask = f > thr; binary_opening (6-conn cross, one iteration, border_value 0); f * mask.
// Done on BIT masks: pack (rl_threshold_pack_kernel), erode, dilate (word-wide logic on 1 bit/voxel), apply.
// Planes [z0, z1) are produced from planes [z0-1, z1+1) of the input bits; neighbours outside the GLOBAL volume
// count as 0 (border_value), ghost planes of a slab are real neighbours.
template <int DILATE>
__global__ void __launch_bounds__(256)
bits_morph6_kernel(const unsigned long long *__restrict__ in, unsigned long long *__restrict__ out, VolGeom v, int wpr, i64 z0, i64 z1,
                   int two_d) {
    const i64 nw = (z1 - z0) * v.ny * wpr;
    const i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nw) return;
    const int w = (int)(t % wpr);
    const i64 row_in_range = t / wpr;
    const i64 y = row_in_range % v.ny, z = z0 + row_in_range / v.ny;
    const i64 row = z * v.ny + y;
    const unsigned long long cur = in[row * wpr + w];
    const unsigned long long lft = (cur << 1) | ((w > 0) ? (in[row * wpr + w - 1] >> 63) : 0ull);           // x-1
    const unsigned long long rgt = (cur >> 1) | ((w + 1 < wpr) ? (in[row * wpr + w + 1] << 63) : 0ull);    // x+1
    const i64 gz = v.gz0 + z;
    // a 2-D image has no Z neighbours in its (4-connected) structuring element: neutral for AND / OR
    const unsigned long long none = DILATE ? 0ull : ~0ull;
    const unsigned long long up = two_d ? none : ((gz > 0) ? in[(row - v.ny) * wpr + w] : 0ull);
    const unsigned long long dn = two_d ? none : ((gz < v.gnz - 1) ? in[(row + v.ny) * wpr + w] : 0ull);
    const unsigned long long no = (y > 0) ? in[(row - 1) * wpr + w] : 0ull;
    const unsigned long long so = (y < v.ny - 1) ? in[(row + 1) * wpr + w] : 0ull;
    unsigned long long r = DILATE ? (cur | lft | rgt | up | dn | no | so) : (cur & lft & rgt & up & dn & no & so);
    const int rem = (int)v.nx - w * 64;
    if (rem < 64) r &= (1ull << rem) - 1ull;          // keep the tail bits of a row at 0
    out[row * wpr + w] = r;
}

__global__ void __launch_bounds__(256)
apply_bits_kernel(const float *__restrict__ f, const unsigned long long *__restrict__ bits, float *__restrict__ out, VolGeom v,
                  int wpr, i64 z0, i64 z1) {
    const i64 qpr = (v.nx + 3) / 4;
    const i64 total = (z1 - z0) * v.ny * qpr;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    const bool vec = (v.nx & 3) == 0;
    for (i64 t = (i64)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
        const i64 row = z0 * v.ny + t / qpr;
        const i64 x0 = (t % qpr) * 4;
        const unsigned int b4 = (unsigned int)(bits[row * wpr + (x0 >> 6)] >> (x0 & 63)) & 0xFu;
        const float *p = f + row * v.nx + x0;
        float *o = out + row * v.nx + x0;
        if (vec) {
            float4 a = *reinterpret_cast<const float4 *>(p);
            // frame * mask: a False mask gives +-0 with the sign of the value, exactly numpy's float * bool
            if (!(b4 & 1u)) a.x *= 0.0f;
            if (!(b4 & 2u)) a.y *= 0.0f;
            if (!(b4 & 4u)) a.z *= 0.0f;
            if (!(b4 & 8u)) a.w *= 0.0f;
            *reinterpret_cast<float4 *>(o) = a;
        } else {
            for (int k = 0; k < 4 && x0 + k < v.nx; ++k) o[k] = ((b4 >> k) & 1u) ? p[k] : p[k] * 0.0f;
        }
    }
}

// Fused finish + threshold pack (filtering.py:926, 964): bit = alive && vesselness > thr.  One wave per row; the
// vesselness is only read where the cumulative mask has bits.  Counts alive voxels > 0 on the counted rows.
__global__ void __launch_bounds__(256)
pack_masked_kernel(const float *__restrict__ f, const unsigned long long *__restrict__ alive, unsigned long long *__restrict__ bits,
                   float thr_host, const float *__restrict__ thr_dev, int nx, i64 row0, i64 row1, int wpr, i64 cnt_row0, i64 cnt_row1,
                   unsigned long long *__restrict__ npos) {
    const float thr = thr_dev ? *thr_dev : thr_host;          // decided by a kernel (nl_tail_enqueue) or by the host
    const i64 wstride = ((i64)gridDim.x * blockDim.x) >> 6;
    const int lane = threadIdx.x & 63;
    unsigned long long cnt = 0;
    // the row's mask words in one coalesced load (lane l holds word l) instead of a dependent load per trip; the NEXT row's words
    // are requested before this row is worked on
    const bool row_words = wpr <= 64;
    const i64 first = row0 + (((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    unsigned long long mine_next = (row_words && first < row1 && lane < wpr) ? alive[first * wpr + lane] : 0ull;
    // ... and this row's result words leave at the top of the next trip, BEFORE its loads: vmcnt counts in order, and a store that is
    // the youngest operation when the prefetched words are taken over would be waited for (see vesselness_queue_kernel)
    unsigned long long st_res = 0ull;
    i64 st_row = -1;
    for (i64 row = first; row < row1; row += wstride) {
        const bool counted = row >= cnt_row0 && row < cnt_row1;
        const float *fr = f + row * nx;
        const unsigned long long mine = mine_next;
        if (row_words) {
            if (st_row >= 0 && lane < wpr) bits[st_row * wpr + lane] = st_res;
            mine_next = (row + wstride < row1 && lane < wpr) ? alive[(row + wstride) * wpr + lane] : 0ull;
            // Round 4: only the words that hold alive voxels are visited, eight of them (eight independent loads per lane) per trip,
            // and the row's result words leave in ONE store (lane l holds word l).  The kernel is bound by its dependent round
            // trips, not by bytes (1.1 B/voxel fetched): a 1024-wide row took 1 + 4 of them, now 1 + 1 (most rows have < 8 words alive).
            unsigned long long nz = __ballot(mine != 0ull), res = 0ull;
            while (nz) {                                                 // uniform
                int wi[8];
                float v[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    wi[k] = nz ? (int)__builtin_ctzll(nz) : -1;
                    nz &= nz - 1ull;
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const unsigned long long a = wi[k] >= 0 ? wave_read_u64(mine, wi[k]) : 0ull;
                    const int x = wi[k] * 64 + lane;
                    v[k] = (((a >> lane) & 1ull) && x < nx) ? fr[x] : 0.0f;   // 0 fails both tests below (thr >= 0)
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    if (wi[k] < 0) break;                                // uniform
                    const unsigned long long b = __ballot(v[k] > thr && v[k] > 0.0f);
                    const unsigned long long pb = __ballot(v[k] > 0.0f);
                    if (counted) cnt += (unsigned long long)__builtin_popcountll(pb);      // wave-uniform
                    if (lane == wi[k]) res = b;
                }
            }
            st_res = res; st_row = row;
            continue;
        }
        for (int w0 = 0; w0 < wpr; w0 += 4) {                          // four words (four independent loads) in flight
            unsigned long long a[4];
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                a[k] = (w0 + k < wpr) ? alive[row * wpr + w0 + k] : 0ull;           // (rows of more than 64 words)
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int x = (w0 + k) * 64 + lane;
                v[k] = (((a[k] >> lane) & 1ull) && x < nx) ? fr[x] : 0.0f;   // 0 fails both tests below (thr >= 0)
            }
            unsigned long long b[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                b[k] = __ballot(v[k] > thr && v[k] > 0.0f);
                const unsigned long long pb = __ballot(v[k] > 0.0f);
                if (counted) cnt += (unsigned long long)__builtin_popcountll(pb);      // wave-uniform
            }
            if (lane < 4 && w0 + lane < wpr) bits[row * wpr + w0 + lane] = lane == 0 ? b[0] : (lane == 1 ? b[1] : (lane == 2 ? b[2] : b[3]));
        }
    }
    if (st_row >= 0 && lane < wpr) bits[st_row * wpr + lane] = st_res;
    block_add_u64(cnt, npos);
}

// filtering.py:969-1000 (`_remove_edges`): per Z plane (a 2-D image is its single plane), the rows holding any non-zero
// value span [rmin, rmax]; min(margin, rmax - rmin + 1) rows at both ends of that span are zeroed.  One workgroup per
// plane; counts the values > 0 that remain (the reference's `sum(frame) > 0` test of a non-negative frame).
__global__ void __launch_bounds__(256)
remove_edges_kernel(float *__restrict__ f, VolGeom v, i64 plane0, int margin, i64 cnt_lo, i64 cnt_hi, unsigned long long *__restrict__ npos) {
    __shared__ int s_min, s_max;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int ny = (int)v.ny, nx = (int)v.nx;
    float *p = f + (plane0 + blockIdx.x) * v.ny * v.nx;
    if (threadIdx.x == 0) { s_min = 0x7fffffff; s_max = -1; }
    __syncthreads();
    unsigned long long total = 0;
    for (int row = w; row < ny; row += 4) {
        const float *r = p + (i64)row * nx;
        bool any = false;
        for (int x = lane; x < nx; x += 64) {
            const float val = r[x];
            any = any || (val != 0.0f);
            total += (val > 0.0f) ? 1ull : 0ull;
        }
        if (__ballot(any) != 0ull && lane == 0) { atomicMin(&s_min, row); atomicMax(&s_max, row); }
    }
    __syncthreads();
    const int rmin = s_min, rmax = s_max;
    unsigned long long removed = 0;
    if (rmax >= 0) {
        const int use = margin < rmax - rmin + 1 ? margin : rmax - rmin + 1;
        // rows [rmin, rmin + use) and [rmax - use + 1, rmax], each once even where the two stretches overlap
        const int a1 = rmin + use, b0 = (rmax - use + 1 > a1) ? rmax - use + 1 : a1;
        const int n_rows = (a1 - rmin) + (rmax + 1 - b0);
        for (int k = w; k < n_rows; k += 4) {
            const int row = k < a1 - rmin ? rmin + k : b0 + (k - (a1 - rmin));
            float *r = p + (i64)row * nx;
            for (int x = lane; x < nx; x += 64) {
                removed += (r[x] > 0.0f) ? 1ull : 0ull;
                r[x] = 0.0f;
            }
        }
    }
    total = wave_sum_u64(total);
    removed = wave_sum_u64(removed);
    const i64 zl = plane0 + blockIdx.x;            // ghost planes are trimmed like the owned ones (the opening reads them) but not counted
    const bool counted = zl >= cnt_lo && zl < cnt_hi;
    block_add_u64(counted ? total - removed : 0ull, npos);   // a wave's difference may wrap; the sums over waves and planes do not
}

// out = opened bit ? vesselness : 0 (filtering.py:966 for a non-negative frame): reads only where bits are set.
// One wave per row, 256 floats (1 KiB) per store instruction; launched with one wave per row (a pure 4 B/voxel write
// wants many small workgroups: 5.9 TB/s against 5.2 with a capped grid-stride grid on this part).
#ifndef APPLY_ROWS
#define APPLY_ROWS 2
#endif
__global__ void __launch_bounds__(256)
apply_bits_pos_kernel(const float *__restrict__ f, const unsigned long long *__restrict__ bits, float *__restrict__ out, VolGeom v,
                      int wpr, i64 z0, i64 z1) {
    const i64 nrows = (z1 - z0) * v.ny;
    const i64 wstride = ((i64)gridDim.x * blockDim.x) >> 6;
    const int lane = threadIdx.x & 63;
    const int nx = (int)v.nx;
    const bool vec = (nx & 3) == 0;
    if (vec && wpr <= 64) {
        // APPLY_ROWS rows per wave: a row is a chain of dependent round trips (mask words -> the values under them -> the stores), and
        // a wave that owns one row has one such chain in flight.
        constexpr int RR = APPLY_ROWS;
        for (i64 r0 = (((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * RR; r0 < nrows; r0 += wstride * RR) {
            unsigned long long mine[RR];
            bool empty[RR];
#pragma unroll
            for (int j = 0; j < RR; ++j) {
                // the row's mask words in one load (lane l holds word l)
                mine[j] = (r0 + j < nrows && lane < wpr) ? bits[(z0 * v.ny + r0 + j) * wpr + lane] : 0ull;
            }
#pragma unroll
            for (int j = 0; j < RR; ++j) empty[j] = __ballot(mine[j] != 0ull) == 0ull;      // uniform
            for (int xb = 0; xb < nx; xb += 1024) {                                       // four 1-KiB pieces (their reads, if any, first) per trip
                float4 a[RR][4];
                unsigned int b4[RR][4];
#pragma unroll
                for (int j = 0; j < RR; ++j) {
                    const float *p = f + (z0 * v.ny + r0 + j) * nx;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int x0 = xb + k * 256 + lane * 4;
                        a[j][k] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                        b4[j][k] = 0u;
                        if (!empty[j] && x0 < nx) {
                            const unsigned long long w = __shfl(mine[j], (x0 >> 6) & 63);
                            b4[j][k] = (unsigned int)(w >> (x0 & 63)) & 0xFu;
                            if (b4[j][k]) a[j][k] = *reinterpret_cast<const float4 *>(p + x0);
                        }
                    }
                }
#pragma unroll
                for (int j = 0; j < RR; ++j) {
                    if (r0 + j >= nrows) break;                                            // uniform
                    float *o = out + (z0 * v.ny + r0 + j) * nx;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int x0 = xb + k * 256 + lane * 4;
                        if (x0 < nx) {
                            if (!(b4[j][k] & 1u)) a[j][k].x = 0.0f;
                            if (!(b4[j][k] & 2u)) a[j][k].y = 0.0f;
                            if (!(b4[j][k] & 4u)) a[j][k].z = 0.0f;
                            if (!(b4[j][k] & 8u)) a[j][k].w = 0.0f;
                            *reinterpret_cast<float4 *>(o + x0) = a[j][k];
                        }
                    }
                }
            }
        }
        return;
    }
    for (i64 r = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6; r < nrows; r += wstride) {
        const i64 row = z0 * v.ny + r;
        const float *p = f + row * nx;
        float *o = out + row * nx;
        for (int x0 = lane * 4; x0 < nx; x0 += 256) {
            const unsigned int b4 = (unsigned int)(bits[row * wpr + (x0 >> 6)] >> (x0 & 63)) & 0xFu;
            if (vec) {
                float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (b4) {
                    a = *reinterpret_cast<const float4 *>(p + x0);
                    if (!(b4 & 1u)) a.x = 0.0f;
                    if (!(b4 & 2u)) a.y = 0.0f;
                    if (!(b4 & 4u)) a.z = 0.0f;
                    if (!(b4 & 8u)) a.w = 0.0f;
                }
                *reinterpret_cast<float4 *>(o + x0) = a;
            } else {
                for (int k = 0; k < 4 && x0 + k < nx; ++k) o[x0 + k] = ((b4 >> k) & 1u) ? p[x0 + k] : 0.0f;
            }
        }
    }
}
