// Kernels of nellie_hip_transitions.hip: label transition counts from voxel matches (DESIGN.md section 26).  A match row is the
// coordinates of a voxel of frame t and of one of frame t + 1; its key is the pair of labels found there.  The rows' keys are counted
// in an open-addressing table in global memory, the occupied slots are compacted with the mask, word populations and scan of
// rank_scan.inc, and a streaming pass paints frame t + 1 through a label -> label table.
#pragma once
#include "rank_scan.inc"

#define TR_EMPTY (~0ull)              // the key word of a free slot: no key is all ones, its halves are labels of at most 2^31 - 1
#define TR_MAX_LABEL ((i64)0x7fffffff)
#define TR_NO_ROW ((i64)0x7fffffffffffffffLL)
// the words a pair leaves beside its table
enum { TR_W_BAD_COORD, TR_W_BAD_LABEL, TR_W_OVERFLOW, TR_W_DROPPED, TR_W_HEADS, TR_WORDS };

// a label frame of int32 or int64 elements
struct TrLabels {
    const void *p;
    int wide;                         // 1: int64, 0: int32
    __device__ __forceinline__ i64 operator[](i64 i) const { return wide ? ((const i64 *)p)[i] : (i64)((const int *)p)[i]; }
};

// Every slot free and without a count, one 16-byte store per slot; the first workgroup also resets the words.
static __global__ __launch_bounds__(256) void tr_clear_kernel(ulonglong2 *__restrict__ table, i64 slots, i64 *__restrict__ words) {
    for (i64 s = (i64)blockIdx.x * 256 + threadIdx.x; s < slots; s += (i64)gridDim.x * 256) table[s] = make_ulonglong2(TR_EMPTY, 0ull);
    if (blockIdx.x == 0 && threadIdx.x < TR_WORDS) words[threadIdx.x] = threadIdx.x <= TR_W_BAD_LABEL ? TR_NO_ROW : 0;
}

// murmur3's 64-bit finaliser: neighbouring labels land far apart
__device__ __forceinline__ u64 tr_mix(u64 k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

// Adds `add` to the count of `key`, which takes the first free slot of its probe sequence when it has none.  A sequence that has
// passed every slot sets the overflow word: the host repeats the pair with a larger table.
__device__ __forceinline__ void tr_insert(ulonglong2 *__restrict__ table, u64 mask, u64 key, u64 add, i64 *__restrict__ words) {
    u64 s = tr_mix(key) & mask;
    for (u64 probes = 0; probes <= mask; ++probes, s = (s + 1) & mask) {
        u64 *slot = (u64 *)&table[s];
        u64 k = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == TR_EMPTY) {
            k = atomicCAS(slot, TR_EMPTY, key);
            if (k == TR_EMPTY) k = key;
        }
        if (k == key) {
            atomicAdd(slot + 1, add);               // its value is not used: the form without a return
            return;
        }
        // a long walk ends as soon as another one has found the table full
        if ((probes & 255) == 255 && __hip_atomic_load(&words[TR_W_OVERFLOW], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) return;
    }
    __hip_atomic_store(&words[TR_W_OVERFLOW], (i64)1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One lane per match row, rows row0 .. row0 + n of the pair in this launch.  Coord: the stored width of the coordinates; prev and
// next are (n, D) rows, D = 2: (y, x), 3: (z, y, x).  A coordinate at or beyond the frame's extent leaves the lowest such row (of the
// pair) in words[TR_W_BAD_COORD] and gathers nothing; a gathered label below 0 or above 2^31 - 1 the lowest such row in
// words[TR_W_BAD_LABEL].  Rows with a label of 0 at either end are counted in words[TR_W_DROPPED].  Matches come in raster order of
// the later frame, so neighbouring rows mostly share their key: within a wave the lane whose key differs from the lane's before it
// heads a run, and only heads touch the table, with the run's length -- one atomic add per run, not per row.  words[TR_W_HEADS]
// counts them.  Integer sums: the table's contents do not depend on the order of arrival.
template <typename Coord>
static __global__ __launch_bounds__(256) void tr_gather_count_kernel(const Coord *__restrict__ prev, const Coord *__restrict__ next, i64 n, i64 row0, int D,
                                                                     i64 nz, i64 ny, i64 nx, TrLabels A, TrLabels B, ulonglong2 *__restrict__ table,
                                                                     u64 mask, i64 *__restrict__ words) {
    const int lane = threadIdx.x & 63;
    i64 dropped = 0, heads = 0;       // of the wave, kept by every lane alike
    for (i64 base = (i64)blockIdx.x * 256; base < n; base += (i64)gridDim.x * 256) {
        const i64 r = base + threadIdx.x;
        u64 key = TR_EMPTY;
        bool zero = false;
        if (r < n) {
            const Coord *p = prev + r * D, *q = next + r * D;
            u64 pz = 0, qz = 0;
            if (D == 3) { pz = (u64)p[0]; qz = (u64)q[0]; }
            const u64 py = (u64)p[D - 2], px = (u64)p[D - 1], qy = (u64)q[D - 2], qx = (u64)q[D - 1];
            if (pz >= (u64)nz || py >= (u64)ny || px >= (u64)nx || qz >= (u64)nz || qy >= (u64)ny || qx >= (u64)nx) {
                atomicMin(&words[TR_W_BAD_COORD], row0 + r);
            } else {
                const i64 a = A[((i64)pz * ny + (i64)py) * nx + (i64)px], b = B[((i64)qz * ny + (i64)qy) * nx + (i64)qx];
                if (a < 0 || a > TR_MAX_LABEL || b < 0 || b > TR_MAX_LABEL) atomicMin(&words[TR_W_BAD_LABEL], row0 + r);
                else if (a == 0 || b == 0) zero = true;
                else key = ((u64)a << 32) | (u64)b;
            }
        }
        dropped += __popcll(__ballot(zero));
        const u64 before = __shfl_up(key, 1);
        const bool head = lane == 0 || key != before;
        const u64 hb = __ballot(head);
        heads += __popcll(__ballot(head && key != TR_EMPTY));
        // once a probe sequence has run through the table the pair is repeated anyway: the rest of the launch inserts nothing, or every
        // further head would walk all the slots of a full table
        const bool full = __hip_atomic_load(&words[TR_W_OVERFLOW], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
        if (head && key != TR_EMPTY && !full) {
            const u64 later = hb & ~((2ull << lane) - 1ull);          // the heads behind this lane (lane 63: none)
            const int len = (later ? __ffsll((long long)later) - 1 : 64) - lane;
            tr_insert(table, mask, key, (u64)len, words);
        }
    }
    if (lane == 0) {
        if (dropped) atomicAdd((u64 *)&words[TR_W_DROPPED], (u64)dropped);
        if (heads) atomicAdd((u64 *)&words[TR_W_HEADS], (u64)heads);
    }
}

// the occupied slots
struct TrOccupied {
    const ulonglong2 *table;
    __device__ __forceinline__ bool operator()(i64 s) const { return table[s].x != TR_EMPTY; }
};

// (key, count) of every occupied slot at its rank, one 16-byte store per entry.  The ballot is taken again from the slot the lane has
// loaded for its entry anyway.  Slot order: the host sorts the entries by key.
static __global__ __launch_bounds__(256) void tr_entries_write_kernel(const ulonglong2 *__restrict__ table, i64 slots, const int *__restrict__ pre,
                                                                     ulonglong2 *__restrict__ out) {
    const i64 s = (i64)blockIdx.x * 256 + threadIdx.x;
    const ulonglong2 e = s < slots ? table[s] : make_ulonglong2(TR_EMPTY, 0ull);
    const u64 b = __ballot(e.x != TR_EMPTY);
    if (e.x != TR_EMPTY) out[pre[s >> 6] + __popcll(b & ((1ull << (s & 63)) - 1ull))] = e;
}

// the largest label of a frame into *top (which starts at its lowest value): one atomic per wave
static __global__ __launch_bounds__(256) void tr_label_max_kernel(TrLabels L, i64 n, i64 *__restrict__ top) {
    i64 m = -TR_NO_ROW - 1;
    for (i64 i = (i64)blockIdx.x * 256 + threadIdx.x; i < n; i += (i64)gridDim.x * 256) {
        const i64 v = L[i];
        m = v > m ? v : m;
    }
    for (int w = 32; w > 0; w >>= 1) {
        const i64 o = __shfl_xor(m, w);
        m = o > m ? o : m;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(top, m);
}

__device__ __forceinline__ int tr_look(const int *__restrict__ lut, i64 n_lut, i64 v) { return v > 0 && v < n_lut ? lut[v] : 0; }

// out[i] = lut[L[i]] for labels in (0, n_lut), 0 elsewhere: four voxels per lane and step, 16-byte loads (two for int64 labels) and
// one 16-byte store; the last n % 4 voxels one by one.
template <bool WIDE>
static __global__ __launch_bounds__(256) void tr_relabel_kernel(const void *__restrict__ labels, i64 n, const int *__restrict__ lut, i64 n_lut,
                                                                int *__restrict__ out) {
    const i64 quads = n >> 2;
    for (i64 q = (i64)blockIdx.x * 256 + threadIdx.x; q < quads; q += (i64)gridDim.x * 256) {
        i64 v[4];
        if (WIDE) {
            const longlong2 lo = ((const longlong2 *)labels)[2 * q], hi = ((const longlong2 *)labels)[2 * q + 1];
            v[0] = lo.x; v[1] = lo.y; v[2] = hi.x; v[3] = hi.y;
        } else {
            const int4 w = ((const int4 *)labels)[q];
            v[0] = w.x; v[1] = w.y; v[2] = w.z; v[3] = w.w;
        }
        ((int4 *)out)[q] = make_int4(tr_look(lut, n_lut, v[0]), tr_look(lut, n_lut, v[1]), tr_look(lut, n_lut, v[2]), tr_look(lut, n_lut, v[3]));
    }
    const i64 i = quads * 4 + threadIdx.x;
    if (blockIdx.x == 0 && i < n) out[i] = tr_look(lut, n_lut, WIDE ? ((const i64 *)labels)[i] : (i64)((const int *)labels)[i]);
}
