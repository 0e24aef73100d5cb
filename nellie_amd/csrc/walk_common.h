// Part of libnellie_hip.so (gfx950): what the three walk kernels (hessian.inc, hessian_pair.inc, hessian_dpp.inc), the resolve kernel
// (resolve.inc) and the host that launches them (nellie_walk.hip, nellie_hv.hip, walk_plan.h) share.  After nl_common.h and device_math.inc.
#pragma once
struct VessP {
    float gamma_sq, alpha_sq, beta_sq;
    int use_thr;
    float thr;
    float max_abs, max_finite;
    int have_prev;           // 1: `pmask64` holds the AND of the h_masks of every earlier scale of this frame
    int cnt_lo, cnt_hi;      // planes whose masked voxels are counted, and whose statistics are taken (the owned ones)
    int first;               // 1: first evaluated scale of the frame (the host zeroes the vesselness volume before it)
    float fsq_min;           // h_mask <=> frob_sq >= fsq_min for finite frob_sq (exact: see mask_threshold_on_fsq)
    int m_inf;               // h_mask of a voxel whose frob_sq is +inf (frob := max finite, filtering.py:421-426)
    unsigned int *nan_flag;  // all_ones only: set when a Hessian with a NaN entry reaches the eigen-solver (the reference's LAPACK call raises there)
    int all_ones;            // Filter.run(mask=False): h_mask = ones_like(image) (filtering.py:566-567) -- NaN Hessians included, which no
                             // comparison with a threshold can express
    float fsq_lo, fsq_hi;    // MODE 2: bracket of the (not yet known) fsq_min
    int qcap;                // queue entries per wave region
    int zchunk;              // planes a workgroup marches (0: HM_ZCHUNK); a multiple of 8
    i64 idx_lo, idx_hi;      // resolve kernel: launch-relative voxel offsets of the counted planes
};

// a response > 0 needs trace < 0 and trace^2 >= frob_sq / 3
#define HM_TRACE_C 0.30f
// Queue entry: (h0..h5, voxel index) = 28 bytes, stored back to back (round 5; 32 bytes with a pad word before: an eighth fewer queue
// bytes written by the walk and read by the resolve kernel).  A region keeps its 32 x qcap bytes.  The 16 + 12 byte accesses
// are dword-aligned only, which global memory instructions of gfx950 take as they are (global_store_dwordx4 / dwordx3).
#define HM_ENT 28
struct __attribute__((packed, aligned(4))) QEnt4 { float a, b, c, d; };
struct __attribute__((packed, aligned(4))) QEnt3 { float a, b, c; };
__device__ __forceinline__ void qent_store(float4 *region, unsigned int slot, float h0, float h1, float h2, float h3, float h4, float h5, unsigned int idx) {
    char *e = reinterpret_cast<char *>(region) + (size_t)__umul24(slot, (unsigned int)HM_ENT);       // slot < 2^24 (qcap): a full-rate multiply
    *reinterpret_cast<QEnt4 *>(e) = QEnt4{h0, h1, h2, h3};
    *reinterpret_cast<QEnt3 *>(e + 16) = QEnt3{h4, h5, __uint_as_float(idx)};
}
__device__ __forceinline__ void qent_load(const float4 *region, unsigned int slot, float4 &a, float4 &b) {
    const char *e = reinterpret_cast<const char *>(region) + (size_t)slot * (size_t)HM_ENT;
    const QEnt4 x = *reinterpret_cast<const QEnt4 *>(e); const QEnt3 y = *reinterpret_cast<const QEnt3 *>(e + 16);
    a = make_float4(x.a, x.b, x.c, x.d); b = make_float4(y.a, y.b, y.c, 0.0f);
}
// ... as ONE comparison: trace |trace| + 0.30 frob_sq < 0 (a ballot less per voxel than the two-sided form: the walk is short of SGPRs)
#ifdef HM_TRACE_ALL       // (test build: every masked voxel is queued and solved; tools/soak_crc.py compares the frames of the two builds)
#define HM_TRACE_OK(tr, fsq) (true)
#else
// A frob_sq that overflowed float32 (+inf, or NaN) says nothing about the trace: such a voxel is solved (its eigenvalues are taken in
// float64 from finite components and can give a response > 0: tools/probe_overflow.py, volumes scaled by 1e16 ... 1e17).  The pair
// walk applies the clause in MODE 1 only: a MODE 2 pass that meets an inf is discarded and redone in MODE 1 (pipeline.py, chain.inc).
#define HM_TRACE_OK(tr, fsq) (((tr) * fabsf(tr) + HM_TRACE_C * (fsq) < 0.0f) || !((fsq) < __int_as_float(0x7f800000)))
#endif
#define HM_TX 64
#define HM_SLOTS 8                    // Z-loop unroll (ring and buffer indices are compile-time inside a group)
#ifndef HM_ZCHUNK
#define HM_ZCHUNK 64
#endif
#define HM_DEPTH 4         // planes in flight in registers; divides HM_SLOTS so that the unrolled loop indexes them statically
#define HM_REGION (HM_ZCHUNK * 64)     // queue entries a wave can produce
#define HM_SPEC_CAP (HM_ZCHUNK * 32)    // MODE 2: entries per region (half the worst case; overflow -> MODE 1)
#define HM_UNDECIDED 0x80000000u       // MODE 2: idx flag of a voxel whose h_mask the resolve kernel decides
// slot of plane zz in the 4-slot LDS ring of raw planes (the one-voxel and the pair kernel; zc0: the chunk's first plane)
#define HG_RSLOT(zz) ((int)(((unsigned)((zz) - zc0 + 8)) & 3u))

// A constant float32 divisor, two exact implementations of a/d:
//  FAST : q = a*y; r = fma(-q,d,a); q' = fma(r,y,q) with y = RN(1/d) -- three float32 instructions.  This
//         sequence is correctly rounded for most but not all d, so nl_hessian_stats PROVES it for the
//         six divisors in use by exhaustion (divcheck_kernel: all 2^23 significands; scaling a by 2^k
//         scales q, r, q' exactly, so one binade covers every normal a) before selecting this path.
//  !FAST: (float)((double)a * RN64(1/d)), exact for every d (see div_c).
//  TWO  : q' = fma(a, yh, a*yl) with yh = RN(1/d), yl = RN(1/d - yh) (Brisebarre & Muller, "Correctly rounded multiplication
//         by arbitrary precision constants") -- two float32 instructions, again exact for most d only and PROVEN the same way
//         before it is selected (FAST = 2; the pair kernel alone has this variant).  One binade again covers every a whose
//         partial product a*yl stays normal (|a| > ~1e-31 / |yl|); below that the sequence can differ in the last bit, like the
//         sub-normal quotients of FAST -- differences of float32 image values are 0 or many orders of magnitude above it.
template <int FAST> struct Dv;
template <> struct Dv<1> {
    float d, y;
    __device__ __forceinline__ float div(float a) const { const float q = a * y; const float r = fmaf(-q, d, a); return fmaf(r, y, q); }
};
template <> struct Dv<2> {
    float yl, y;
    __device__ __forceinline__ float div(float a) const { return fmaf(a, y, a * yl); }
};
template <> struct Dv<0> {
    double r;
    __device__ __forceinline__ float div(float a) const { return (float)((double)a * r); }
};
template <int FAST> struct HessDv { Dv<FAST> z, y, x, z2, y2, x2; };   // float32(h) and float32(2h) per axis

// Global queue of voxels to solve.  Entry e = two float4: (h0,h1,h2,h3), (h4,h5,idx,-) with idx the voxel offset
// relative to the first plane of the launch.  Wave w of workgroup b owns entries [r*HM_REGION, (r+1)*HM_REGION)
// with r = b*waves_per_group + w and reports how many it wrote in count[r].
struct VQueue {
    float4 *ent;
    unsigned int *count;
};

template <int M>
__global__ void __launch_bounds__(256)
divcheck_kernel(Dv<M> dv, float d, unsigned int *__restrict__ bad) {
    const unsigned int i = blockIdx.x * 256u + threadIdx.x;               // 2^23 significands of [1,2)
    const float a = __uint_as_float(0x3f800000u | i);
    if (dv.div(a) != a / d || dv.div(-a) != -a / d) atomicOr(bad, 1u);
}
