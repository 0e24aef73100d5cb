// Part of libnellie_hip.so (gfx950): included by nellie_hv.hip after walk_common.h (VessP, VQueue, Dv, HessDv, HM_*).
// =================================================================================================
// Hessian walk, two voxels per thread (rows y and y + RS of the tile), packed float32 arithmetic
// =================================================================================================
// Same algorithm, same modes, same outputs as hessian_g_kernel (see hessian.inc) -- bit for bit: every float32
// operation is the same IEEE operation, only issued as v_pk_{add,mul,fma}_f32 on the PAIR (voxel A, voxel B).
//
// Why: measured on this part (tools/ubench/valu_issue.hip) a wave issues at most one instruction every ~4.9 cycles
// whatever its kind (VALU, SALU, LDS), a SIMD about one every 1.65 cycles with four waves, and a packed float32
// operation costs 2.7 cycles for two results against 2 x 1.7.  hessian_g_kernel ran ~140 instructions per wave and
// plane (one barrier per plane, 630 SIMD cycles per wave-plane measured against 231 of pure issue): the walk is bound
// by the LENGTH of each wave's instruction stream between two barriers and by the latencies it cannot cover with one
// dependent chain per lane.  Two voxels per lane halve the instructions per voxel (address arithmetic, LDS
// instructions, ballots' bookkeeping, the loop itself, the barrier) and give every lane two independent chains.
//
// Data layout: EVERYTHING that lives in LDS is stored as the pair.  A workgroup of 64 x RS threads owns a tile of
// TY = 2 RS rows x 64 columns; thread (lx, ly) owns rows ly and ly + RS ("pair-row" ly).
//   raw ring   [4][RS + 4][68] float2 : pair-row p in [-2, RS + 2) holds (I(row p), I(row p + RS)); the four rows around
//                                        row RS are therefore staged twice (once per component)
//   gradients  [2][RS + 2][66] float4 (gz_A, gz_B, gy_A, gy_B) + [2][RS + 2][66] float2 (gx_A, gx_B), pair-rows -1 .. RS:
//                                        the halo pair-rows hold (g(row -1), g(row RS - 1)) and (g(row RS), g(row TY))
// so every operand of every packed instruction arrives as one aligned 64-bit register pair straight from a
// ds_read_b64 / ds_read_b128 -- no lane shuffles, no operand-pairing moves (what made the SLP-vectorised build of
// hessian_g_kernel slower).  All LDS addresses of the second stage are the thread's own tile position +- a constant:
//   * X faces and tiles that stick out of the volume in X: raw columns are loaded with clamped indices, and every
//     gradient element (own or halo) is evaluated AT ITS CLAMPED COLUMN, so "the neighbour of a face voxel is the voxel
//     itself" (np.gradient's one-sided formula) is what the tile holds (+ the divisor select);
//   * Y faces cannot be done that way (the two components of a pair would need different addresses), so tiles that
//     touch a Y face -- 2 tile rows of ny / TY -- take a workgroup-uniform branch that re-reads the own gradient and
//     selects it per component;
//   * Z faces: the rolled (non-unrolled) step with clamped plane slots, as in hessian_g_kernel.
// Queue: wave w of workgroup b owns region b * RS + w with room for 2 x the entries of a 64-voxel row segment.
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));
__device__ __forceinline__ v2f fma2(v2f a, v2f b, v2f c) { return __builtin_elementwise_fma(a, b, c); }

// Division of a pair by ONE wave-uniform constant (both components): the constant lives in SGPRs and the packed
// instructions broadcast it (op_sel), so divisors cost no vector registers at all.  Faces: np.gradient divides by h
// instead of 2h there, and RN(a / h) = 2 RN(a / 2h) exactly (a power-of-two scaling; sub-normal quotients excepted, as
// everywhere in this file), so every lane divides by 2h and the face lanes double the quotient -- inside
// workgroup-uniform branches that only the tiles touching a face of the volume ever enter.
template <int FAST> struct Dv1;
template <> struct Dv1<1> {
    float d, y;
    __device__ __forceinline__ v2f div(v2f a) const {
        const v2f ys = v2f{y, y}, ds = v2f{d, d};
        const v2f q = a * ys; const v2f r = fma2(-q, ds, a); return fma2(r, ys, q);
    }
};
template <> struct Dv1<2> {               // two packed instructions: fma(a, yh, a * yl), see hessian.inc
    float yl, y;
    __device__ __forceinline__ v2f div(v2f a) const {
        const v2f ys = v2f{y, y}, ls = v2f{yl, yl};
        return fma2(a, ys, a * ls);
    }
};
template <> struct Dv1<0> {
    double r;
    __device__ __forceinline__ v2f div(v2f a) const { v2f o; o.x = (float)((double)a.x * r); o.y = (float)((double)a.y * r); return o; }
};
// several independent divisions issued in lockstep (a dependent packed operation straight behind its producer costs a
// wait state; in source order the scheduler finds the interleaving more reliably)
template <int FAST>
__device__ __forceinline__ void div3(const Dv1<FAST> &d0, v2f &a0, const Dv1<FAST> &d1, v2f &a1, const Dv1<FAST> &d2, v2f &a2) {
    if constexpr (FAST == 2) {
        const v2f y0 = v2f{d0.y, d0.y}, y1 = v2f{d1.y, d1.y}, y2 = v2f{d2.y, d2.y};
        const v2f l0 = v2f{d0.yl, d0.yl}, l1 = v2f{d1.yl, d1.yl}, l2 = v2f{d2.yl, d2.yl};
        const v2f t0 = a0 * l0, t1 = a1 * l1, t2 = a2 * l2;
        a0 = fma2(a0, y0, t0); a1 = fma2(a1, y1, t1); a2 = fma2(a2, y2, t2);
    } else if constexpr (FAST == 1) {
        const v2f y0 = v2f{d0.y, d0.y}, y1 = v2f{d1.y, d1.y}, y2 = v2f{d2.y, d2.y};
        const v2f e0 = v2f{d0.d, d0.d}, e1 = v2f{d1.d, d1.d}, e2 = v2f{d2.d, d2.d};
        const v2f q0 = a0 * y0, q1 = a1 * y1, q2 = a2 * y2;
        const v2f r0 = fma2(-q0, e0, a0), r1 = fma2(-q1, e1, a1), r2 = fma2(-q2, e2, a2);
        a0 = fma2(r0, y0, q0); a1 = fma2(r1, y1, q1); a2 = fma2(r2, y2, q2);
    } else { a0 = d0.div(a0); a1 = d1.div(a1); a2 = d2.div(a2); }
}
__device__ __forceinline__ Dv1<1> dv1_of(const Dv<1> &a) { return Dv1<1>{a.d, a.y}; }
__device__ __forceinline__ Dv1<2> dv1_of(const Dv<2> &a) { return Dv1<2>{a.yl, a.y}; }
__device__ __forceinline__ Dv1<0> dv1_of(const Dv<0> &a) { return Dv1<0>{a.r}; }
__device__ __forceinline__ void dbl_if(v2f &q, bool cx, bool cy) { q.x = cx ? q.x + q.x : q.x; q.y = cy ? q.y + q.y : q.y; }

// m = max(m, |a|, |b|) in one instruction (fmaxf on the results of packed operations draws a canonicalising v_max per
// operand from the compiler; the hardware instruction ignores NaN operands exactly like fmaxf)
__device__ __forceinline__ void max3_abs(float &m, float a, float b) { asm("v_max3_f32 %0, %0, |%1|, |%2|" : "+v"(m) : "v"(a), "v"(b)); }
__device__ __forceinline__ void max3_f(float &m, float a, float b) { asm("v_max3_f32 %0, %0, %1, %2" : "+v"(m) : "v"(a), "v"(b)); }

// alive words of plane UU into lanes 8 k + UU of the pair (alo, ahi): constant lane numbers, one v_writelane each
template <int UU, int K>
__device__ __forceinline__ void hv_put(int &alo, int &ahi, const unsigned long long (&a)[K]) {
    if constexpr (K >= 1) { asm("v_writelane_b32 %0, %1, %2" : "+v"(alo) : "s"((int)(unsigned int)a[0]), "n"(UU)); asm("v_writelane_b32 %0, %1, %2" : "+v"(ahi) : "s"((int)(unsigned int)(a[0] >> 32)), "n"(UU)); }
    if constexpr (K >= 2) { asm("v_writelane_b32 %0, %1, %2" : "+v"(alo) : "s"((int)(unsigned int)a[1]), "n"(8 + UU)); asm("v_writelane_b32 %0, %1, %2" : "+v"(ahi) : "s"((int)(unsigned int)(a[1] >> 32)), "n"(8 + UU)); }
    if constexpr (K >= 3) { asm("v_writelane_b32 %0, %1, %2" : "+v"(alo) : "s"((int)(unsigned int)a[2]), "n"(16 + UU)); asm("v_writelane_b32 %0, %1, %2" : "+v"(ahi) : "s"((int)(unsigned int)(a[2] >> 32)), "n"(16 + UU)); }
    if constexpr (K >= 4) { asm("v_writelane_b32 %0, %1, %2" : "+v"(alo) : "s"((int)(unsigned int)a[3]), "n"(24 + UU)); asm("v_writelane_b32 %0, %1, %2" : "+v"(ahi) : "s"((int)(unsigned int)(a[3] >> 32)), "n"(24 + UU)); }
}

// Queue entries straight from the pairs: v_pk_mov_b32 picks the A (low) or B (high) halves of two pair registers into one aligned register
// pair, so a voxel's six components reach the registers of its two wide stores in three instructions instead of six moves.
__device__ __forceinline__ v2f pk_lo(v2f a, v2f b) { v2f r; asm("v_pk_mov_b32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,0]" : "=v"(r) : "v"(a), "v"(b)); return r; }
__device__ __forceinline__ v2f pk_hi(v2f a, v2f b) { v2f r; asm("v_pk_mov_b32 %0, %1, %2 op_sel:[1,1] op_sel_hi:[1,1]" : "=v"(r) : "v"(a), "v"(b)); return r; }
template <int HI>
__device__ __forceinline__ void qent_store_pairs(float4 *region, unsigned int slot, v2f h0, v2f h1, v2f h2, v2f h3, v2f h4, v2f h5, unsigned int idx) {
    const v2f a = HI ? pk_hi(h0, h1) : pk_lo(h0, h1), b = HI ? pk_hi(h2, h3) : pk_lo(h2, h3), c = HI ? pk_hi(h4, h5) : pk_lo(h4, h5);
    char *e = reinterpret_cast<char *>(region) + (size_t)__umul24(slot, (unsigned int)HM_ENT);
    *reinterpret_cast<QEnt4 *>(e) = QEnt4{a.x, a.y, b.x, b.y};
    *reinterpret_cast<QEnt3 *>(e + 16) = QEnt3{c.x, c.y, __uint_as_float(idx)};
}

#define HV_RP (HM_TX + 4)              // raw tile pitch (pair elements)
#define HV_GP (HM_TX + 2)              // gradient tile pitch
#ifndef HV_DEPTH
#define HV_DEPTH 1                     // planes in flight in registers; divides HM_SLOTS (2 cost registers: measured slower, see DESIGN)
#endif
// Order of a step (round 4): the raw plane in flight lands in LDS and the next plane's loads go out BEFORE the step's queue stores -- the loads
// have a whole step to arrive, and the landing's vmcnt(0) does not wait for the stores (1.397 vs 1.456 ms per launch at 512 x 1024 x 1024
// against "landing + loads at the end of the step"; the third order, loads after the stores, lay between: docs/HISTORY.md).
// NP = pair-rows per lane: 1 (two voxels per lane, 64 x RS threads) or 2 (FOUR voxels per lane: thread (lx, ly) owns pair-rows
// 2 ly and 2 ly + 1, i.e. rows 2 ly, 2 ly + 1, 2 ly + RS, 2 ly + 1 + RS of the same tile; 64 x RS / 2 threads, the LDS layout unchanged)
template <int RS, int NP = 1> struct HVCfg {
    static constexpr int NT = HM_TX * RS / NP, TY = 2 * RS;
    static constexpr int RPLANE = HV_RP * (RS + 4);
    static constexpr int GPLANE = HV_GP * (RS + 2);
    static constexpr int NHALO = 2 * HM_TX + 2 * RS;
    static constexpr int NJ = (RPLANE + NT - 1) / NT;       // pair elements a thread stages per plane
    static constexpr int RSLOT = NJ * NT;                    // slot pitch: every thread writes NJ elements, no predicate
    static constexpr int lds_bytes() { return 2 * GPLANE * 24 + 4 * RSLOT * 8 + 256; }
};

template <int MODE, int RS, int FAST, int NP = 1>
#ifndef HV_WAVES
#define HV_WAVES 4
#endif
__global__ void __launch_bounds__(HM_TX * RS / NP, HV_WAVES / NP)
hessian_v_kernel(const float *__restrict__ g, unsigned long long *__restrict__ cmask64,
                 const unsigned long long *__restrict__ pmask64, int wpr,
                 VolGeom v, HessDv<FAST> hr, VessP vp, VQueue vq, int z0, int z1, int ntx, int nty,
                 unsigned int *__restrict__ res, unsigned long long *__restrict__ mask_count, const float *__restrict__ dev_lohi) {
    // MODE 2 inside a device-resident threshold chain (chain.inc): the bracket was decided by a kernel, not by the host
    const float fsq_lo_ = (MODE == 2 && dev_lohi) ? dev_lohi[0] : vp.fsq_lo, fsq_hi_ = (MODE == 2 && dev_lohi) ? dev_lohi[1] : vp.fsq_hi;
    constexpr int NT = HVCfg<RS, NP>::NT, TY = HVCfg<RS, NP>::TY, RPLANE = HVCfg<RS, NP>::RPLANE, GPLANE = HVCfg<RS, NP>::GPLANE;
    constexpr int NHALO = HVCfg<RS, NP>::NHALO, NJ = HVCfg<RS, NP>::NJ, RSLOT = HVCfg<RS, NP>::RSLOT;
    constexpr int NW = RS / NP;                              // waves of the workgroup
    static_assert(NHALO <= NT, "one halo element per thread");
    constexpr int RP = HV_RP, GP = HV_GP;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    v2f *ga = (v2f *)smem;                                   // [2][GPLANE][2]: (gz_A, gz_B), (gy_A, gy_B) -- read as two v2f so that
                                                             // the differences are packed operations (a v4f subtraction is scalarised)
    v2f *gx = ga + 4 * GPLANE;                               // [2][GPLANE] (gx_A, gx_B)
    v2f *rp = gx + 2 * GPLANE;                               // [4][RSLOT] raw pair planes
    float *s_red = (float *)(rp + 4 * RSLOT);                // 64 floats of reduction scratch
    const int tid = threadIdx.x;
    const int lx = tid & 63, ly = tid >> 6;
    const unsigned nblk = gridDim.x;
    unsigned bid = blockIdx.x;
    if ((nblk & 7u) == 0u) bid = (bid & 7u) * (nblk >> 3) + (bid >> 3);     // XCD-aware remap (speed only)
    const int tx = bid % ntx;
    const int ty = (bid / ntx) % nty;
    const int zc = bid / (ntx * nty);
    // wave-uniform by construction; saying so once keeps everything derived from them (plane slots, the scalar offsets of
    // the buffer loads, the loop itself) in SGPRs
    const int zch = vp.zchunk > 0 ? vp.zchunk : HM_ZCHUNK;
    const int zc0 = __builtin_amdgcn_readfirstlane(z0 + zc * zch);
    const int zc1 = (zc0 + zch < z1) ? zc0 + zch : z1;
    const int nx = (int)v.nx, ny = (int)v.ny;
    const i64 sz = v.ny * v.nx;
    const int gz0 = (int)v.gz0, gnz = (int)v.gnz;
    const int xbase = tx * HM_TX - 2, ybase = ty * TY - 2;      // tile coordinates of raw element (pair-row -2, col -2)
    const int x = xbase + 2 + lx, yA = ybase + 2 + ly * NP, yB = yA + RS;     // rows of pair-row q: yA + q, yB + q
    // uniform per workgroup: every voxel of the tile exists / some row of the tile is a Y face of the volume
    const bool all_valid = (tx * HM_TX + HM_TX <= nx) && (ty * TY + TY <= ny);
    const bool yface = (ty == 0) || (ty * TY + TY + 1 >= ny);

    auto clampi = [](int q, int n) -> int { return q < 0 ? 0 : (q > n - 1 ? n - 1 : q); };
    // raw pair elements this thread stages per plane: element e = tid + j*NT -> pair-row e / RP - 2, column e % RP - 2;
    // byte offsets inside a plane (a plane holds < 2^30 voxels: see nl_ctx_create)
    unsigned int offA[NJ], offB[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int e = tid + j * NT;
        const int ee = e < RPLANE ? e : tid;                // past the tile: re-read the first element (lands in the slot's padding)
        const int pr = ee / RP, pc = ee % RP;
        const int xx = clampi(xbase + pc, nx);
        offA[j] = (unsigned int)(clampi(ybase + pr, ny) * nx + xx) * 4u;
        offB[j] = (unsigned int)(clampi(ybase + pr + RS, ny) * nx + xx) * 4u;
    }
    auto zclamp = [&](int zz) -> int {
        const int gg = gz0 + zz;
        return gg < 0 ? -gz0 : (gg > gnz - 1 ? gnz - 1 - gz0 : zz);
    };
    auto face = [&](int q, int n) -> bool { return q == 0 || q == n - 1; };

    // gradient elements: the thread's own pair and (tid < NHALO) one pair of the cross halo.  Columns are evaluated at
    // their clamped position (see the header); G offset = (pair-row + 1) * GP + col + 1, raw = (pair-row + 2) * RP + col + 2.
    const int xc = x < nx ? x : nx - 1;
    const int r_own = (ly * NP + 2) * RP + (xc - xbase), g_own = (ly * NP + 1) * GP + lx + 1;    // pair-row q: + q * RP, + q * GP
    int hpr = 0, hcol = 0;
    if (tid < HM_TX) { hpr = -1; hcol = tid; }
    else if (tid < 2 * HM_TX) { hpr = RS; hcol = tid - HM_TX; }
    else if (tid < 2 * HM_TX + RS) { hpr = tid - 2 * HM_TX; hcol = -1; }
    else if (tid < NHALO) { hpr = tid - 2 * HM_TX - RS; hcol = HM_TX; }
    const int hx = clampi(xbase + 2 + hcol, nx);
    const int r_halo = (hpr + 2) * RP + (hx - xbase), g_halo = (hpr + 1) * GP + hcol + 1;
    const int hyA = ybase + 2 + hpr, hyB = hyA + RS;
    const Dv1<FAST> dz_in = dv1_of(hr.z2), dy_in = dv1_of(hr.y2), dx_in = dv1_of(hr.x2);
    // uniform: the tile (its halo included) touches an X / a Y face of the volume
    const bool xface = (tx == 0) || (tx * HM_TX + HM_TX + 1 >= nx);

    struct G6 { v2f z, y, x; };
    // first derivatives of a plane at raw offset r, from the raw pair planes below / at / above it; (ya, yb, xq) = the
    // rows and the (clamped) column the element stands for
    // Faces in Y / X: the quotient by 2h, doubled (header).  The doubling is a multiplication by a per-element factor 1.0 / 2.0
    // (exact either way); which elements sit on a face does not change along the march, so the factors are formed once per
    // thread and the edge copy of the loop carries them as ONE register of bits (fbits: bit 0 own column, bits 1-3 the halo
    // element's column / row A / row B; the own rows are wave-uniform: scalars) instead of re-deriving three lane masks with
    // compares in each of the three places of every step that need them -- 285 instead of 322 instructions per edge step.
    auto fac_of_bit = [](unsigned int bits, int k) -> float { return __uint_as_float(0x3f800000u + (((bits >> k) & 1u) << 23)); };
    auto grad_at = [&](const v2f *Pm, const v2f *P0, const v2f *Pp, const int r, const Dv1<FAST> &dz, const v2f fy, const float fx, auto ec) -> G6 {
        v2f gzv = Pp[r] - Pm[r], gyv = P0[r + RP] - P0[r - RP], gxv = P0[r + 1] - P0[r - 1];
        div3(dz, gzv, dy_in, gyv, dx_in, gxv);
        if (decltype(ec)::value) { gyv = gyv * fy; gxv = gxv * v2f{fx, fx}; }
        return G6{gzv, gyv, gxv};
    };
    const unsigned int fbits = (face(xc, nx) ? 1u : 0u) | (face(hx, nx) ? 2u : 0u) | (face(hyA, ny) ? 4u : 0u) | (face(hyB, ny) ? 8u : 0u);
    const int yuA_ = __builtin_amdgcn_readfirstlane(yA);                     // the own rows are the same for the whole wave
    float ofyA[NP], ofyB[NP];
#pragma unroll
    for (int q = 0; q < NP; ++q) { ofyA[q] = face(yuA_ + q, ny) ? 2.0f : 1.0f; ofyB[q] = face(yuA_ + q + RS, ny) ? 2.0f : 1.0f; }
    // Raw planes are fetched with buffer loads: resource = the planes [pmin, pmax] this chunk touches (< 4 GiB, checked by
    // the launcher), per-lane byte offset inside a plane in a VGPR, the plane in the scalar offset -- one instruction
    // per load, no 64-bit address arithmetic, and the compiler counts them (vmcnt) like any other load.
    const int pmin = zclamp(zc0 - 2), pmax = zclamp(zc1 + 1);
    const unsigned int plane_bytes = (unsigned int)sz * 4u;
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void *)(g + (i64)pmin * sz), 0, (int)((unsigned int)(pmax - pmin + 1) * plane_bytes), 0x00020000);
    auto ldg = [&](unsigned int soff, unsigned int boff) -> float {
        // soff is wave-uniform by construction; saying so keeps it in an SGPR (a VGPR here makes every load a waterfall loop)
        return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)boff, __builtin_amdgcn_readfirstlane((int)soff), 0));
    };
    auto stage_plane = [&](v2f *dst, int pz) {     // prologue only: global -> LDS directly
        const unsigned int so = (unsigned int)(pz - pmin) * plane_bytes;
#pragma unroll
        for (int j = 0; j < NJ; ++j) dst[tid + j * NT] = v2f{ldg(so, offA[j]), ldg(so, offB[j])};
    };

    // ---- prologue: planes zc0-2 .. zc0+1, the gradient tile of plane zc0, the own Z derivatives of zc0-1 and zc0
    for (int pz = pmin; pz <= pmax && pz <= zc0 + 1; ++pz) stage_plane(rp + HG_RSLOT(pz) * RSLOT, pz);
    __syncthreads();
    v2f gz_m1[NP], gz_c[NP];                   // d/dz at the own voxels on planes z-1 and z
    {
        const v2f *Pm2 = rp + HG_RSLOT(zclamp(zc0 - 2)) * RSLOT, *Pm1 = rp + HG_RSLOT(zclamp(zc0 - 1)) * RSLOT;
        const v2f *P0 = rp + HG_RSLOT(zc0) * RSLOT, *Pp1 = rp + HG_RSLOT(zclamp(zc0 + 1)) * RSLOT;
        const Dv1<FAST> dzm = dv1_of(face(gz0 + zc0 - 1, gnz) ? hr.z : hr.z2), dz0 = dv1_of(face(gz0 + zc0, gnz) ? hr.z : hr.z2);
#pragma unroll
        for (int q = 0; q < NP; ++q) {
            gz_m1[q] = dzm.div(P0[r_own + q * RP] - Pm2[r_own + q * RP]);
            const G6 G = grad_at(Pm1, P0, Pp1, r_own + q * RP, dz0, v2f{ofyA[q], ofyB[q]}, fac_of_bit(fbits, 0), std::true_type{});
            gz_c[q] = G.z;
            ga[2 * (g_own + q * GP)] = G.z; ga[2 * (g_own + q * GP) + 1] = G.y; gx[g_own + q * GP] = G.x;                       // buffer 0
        }
        if (tid < NHALO) {
            const G6 H = grad_at(Pm1, P0, Pp1, r_halo, dz0, v2f{fac_of_bit(fbits, 2), fac_of_bit(fbits, 3)}, fac_of_bit(fbits, 1), std::true_type{});
            ga[2 * g_halo] = H.z; ga[2 * g_halo + 1] = H.y; gx[g_halo] = H.x;
        }
    }
    __syncthreads();
    if (zc0 + 2 <= pmax) stage_plane(rp + HG_RSLOT(zc0 + 2) * RSLOT, zc0 + 2);      // takes the slot of zc0-2
    float ra[HV_DEPTH][NJ], rb[HV_DEPTH][NJ];          // planes z+3 .. z+3+HV_DEPTH-1 in flight
#pragma unroll
    for (int d = 0; d < HV_DEPTH; ++d) {
        const int pz = zc0 + 3 + d;
        const unsigned int so = (unsigned int)((pz < pmax ? pz : pmax) - pmin) * plane_bytes;
#pragma unroll
        for (int j = 0; j < NJ; ++j) { ra[d][j] = ldg(so, offA[j]); rb[d][j] = ldg(so, offB[j]); }
    }
    __syncthreads();

    float mabs = 0.0f, mabs2 = 0.0f, mfrob = 0.0f;       // two chains for max |H|: consecutive updates do not wait for each other
    int anyinf = 0;
    const int lane = tid & 63;
    const int yuA = __builtin_amdgcn_readfirstlane(yA), yuB = yuA + RS;
    // mask rows of the wave, k = 2 q + (0: A, 1: B)
    bool row_ok[2 * NP];
    i64 wordr[2 * NP];
#pragma unroll
    for (int k = 0; k < 2 * NP; ++k) {
        const int yr = (k & 1 ? yuB : yuA) + (k >> 1);
        row_ok[k] = yr < ny;
        wordr[k] = (i64)(row_ok[k] ? yr : 0) * wpr + tx;
    }
    const i64 wplane = (i64)ny * wpr;
    const unsigned int region = (bid * (unsigned)NW + (unsigned)__builtin_amdgcn_readfirstlane(ly));
    float4 *qent = MODE != 0 ? vq.ent + (size_t)region * (size_t)vp.qcap * 2 : nullptr;
    unsigned int qn = 0;
    unsigned int cnt = 0;
    const unsigned long long no_prev = vp.have_prev ? 0ull : ~0ull;
    const unsigned int plane_u = (unsigned int)sz;
    const unsigned int idx_rowA = (unsigned int)(yA * nx + x), idx_rowB = (unsigned int)(yB * nx + x);      // pair-row q: + q * nx
    // lane k*8 + u of a wave fetches / writes the mask word of row k (A, B of pair-row 0, then of pair-row 1), plane z + u of an unrolled group
    i64 word_lane = wordr[0];
    bool row_lane_ok = row_ok[0];
#pragma unroll
    for (int k = 1; k < 2 * NP; ++k) if ((lane >> 3) == k) { word_lane = wordr[k]; row_lane_ok = row_ok[k]; }
    const float f_inf = __int_as_float(0x7f800000);

    // One plane step.  U >= 0: compile-time ring / buffer indices, every plane involved is interior in Z.
    // prevA / prevB: cumulative mask words of the earlier scales for the two rows; returns the new words through aliveA/B.
    // E (compile time): the tile touches a face of the volume in X or Y or sticks out of it -- the unrolled loop exists
    // twice, and the copy the interior tiles run has none of the face handling in it.
    // prev[k] / alive[k]: mask words of row k = 2 q + (0: A, 1: B)
    auto step = [&](const int z, auto uc, auto ec, const unsigned long long (&prev)[2 * NP], unsigned long long (&alive)[2 * NP]) {
        constexpr int U = decltype(uc)::value;
        constexpr bool E = decltype(ec)::value;
        // the second stage's operands (gradient tile of plane z, complete since the last barrier) are requested FIRST: their
        // LDS latency then passes behind the first stage instead of being exposed a second time in the middle of the step
        const int b0 = ((U >= 0) ? (U & 1) : ((z - zc0) & 1)) * GPLANE;
        // ---- stage A: first derivatives of plane z+1 (tile + halo) into buffer (z+1-zc0)&1
        v2f gz_p1[NP];
        {
            const v2f *Pm, *P0, *Pp;
            Dv1<FAST> dz1;
            int b1;
            if (U >= 0) {
                Pm = rp + (U & 3) * RSLOT; P0 = rp + ((U + 1) & 3) * RSLOT; Pp = rp + ((U + 2) & 3) * RSLOT;
                dz1 = dz_in;
                b1 = ((U + 1) & 1) * GPLANE;
            } else {
                Pm = rp + HG_RSLOT(zclamp(z)) * RSLOT; P0 = rp + HG_RSLOT(zclamp(z + 1)) * RSLOT;
                Pp = rp + HG_RSLOT(zclamp(z + 2)) * RSLOT;
                dz1 = dv1_of(face(gz0 + z + 1, gnz) ? hr.z : hr.z2);
                b1 = ((z + 1 - zc0) & 1) * GPLANE;
            }
            unsigned int fb = fbits;
            if (E) asm volatile("" : "+v"(fb));             // the factors are re-formed from the bits where they are used: hoisted, they would
                                                            // each hold a register across the loop
#pragma unroll
            for (int q = 0; q < NP; ++q) {
                const G6 G = grad_at(Pm, P0, Pp, r_own + q * RP, dz1, v2f{ofyA[q], ofyB[q]}, fac_of_bit(fb, 0), ec);
                gz_p1[q] = G.z;
                ga[2 * (b1 + g_own + q * GP)] = G.z; ga[2 * (b1 + g_own + q * GP) + 1] = G.y; gx[b1 + g_own + q * GP] = G.x;
            }
            if (tid < NHALO) {
                const G6 H = grad_at(Pm, P0, Pp, r_halo, dz1, v2f{fac_of_bit(fb, 2), fac_of_bit(fb, 3)}, fac_of_bit(fb, 1), ec);
                ga[2 * (b1 + g_halo)] = H.z; ga[2 * (b1 + g_halo) + 1] = H.y; gx[b1 + g_halo] = H.x;
            }
        }
        // scalar offset of the plane that goes in flight now (clamped to pmax: past the chunk's end a harmless re-read), from the
        // step's own plane number: scalar arithmetic, nothing carried round the loop (a loop-carried offset ended up as VALU
        // arithmetic on a VGPR copy + v_readfirstlane + 5 wait states in front of the loads of every plane)
        const unsigned int pf = (unsigned int)((z + 3 + HV_DEPTH < pmax ? z + 3 + HV_DEPTH : pmax) - pmin) * plane_bytes;
        auto land = [&]() {                 // registers of the oldest plane in flight -> its ring slot
            if (U >= 0) {
                constexpr int R = (U >= 0 ? U : 0) % HV_DEPTH;
                v2f *dst = rp + ((U + 3) & 3) * RSLOT;
#pragma unroll
                for (int j = 0; j < NJ; ++j) dst[tid + j * NT] = v2f{ra[R][j], rb[R][j]};
            } else {
                if (z + 3 <= pmax) {
                    v2f *dst = rp + HG_RSLOT(z + 3) * RSLOT;
#pragma unroll
                    for (int j = 0; j < NJ; ++j) dst[tid + j * NT] = v2f{ra[0][j], rb[0][j]};
                }
#pragma unroll
                for (int d = 0; d + 1 < HV_DEPTH; ++d)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) { ra[d][j] = ra[d + 1][j]; rb[d][j] = rb[d + 1][j]; }
            }
        };
        auto fetch = [&]() {                // its registers take the next plane
            constexpr int R = (U >= 0) ? ((U >= 0 ? U : 0) % HV_DEPTH) : (HV_DEPTH - 1);
#pragma unroll
            for (int j = 0; j < NJ; ++j) { ra[R][j] = ldg(pf, offA[j]); rb[R][j] = ldg(pf, offB[j]); }
        };
        // ---- stage B: Hessians of plane z from buffer (z-zc0)&1
        const bool stat_plane = (z >= vp.cnt_lo && z < vp.cnt_hi);
        v2f h0[NP], h1[NP], h2[NP], h3[NP], h4[NP], h5[NP], fsq[NP];
#pragma unroll
        for (int q = 0; q < NP; ++q) {
        const v2f *T0 = ga + 2 * (b0 + g_own + q * GP);
        v2f upz = T0[-2 * GP], upy = T0[-2 * GP + 1], dnz = T0[2 * GP], dny = T0[2 * GP + 1];
        const v2f lfz = T0[-2], lfy = T0[-1], rtz = T0[2], rty = T0[3];
        const v2f lfx = gx[b0 + g_own + q * GP - 1], rtx = gx[b0 + g_own + q * GP + 1];
        if (E && yface) {                   // uniform: the neighbour of a Y-face voxel is the voxel itself
            const v2f ownz = T0[0], owny = T0[1];
            int yv = yA + q;
            asm volatile("" : "+v"(yv));    // keep the four compares inside this rare branch (hoisted, they pin 8 SGPRs)
            if (yv == 0) { upz.x = ownz.x; upy.x = owny.x; }
            if (yv + RS == 0) { upz.y = ownz.y; upy.y = owny.y; }
            if (yv == ny - 1) { dnz.x = ownz.x; dny.x = owny.x; }
            if (yv + RS == ny - 1) { dnz.y = ownz.y; dny.y = owny.y; }
        }
        h1[q] = dnz - upz; h2[q] = rtz - lfz; h3[q] = dny - upy; h4[q] = rty - lfy; h5[q] = rtx - lfx;
        if (U >= 0) {
            h0[q] = gz_p1[q] - gz_m1[q];
            div3(dz_in, h0[q], dy_in, h1[q], dx_in, h2[q]);
        } else {
            const int gz = gz0 + z;
            const bool z_lo = (gz == 0), z_hi = (gz == gnz - 1);
            h0[q] = (z_hi ? gz_c[q] : gz_p1[q]) - (z_lo ? gz_c[q] : gz_m1[q]);
            div3(dv1_of((z_lo || z_hi) ? hr.z : hr.z2), h0[q], dy_in, h1[q], dx_in, h2[q]);
        }
        div3(dy_in, h3[q], dx_in, h4[q], dx_in, h5[q]);
        if (E) {
            unsigned int fbb = fbits;
            asm volatile("" : "+v"(fbb));
            const float fxo = fac_of_bit(fbb, 0);
            const v2f fyy = v2f{ofyA[q], ofyB[q]}, fxx = v2f{fxo, fxo};
            h1[q] = h1[q] * fyy; h3[q] = h3[q] * fyy;
            h2[q] = h2[q] * fxx; h4[q] = h4[q] * fxx; h5[q] = h5[q] * fxx;
        }
        // frob_sq_of(): a = h0^2 + h3^2 + h5^2; b = 2 (h1^2 + h2^2 + h4^2); a + b -- numpy's association, both voxels at once
        const v2f fa = h0[q] * h0[q] + h3[q] * h3[q] + h5[q] * h5[q];
        const v2f fb = 2.0f * (h1[q] * h1[q] + h2[q] * h2[q] + h4[q] * h4[q]);
        fsq[q] = fa + fb;
        gz_m1[q] = gz_c[q]; gz_c[q] = gz_p1[q];
        }
        // MODE 2 takes the statistics on every plane of the walk, ghost planes of a slab included: those are copies of planes a
        // neighbour owns, evaluated from identical inputs, so the maxima over all ranks are the same -- and no branch per plane.
        // (The h_mask COUNT below stays on the owned planes: it is a sum.)
        if (MODE == 0 || MODE == 2) {
#pragma unroll
            for (int q = 0; q < NP; ++q) {
            if (!E || all_valid) {          // uniform
                max3_abs(mabs, h0[q].x, h0[q].y); max3_abs(mabs2, h1[q].x, h1[q].y); max3_abs(mabs, h2[q].x, h2[q].y);
                max3_abs(mabs2, h3[q].x, h3[q].y); max3_abs(mabs, h4[q].x, h4[q].y); max3_abs(mabs2, h5[q].x, h5[q].y);
                // +inf included: if one turns up (mfrob = inf at the end) the largest FINITE value is not known from
                // this pass; MODE 2 then reports the inf flag only and the host takes the statistics with MODE 0
                if (MODE == 2) max3_f(mfrob, fsq[q].x, fsq[q].y);
            } else {                        // tiles sticking out of the volume hold clamped copies there
                int xv = x;
                asm volatile("" : "+v"(xv));
                const bool okA = (xv < nx) && (yA + q < ny), okB = (xv < nx) && (yB + q < ny);
                float ma = 0.0f, mb = 0.0f;
                max3_abs(ma, h0[q].x, h1[q].x); max3_abs(ma, h2[q].x, h3[q].x); max3_abs(ma, h4[q].x, h5[q].x);
                max3_abs(mb, h0[q].y, h1[q].y); max3_abs(mb, h2[q].y, h3[q].y); max3_abs(mb, h4[q].y, h5[q].y);
                max3_f(mabs, okA ? ma : 0.0f, okB ? mb : 0.0f);
                if (MODE == 2) max3_f(mfrob, okA ? fsq[q].x : 0.0f, okB ? fsq[q].y : 0.0f);
            }
            if (MODE == 0) {
                int xv = x;
                asm volatile("" : "+v"(xv));
                const bool okA = !E || all_valid || ((xv < nx) && (yA + q < ny)), okB = !E || all_valid || ((xv < nx) && (yB + q < ny));
                const float fqa = okA ? fsq[q].x : 0.0f, fqb = okB ? fsq[q].y : 0.0f;
                if (fqa == f_inf || fqb == f_inf) anyinf = 1;
                mfrob = fmaxf(mfrob, fmaxf(fqa == f_inf ? 0.0f : fqa, fqb == f_inf ? 0.0f : fqb));
            }
            }
        }
#pragma unroll
        for (int k = 0; k < 2 * NP; ++k) alive[k] = 0ull;
        land();
        fetch();
        asm volatile("" ::: "memory");
        if (MODE != 0) {
            const unsigned int zoff = (unsigned int)(z - z0) * plane_u;
#pragma unroll
            for (int q = 0; q < NP; ++q) {
            // everything below is logic on 64-bit lane masks (a float compare IS its ballot on a wave64 machine)
            unsigned long long MA, MB, UA = 0ull, UB = 0ull;
            if (MODE == 1) {
                const unsigned long long inf_ok = vp.m_inf ? ~0ull : 0ull;
                const unsigned long long ones = vp.all_ones ? ~0ull : 0ull;          // Filter.run(mask=False)
                MA = (__ballot(fsq[q].x >= vp.fsq_min) & (__ballot(fsq[q].x < f_inf) | inf_ok)) | ones;
                MB = (__ballot(fsq[q].y >= vp.fsq_min) & (__ballot(fsq[q].y < f_inf) | inf_ok)) | ones;
            } else {
                // Round 6: nothing of the two rows reaches the lower end of the bracket -> no mask bit, no count, no entry: the trace test, the
                // slot arithmetic and the stores below are skipped (on the later scales that is most row pairs; lanes that stand for no voxel
                // may keep a pair from being skipped, never the other way round).
                UA = __ballot(fsq[q].x >= fsq_lo_); UB = __ballot(fsq[q].y >= fsq_lo_);
                if ((UA | UB) == 0ull) continue;
                MA = __ballot(fsq[q].x >= fsq_hi_); UA &= ~MA;
                MB = __ballot(fsq[q].y >= fsq_hi_); UB &= ~MB;
            }
            if (E && !all_valid) {
                int xv = x;
                asm volatile("" : "+v"(xv));
                const unsigned long long VA = __ballot((xv < nx) && (yA + q < ny)), VB = __ballot((xv < nx) && (yB + q < ny));
                MA &= VA; MB &= VB; UA &= VA; UB &= VB;
            }
            // only trace < 0 with trace^2 >= 0.30 frob_sq can give a response > 0 (HM_TRACE_OK, head of hessian.inc): everything
            // else stays out of the queue
            const v2f tr = h0[q] + h3[q] + h5[q];
            const v2f ts = v2f{tr.x * fabsf(tr.x), tr.y * fabsf(tr.y)} + HM_TRACE_C * fsq[q];
#ifdef HM_TRACE_ALL
            const unsigned long long SA = __ballot(ts.x == ts.x) | __ballot(ts.x != ts.x), SB = SA;     // all lanes, not a constant
#else
            unsigned long long SA = __ballot(ts.x < 0.0f), SB = __ballot(ts.y < 0.0f);
            if (MODE == 1) {                    // frob_sq overflowed: no statement about the trace, the voxel is solved (HM_TRACE_OK)
                SA |= ~__ballot(fsq[q].x < f_inf); SB |= ~__ballot(fsq[q].y < f_inf);
            }
#endif
            const unsigned long long aliveA = MA & prev[2 * q], aliveB = MB & prev[2 * q + 1];          // (no earlier scale: the caller passes all ones)
            alive[2 * q] = aliveA; alive[2 * q + 1] = aliveB;
            cnt += stat_plane ? (unsigned int)(__builtin_popcountll(MA) + __builtin_popcountll(MB)) : 0u;
            // MODE 2: an undecided voxel is queued whatever its trace or the earlier masks say (the resolve kernel needs it
            // for the h_mask count and the mask bit)
            const unsigned long long QA = (aliveA & SA) | UA, QB = (aliveB & SB) | UB;
            const unsigned int nA = (unsigned int)__builtin_popcountll(QA), nB = (unsigned int)__builtin_popcountll(QB);
            // (A wave-uniform "does the whole batch fit" test instead of the per-lane one below was measured slower: 1.57 vs 1.54 ms.)
            if (__builtin_amdgcn_inverse_ballot_w64(QA)) {
                const unsigned int slot = qn + __builtin_amdgcn_mbcnt_hi((unsigned int)(QA >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)QA, 0u));
                if (MODE == 1 || slot < (unsigned int)vp.qcap) {
                    unsigned int idx = zoff + idx_rowA + (unsigned int)(q * nx);
                    if (MODE == 2 && __builtin_amdgcn_inverse_ballot_w64(UA)) idx |= HM_UNDECIDED;
                    qent_store_pairs<0>(qent, slot, h0[q], h1[q], h2[q], h3[q], h4[q], h5[q], idx);
                }
            }
            if (__builtin_amdgcn_inverse_ballot_w64(QB)) {
                const unsigned int slot = qn + nA + __builtin_amdgcn_mbcnt_hi((unsigned int)(QB >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)QB, 0u));
                if (MODE == 1 || slot < (unsigned int)vp.qcap) {
                    unsigned int idx = zoff + idx_rowB + (unsigned int)(q * nx);
                    if (MODE == 2 && __builtin_amdgcn_inverse_ballot_w64(UB)) idx |= HM_UNDECIDED;
                    qent_store_pairs<1>(qent, slot, h0[q], h1[q], h2[q], h3[q], h4[q], h5[q], idx);
                }
            }
            qn += nA + nB;
            }
        }
        // (plane z+3 landed in the slot of plane z-1 and plane z+3+HV_DEPTH went in flight above: static register indices in the
        // unrolled steps, unconditional loads -- see hessian_g_kernel)
        __syncthreads();
    };
    auto step_rolled = [&](const int z) {
        unsigned long long pv[2 * NP], av[2 * NP];
#pragma unroll
        for (int k = 0; k < 2 * NP; ++k) pv[k] = (MODE != 0) ? (pmask64[(i64)z * wplane + wordr[k]] | no_prev) : 0ull;
        step(z, std::integral_constant<int, -1>{}, std::true_type{}, pv, av);
        if (MODE != 0 && lane == 0) {
#pragma unroll
            for (int k = 0; k < 2 * NP; ++k) if (row_ok[k]) cmask64[(i64)z * wplane + wordr[k]] = av[k];
        }
    };

    const bool edge = xface || yface || !all_valid;
    auto group = [&](const int z, auto ec) {           // eight unrolled steps, every plane interior in Z
        if (MODE != 0) {
            const unsigned long long pv = pmask64[(i64)(z + (lane & 7)) * wplane + word_lane] | no_prev;
            int plo = (int)(unsigned int)pv, phi = (int)(unsigned int)(pv >> 32);
            int alo = 0, ahi = 0;
#define HV_STEP1(UU)                                                                                              \
            {                                                                                                     \
                unsigned long long p_[2 * NP], a_[2 * NP];                                                        \
                _Pragma("unroll") for (int k = 0; k < 2 * NP; ++k)                                                \
                    p_[k] = ((unsigned long long)(unsigned int)__builtin_amdgcn_readlane(phi, 8 * k + UU) << 32) | \
                            (unsigned int)__builtin_amdgcn_readlane(plo, 8 * k + UU);                             \
                step(z + UU, std::integral_constant<int, UU>{}, ec, p_, a_);                                      \
                hv_put<UU, 2 * NP>(alo, ahi, a_);                                                                 \
            }
            HV_STEP1(0) HV_STEP1(1) HV_STEP1(2) HV_STEP1(3) HV_STEP1(4) HV_STEP1(5) HV_STEP1(6) HV_STEP1(7)
#undef HV_STEP1
            if (lane < 16 * NP && row_lane_ok)
                cmask64[(i64)(z + (lane & 7)) * wplane + word_lane] = ((unsigned long long)(unsigned int)ahi << 32) | (unsigned int)alo;
        } else {
            unsigned long long p_[2 * NP] = {}, a_[2 * NP];
            step(z + 0, std::integral_constant<int, 0>{}, ec, p_, a_); step(z + 1, std::integral_constant<int, 1>{}, ec, p_, a_);
            step(z + 2, std::integral_constant<int, 2>{}, ec, p_, a_); step(z + 3, std::integral_constant<int, 3>{}, ec, p_, a_);
            step(z + 4, std::integral_constant<int, 4>{}, ec, p_, a_); step(z + 5, std::integral_constant<int, 5>{}, ec, p_, a_);
            step(z + 6, std::integral_constant<int, 6>{}, ec, p_, a_); step(z + 7, std::integral_constant<int, 7>{}, ec, p_, a_);
        }
    };
    {
        int z = zc0;
        for (; z + HM_SLOTS <= zc1; z += HM_SLOTS) {
            // planes z-1 .. z+9 interior?  ((z - zc0) % 8 == 0 here)
            if (gz0 + z >= 2 && gz0 + z + HM_SLOTS - 1 <= gnz - 3) {
                if (edge) group(z, std::true_type{}); else group(z, std::false_type{});
            } else {
                for (int u = 0; u < HM_SLOTS; ++u) step_rolled(z + u);
            }
        }
        for (; z < zc1; ++z) step_rolled(z);
    }

    const int w = tid >> 6;
    __syncthreads();
    if (MODE == 0 || MODE == 2) {
        if (MODE == 2 && mfrob == f_inf) { anyinf = 1; mfrob = 0.0f; }       // see the statistics of step()
        mabs = wave_max_f(fmaxf(mabs, mabs2)); mfrob = wave_max_f(mfrob); anyinf = wave_or_i(anyinf);
        if ((tid & 63) == 0) { s_red[w] = mabs; s_red[16 + w] = mfrob; s_red[32 + w] = anyinf ? 1.0f : 0.0f; }
        __syncthreads();
        if (tid == 0) {
            float a = 0.0f, b = 0.0f, c = 0.0f;
            for (int k = 0; k < NW; ++k) { a = fmaxf(a, s_red[k]); b = fmaxf(b, s_red[16 + k]); c = fmaxf(c, s_red[32 + k]); }
            if (a > 0.0f && __float_as_uint(a) > __hip_atomic_load(&res[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&res[0], __float_as_uint(a));
            if (b > 0.0f && __float_as_uint(b) > __hip_atomic_load(&res[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(&res[1], __float_as_uint(b));
            if (c > 0.0f) atomicOr(&res[2], 1u);
        }
    }
    if (MODE != 0) {
        __syncthreads();
        if (lane == 0) {
            vq.count[region] = qn;
            if (MODE == 2 && qn > (unsigned int)vp.qcap) atomicOr(&res[3], 1u);     // region overflow: the scale is redone
        }
        unsigned int *s_cnt = (unsigned int *)s_red;
        if (lane == 0) s_cnt[w] = cnt;
        __syncthreads();
        if (tid == 0) {
            unsigned long long t = 0;
            for (int k = 0; k < NW; ++k) t += s_cnt[k];
            if (t) atomicAdd(mask_count, t);
        }
    }
}
