// Part of libnellie_hip.so (gfx950): the one-voxel walk, included by nellie_walk.hip after walk_common.h; see include/nellie_amd.h for the C-ABI.
// =================================================================================================
// kernel: Hessian statistics and the per-scale vesselness update, one voxel per thread
// =================================================================================================
// -------------------------------------------------------------------------------------------------
// Z-marching, LDS-tiled Hessian kernel.  A 512-thread workgroup owns an 8(y) x 64(x) column tile and walks a
// chunk of HM_ZCHUNK planes, one barrier per plane; raw planes are read from HBM exactly once (+ halo), several
// planes ahead, into registers and dropped into a 4-slot LDS ring.
//   MODE 0: statistics (max |H_ij|, max finite frob_sq, any inf)                       filtering.py:555-562
//   MODE 1: vesselness update for a KNOWN mask threshold fsq_min                        filtering.py:563-584
//   MODE 2: statistics AND vesselness candidates in ONE pass, for a threshold only known to lie in
//           [fsq_lo, fsq_hi] (see below); the resolve kernel settles the voxels in between.
// The stage output is max_s(v_s) * prod_s(h_mask_s) (filtering.py:846-850, 926), so a voxel rejected by the
// h_mask of ANY scale ends as 0: each scale writes the AND of its own h_mask with the previous scale's cumulative
// mask (1 bit/voxel) and solves only voxels still alive.  Of those, only a voxel whose Hessian trace is clearly
// NEGATIVE can have its two largest-|.| eigenvalues both <= 0: with |l1| <= |l2| <= |l3| and l2, l3 <= 0 the trace is
// l1 + l2 + l3 <= |l1| - |l2| - |l3| <= -|l3| <= -||H||_F / sqrt(3), i.e. trace < 0 and trace^2 >= frob_sq / 3.  Every other
// voxel has the 0 of filtering.py:762-763 without an eigen-solve (HM_TRACE_OK below: the constant 0.30 instead of 1/3 is
// five orders of magnitude more slack than the float32 rounding of trace, frob_sq and the eigenvalues needs).  Round 4: this
// two-sided test; rounds 1-3 only excluded trace > 1e-3 ||H||_F, which queued 46 % of the masked voxels of a noisy first
// scale where this queues 35 % (27 % have a response > 0) -- a quarter fewer 32-byte entries written and read.  The remaining voxels (scattered) are COMPACTED into a global
// queue (VQueue: 6 Hessian components + voxel index per entry).  Every wave owns a fixed region of that queue --
// it handles one 64-voxel row segment over HM_ZCHUNK planes -- and appends with plain stores at a wave-uniform
// cursor: no atomics, no LDS queue, no extra barriers.  The float64 eigen-solve + Frangi response then runs as a
// dense kernel over the regions, so the marching kernel stays lean (registers, occupancy, static LDS addressing).
//
// MODE 2 -- why one pass is enough.  The h_mask threshold needs max |H_ij| over the WHOLE volume
// (filtering.py:555-562) before any voxel can be masked, which is why the reference (and MODE 0 + MODE 1) walk
// the Hessian twice per scale.  But thresholding frob/max_abs against a histogram threshold of the same
// normalised samples is, up to float32 rounding and histogram binning, independent of max_abs: the host
// predicts fsq_min from the sample lattice alone and brackets it by a few histogram bins.  One pass then takes the
// statistics, treats frob_sq >= fsq_hi as masked, frob_sq < fsq_lo as not masked, and queues the few voxels in
// between flagged "undecided".  Afterwards the host computes the exact fsq_min as before; if it lies inside the
// bracket the resolve kernel applies the exact test to the undecided entries (results identical to MODE 0 + 1 bit
// for bit), otherwise -- or if a region overflowed, or an inf turned up -- the scale is redone with MODE 1.
// -------------------------------------------------------------------------------------------------
// -------------------------------------------------------------------------------------------------
// The FIRST derivatives are shared through LDS.  np.gradient applied twice
// evaluates every first derivative several times when it is fused per voxel (d/dz g at (y+-1,x), (y,x+-1) and
// (z+-1): six times; d/dy g four times; d/dx g twice): 18 exact divisions per voxel.  Here a workgroup computes
// the three first derivatives of plane z+1 ONCE per tile element (tile + a one-voxel cross halo) into a
// double-buffered LDS tile of float4 (gz, gy, gx, -) while it differences the tile of plane z (written one step
// earlier) into the six Hessian components: 3 + 6 divisions per voxel, four wide LDS reads for the second stage.
// The first derivative along Z at the voxel's own column stays in registers across three steps (h_zz).
// Raw planes: 4-slot LDS ring (planes z, z+1, z+2 are read while z+3 lands), +-2 halo, indices clamped at the
// volume faces (replicated edges), so only divisors -- float32(h) at a face, float32(2h) inside -- need selects.
// -------------------------------------------------------------------------------------------------
#define HG_RP (HM_TX + 4)              // raw tile pitch
#define HG_GP (HM_TX + 2)              // gradient tile pitch
template <int TY> struct HGCfg {
    static constexpr int NT = HM_TX * TY;
    static constexpr int RPLANE = HG_RP * (TY + 4);
    static constexpr int GPLANE = HG_GP * (TY + 2);
    static constexpr int NHALO = 2 * HM_TX + 2 * TY;    // cross halo of the gradient tile (no corners)
    static constexpr int lds_bytes() { return 2 * GPLANE * 16 + 4 * RPLANE * 4 + 256; }
};

template <int MODE, int TY, bool FAST>
#ifndef HG_WAVES
#define HG_WAVES 4
#endif
__global__ void __launch_bounds__(HM_TX * TY, HG_WAVES)
hessian_g_kernel(const float *__restrict__ g, unsigned long long *__restrict__ cmask64,
                 const unsigned long long *__restrict__ pmask64, int wpr,
                 VolGeom v, HessDv<FAST> hr, VessP vp, VQueue vq, int z0, int z1, int ntx, int nty,
                 unsigned int *__restrict__ res, unsigned long long *__restrict__ mask_count) {
    constexpr int NT = HGCfg<TY>::NT, RPLANE = HGCfg<TY>::RPLANE, GPLANE = HGCfg<TY>::GPLANE, NHALO = HGCfg<TY>::NHALO;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float4 *gt = (float4 *)smem;                             // [2][GPLANE] first derivatives (gz, gy, gx, -)
    float *rp = (float *)(gt + 2 * GPLANE);                  // [4][RPLANE] raw planes
    float *s_red = rp + 4 * RPLANE;                          // 64 floats of reduction scratch
    const int tid = threadIdx.x;
    const int lx = tid & 63, ly = tid >> 6;
    const unsigned nblk = gridDim.x;
    unsigned bid = blockIdx.x;
    if ((nblk & 7u) == 0u) bid = (bid & 7u) * (nblk >> 3) + (bid >> 3);
    // ^ XCD-aware remap: workgroup b runs on XCD b % 8; give each XCD a contiguous run of tiles so that neighbouring
    //   tiles (shared halos) meet in the same L2.  Speed only, never correctness.
    const int tx = bid % ntx;
    const int ty = (bid / ntx) % nty;
    const int zc = bid / (ntx * nty);
    const int zch = vp.zchunk > 0 ? vp.zchunk : HM_ZCHUNK;
    const int zc0 = z0 + zc * zch;
    const int zc1 = (zc0 + zch < z1) ? zc0 + zch : z1;
    const int nx = (int)v.nx, ny = (int)v.ny;
    const i64 sz = v.ny * v.nx;
    const int gz0 = (int)v.gz0, gnz = (int)v.gnz;
    const int xbase = tx * HM_TX - 2, ybase = ty * TY - 2;
    const int x = xbase + 2 + lx, y = ybase + 2 + ly;
    const bool valid = (x < nx) && (y < ny);

    // raw tile elements this thread stages per plane (a thread without a second one re-reads its first)
    int off0, off1;
    bool two;
    {
        int yy = ybase + tid / HG_RP, xx = xbase + tid % HG_RP;
        yy = yy < 0 ? 0 : (yy > ny - 1 ? ny - 1 : yy);
        xx = xx < 0 ? 0 : (xx > nx - 1 ? nx - 1 : xx);
        off0 = yy * nx + xx;
        off1 = off0;
        const int e1 = tid + NT;
        two = e1 < RPLANE;
        if (two) {
            int y1 = ybase + e1 / HG_RP, x1 = xbase + e1 % HG_RP;
            y1 = y1 < 0 ? 0 : (y1 > ny - 1 ? ny - 1 : y1);
            x1 = x1 < 0 ? 0 : (x1 > nx - 1 ? nx - 1 : x1);
            off1 = y1 * nx + x1;
        }
    }
    auto zclamp = [&](int zz) -> int {
        const int gg = gz0 + zz;
        return gg < 0 ? -gz0 : (gg > gnz - 1 ? gnz - 1 - gz0 : zz);
    };
    auto face = [&](int q, int n) -> bool { return q == 0 || q == n - 1; };

    // gradient-tile elements: the thread's own voxel and (tid < NHALO) one element of the cross halo.
    // (gy, gx) in [-1, TY] x [-1, 64] are tile coordinates; raw offset = (gy+2)*RP + gx+2, G offset = (gy+1)*GP + gx+1.
    const int r_own = (ly + 2) * HG_RP + lx + 2, g_own = (ly + 1) * HG_GP + lx + 1;
    int hgy = 0, hgx = 0;
    const bool has_halo = tid < NHALO;
    if (tid < HM_TX) { hgy = -1; hgx = tid; }
    else if (tid < 2 * HM_TX) { hgy = TY; hgx = tid - HM_TX; }
    else if (tid < 2 * HM_TX + TY) { hgy = tid - 2 * HM_TX; hgx = -1; }
    else if (has_halo) { hgy = tid - 2 * HM_TX - TY; hgx = HM_TX; }
    const int r_halo = (hgy + 2) * HG_RP + hgx + 2, g_halo = (hgy + 1) * HG_GP + hgx + 1;
    const Dv<FAST> dvy_own = face(y, ny) ? hr.y : hr.y2, dvx_own = face(x, nx) ? hr.x : hr.x2;
    const Dv<FAST> dvy_halo = face(ybase + 2 + hgy, ny) ? hr.y : hr.y2, dvx_halo = face(xbase + 2 + hgx, nx) ? hr.x : hr.x2;
    // second stage: neighbours inside the gradient tile; at a face the "neighbour" is the voxel itself
    const bool y_lo = (y == 0), y_hi = (y == ny - 1), x_lo = (x == 0), x_hi = (x == nx - 1);
    const int g_up = g_own - (y_lo ? 0 : HG_GP), g_dn = g_own + (y_hi ? 0 : HG_GP);
    const int g_lf = g_own - (x_lo ? 0 : 1), g_rt = g_own + (x_hi ? 0 : 1);

    // first derivatives of plane zz at raw offset r, from the raw planes zz-1 / zz / zz+1 (clamped by the caller)
    auto grad_at = [&](const float *Pm, const float *P0, const float *Pp, const int r, const Dv<FAST> dz, const Dv<FAST> dy,
                       const Dv<FAST> dx) -> float4 {
        return make_float4(dz.div(Pp[r] - Pm[r]), dy.div(P0[r + HG_RP] - P0[r - HG_RP]), dx.div(P0[r + 1] - P0[r - 1]), 0.0f);
    };

    // ---- prologue: planes zc0-2 .. zc0+1, the gradient tile of plane zc0, the own Z derivatives of zc0-1 and zc0
    const int pmin = zclamp(zc0 - 2), pmax = zclamp(zc1 + 1);
    for (int pz = pmin; pz <= pmax && pz <= zc0 + 1; ++pz) {
        float *dst = rp + HG_RSLOT(pz) * RPLANE;
        const float *src = g + (i64)pz * sz;
        dst[tid] = src[off0];
        if (two) dst[tid + NT] = src[off1];
    }
    __syncthreads();
    float gz_m1, gz_c;                         // d/dz at the own voxel on planes z-1 and z
    {
        const float *Pm2 = rp + HG_RSLOT(zclamp(zc0 - 2)) * RPLANE, *Pm1 = rp + HG_RSLOT(zclamp(zc0 - 1)) * RPLANE;
        const float *P0 = rp + HG_RSLOT(zc0) * RPLANE, *Pp1 = rp + HG_RSLOT(zclamp(zc0 + 1)) * RPLANE;
        const Dv<FAST> dzm = face(gz0 + zc0 - 1, gnz) ? hr.z : hr.z2, dz0 = face(gz0 + zc0, gnz) ? hr.z : hr.z2;
        gz_m1 = dzm.div(P0[r_own] - Pm2[r_own]);
        const float4 G = grad_at(Pm1, P0, Pp1, r_own, dz0, dvy_own, dvx_own);
        gz_c = G.x;
        gt[g_own] = G;                                                                  // buffer (zc0 - zc0) & 1 = 0
        if (has_halo) gt[g_halo] = grad_at(Pm1, P0, Pp1, r_halo, dz0, dvy_halo, dvx_halo);
    }
    __syncthreads();
    if (zc0 + 2 <= pmax) {                      // plane zc0+2 takes the slot of zc0-2
        float *dst = rp + HG_RSLOT(zc0 + 2) * RPLANE;
        const float *src = g + (i64)(zc0 + 2) * sz;
        dst[tid] = src[off0];
        if (two) dst[tid + NT] = src[off1];
    }
    float ra[HM_DEPTH], rb[HM_DEPTH];          // planes z+3 .. z+3+HM_DEPTH-1 in flight
#pragma unroll
    for (int d = 0; d < HM_DEPTH; ++d) {
        const int pz = zc0 + 3 + d;
        const float *src = g + (i64)(pz < pmax ? pz : pmax) * sz;
        ra[d] = src[off0];
        rb[d] = src[off1];
    }
    __syncthreads();

    const Dv<FAST> rdy = (y_lo || y_hi) ? hr.y : hr.y2;
    const Dv<FAST> rdx = (x_lo || x_hi) ? hr.x : hr.x2;
    float mabs = 0.0f, mfrob = 0.0f;
    int anyinf = 0;
    const int lane = tid & 63;
    const int yu = __builtin_amdgcn_readfirstlane(y);
    const bool row_ok = yu < ny;
    const i64 word0 = (i64)(row_ok ? yu : 0) * wpr + tx;
    const i64 wplane = (i64)ny * wpr;
    const unsigned int region = (bid * (unsigned)(NT / 64) + (unsigned)__builtin_amdgcn_readfirstlane(ly));
    float4 *qent = MODE != 0 ? vq.ent + (size_t)region * (size_t)vp.qcap * 2 : nullptr;
    unsigned int qn = 0;
    unsigned int cnt = 0;
    const unsigned long long no_prev = vp.have_prev ? 0ull : ~0ull;
    const unsigned int plane_u = (unsigned int)sz, idx_row = (unsigned int)(y * nx + x);   // voxel offsets fit 31 bits
    // the plane that goes in flight next (clamped to pmax: past the chunk's end a harmless re-read)
    const float *pf = g + (i64)(zc0 + 3 + HM_DEPTH < pmax ? zc0 + 3 + HM_DEPTH : pmax) * sz;

    // One plane step.  U >= 0: compile-time ring / buffer indices, every plane involved is interior.
    auto step = [&](const int z, auto uc, const unsigned long long prev) -> unsigned long long {
        constexpr int U = decltype(uc)::value;
        // ---- stage A: first derivatives of plane z+1 (tile + halo) into buffer (z+1-zc0)&1
        float gz_p1;
        {
            const float *Pm, *P0, *Pp;
            Dv<FAST> dz1;
            float4 *T1;
            if (U >= 0) {
                Pm = rp + (U & 3) * RPLANE; P0 = rp + ((U + 1) & 3) * RPLANE; Pp = rp + ((U + 2) & 3) * RPLANE;
                dz1 = hr.z2;
                T1 = gt + ((U + 1) & 1) * GPLANE;
            } else {
                Pm = rp + HG_RSLOT(zclamp(z)) * RPLANE; P0 = rp + HG_RSLOT(zclamp(z + 1)) * RPLANE;
                Pp = rp + HG_RSLOT(zclamp(z + 2)) * RPLANE;
                dz1 = face(gz0 + z + 1, gnz) ? hr.z : hr.z2;
                T1 = gt + ((z + 1 - zc0) & 1) * GPLANE;
            }
            const float4 G = grad_at(Pm, P0, Pp, r_own, dz1, dvy_own, dvx_own);
            gz_p1 = G.x;
            T1[g_own] = G;
            if (has_halo) T1[g_halo] = grad_at(Pm, P0, Pp, r_halo, dz1, dvy_halo, dvx_halo);
        }
        // ---- stage B: Hessian of plane z from buffer (z-zc0)&1
        bool m = false, solve = false, undecided = false;
        const bool stat_plane = (z >= vp.cnt_lo && z < vp.cnt_hi);
        float h[6];
        if (valid) {
            const float4 *T0 = gt + ((U >= 0) ? (U & 1) : ((z - zc0) & 1)) * GPLANE;
            const float2 up = *reinterpret_cast<const float2 *>(T0 + g_up), dn = *reinterpret_cast<const float2 *>(T0 + g_dn);
            const float4 lf = T0[g_lf], rt = T0[g_rt];
            if (U >= 0) {
                h[0] = hr.z2.div(gz_p1 - gz_m1);
            } else {
                const int gz = gz0 + z;
                const bool z_lo = (gz == 0), z_hi = (gz == gnz - 1);
                const Dv<FAST> rdz = (z_lo || z_hi) ? hr.z : hr.z2;
                h[0] = rdz.div((z_hi ? gz_c : gz_p1) - (z_lo ? gz_c : gz_m1));
            }
            h[1] = rdy.div(dn.x - up.x);
            h[2] = rdx.div(rt.x - lf.x);
            h[3] = rdy.div(dn.y - up.y);
            h[4] = rdx.div(rt.y - lf.y);
            h[5] = rdx.div(rt.z - lf.z);
            const float fsq = frob_sq_of(h);
            if (MODE == 0 || (MODE == 2 && stat_plane)) {
#pragma unroll
                for (int k = 0; k < 6; ++k) mabs = fmaxf(mabs, fabsf(h[k]));
                if (isinf(fsq)) anyinf = 1; else mfrob = fmaxf(mfrob, fsq);
            }
            if (MODE != 0) {
                if (MODE == 1) m = vp.all_ones || ((fsq >= vp.fsq_min) && (fsq < __int_as_float(0x7f800000) || vp.m_inf));
                else { m = fsq >= vp.fsq_hi; undecided = (fsq >= vp.fsq_lo) && !m; }
                const float tr = h[0] + h[3] + h[5];
                solve = HM_TRACE_OK(tr, fsq);                   // see the head of this file
            }
        }
        gz_m1 = gz_c; gz_c = gz_p1;
        unsigned long long alive = 0ull;
        if (MODE != 0) {
            const unsigned long long bal = __ballot(m);
            const unsigned long long pmask = prev | no_prev;                  // wave-uniform
            alive = bal & pmask;
            if (stat_plane) cnt += (unsigned int)__builtin_popcountll(bal);
            // MODE 2: an undecided voxel is queued whatever its trace or the earlier masks say (the resolve kernel
            // needs it for the h_mask count and the mask bit); everything else as in MODE 1
            bool q = m && solve && __builtin_amdgcn_inverse_ballot_w64(pmask);  // this lane's bit of pmask
            if (MODE == 2) q = q || undecided;
            const unsigned long long qb = __ballot(q);
            if (q) {
                const unsigned int slot = qn + __builtin_amdgcn_mbcnt_hi((unsigned int)(qb >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)qb, 0u));
                if (MODE == 1 || slot < (unsigned int)vp.qcap) {
                    unsigned int idx = (unsigned int)(z - z0) * plane_u + idx_row;
                    if (MODE == 2 && undecided) idx |= HM_UNDECIDED;
                    qent_store(qent, slot, h[0], h[1], h[2], h[3], h[4], h[5], idx);
                }
            }
            qn += (unsigned int)__builtin_popcountll(qb);
        }
        // ---- plane z+3 lands in the slot of plane z-1; plane z+3+HM_DEPTH goes in flight.
        // Unrolled steps address the in-flight registers statically (U % HM_DEPTH): rotating them would make every
        // step wait for ALL outstanding loads.  Loads are unconditional (clamped plane) so that they can be counted.
        if (U >= 0) {
            constexpr int R = (U >= 0 ? U : 0) % HM_DEPTH;
            float *dst = rp + ((U + 3) & 3) * RPLANE;
            dst[tid] = ra[R];
            if (two) dst[tid + NT] = rb[R];
            ra[R] = pf[off0];
            rb[R] = pf[off1];
        } else {
            if (z + 3 <= pmax) {
                float *dst = rp + HG_RSLOT(z + 3) * RPLANE;
                dst[tid] = ra[0];
                if (two) dst[tid + NT] = rb[0];
            }
#pragma unroll
            for (int d = 0; d + 1 < HM_DEPTH; ++d) { ra[d] = ra[d + 1]; rb[d] = rb[d + 1]; }
            ra[HM_DEPTH - 1] = pf[off0];
            rb[HM_DEPTH - 1] = pf[off1];
        }
        if (z + 4 + HM_DEPTH <= pmax) pf += sz;
        __syncthreads();
        return alive;
    };
    auto step_rolled = [&](const int z) {
        unsigned long long prev = 0ull;
        if (MODE != 0) prev = pmask64[(i64)z * wplane + word0];
        const unsigned long long alive = step(z, std::integral_constant<int, -1>{}, prev);
        if (MODE != 0 && lane == 0 && row_ok) cmask64[(i64)z * wplane + word0] = alive;
    };

    {
        int z = zc0;
        for (; z + HM_SLOTS <= zc1; z += HM_SLOTS) {
            // planes z-1 .. z+9 interior?  ((z - zc0) % 8 == 0 here)
            if (gz0 + z >= 2 && gz0 + z + HM_SLOTS - 1 <= gnz - 3) {
                if (MODE != 0) {
                    const unsigned long long pv = pmask64[(i64)(z + (lane & 7)) * wplane + word0];
                    int plo = (int)(unsigned int)pv, phi = (int)(unsigned int)(pv >> 32);
                    int alo = 0, ahi = 0;
#define HG_STEP1(UU)                                                                                              \
                    {                                                                                             \
                        const unsigned long long p_ = ((unsigned long long)(unsigned int)__builtin_amdgcn_readlane(phi, UU) << 32) | \
                                                      (unsigned int)__builtin_amdgcn_readlane(plo, UU);           \
                        const unsigned long long a_ = step(z + UU, std::integral_constant<int, UU>{}, p_);        \
                        alo = (lane == UU) ? (int)(unsigned int)a_ : alo;                                         \
                        ahi = (lane == UU) ? (int)(unsigned int)(a_ >> 32) : ahi;                                 \
                    }
                    HG_STEP1(0) HG_STEP1(1) HG_STEP1(2) HG_STEP1(3) HG_STEP1(4) HG_STEP1(5) HG_STEP1(6) HG_STEP1(7)
#undef HG_STEP1
                    if (lane < 8 && row_ok)
                        cmask64[(i64)(z + lane) * wplane + word0] = ((unsigned long long)(unsigned int)ahi << 32) | (unsigned int)alo;
                } else {
                    step(z + 0, std::integral_constant<int, 0>{}, 0ull); step(z + 1, std::integral_constant<int, 1>{}, 0ull);
                    step(z + 2, std::integral_constant<int, 2>{}, 0ull); step(z + 3, std::integral_constant<int, 3>{}, 0ull);
                    step(z + 4, std::integral_constant<int, 4>{}, 0ull); step(z + 5, std::integral_constant<int, 5>{}, 0ull);
                    step(z + 6, std::integral_constant<int, 6>{}, 0ull); step(z + 7, std::integral_constant<int, 7>{}, 0ull);
                }
            } else {
                for (int u = 0; u < HM_SLOTS; ++u) step_rolled(z + u);
            }
        }
        for (; z < zc1; ++z) step_rolled(z);
    }

    const int w = tid >> 6;
    __syncthreads();
    if (MODE == 0 || MODE == 2) {
        mabs = wave_max_f(mabs); mfrob = wave_max_f(mfrob); anyinf = wave_or_i(anyinf);
        if ((tid & 63) == 0) { s_red[w] = mabs; s_red[16 + w] = mfrob; s_red[32 + w] = anyinf ? 1.0f : 0.0f; }
        __syncthreads();
        if (tid == 0) {
            float a = 0.0f, b = 0.0f, c = 0.0f;
            for (int k = 0; k < NT / 64; ++k) { a = fmaxf(a, s_red[k]); b = fmaxf(b, s_red[16 + k]); c = fmaxf(c, s_red[32 + k]); }
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
            for (int k = 0; k < NT / 64; ++k) t += s_cnt[k];
            if (t) atomicAdd(mask_count, t);
        }
    }
}
