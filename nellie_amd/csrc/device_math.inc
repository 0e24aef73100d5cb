// Part of libnellie_hip.so (gfx950): included by nellie_hip.hip, see include/nellie_amd.h for the C-ABI.
// =================================================================================================
// device helpers
// =================================================================================================
struct VolGeom {
    i64 nzl, ny, nx;   // local shape
    i64 gz0, gnz;      // global placement of local plane 0, global plane count
    int chunk = 128;   // line chunk a thread of the marching Gaussian kernels walks (its 2R halo elements are read again
                       // by the neighbouring chunk: 256 on large volumes, where there are workgroups to spare)
};

struct HessP {
    float hz, hy, hx;      // float32(h)      : one-sided divisor at a face
    float hz2, hy2, hx2;   // float32(2.0*h)  : central divisor
};

// scipy NI_EXTEND_REFLECT (d c b a | a b c d | d c b a)
__device__ __forceinline__ i64 reflect_idx(i64 i, i64 n) {
    if (i >= 0 && i < n) return i;
    i64 p = 2 * n;
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - 1 - i : i;
}

// Exactly rounded float32 division by a constant d, given rcp = RN64(1/d):
//   a/d = (float)((double)a * rcp).
// Why it is exact: a/d can never sit closer than ~2^-48 (relative) to a float32 rounding boundary
// (a - m*d is a non-zero integer multiple of 2^-47 for 24-bit a, d and a 25-bit midpoint m), while the
// float64 product carries a relative error <= 2^-52, so the final rounding lands on the IEEE quotient.
// (Sub-normal quotients are the one exception; differences of image intensities never get there.)
// 3 instructions instead of the ~12 of an IEEE division; checked bit-for-bit on 1.2e9 operands.
__device__ __forceinline__ float div_c(float a, double rcp) { return (float)((double)a * rcp); }

// wave64 reductions (CDNA wavefront = 64 lanes)
__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ float wave_min_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// *dst += sum over the workgroup's waves of `wave_value` (taken from lane 0 of each wave); every thread of a workgroup
// of up to 1024 threads must call it.  One atomic per workgroup: atomics on one address retire ~10 ns apart, so a
// per-wave atomic in a 32k-wave grid costs 0.3 ms by itself.
__device__ __forceinline__ void block_add_u64(unsigned long long wave_value, unsigned long long *dst) {
    __shared__ unsigned long long s_blk[16];
    const int w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    if ((threadIdx.x & 63) == 0) s_blk[w] = wave_value;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int k = 0; k < nw; ++k) t += s_blk[k];
        if (t) atomicAdd(dst, t);
    }
}

// lane `src`'s 64-bit value in every lane; `src` must be wave-uniform (v_readlane_b32 x 2 instead of a ds_bpermute round trip)
__device__ __forceinline__ unsigned long long wave_read_u64(unsigned long long v, int src) {
    const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)v, src);
    const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ int wave_or_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o, 64);
    return v;
}

// -------------------------------------------------------------------------------------------------
// np.gradient applied twice (filtering.py:518-536), fused: every first derivative is rounded to
// float32 (true IEEE division by float32(2h) / float32(h)) before it is differenced again.
// Faces use clamped indices + the one-sided divisor, independently at both stages.
// Component order = the reference's (hxx,hxy,hxz,hyy,hyz,hzz) with "x" = axis 0 (Z).
// -------------------------------------------------------------------------------------------------
__device__ __forceinline__ void hessian_at(const float *__restrict__ g, const VolGeom &v, const HessP &hp,
                                           i64 z, i64 y, i64 x, float h[6]) {
    const i64 sy = v.nx, sz = v.ny * v.nx;
    const i64 gz = v.gz0 + z;
    // outer-difference sites and divisors
    const bool z_lo = (gz == 0), z_hi = (gz == v.gnz - 1);
    const bool y_lo = (y == 0), y_hi = (y == v.ny - 1);
    const bool x_lo = (x == 0), x_hi = (x == v.nx - 1);
    const i64 zl = z_lo ? z : z - 1, zh = z_hi ? z : z + 1;
    const i64 yl = y_lo ? y : y - 1, yh = y_hi ? y : y + 1;
    const i64 xl = x_lo ? x : x - 1, xh = x_hi ? x : x + 1;
    const float dz = (z_lo || z_hi) ? hp.hz : hp.hz2;
    const float dy = (y_lo || y_hi) ? hp.hy : hp.hy2;
    const float dx = (x_lo || x_hi) ? hp.hx : hp.hx2;

    auto F = [&](i64 zz, i64 yy, i64 xx) -> float { return g[zz * sz + yy * sy + xx]; };
    auto GZ = [&](i64 zz, i64 yy, i64 xx) -> float {
        const i64 gg = v.gz0 + zz;
        const bool lo = (gg == 0), hi = (gg == v.gnz - 1);
        const float a = F(lo ? zz : zz - 1, yy, xx), b = F(hi ? zz : zz + 1, yy, xx);
        return (b - a) / ((lo || hi) ? hp.hz : hp.hz2);
    };
    auto GY = [&](i64 zz, i64 yy, i64 xx) -> float {
        const bool lo = (yy == 0), hi = (yy == v.ny - 1);
        const float a = F(zz, lo ? yy : yy - 1, xx), b = F(zz, hi ? yy : yy + 1, xx);
        return (b - a) / ((lo || hi) ? hp.hy : hp.hy2);
    };
    auto GX = [&](i64 zz, i64 yy, i64 xx) -> float {
        const bool lo = (xx == 0), hi = (xx == v.nx - 1);
        const float a = F(zz, yy, lo ? xx : xx - 1), b = F(zz, yy, hi ? xx : xx + 1);
        return (b - a) / ((lo || hi) ? hp.hx : hp.hx2);
    };
    h[0] = (GZ(zh, y, x) - GZ(zl, y, x)) / dz;   // hxx = d0 g0
    h[1] = (GZ(z, yh, x) - GZ(z, yl, x)) / dy;   // hxy = d1 g0
    h[2] = (GZ(z, y, xh) - GZ(z, y, xl)) / dx;   // hxz = d2 g0
    h[3] = (GY(z, yh, x) - GY(z, yl, x)) / dy;   // hyy = d1 g1
    h[4] = (GY(z, y, xh) - GY(z, y, xl)) / dx;   // hyz = d2 g1
    h[5] = (GX(z, y, xh) - GX(z, y, xl)) / dx;   // hzz = d2 g2
}

// The 2-D image case (im_info.no_z; filtering.py:461-490): "x" = axis 0 (Y), "y" = axis 1 (X).
// Component order (hxx, hxy, hyy).  True IEEE divisions: 2-D frames are small, speed is not the point.
__device__ __forceinline__ void hessian2d_at(const float *__restrict__ g, const VolGeom &v, const HessP &hp,
                                             i64 y, i64 x, float h[3]) {
    const i64 sy = v.nx;
    const bool y_lo = (y == 0), y_hi = (y == v.ny - 1);
    const bool x_lo = (x == 0), x_hi = (x == v.nx - 1);
    const i64 yl = y_lo ? y : y - 1, yh = y_hi ? y : y + 1;
    const i64 xl = x_lo ? x : x - 1, xh = x_hi ? x : x + 1;
    const float dy = (y_lo || y_hi) ? hp.hy : hp.hy2;
    const float dx = (x_lo || x_hi) ? hp.hx : hp.hx2;
    auto F = [&](i64 yy, i64 xx) -> float { return g[yy * sy + xx]; };
    auto GY = [&](i64 yy, i64 xx) -> float {
        const bool lo = (yy == 0), hi = (yy == v.ny - 1);
        return (F(hi ? yy : yy + 1, xx) - F(lo ? yy : yy - 1, xx)) / ((lo || hi) ? hp.hy : hp.hy2);
    };
    auto GX = [&](i64 yy, i64 xx) -> float {
        const bool lo = (xx == 0), hi = (xx == v.nx - 1);
        return (F(yy, hi ? xx : xx + 1) - F(yy, lo ? xx : xx - 1)) / ((lo || hi) ? hp.hx : hp.hx2);
    };
    h[0] = (GY(yh, x) - GY(yl, x)) / dy;   // hxx = d0 g0
    h[1] = (GY(y, xh) - GY(y, xl)) / dx;   // hxy = d1 g0
    h[2] = (GX(y, xh) - GX(y, xl)) / dx;   // hyy = d1 g1
}

// filtering.py:488: hxx**2 + hyy**2 + 2.0*(hxy**2), float32, left to right
__device__ __forceinline__ float frob_sq2_of(const float h[3]) {
    const float a = h[0] * h[0] + h[2] * h[2];
    const float b = 2.0f * (h[1] * h[1]);
    return a + b;
}

// filtering.py:675-690: closed-form eigenvalues of the 2x2 Hessian in float32, smaller |.| first
__device__ __forceinline__ void eig2_sorted_abs(const float h[3], float &e1, float &e2) {
    const float trace = h[0] + h[2];
    const float diff = h[0] - h[2];
    const float delta = sqrtf(diff * diff + 4.0f * (h[1] * h[1]));
    const float l1 = 0.5f * (trace - delta);
    const float l2 = 0.5f * (trace + delta);
    const bool swap = fabsf(l1) > fabsf(l2);
    e1 = swap ? l2 : l1;
    e2 = swap ? l1 : l2;
}

// filtering.py:732-741, 762-766 (2-D branch)
__device__ __forceinline__ float frangi2(float e1, float e2, float beta_sq, float gamma_sq) {
    const float rb = fabsf(e1) / (fabsf(e2) + 1e-12f);
    const float rb_sq = rb * rb;
    const float s_sq = e1 * e1 + e2 * e2;
    float v = expf(-(rb_sq / beta_sq)) * (1.0f - expf(-(s_sq / gamma_sq)));
    if (e2 > 0.0f) v = 0.0f;
    if (!(fabsf(v) <= 3.402823466e38f)) v = 0.0f;   // nan_to_num(nan=0, posinf=0, neginf=0)
    return v;
}

// filtering.py:538-543, float32, numpy's left-to-right association
__device__ __forceinline__ float frob_sq_of(const float h[6]) {
    const float a = h[0] * h[0] + h[3] * h[3] + h[5] * h[5];
    const float b = 2.0f * (h[1] * h[1] + h[2] * h[2] + h[4] * h[4]);
    return a + b;
}

// frob = sqrt(frob_sq)/max_abs with +inf -> max finite (filtering.py:421-426, 562)
__device__ __forceinline__ float frob_norm(float fsq, float max_abs, float max_finite) {
    float fr = sqrtf(fsq) / max_abs;
    if (isinf(fr)) fr = max_finite;
    return fr;
}

// -------------------------------------------------------------------------------------------------
// numpy.linalg.eigvalsh on a float32 3x3 symmetric matrix = float64 LAPACK result cast to
// float32 (numpy/linalg/_linalg.py computes in double).  Closed form in float64 (Smith 1961),
// then the |lambda| ordering of filtering.py:583-584 and the Frangi response of
// filtering.py:744-766 in float32.
// -------------------------------------------------------------------------------------------------
__device__ __forceinline__ void eig3_sorted_abs_libm(const float h[6], float &l1, float &l2, float &l3) {
    const double a00 = h[0], a01 = h[1], a02 = h[2], a11 = h[3], a12 = h[4], a22 = h[5];
    const double q = (a00 + a11 + a22) / 3.0;
    const double b00 = a00 - q, b11 = a11 - q, b22 = a22 - q;
    const double p2 = (b00 * b00 + b11 * b11 + b22 * b22 + 2.0 * (a01 * a01 + a02 * a02 + a12 * a12)) / 6.0;
    const double p = sqrt(p2);
    const double det = b00 * (b11 * b22 - a12 * a12) - a01 * (a01 * b22 - a12 * a02) + a02 * (a01 * a12 - b11 * a02);
    double r = (p2 > 0.0) ? det / (2.0 * p2 * p) : 0.0;
    r = r < -1.0 ? -1.0 : (r > 1.0 ? 1.0 : r);
    const double phi = acos(r) / 3.0;
    const double e_max = q + 2.0 * p * cos(phi);
    const double e_min = q + 2.0 * p * cos(phi + 2.0943951023931953 /* 2*pi/3 */);
    const double e_mid = 3.0 * q - e_max - e_min;
    float a = (float)e_min, b = (float)e_mid, c = (float)e_max;   // ascending, as eigvalsh returns
    // stable insertion sort by |.| (numpy argsort of 3 elements)
    float ka = fabsf(a), kb = fabsf(b), kc = fabsf(c);
    if (kb < ka) { float t = a; a = b; b = t; t = ka; ka = kb; kb = t; }
    if (kc < kb) {
        float t = b; b = c; c = t; t = kb; kb = kc; kc = t;
        if (kb < ka) { t = a; a = b; b = t; t = ka; ka = kb; kb = t; }
    }
    l1 = a; l2 = b; l3 = c;
}

// 1/sqrt(x) in float64 from the hardware estimate + two Newton steps (x > 0, normal range)
__device__ __forceinline__ double rsqrt_f64(double x) {
    double y = __builtin_amdgcn_rsq(x);
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const double t = x * y;
        const double e = fma(-t, y, 1.0);
        y = fma(0.5 * y, e, y);
    }
    return y;
}

// Stable |lambda| ordering of three ascending values (numpy argsort on 3 elements = insertion sort)
__device__ __forceinline__ void sort3_abs(float a, float b, float c, float &l1, float &l2, float &l3) {
    float ka = fabsf(a), kb = fabsf(b), kc = fabsf(c);
    if (kb < ka) { float t = a; a = b; b = t; t = ka; ka = kb; kb = t; }
    if (kc < kb) {
        float t = b; b = c; c = t; t = kb; kb = kc; kc = t;
        if (kb < ka) { t = a; a = b; b = t; t = ka; ka = kb; kb = t; }
    }
    l1 = a; l2 = b; l3 = c;
}

// Production eigen-solve: the same closed form, no libm.  With r = det(B)/(2 p^3) in [-1,1] and
// phi = acos(|r|)/3 in [0, pi/6], c = cos(phi) is the largest root of 4c^3 - 3c = |r| (c in [0.866,1],
// derivative 12c^2-3 in [6,9]: well conditioned): degree-4 starting polynomial (4.5e-6) + two Newton
// steps with a float32 reciprocal of the derivative -> 1e-16.  s = sin(phi) = sqrt(1-c^2).
//   r >= 0: e_max = q + 2pc, e_min = q - p(c + sqrt3 s);   r < 0: e_min = q - 2pc, e_max = q + p(c + sqrt3 s)
// Accuracy ~1e-16 * ||A|| (near-degenerate pairs ~1e-8 * ||A||, exactly like the acos form), so the
// float32-rounded eigenvalues equal LAPACK's except with probability ~1e-9 per value.
__device__ __forceinline__ void eig3_sorted_abs(const float h[6], float &l1, float &l2, float &l3) {
    const double a00 = h[0], a01 = h[1], a02 = h[2], a11 = h[3], a12 = h[4], a22 = h[5];
    const double q = (a00 + a11 + a22) * (1.0 / 3.0);
    const double b00 = a00 - q, b11 = a11 - q, b22 = a22 - q;
    const double off = fma(a01, a01, fma(a02, a02, a12 * a12));
    const double p2 = (fma(b00, b00, fma(b11, b11, b22 * b22)) + 2.0 * off) * (1.0 / 6.0);
    const double m0 = fma(b11, b22, -(a12 * a12));
    const double m1 = fma(a01, b22, -(a12 * a02));
    const double m2 = fma(a01, a12, -(b11 * a02));
    const double det = fma(b00, m0, fma(-a01, m1, a02 * m2));
    float ea, eb, ec;
    if (p2 > 0.0) {
        const double y = rsqrt_f64(p2);
        const double p = p2 * y;
        double r = 0.5 * det * (y * y * y);
        const bool neg = r < 0.0;
        double ra = fabs(r);
        ra = ra > 1.0 ? 1.0 : ra;
        double c = fma(fma(fma(fma(-0.004099405456413993, ra, 0.017642364887819385), ra, -0.046005261357895906), ra,
                           0.16642901838062307), ra, 0.866029853359238);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double t = c * c;
            const double f = fma(c, fma(4.0, t, -3.0), -ra);
            const double fp = fma(12.0, t, -3.0);
            c = fma(-f, (double)__builtin_amdgcn_rcpf((float)fp), c);
        }
        c = c > 1.0 ? 1.0 : c;
        const double s2 = fma(-c, c, 1.0);
        const double s = s2 > 0.0 ? s2 * rsqrt_f64(s2) : 0.0;
        const double t1 = 2.0 * p * c;
        const double t2 = p * fma(1.7320508075688772, s, c);
        const double e_max = neg ? q + t2 : q + t1;
        const double e_min = neg ? q - t1 : q - t2;
        const double e_mid = 3.0 * q - e_max - e_min;
        ea = (float)e_min; eb = (float)e_mid; ec = (float)e_max;
    } else {
        ea = eb = ec = (float)q;          // p2 == 0 (multiple of the identity) or NaN
    }
    sort3_abs(ea, eb, ec, l1, l2, l3);
}

__device__ __forceinline__ float frangi3(float l1, float l2, float l3, float alpha_sq, float beta_sq, float gamma_sq) {
    const float al2 = fabsf(l2), al3 = fabsf(l3);
    const float ra = al2 / (al3 + 1e-12f);
    const float ra_sq = ra * ra;
    const float rb = al2 / (sqrtf(fabsf(l2 * l3)) + 1e-12f);
    const float rb_sq = rb * rb;
    const float s_sq = l1 * l1 + l2 * l2 + l3 * l3;
    const float A = 1.0f - expf(-(ra_sq / alpha_sq));
    const float B = expf(-(rb_sq / beta_sq));
    const float C = 1.0f - expf(-(s_sq / gamma_sq));
    float v = A * B * C;
    if (l3 > 0.0f) v = 0.0f;
    if (l2 > 0.0f) v = 0.0f;
    if (!(fabsf(v) <= 3.402823466e38f)) v = 0.0f;   // nan_to_num(nan=0, posinf=0, neginf=0)
    return v;
}
