// k_camera_kb8.hpp - KannalaBrandt8::project(const cv::Point3f&) (reference src/CameraModels/KannalaBrandt8.cpp:28-44), the camera model of
// the two-camera (fisheye, Nleft != -1) rigs, with the libm calls it makes restated for the device: atan2f / atanf as the binary32 (flt-32)
// routines of glibc 2.35 evaluate them, sinf / cosf as k_describe_body.hpp's sincosGlibc does (the same statement, repeated here so that this
// header stands alone: |psi| <= pi lies inside the range that routine reduces, negative arguments take the same path).  Every operation is
// rounded individually in binary32 (the reference's x86-64 build has no FMA), the sine / cosine polynomials in binary64 as libm has them.
// Every Nleft != -1 / bRight branch projects with this: isInFrustumChecks (k_frustum_two_eyes_point.hpp) and Fuse's bRight
// (k_fuse_two_eyes.hip) are built on it.  It is built once, here.  cos(psi) / sin(psi) on a float are taken as the float overloads (DESIGN.md §2 divergence (3)).
// sqrtf is sqrtFloat32 of k_small_math.hpp, the one thing this header takes from another.
// Plain arithmetic only: compiles for the host behind tests/cpp/host_shim (tests/cpp/kb8_host_check.cpp proves each routine against libm).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_small_math.hpp"

namespace orbx {

// atanf: the argument is reduced against 7/16, 11/16, 19/16, 39/16 to one of atan(0.5), atan(1), atan(1.5), pi/2 (hi + lo pairs) plus the
// arc tangent of a small remainder, an odd 11-term polynomial split into its even and odd halves.
__device__ __forceinline__ float atanf32(float x) {
    // atan(0.5), atan(1), atan(1.5), pi/2 as hi + lo (scalars, not a table: nothing here is indexed at run time)
    const float hi0 = 4.6364760399e-01f, hi1 = 7.8539812565e-01f, hi2 = 9.8279368877e-01f, hi3 = 1.5707962513e+00f;
    const float lo0 = 5.0121582440e-09f, lo1 = 3.7748947079e-08f, lo2 = 3.4473217170e-08f, lo3 = 7.5497894159e-08f;
    const float aT0 = 3.3333334327e-01f, aT1 = -2.0000000298e-01f, aT2 = 1.4285714924e-01f, aT3 = -1.1111110449e-01f,
                aT4 = 9.0908870101e-02f, aT5 = -7.6918758452e-02f, aT6 = 6.6610731184e-02f, aT7 = -5.8335702866e-02f,
                aT8 = 4.9768779427e-02f, aT9 = -3.6531571299e-02f, aT10 = 1.6285819933e-02f;
    const uint32_t bits = __float_as_uint(x), ix = bits & 0x7fffffffu;
    const bool neg = (bits >> 31) != 0;
    if (ix >= 0x4c000000u) {                               // |x| >= 2^25 (not 2^26), infinities and NaN
        if (ix > 0x7f800000u) return __fadd_rn(x, x);
        const float r = __fadd_rn(hi3, lo3);
        return neg ? -r : r;
    }
    bool reduced = false;
    float hi = 0.0f, lo = 0.0f;
    if (ix < 0x3ee00000u) {                                // |x| < 7/16: no reduction
        if (ix < 0x31000000u) return x;                    // |x| < 2^-29
    } else {
        reduced = true;
        x = fabsf(x);
        if (ix < 0x3f980000u) {                            // |x| < 19/16
            if (ix < 0x3f300000u) { hi = hi0; lo = lo0; x = __fdiv_rn(__fsub_rn(__fmul_rn(2.0f, x), 1.0f), __fadd_rn(2.0f, x)); }      // 7/16 <= |x| < 11/16
            else { hi = hi1; lo = lo1; x = __fdiv_rn(__fsub_rn(x, 1.0f), __fadd_rn(x, 1.0f)); }
        } else {
            if (ix < 0x401c0000u) { hi = hi2; lo = lo2; x = __fdiv_rn(__fsub_rn(x, 1.5f), __fadd_rn(1.0f, __fmul_rn(1.5f, x))); }      // |x| < 39/16
            else { hi = hi3; lo = lo3; x = __fdiv_rn(-1.0f, x); }
        }
    }
    const float z = __fmul_rn(x, x), w = __fmul_rn(z, z);
    auto step = [&](float c, float acc) { return __fadd_rn(c, __fmul_rn(w, acc)); };
    const float s1 = __fmul_rn(z, step(aT0, step(aT2, step(aT4, step(aT6, step(aT8, aT10))))));
    const float s2 = __fmul_rn(w, step(aT1, step(aT3, step(aT5, step(aT7, aT9)))));
    const float xs = __fmul_rn(x, __fadd_rn(s1, s2));
    if (!reduced) return __fsub_rn(x, xs);
    const float r = __fsub_rn(hi, __fsub_rn(__fsub_rn(xs, lo), x));
    return neg ? -r : r;
}

// atan2f(y, x): the table of zeros and infinities, then atanf(|y / x|) moved to the quadrant of (x, y)
__device__ __forceinline__ float atan2f32(float y, float x) {
    const float tiny = 1.0e-30f, pi = 3.1415927410e+00f, pi_o_2 = 1.5707963705e+00f, pi_o_4 = 7.8539818525e-01f, pi_lo = -8.7422776573e-08f;
    const uint32_t hx = __float_as_uint(x), hy = __float_as_uint(y), ix = hx & 0x7fffffffu, iy = hy & 0x7fffffffu;
    if (ix > 0x7f800000u || iy > 0x7f800000u) return __fadd_rn(x, y);
    if (hx == 0x3f800000u) return atanf32(y);
    const int m = (int)(hy >> 31) | (int)((hx >> 30) & 2u);      // sign(y) | 2 * sign(x)
    const bool yneg = (hy >> 31) != 0;
    if (iy == 0) return m < 2 ? y : (m == 2 ? __fadd_rn(pi, tiny) : __fsub_rn(-pi, tiny));
    if (ix == 0) return yneg ? __fsub_rn(-pi_o_2, tiny) : __fadd_rn(pi_o_2, tiny);
    if (ix == 0x7f800000u) {
        if (iy == 0x7f800000u) {
            const float q3 = __fmul_rn(3.0f, pi_o_4);
            return m == 0 ? __fadd_rn(pi_o_4, tiny) : m == 1 ? __fsub_rn(-pi_o_4, tiny) : m == 2 ? __fadd_rn(q3, tiny) : __fsub_rn(-q3, tiny);
        }
        return m == 0 ? 0.0f : m == 1 ? -0.0f : m == 2 ? __fadd_rn(pi, tiny) : __fsub_rn(-pi, tiny);
    }
    if (iy == 0x7f800000u) return yneg ? __fsub_rn(-pi_o_2, tiny) : __fadd_rn(pi_o_2, tiny);
    const int k = ((int)iy - (int)ix) >> 23;
    float z;
    if (k > 60) z = __fadd_rn(pi_o_2, __fmul_rn(0.5f, pi_lo));      // |y / x| > 2^60
    else if ((hx >> 31) && k < -60) z = 0.0f;                        // |y| / x < -2^-60
    else z = atanf32(fabsf(__fdiv_rn(y, x)));
    switch (m) {
        case 0: return z;
        case 1: return -z;
        case 2: return __fsub_rn(pi, __fsub_rn(z, pi_lo));
        default: return __fsub_rn(__fsub_rn(z, pi_lo), pi);
    }
}

// sinf / cosf as glibc >= 2.28 evaluates them for |y| < 120 (here: [-pi, pi]): double-precision minimax polynomials after a quadrant
// reduction.  The statement of k_describe_body.hpp's sincosGlibc; a negative y gives a negative quadrant n, whose low bits select
// polynomial and sign as they do for a positive one.
__device__ __forceinline__ void kb8SinCos(float y, float* s_out, float* c_out) {
    const double hpi_inv = 0x1.45F306DC9C883p+23, hpi = 0x1.921FB54442D18p0;
    const double C0 = 0x1p0, C1 = -0x1.ffffffd0c621cp-2, C2 = 0x1.55553e1068f19p-5, C3 = -0x1.6c087e89a359dp-10, C4 = 0x1.99343027bf8c3p-16;
    const double S1 = -0x1.555545995a603p-3, S2 = 0x1.1107605230bc4p-7, S3 = -0x1.994eb3774cf24p-13;
    double x = (double)y;
    const unsigned top12 = (__float_as_uint(y) >> 20) & 0x7ff;
    int n = 0;
    if (top12 < 0x3f4) {
        if (top12 < 0x398) { *s_out = y; *c_out = 1.0f; return; }
    } else {
        const double r = __dmul_rn(x, hpi_inv);
        n = ((int)r + 0x800000) >> 24;
        x = __dsub_rn(x, __dmul_rn((double)n, hpi));
    }
    const double x2 = __dmul_rn(x, x);
    auto polySin = [&](double xx) {
        const double x3 = __dmul_rn(xx, x2), s1 = __dadd_rn(S2, __dmul_rn(x2, S3)), x7 = __dmul_rn(x3, x2), s = __dadd_rn(xx, __dmul_rn(x3, S1));
        return __dadd_rn(s, __dmul_rn(x7, s1));
    };
    auto polyCos = [&](double sg) {
        const double x4 = __dmul_rn(x2, x2), c2 = __dadd_rn(sg * C3, __dmul_rn(x2, sg * C4)), c1 = __dadd_rn(sg * C0, __dmul_rn(x2, sg * C1)),
                     x6 = __dmul_rn(x4, x2), c = __dadd_rn(c1, __dmul_rn(x4, sg * C2));
        return __dadd_rn(c, __dmul_rn(x6, c2));
    };
    const bool odd = (n & 1) != 0;
    const int ns = odd ? n + 1 : n, nc = odd ? n : n + 1;
    const double sgnS = ((ns & 3) == 1 || (ns & 3) == 2) ? -1.0 : 1.0;
    const float ps = (float)polySin(x * sgnS), pc = (float)polyCos((nc & 2) ? -1.0 : 1.0);
    *s_out = odd ? pc : ps;
    *c_out = odd ? ps : pc;
}

// KannalaBrandt8::project: k = mvParameters[0..7] = fx, fy, cx, cy, k1, k2, k3, k4
__device__ __forceinline__ void kb8Project(const float (&k)[8], float x, float y, float z, float& u, float& v) {
    const float x2y2 = __fadd_rn(__fmul_rn(x, x), __fmul_rn(y, y));
    const float theta = atan2f32(sqrtFloat32(x2y2), z);
    const float psi = atan2f32(y, x);
    const float theta2 = __fmul_rn(theta, theta), theta3 = __fmul_rn(theta, theta2), theta5 = __fmul_rn(theta3, theta2),
                theta7 = __fmul_rn(theta5, theta2), theta9 = __fmul_rn(theta7, theta2);
    const float r = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(theta, __fmul_rn(k[4], theta3)), __fmul_rn(k[5], theta5)), __fmul_rn(k[6], theta7)),
                              __fmul_rn(k[7], theta9));
    float s, c;
    kb8SinCos(psi, &s, &c);
    u = __fadd_rn(__fmul_rn(__fmul_rn(k[0], r), c), k[2]);
    v = __fadd_rn(__fmul_rn(__fmul_rn(k[1], r), s), k[3]);
}

// sqrtFloat32's earlier name, ONLY for tests/cpp/kb8_host_check.cpp, which the existing tests build as it is; the library does not call it
__device__ __forceinline__ float kb8Sqrt(float x) { return sqrtFloat32(x); }

}  // namespace orbx
