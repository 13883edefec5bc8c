// k_camera_kb8_unproject.hpp - the inverse half of the KannalaBrandt8 camera (reference src/CameraModels/KannalaBrandt8.cpp), beside
// k_camera_kb8.hpp's forward half: unproject (:103-130), Triangulate (:424-437), TriangulateMatches (:336-405) and so epipolarConstrain
// (:237-240, TriangulateMatches(...) > 0.0001f), with what they call restated for the device:
//   tanf32              std::tan(float) as glibc 2.35's binary32 routine evaluates it (s_tanf.c with k_tanf.c's polynomial kernel in
//                       binary32 and s_sincosf.h's argument reduction in binary64), on every float (tests/cpp/kb8_unproject_host_check.cpp
//                       compares every float of [-pi/2 - 1, pi/2 + 1], unproject's range plus slack, and a structured set outside it);
//   kb8Unproject        :103-130, every operation rounded on its own in binary32;
//   kb8TriangulateMatches  :336-405 on the above and on nullVector4 (k_small_svd.hpp: vt.row(3) of cv::SVD::compute on the 4x4 A).
// Takes kb8Project and atan2f32 from k_camera_kb8.hpp, nullVector4 from k_small_svd.hpp, sqrtFloat32 from k_small_math.hpp, gemmRow and
// dot3Double from k_match_helpers.hpp.
// Plain arithmetic only: compiles for the host behind tests/cpp/host_shim (tests/cpp/kb8_unproject_host_check.cpp).
#pragma once
#include "k_camera_kb8.hpp"
#include "k_match_helpers.hpp"
#include "k_small_math.hpp"
#include "k_small_svd.hpp"

namespace orbx {

// __kernel_tanf(x, y, iy) of k_tanf.c: tan(x + y) for iy = 1, -1 / tan(x + y) for iy = -1, |x| <= pi/4 (+ rounding)
__device__ __forceinline__ float kernelTanf32(float x, float y, int iy) {
    const float pio4 = 7.8539812565e-01f, pio4lo = 3.7748947079e-08f;
    const float T0 = 3.3333334327e-01f, T1 = 1.3333334029e-01f, T2 = 5.3968254477e-02f, T3 = 2.1869488060e-02f, T4 = 8.8632395491e-03f,
                T5 = 3.5920790397e-03f, T6 = 1.4562094584e-03f, T7 = 5.8804126456e-04f, T8 = 2.4646313977e-04f, T9 = 7.8179444245e-05f,
                T10 = 7.1407252108e-05f, T11 = -1.8558637748e-05f, T12 = 2.5907305826e-05f;
    const uint32_t hx = __float_as_uint(x), ix = hx & 0x7fffffffu;
    const bool neg = (hx >> 31) != 0;
    if (ix < 0x39000000u) {                                   // |x| < 2^-13: (int)x == 0 always
        if (iy == 1) return x;
        if (ix == 0) return __fdiv_rn(1.0f, fabsf(x));
        return __fdiv_rn(-1.0f, x);
    }
    const bool big = ix >= 0x3f2ca140u;                       // |x| >= 0.6744
    if (big) {
        if (neg) { x = -x; y = -y; }
        const float z = __fsub_rn(pio4, x), w = __fsub_rn(pio4lo, y);
        x = __fadd_rn(z, w); y = 0.0f;
        if (fabsf(x) < 0x1p-13f) {
            const int sg = neg ? -1 : 1;
            return __fmul_rn((float)(sg * iy), __fsub_rn(1.0f, __fmul_rn((float)(2 * iy), x)));
        }
    }
    float z = __fmul_rn(x, x), w = __fmul_rn(z, z);
    auto step = [&](float c, float acc) { return __fadd_rn(c, __fmul_rn(w, acc)); };
    float r = step(T1, step(T3, step(T5, step(T7, step(T9, T11)))));
    float v = __fmul_rn(z, step(T2, step(T4, step(T6, step(T8, step(T10, T12))))));
    float s = __fmul_rn(z, x);
    r = __fadd_rn(y, __fmul_rn(z, __fadd_rn(__fmul_rn(s, __fadd_rn(r, v)), y)));
    r = __fadd_rn(r, __fmul_rn(T0, s));
    w = __fadd_rn(x, r);
    if (big) {
        v = (float)iy;
        const float q = __fdiv_rn(__fmul_rn(w, w), __fadd_rn(w, v));
        const float t = __fsub_rn(v, __fmul_rn(2.0f, __fsub_rn(x, __fsub_rn(q, r))));
        return __fmul_rn(neg ? -1.0f : 1.0f, t);
    }
    if (iy == 1) return w;
    // -1 / (x + r), accurately
    z = __uint_as_float(__float_as_uint(w) & 0xfffff000u);
    v = __fsub_rn(r, __fsub_rn(z, x));
    const float a = __fdiv_rn(-1.0f, w);
    const float t = __uint_as_float(__float_as_uint(a) & 0xfffff000u);
    s = __fadd_rn(1.0f, __fmul_rn(t, z));
    return __fadd_rn(t, __fmul_rn(a, __fadd_rn(s, __fmul_rn(t, v))));
}

// tanf (s_tanf.c): |x| <= pi/4 goes to the kernel as it is; otherwise the argument is reduced in binary64 as sinf / cosf reduce theirs
// (s_sincosf.h): below 120 by x - n * pi/2 with n = round(x * 2/pi) taken from a 2^24-scaled product, from 120 up by a 192-bit window of
// 2 / pi (reduceLarge); the reduced double is split into a float and the float of the remainder, and n's parity selects tan or -1 / tan.
__device__ __forceinline__ double tanReduceLarge(uint32_t xi, int* np) {
    // 4 / pi in 32-bit windows that advance by 8 bits (__inv_pio4)
    static constexpr uint32_t kInvPio4[24] = {0x000000a2u, 0x0000a2f9u, 0x00a2f983u, 0xa2f9836eu, 0xf9836e4eu, 0x836e4e44u, 0x6e4e4415u, 0x4e441529u,
                                              0x441529fcu, 0x1529fc27u, 0x29fc2757u, 0xfc2757d1u, 0x2757d1f5u, 0x57d1f534u, 0xd1f534ddu, 0xf534ddc0u,
                                              0x34ddc0dbu, 0xddc0db62u, 0xc0db6295u, 0xdb629599u, 0x6295993cu, 0x95993c43u, 0x993c4390u, 0x3c439041u};
    const uint32_t* arr = &kInvPio4[(xi >> 26) & 15];
    const int shift = (int)((xi >> 23) & 7);
    xi = ((xi & 0xffffffu) | 0x800000u) << shift;
    uint64_t res0 = (uint64_t)(uint32_t)(xi * arr[0]);
    const uint64_t res1 = (uint64_t)xi * arr[4], res2 = (uint64_t)xi * arr[8];
    res0 = (res2 >> 32) | (res0 << 32);
    res0 += res1;
    const uint64_t n = (res0 + (1ull << 61)) >> 62;
    res0 -= n << 62;
    *np = (int)n;
    return __dmul_rn((double)(int64_t)res0, 0x1.921FB54442D18p-62);
}
__device__ __forceinline__ float tanf32(float x) {
    const double hpi_inv = 0x1.45F306DC9C883p+23, hpi = 0x1.921FB54442D18p0;
    const uint32_t hx = __float_as_uint(x), ix = hx & 0x7fffffffu;
    if (ix <= 0x3f490fdau) return kernelTanf32(x, 0.0f, 1);
    if (ix >= 0x7f800000u) return __fsub_rn(x, x);            // infinities and NaN
    double xr;
    int n;
    if (((hx >> 20) & 0x7ffu) <= 0x42eu) {                    // |x| < 120
        const double r = __dmul_rn((double)x, hpi_inv);
        n = ((int)r + 0x800000) >> 24;
        xr = __dsub_rn((double)x, __dmul_rn((double)n, hpi));
    } else {
        xr = tanReduceLarge(hx, &n);
        if (hx >> 31) xr = -xr;
    }
    const float y0 = (float)xr, y1 = (float)__dsub_rn(xr, (double)y0);
    return kernelTanf32(y0, y1, 1 - ((n & 1) << 1));
}

// fmaxf / fminf: a NaN operand gives the other one
__device__ __forceinline__ float kb8Fmax(float a, float b) { return a != a ? b : b != b ? a : (a < b ? b : a); }
__device__ __forceinline__ float kb8Fmin(float a, float b) { return a != a ? b : b != b ? a : (b < a ? b : a); }

// KannalaBrandt8::unproject (:103-130): the ray (rx, ry, 1) of pixel (u, v).  k = mvParameters[0..7].
//   * fminf(fmaxf(-CV_PI / 2.f, theta_d), CV_PI / 2.f): CV_PI is a double, CV_PI / 2.f a double quotient, and fmaxf / fminf take floats: the
//     bound each call sees is (float)(pi / 2) = 0x3fc90fdb.  A NaN theta_d leaves fmaxf as -pi/2 (fmaxf returns its other operand), and
//     the scale stays 1;
//   * theta_d > 1e-8 promotes theta_d to double;
//   * precision is `const float precision` = 1e-6 (KannalaBrandt8.h): fabsf(theta_fix) < precision compares two floats, which is the compare
//     of their promotions;
//   * std::tan on a float is the float overload (DESIGN.md §2 divergence (3)).
__device__ __forceinline__ void kb8Unproject(const float (&k)[8], float u, float v, float& rx, float& ry) {
    const float pio2 = 1.5707963705e+00f, precision = 1e-6f;
    const float pwx = __fdiv_rn(__fsub_rn(u, k[2]), k[0]), pwy = __fdiv_rn(__fsub_rn(v, k[3]), k[1]);
    float scale = 1.0f;
    float theta_d = sqrtFloat32(__fadd_rn(__fmul_rn(pwx, pwx), __fmul_rn(pwy, pwy)));
    theta_d = kb8Fmin(kb8Fmax(-pio2, theta_d), pio2);
    if ((double)theta_d > 1e-8) {
        float theta = theta_d;
        for (int j = 0; j < 10; j++) {
            const float theta2 = __fmul_rn(theta, theta), theta4 = __fmul_rn(theta2, theta2), theta6 = __fmul_rn(theta4, theta2),
                        theta8 = __fmul_rn(theta4, theta4);
            const float a = __fmul_rn(k[4], theta2), b = __fmul_rn(k[5], theta4), c = __fmul_rn(k[6], theta6), d = __fmul_rn(k[7], theta8);
            const float num = __fsub_rn(__fmul_rn(theta, __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(1.0f, a), b), c), d)), theta_d);
            const float den = __fadd_rn(__fadd_rn(__fadd_rn(__fadd_rn(1.0f, __fmul_rn(3.0f, a)), __fmul_rn(5.0f, b)), __fmul_rn(7.0f, c)),
                                        __fmul_rn(9.0f, d));
            const float fix = __fdiv_rn(num, den);
            theta = __fsub_rn(theta, fix);
            if (fabsf(fix) < precision) break;
        }
        scale = __fdiv_rn(tanf32(theta), theta_d);
    }
    rx = __fmul_rn(pwx, scale);
    ry = __fmul_rn(pwy, scale);
}

// what depends on the eye combination only: R12 (row-major), R21 = R12.t(), t21 = -R21*t12 (one gemm, alpha = -1; :365-366)
struct Kb8Relative { float R12[9], R21[9], t21[3]; };
__device__ __forceinline__ void kb8RelativeFrom(const float* R12, const float* t12, Kb8Relative& q) {
    const float t[3] = {t12[0], t12[1], t12[2]};
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) { q.R12[3 * r + c] = R12[3 * r + c]; q.R21[3 * r + c] = R12[3 * c + r]; }
    for (int r = 0; r < 3; r++) q.t21[r] = gemmRow(q.R21[3 * r], q.R21[3 * r + 1], q.R21[3 * r + 2], t, -1.0, 0.f, false);
}

// why kb8TriangulateMatches left (== ORBX_TRIANGULATE_*)
enum { kTriOk = 0, kTriParallax, kTriZ1, kTriZ2, kTriError1, kTriError2 };

// KannalaBrandt8::TriangulateMatches (:336-405) on rays already unprojected: ray1 = (r1x, r1y, 1) of kp1 under camera 1, ray2 of kp2 under
// camera 2.  gate1 = 5.991 * sigmaLevel, gate2 = 5.991 * unc, the float promoted and the product in double (:388, :398).  Returns z1 or -1;
// x3D is the triangulated point, zeros when the parallax test left (callers use it only when the result is accepted).
// Roundings ("parity unpinned" where a cv::MatExpr hides them):
//   r21 = R12*r2 one gemmRow per row; Mat::dot and cv::norm accumulate products in double, the quotient is rounded to float, the compare
//   with 0.9998 is in double; a row of A is float(p * T.row(2)[c]) - T.row(r)[c], each rounded in float; x3D = v[0..2] / v[3] is a float
//   division per element; z2 is a double sum rounded once; x3D2 = R21*x3D + t21 one gemmRow with the addend per row.
// A zero fourth component gives infinities or NaN, on which every <= and > below is false: the result is that NaN or infinity's z1, and
// epipolarConstrain's z > 0.0001f decides (NaN rejects).
__device__ __forceinline__ float kb8TriangulateMatches(const float (&k1)[8], const float (&k2)[8], float r1x, float r1y, float r2x, float r2y,
                                                       float u1, float v1, float u2, float v2, const Kb8Relative& q, double gate1,
                                                       double gate2, float (&x3D)[3], int& why) {
    const float r2[3] = {r2x, r2y, 1.0f};
    float r21[3];
#pragma unroll
    for (int r = 0; r < 3; r++) r21[r] = gemmRow(q.R12[3 * r], q.R12[3 * r + 1], q.R12[3 * r + 2], r2, 1.0, 0.f, false);
    const double dot = dot3Double(r1x, r1y, 1.0f, r21[0], r21[1], r21[2]);
    const double n1 = __dsqrt_rn(dot3Double(r1x, r1y, 1.0f, r1x, r1y, 1.0f)), n2 = __dsqrt_rn(dot3Double(r21[0], r21[1], r21[2], r21[0], r21[1], r21[2]));
    const float cosParallaxRays = (float)__ddiv_rn(dot, __dmul_rn(n1, n2));
    // From here on nothing returns early: every stage is computed for every lane and the FIRST failing test decides at the end.  The lanes
    // of a wave run in lockstep, so a lane that left early would wait for the others anyway, and each early return is a divergent region
    // whose saved exec mask stays live across the two projections below (the search kernel spilled scalar registers over them).
    const bool leftParallax = (double)cosParallaxRays > 0.9998;
    // A (:428-431): Tcw1 is the identity, Tcw2 = [R21 | t21]
    float A[16];
    const float I[12] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
    float T2[12];
#pragma unroll
    for (int r = 0; r < 3; r++) { T2[4 * r] = q.R21[3 * r]; T2[4 * r + 1] = q.R21[3 * r + 1]; T2[4 * r + 2] = q.R21[3 * r + 2]; T2[4 * r + 3] = q.t21[r]; }
#pragma unroll
    for (int c = 0; c < 4; c++) {
        A[c] = __fsub_rn(__fmul_rn(r1x, I[8 + c]), I[c]);
        A[4 + c] = __fsub_rn(__fmul_rn(r1y, I[8 + c]), I[4 + c]);
        A[8 + c] = __fsub_rn(__fmul_rn(r2x, T2[8 + c]), T2[c]);
        A[12 + c] = __fsub_rn(__fmul_rn(r2y, T2[8 + c]), T2[4 + c]);
    }
    float vt[4];
    nullVector4(A, vt);
#pragma unroll
    for (int r = 0; r < 3; r++) x3D[r] = __fdiv_rn(vt[r], vt[3]);
    const float z1 = x3D[2];
    const float z2 = (float)__dadd_rn(dot3Double(q.R21[6], q.R21[7], q.R21[8], x3D[0], x3D[1], x3D[2]), (double)q.t21[2]);
    float pu, pv;
    kb8Project(k1, x3D[0], x3D[1], x3D[2], pu, pv);
    const float e1x = __fsub_rn(pu, u1), e1y = __fsub_rn(pv, v1);
    const bool leftError1 = (double)__fadd_rn(__fmul_rn(e1x, e1x), __fmul_rn(e1y, e1y)) > gate1;
    float x2[3];
#pragma unroll
    for (int r = 0; r < 3; r++) x2[r] = gemmRow(q.R21[3 * r], q.R21[3 * r + 1], q.R21[3 * r + 2], x3D, 1.0, q.t21[r], true);
    kb8Project(k2, x2[0], x2[1], x2[2], pu, pv);
    const float e2x = __fsub_rn(pu, u2), e2y = __fsub_rn(pv, v2);
    const bool leftError2 = (double)__fadd_rn(__fmul_rn(e2x, e2x), __fmul_rn(e2y, e2y)) > gate2;
    // the reference's order of returns (:345, :373, :378, :388, :398)
    why = leftParallax ? kTriParallax : z1 <= 0.0f ? kTriZ1 : z2 <= 0.0f ? kTriZ2 : leftError1 ? kTriError1 : leftError2 ? kTriError2 : kTriOk;
    if (leftParallax) x3D[0] = x3D[1] = x3D[2] = 0.0f;
    return why == kTriOk ? z1 : -1.0f;
}

}  // namespace orbx
