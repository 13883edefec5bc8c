// k_acosf.hpp - std::acos(float) as glibc 2.35's binary32 routine evaluates it (sysdeps/ieee754/flt-32/e_acosf.c: the rational
// approximation of asin on [0, 0.5], the half-angle forms beyond it), every operation rounded on its own in binary32, restated for the
// device in the manner of k_camera_kb8.hpp.  TwoViewReconstruction::CheckRT (reference src/TwoViewReconstruction.cc:904) calls it through
// `using namespace std` on a float.  tests/cpp/two_view_host_check.cpp compares it with the host libm on every float of [0.9, 1], on a
// fixed stride over the rest of [-1, 1] and on the values outside the domain (which give NaN).
// Takes sqrtFloat32 from k_small_math.hpp.  Plain arithmetic only: compiles for the host behind tests/cpp/host_shim.
#pragma once
#include "k_small_math.hpp"

namespace orbx {

__device__ __forceinline__ float acosfRational(float z) {      // p / q of e_acosf.c
    const float pS0 = 1.6666667163e-01f, pS1 = -3.2556581497e-01f, pS2 = 2.0121252537e-01f, pS3 = -4.0055535734e-02f, pS4 = 7.9153501429e-04f,
                pS5 = 3.4793309169e-05f, qS1 = -2.4033949375e+00f, qS2 = 2.0209457874e+00f, qS3 = -6.8828397989e-01f, qS4 = 7.7038154006e-02f;
    auto step = [&](float c, float acc) { return __fadd_rn(c, __fmul_rn(z, acc)); };
    const float p = __fmul_rn(z, step(pS0, step(pS1, step(pS2, step(pS3, step(pS4, pS5))))));
    const float q = step(1.0f, step(qS1, step(qS2, step(qS3, qS4))));
    return __fdiv_rn(p, q);
}

__device__ __forceinline__ float acosFloat32(float x) {
    const float pi = 3.1415925026e+00f, pio2_hi = 1.5707962513e+00f, pio2_lo = 7.5497894159e-08f;
    const uint32_t hx = __float_as_uint(x), ix = hx & 0x7fffffffu;
    const bool neg = (hx >> 31) != 0;
    if (ix == 0x3f800000u) return neg ? __fadd_rn(pi, __fmul_rn(2.0f, pio2_lo)) : 0.0f;      // |x| == 1
    if (ix > 0x3f800000u) { const float d = __fsub_rn(x, x); return __fdiv_rn(d, d); }       // |x| > 1, infinities, NaN: NaN
    if (ix < 0x3f000000u) {                                                                   // |x| < 0.5
        if (ix <= 0x23000000u) return __fadd_rn(pio2_hi, pio2_lo);
        const float r = acosfRational(__fmul_rn(x, x));
        return __fsub_rn(pio2_hi, __fsub_rn(x, __fsub_rn(pio2_lo, __fmul_rn(r, x))));
    }
    if (neg) {                                                                                // x <= -0.5
        const float z = __fmul_rn(__fadd_rn(1.0f, x), 0.5f), r = acosfRational(z), s = sqrtFloat32(z);
        const float w = __fsub_rn(__fmul_rn(r, s), pio2_lo);
        return __fsub_rn(pi, __fmul_rn(2.0f, __fadd_rn(s, w)));
    }
    const float z = __fmul_rn(__fsub_rn(1.0f, x), 0.5f), s = sqrtFloat32(z);                      // x >= 0.5
    const float df = __uint_as_float(__float_as_uint(s) & 0xfffff000u);
    const float c = __fdiv_rn(__fsub_rn(z, __fmul_rn(df, df)), __fadd_rn(s, df));
    const float r = acosfRational(z), w = __fadd_rn(__fmul_rn(r, s), c);
    return __fmul_rn(2.0f, __fadd_rn(df, w));
}

}  // namespace orbx
