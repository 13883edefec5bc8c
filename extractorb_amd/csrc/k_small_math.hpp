// k_small_math.hpp - the scalar and three-vector arithmetic that the geometry entries share, each stated ONCE under a name that belongs to no
// feature: the float square root, the quiet NaN, the library's binary64 atan2 / sin / cos, the draw
// without replacement from raw rand() values, Pinhole project / unproject, a 3x4 pose times a point, and the one wave question the
// statements ask (waveAny).  Every one of them is a definition the project owns ("parity unpinned") or a line of the
// reference that several entries restate; a correction here reaches every user.  The Jacobi routines are k_small_svd.hpp's.
// A LEAF: it takes gemmRow from k_match_helpers.hpp and nothing from any feature header.  (dot3Double stands there too, beside gemmRow:
// the per-frame matchers call it, and their host builds know only the words that header uses.)
// Plain arithmetic (waveAny is the lane's own bit in the host build, ORBX_HOST_ROW): compiles for the host behind tests/cpp/host_shim, and
// tests/cpp/small_math_check.cpp tests these statements directly.  A device word this header gains needs its stand-in in the shim.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_match_helpers.hpp"

namespace orbx {

// sqrtf.  Not __fsqrt_rn: without OCML_BASIC_ROUNDED_OPERATIONS HIP maps that name to the hardware's approximate root (1 ulp), which moved
// 3 % of the KannalaBrandt8 projections by one float.  The correctly rounded binary64 root of a binary32 number, rounded to binary32, is the
// correctly rounded binary32 root (53 >= 2 * 24 + 2 bits), and __dsqrt_rn is IEEE.
__device__ __forceinline__ float sqrtFloat32(float x) { return (float)__dsqrt_rn((double)x); }

// THE quiet NaN: which NaN 0 * inf gives differs between host and device arithmetic, so every NaN leaves in a result row as this one
__device__ __forceinline__ float quietNaN() { return __uint_as_float(0x7fc00000u); }
__device__ __forceinline__ float canonNaN(float x) { return x != x ? quietNaN() : x; }
__device__ __forceinline__ double canonNaN(double x) { return x != x ? (double)quietNaN() : x; }

// whether any lane of the wave says so (a ballot; the lane's own bit in the host build, where a wave is one lane)
#ifdef ORBX_HOST_ROW
__device__ __forceinline__ bool waveAny(bool b) { return b; }
#else
__device__ __forceinline__ bool waveAny(bool b) { return __ballot(b) != 0ull; }
#endif

// ---- the double functions -----------------------------------------------------------------------------------------------------------------
// The double atan2 / sin / cos of Sim3Solver and PoseOptimization, stated in plain binary64 operations so that the host build and the device
// agree by construction: atan of a ratio in [0, 1] by two half-angle steps t / (1 + sqrt(1 + t^2)) and twelve terms of the odd series, moved
// to the octant by pi / 2 and pi as hi + lo pairs; sin / cos by a three-part reduction against pi / 2 and the Taylor series to r^19 / r^20.
// Not libm's roundings (docs/history/r24_sim3_solver.md measures the difference).  atan2Double is stated for y >= 0 (a norm); a NaN argument
// gives NaN, sinCosDouble of a NaN, of a negative angle or of more than 2^20 gives NaN.
// atan(t), 0 <= t <= 1
__device__ __forceinline__ double atanUnitDouble(double t) {
    const double t1 = __ddiv_rn(t, __dadd_rn(1.0, __dsqrt_rn(__dadd_rn(1.0, __dmul_rn(t, t)))));
    const double t2 = __ddiv_rn(t1, __dadd_rn(1.0, __dsqrt_rn(__dadd_rn(1.0, __dmul_rn(t1, t1)))));      // <= tan(pi / 16)
    const double z = __dmul_rn(t2, t2);
    double acc = __ddiv_rn(1.0, 23.0);
#pragma unroll
    for (int k = 10; k >= 0; k--) acc = __dsub_rn(__ddiv_rn(1.0, (double)(2 * k + 1)), __dmul_rn(z, acc));
    return __dmul_rn(4.0, __dmul_rn(t2, acc));
}
// atan2(y, x) for y >= 0
__device__ __forceinline__ double atan2Double(double y, double x) {
    const double pio2Hi = 0x1.921fb54442d18p+0, pio2Lo = 0x1.1a62633145c07p-54, piHi = 0x1.921fb54442d18p+1, piLo = 0x1.1a62633145c07p-53;
    if (y != y || x != x) return (double)quietNaN();
    const double ax = fabs(x), big = y > ax ? y : ax, small = y > ax ? ax : y;
    double a = big == 0.0 ? 0.0 : atanUnitDouble(big == small ? 1.0 : __ddiv_rn(small, big));     // (inf / inf is atan(1))
    if (y > ax) a = __dadd_rn(__dsub_rn(pio2Hi, a), pio2Lo);
    if (x < 0.0) a = __dadd_rn(__dsub_rn(piHi, a), piLo);
    return a;
}
__device__ __forceinline__ void sinCosDouble(double theta, double& s, double& c) {
    if (!(theta >= 0.0 && theta < 1048576.0)) { s = c = (double)quietNaN(); return; }
    const double twoOverPi = 0x1.45f306dc9c883p-1, p1 = 0x1.921fb54400000p+0, p2 = 0x1.0b4611a600000p-34, p3 = 0x1.3198a2e037073p-69;
    const int k = (int)__dadd_rn(__dmul_rn(theta, twoOverPi), 0.5);
    const double kd = (double)k;
    const double r = __dsub_rn(__dsub_rn(__dsub_rn(theta, __dmul_rn(kd, p1)), __dmul_rn(kd, p2)), __dmul_rn(kd, p3));
    const double z = __dmul_rn(r, r);
    // sin r = r * (1 - z/3! + ... - z^9/19!), cos r = 1 - z/2! + ... + z^10/20!
    const double sd[10] = {1.0, 6.0, 120.0, 5040.0, 362880.0, 39916800.0, 6227020800.0, 1307674368000.0, 355687428096000.0, 121645100408832000.0};
    const double cd[11] = {1.0, 2.0, 24.0, 720.0, 40320.0, 3628800.0, 479001600.0, 87178291200.0, 20922789888000.0, 6402373705728000.0,
                           2432902008176640000.0};
    double ps = __ddiv_rn(1.0, sd[9]), pc = __ddiv_rn(1.0, cd[10]);
#pragma unroll
    for (int i = 8; i >= 0; i--) ps = __dsub_rn(__ddiv_rn(1.0, sd[i]), __dmul_rn(z, ps));
#pragma unroll
    for (int i = 9; i >= 0; i--) pc = __dsub_rn(__ddiv_rn(1.0, cd[i]), __dmul_rn(z, pc));
    const double sr = __dmul_rn(r, ps), cr = pc;
    const int quad = k & 3;
    s = quad == 0 ? sr : quad == 1 ? cr : quad == 2 ? -sr : -cr;
    c = quad == 0 ? cr : quad == 1 ? -sr : quad == 2 ? -cr : sr;
}

// ---- the draw without replacement ---------------------------------------------------------------------------------------------------------
// K indices out of [0, N) from K raw rand() values r (ints of [0, 2^31 - 1]), as TwoViewReconstruction's mvSets (K = 8) and Sim3Solver's
// iterate (K = 3) draw them: randi = int(((double)r / 2147483648.0) * size) (DUtils/Random.cpp:47-50) with size = N - j, idx = avail[randi],
// avail[randi] = avail.back(), pop_back.  The list is the identity with at most K displaced slots, kept in registers.  randi is clamped
// into [0, size - 1]: a value outside [0, 2^31 - 1] is the caller's error and must not index outside the list.
template <int K>
__device__ __forceinline__ void drawSet(const int* __restrict__ raw, int N, int (&idx)[K]) {
    int slot[K], val[K];
#pragma unroll
    for (int j = 0; j < K; j++) {
        const int size = N - j;
        int randi = (int)__dmul_rn(__ddiv_rn((double)raw[j], 2147483648.0), (double)size);
        randi = max(0, min(randi, size - 1));
        int va = randi, vb = size - 1;
#pragma unroll
        for (int t = 0; t < j; t++) {                       // ascending: the latest displacement of a slot wins
            if (slot[t] == randi) va = val[t];
            if (slot[t] == size - 1) vb = val[t];
        }
        idx[j] = va; slot[j] = randi; val[j] = vb;
    }
}

// ---- Pinhole and a pose ---------------------------------------------------------------------------------------------------------------------
// Pinhole::project (Pinhole.cpp:30-33) fx * x / z + cx and Pinhole::unproject (:59-62) (u - cx) / fx in binary32 as written, k = fx, fy, cx, cy
__device__ __forceinline__ void pinholeProject(const float (&k)[8], float x, float y, float z, float& u, float& v) {
    u = __fadd_rn(__fdiv_rn(__fmul_rn(k[0], x), z), k[2]);
    v = __fadd_rn(__fdiv_rn(__fmul_rn(k[1], y), z), k[3]);
}
__device__ __forceinline__ void pinholeUnproject(const float (&k)[8], float u, float v, float& x, float& y) {
    x = __fdiv_rn(__fsub_rn(u, k[2]), k[0]);
    y = __fdiv_rn(__fsub_rn(v, k[3]), k[1]);
}
// Rcw * X + tcw of a 3x4 row-major T: one gemmRow per row with the addend
__device__ __forceinline__ void transformPoint(const float* T, const float (&X)[3], float (&out)[3]) {
#pragma unroll
    for (int r = 0; r < 3; r++) out[r] = gemmRow(T[4 * r], T[4 * r + 1], T[4 * r + 2], X, 1.0, T[4 * r + 3], true);
}

}  // namespace orbx
