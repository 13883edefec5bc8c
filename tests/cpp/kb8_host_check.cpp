// kb8_host_check.cpp - extractorb_amd/csrc/k_camera_kb8.hpp compiled for the HOST (tests/cpp/host_shim stands in for the device vocabulary)
// against the host libm: atan2f32 / atanf32 against atan2f / atanf, kb8SinCos against sinf / cosf, kb8Project against a plain line-by-line
// statement of KannalaBrandt8::project (reference src/CameraModels/KannalaBrandt8.cpp:28-44) that calls libm.  Built as a shared library
// (tests/test_kb8_math.py): the check_* functions return the number of mismatching results (a result matches when its bytes are equal, or
// when both are NaN: which operand's payload an addition of two NaNs keeps is the hardware's choice, not the algorithm's) and print the
// first few; the kb8_* functions hand the header's routines to the Python walks.
#include "host_shim/kb8_shim.h"

#include <cmath>
#include <cstdio>
#include <mutex>
#include <thread>
#include <vector>

#include "../../extractorb_amd/csrc/k_camera_kb8.hpp"

using namespace orbx;

namespace {
std::mutex g_print;
int g_printed = 0;

inline uint32_t bitsOf(float f) { return __float_as_uint(f); }
inline bool same(float a, float b) { return bitsOf(a) == bitsOf(b) || (a != a && b != b); }

void report(const char* what, float a, float b, float got, float want) {
    std::lock_guard<std::mutex> lk(g_print);
    if (g_printed++ < 12)
        std::printf("%s(%a [%08x], %a [%08x]) = %a [%08x], libm %a [%08x]\n", what, a, bitsOf(a), b, bitsOf(b), got, bitsOf(got), want, bitsOf(want));
}

inline long atan2Mismatch(float y, float x) {
    const float got = orbx::atan2f32(y, x), want = atan2f(y, x);
    if (same(got, want)) return 0;
    report("atan2f", y, x, got, want);
    return 1;
}
inline long atanMismatch(float x) {
    const float got = orbx::atanf32(x), want = atanf(x);
    if (same(got, want)) return 0;
    report("atanf", x, 0.f, got, want);
    return 1;
}

struct Rng {                                               // splitmix64
    uint64_t s;
    uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
};

int threadCount() { const unsigned h = std::thread::hardware_concurrency(); return (int)std::min(16u, std::max(1u, h)); }

template <class F>
long parallel(long n, F body) {                            // body(begin, end, thread) -> mismatches
    const int T = threadCount();
    std::vector<long> bad(T, 0);
    std::vector<std::thread> th;
    for (int t = 0; t < T; t++) th.emplace_back([&, t] { bad[t] = body(n * t / T, n * (t + 1) / T, t); });
    for (auto& x : th) x.join();
    long s = 0;
    for (long b : bad) s += b;
    return s;
}

// the plain statement: the reference's lines with libm
void projectLibm(const float* k, float x, float y, float z, float& u, float& v) {
    const float x2_plus_y2 = x * x + y * y;
    const float theta = atan2f(sqrtf(x2_plus_y2), z);
    const float psi = atan2f(y, x);
    const float theta2 = theta * theta;
    const float theta3 = theta * theta2;
    const float theta5 = theta3 * theta2;
    const float theta7 = theta5 * theta2;
    const float theta9 = theta7 * theta2;
    const float r = theta + k[4] * theta3 + k[5] * theta5 + k[6] * theta7 + k[7] * theta9;
    u = k[0] * r * cosf(psi) + k[2];
    v = k[1] * r * sinf(psi) + k[3];
}
}  // namespace

extern "C" {

float kb8_atan2f(float y, float x) { return orbx::atan2f32(y, x); }
float kb8_atanf(float x) { return orbx::atanf32(x); }
float kb8_sqrtf(float x) { return kb8Sqrt(x); }
float kb8_sinf(float x) { float s, c; kb8SinCos(x, &s, &c); return s; }
float kb8_cosf(float x) { float s, c; kb8SinCos(x, &s, &c); return c; }
void kb8_project(const float* k8, int n, const float* xyz, float* uv) {
    float k[8];
    for (int i = 0; i < 8; i++) k[i] = k8[i];
    for (int i = 0; i < n; i++) kb8Project(k, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], uv[2 * i], uv[2 * i + 1]);
}
void kb8_project_libm(const float* k8, int n, const float* xyz, float* uv) {
    for (int i = 0; i < n; i++) projectLibm(k8, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], uv[2 * i], uv[2 * i + 1]);
}

// The structured set.  out3: pairs compared by each part (exponent grid, thresholds and k boundaries, specials).
long kb8_check_atan2_structured(long* out3) {
    const uint32_t mant[4] = {0u, 1u, 0x400000u, 0x7fffffu};
    long n0 = 0, n1 = 0, n2 = 0;
    // every pair of exponents (zero / subnormal and infinity / NaN included) with a few mantissas, all four sign combinations
    long bad = parallel(256, [&](long b, long e, int) {
        long m = 0;
        for (long ey = b; ey < e; ey++)
            for (uint32_t ex = 0; ex < 256; ex++)
                for (uint32_t my : mant) for (uint32_t mx : mant) for (uint32_t sg = 0; sg < 4; sg++)
                    m += atan2Mismatch(__uint_as_float(((sg & 1) << 31) | ((uint32_t)ey << 23) | my), __uint_as_float(((sg >> 1) << 31) | (ex << 23) | mx));
        return m;
    });
    n0 = 256L * 256 * 16 * 4;
    // atanf's thresholds at -1 / 0 / +1 ulp: directly, through x == 1, and as the exact quotient of a division (both signs of x and y, several
    // scales: t * s / s = t for powers of two s)
    const float thr[6] = {7.0f / 16, 11.0f / 16, 19.0f / 16, 39.0f / 16, 0x1p25f, 0x1p-29f};
    for (float t : thr)
        for (int d = -1; d <= 1; d++) {
            const float y = __uint_as_float(bitsOf(t) + (uint32_t)d);
            for (float sy : {1.0f, -1.0f}) {
                bad += atanMismatch(sy * y); n1++;
                bad += atan2Mismatch(sy * y, 1.0f); n1++;
                for (float s : {2.0f, -2.0f, 0x1p-20f, -0x1p40f, 0.5f}) { bad += atan2Mismatch(sy * y * s, s); n1++; }
            }
        }
    // the k = (iy - ix) >> 23 boundaries: k > 60 and, for x < 0, k < -60, at -1 / 0 / +1 ulp of the exponent gap, for several x
    for (uint32_t ix : {0x00800000u, 0x00800001u, 0x1f123456u, 0x20000000u, 0x207fffffu, 0x00000001u, 0x00400000u})
        for (int gap : {59, 60, 61, 62})
            for (int d = -1; d <= 1; d++)
                for (uint32_t sg = 0; sg < 4; sg++) {
                    const uint32_t iy = ix + ((uint32_t)gap << 23) + (uint32_t)d;
                    if (iy < 0x7f800000u) {
                        bad += atan2Mismatch(__uint_as_float(((sg & 1) << 31) | iy), __uint_as_float(((sg >> 1) << 31) | ix)); n1++;      // y >> x
                        bad += atan2Mismatch(__uint_as_float(((sg & 1) << 31) | ix), __uint_as_float(((sg >> 1) << 31) | iy)); n1++;      // y << x
                    }
                }
    // zeros, infinities, x == 1, extremes, NaN: every pair
    const float sp[] = {0.0f, -0.0f, INFINITY, -INFINITY, 1.0f, -1.0f, 0x1p-149f, -0x1p-149f, 0x1p-126f, -0x1p-126f, 3.4028234664e38f, -3.4028234664e38f,
                        NAN, 0.5f, -2.5f, 1e-30f, 1e30f};
    for (float y : sp) for (float x : sp) { bad += atan2Mismatch(y, x); n2++; }
    for (float x : sp) { bad += atanMismatch(x); n2++; }
    if (out3) { out3[0] = n0; out3[1] = n1; out3[2] = n2; }
    return bad;
}

// n pseudo-random pairs: the first half raw bit patterns, the second half a 2^-16 fixed-point grid over +-128
long kb8_check_atan2_random(long n, unsigned long long seed) {
    return parallel(n, [&](long b, long e, int t) {
        Rng r{seed * 0x2545f4914f6cdd1dull + (uint64_t)t};
        long m = 0;
        for (long i = b; i < e; i++) {
            const uint64_t w = r.next();
            float y, x;
            if (i < n / 2) { y = __uint_as_float((uint32_t)w); x = __uint_as_float((uint32_t)(w >> 32)); }
            else {
                y = (float)((int)((uint32_t)w % (256u << 16)) - (128 << 16)) * 0x1p-16f;
                x = (float)((int)((uint32_t)(w >> 32) % (256u << 16)) - (128 << 16)) * 0x1p-16f;
            }
            m += atan2Mismatch(y, x);
        }
        return m;
    });
}

// every float whose magnitude is in [0, pi] (bits 0 .. 0x40490fdb), with the sign bit set (negative != 0) or clear
long kb8_check_sincos(int negative) {
    const long n = 0x40490fdbL + 1;
    const uint32_t sign = negative ? 0x80000000u : 0u;
    return parallel(n, [&](long b, long e, int) {
        long m = 0;
        for (long i = b; i < e; i++) {
            const float y = __uint_as_float(sign | (uint32_t)i);
            float s, c;
            kb8SinCos(y, &s, &c);
            const float ws = sinf(y), wc = cosf(y);
            if (!same(s, ws)) { m++; report("sinf", y, 0.f, s, ws); }
            if (!same(c, wc)) { m++; report("cosf", y, 0.f, c, wc); }
        }
        return m;
    });
}

// kb8Project against the plain statement on n pseudo-random points (a third of them with z <= 0, some with x = y = 0, huge and tiny ratios)
long kb8_check_project(long n, unsigned long long seed) {
    const float k[8] = {190.97847715128717f, 190.9733070521226f, 254.93170605935475f, 256.8974428996504f,
                        0.0034823894022493434f, 0.0007150348452162257f, -0.0020532361418706202f, 0.00020293673591811182f};
    return parallel(n, [&](long b, long e, int t) {
        Rng r{seed * 0x9e3779b97f4a7c15ull + 77u * (uint64_t)t};
        long m = 0;
        for (long i = b; i < e; i++) {
            const uint64_t w0 = r.next(), w1 = r.next();
            auto U = [](uint32_t v) { return (float)(int)(v % 2000001u - 1000000u) * 1e-5f; };      // [-10, 10]
            float x = U((uint32_t)w0), y = U((uint32_t)(w0 >> 32)), z = U((uint32_t)w1);
            const unsigned kind = (unsigned)(w1 >> 32) % 16u;
            if (kind == 0) { x = 0.f; y = 0.f; }
            if (kind == 1) z = 0.f;
            if (kind == 2) { x *= 1e-30f; }
            if (kind == 3) { y *= 1e30f; }
            if (kind == 4) { z *= 1e-38f; }
            if (kind == 5) { x = __uint_as_float((uint32_t)w0); y = __uint_as_float((uint32_t)(w0 >> 32)); z = __uint_as_float((uint32_t)w1); }
            float u, v, wu, wv;
            kb8Project(k, x, y, z, u, v);
            projectLibm(k, x, y, z, wu, wv);
            if (!same(u, wu)) { m++; report("project.u", x, y, u, wu); }
            if (!same(v, wv)) { m++; report("project.v", x, y, v, wv); }
        }
        return m;
    });
}

}  // extern "C"
