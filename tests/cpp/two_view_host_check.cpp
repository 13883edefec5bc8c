// two_view_host_check.cpp - extractorb_amd/csrc/k_two_view.hpp, the statement of k_two_view.hip, compiled for the HOST (tests/cpp/host_shim
// stands in for the device vocabulary) with a wave of one lane: the three kernels' bodies run as the launch wrapper orders them, on a
// workspace of exactly the entry's sizes.
// Three uses, all without a GPU:
//   * as a shared library (tests/test_two_view.py): tv_host() over the scenes of the GPU tests, compared with the walk byte for byte;
//     tv_draw_set(), tv_null9(), tv_svd3() for the pieces;
//   * tv_check_acos(): acosFloat32 against the host libm on EVERY float of [0.9, 1], on a fixed stride over the rest of [-1, 1] and on values
//     outside the domain;
//   * as a stand-alone program (-DTWO_VIEW_HOST_MAIN) under -fsanitize=address,undefined on exact-size heap blocks: counts past the
//     capacity and negative, bad indices, fewer than eight matches, wild rand() values, NaN keypoints, iterations = 1.
#include "host_shim/two_view_shim.h"

#include <cstdio>
#include <random>
#include <vector>

#include "../../extractorb_amd/csrc/k_two_view.hpp"

using namespace orbx;

namespace { bool g_zeroF = false; }

extern "C" {

// tv_set_zero_f(1): tv_host then zeroes every F score between the hypotheses and the decision - what FindFundamental leaves when no
// iteration scores above 0 (SF == 0, the F inliers empty): the one route on which the decision sees no F winner
void tv_set_zero_f(int on) { g_zeroF = on != 0; }
// tvRankHit on host arrays
int tv_rank_hit(const float* cosv, const uint8_t* counted, int N, float v, int idx) { return tvRankHit(cosv, counted, N, v, idx) ? 1 : 0; }
// CheckRT's loop body for one match under motion (R9, t3): out5 = counted, good, then the point; *cosPar
void tv_check_point(const float* R9, const float* t3, const float* cam4, float sigma, float u1, float v1, float u2, float v2, float* out5, float* cosPar) {
    TwoViewParams q{};
    q.fx = cam4[0]; q.fy = cam4[1]; q.cx = cam4[2]; q.cy = cam4[3]; q.sigma = sigma;
    float R[9], t[3], mo[kTvMotionFloats];
    for (int c = 0; c < 9; c++) R[c] = R9[c];
    for (int c = 0; c < 3; c++) t[c] = t3[c];
    tvStoreMotion(mo, R, t, q);
    const TvPoint pt = tvCheckPoint(true, mo, q, (float)(4.0 * (double)(sigma * sigma)), u1, v1, u2, v2);
    out5[0] = pt.counted; out5[1] = pt.good; out5[2] = pt.p[0]; out5[3] = pt.p[1]; out5[4] = pt.p[2];
    *cosPar = pt.cosPar;
}
// the end of ReconstructF / ReconstructH on given counts and parallaxes: the status, *chosen
int tv_decide(int model, const int* nGood8, const float* parallax8, int N, float minParallax, int minTriangulated, int* chosen) {
    TwoViewParams q{};
    q.minParallax = minParallax; q.minTriangulated = minTriangulated;
    return tvDecide(model, nGood8, parallax8, N, q, *chosen);
}

// the arguments of orbx_reconstruct_two_views_device on host arrays; cam4 = fx, fy, cx, cy; result: n_pairs rows of orbx_two_view_result
void tv_host(int nPairs, int f1First, int f1Step, int f2First, int f2Step, const void* kps, const int* nOut, int capacity, int* matches12,
             int* nMatches, const float* cam4, float sigma, int iterations, float minParallax, int minTriangulated, float rhThreshold,
             const int* rnd, int prune, void* result, float* p3d, uint8_t* tri) {
    TwoViewParams q{};
    q.fx = cam4[0]; q.fy = cam4[1]; q.cx = cam4[2]; q.cy = cam4[3];
    q.sigma = sigma; q.minParallax = minParallax; q.rhThreshold = rhThreshold;
    q.iterations = iterations; q.minTriangulated = minTriangulated; q.prune = prune != 0; q.capacity = capacity;
    q.f1First = f1First; q.f1Step = f1Step; q.f2First = f2First; q.f2Step = f2Step;
    const size_t entries = (size_t)nPairs * capacity, hyps = (size_t)nPairs * 2 * iterations;
    std::vector<TvPrep> prep(nPairs);
    std::vector<int> first(entries, -1), second(entries, -1);
    std::vector<float> score(hyps, NAN), mats(hyps * 9, NAN), cosv(entries, NAN);
    std::vector<uint8_t> inl(entries, 0xEE), counted(entries, 0xEE);
    const TvWork w{prep.data(), first.data(), second.data(), score.data(), mats.data(), inl.data(), counted.data(), cosv.data()};
    for (int p = 0; p < nPairs; p++) tvPreparePair(0, p, (const Keypoint*)kps, nOut, matches12, q, w, (TwoViewResult*)result, p3d, tri);
    for (int p = 0; p < nPairs; p++)
        for (int model = 0; model < 2; model++)
            for (int it = 0; it < iterations; it++) {
                std::vector<float> lds(kTvHypLdsFloats, NAN);      // exactly the kernel's LDS
                tvHypothesisWave<false>(0, p, model, it, (const Keypoint*)kps, rnd, q, w, lds.data());
            }
    if (g_zeroF)
        for (int p = 0; p < nPairs; p++)
            for (int it = 0; it < iterations; it++) score[((size_t)p * 2 + 1) * iterations + it] = 0.0f;
    for (int p = 0; p < nPairs; p++) {
        std::vector<float> lds(kTvDecideLdsFloats, NAN);
        tvDecidePair(0, p, (const Keypoint*)kps, matches12, nMatches, q, w, (TwoViewResult*)result, p3d, tri, lds.data());
    }
}
int tv_result_bytes() { return (int)sizeof(TwoViewResult); }
void tv_draw_set(const int* r8, int N, int* idx8) {
    int idx[8];
    tvDrawSet(r8, N, idx);
    for (int j = 0; j < 8; j++) idx8[j] = idx[j];
}
// vt.row(8) of the rows x 9 matrix A (rows = 16 or 8)
void tv_null9(const float* A, int rows, float* out9) {
    std::vector<float> W(A, A + rows * 9), A0(A, A + rows * 9), V(81, NAN);
    float out[9];
    if (rows == 16) nullVector9<16>(W.data(), A0.data(), V.data(), out);
    else nullVector9<8>(W.data(), A0.data(), V.data(), out);
    for (int c = 0; c < 9; c++) out9[c] = out[c];
}
void tv_svd3(const float* A9, float* U9, float* w3, float* Vt9) {
    float A[9], U[9], w[3], Vt[9];
    for (int c = 0; c < 9; c++) A[c] = A9[c];
    svd3(A, U, w, Vt);
    for (int c = 0; c < 9; c++) { U9[c] = U[c]; Vt9[c] = Vt[c]; }
    for (int c = 0; c < 3; c++) w3[c] = w[c];
}
float tv_acosf(float x) { return acosFloat32(x); }
// acosFloat32 against acosf: every float of [0.9, 1], every `stride`-th bit pattern of [-1, 1], values outside the domain; the mismatches
long tv_check_acos(int stride, long* tested) {
    long bad = 0, n = 0;
    auto one = [&](float x) {
        const float got = acosFloat32(x), want = acosf(x);
        n++;
        if (got != got && want != want) return;
        if (__float_as_uint(got) != __float_as_uint(want)) bad++;
    };
    for (uint32_t bits = __float_as_uint(0.9f); bits <= 0x3f800000u; bits++) one(__uint_as_float(bits));
    for (uint32_t bits = 0; bits <= 0x3f800000u; bits += (uint32_t)stride) { one(__uint_as_float(bits)); one(__uint_as_float(bits | 0x80000000u)); }
    const uint32_t outside[] = {0x3f800001u, 0xbf800001u, 0x40000000u, 0xc0000000u, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7f7fffffu,
                                0x00000001u, 0x80000001u, 0x23000000u, 0x23000001u, 0x3effffffu, 0x3f000000u, 0xbf000000u, 0xbf800000u, 0x80000000u};
    for (uint32_t b : outside) one(__uint_as_float(b));
    if (tested) *tested = n;
    return bad;
}

}  // extern "C"

#ifdef TWO_VIEW_HOST_MAIN
int main() {
    std::mt19937 rng(23);
    auto U = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
    const float cam[4] = {458.f, 457.f, 367.f, 248.f};
    long accepted = 0, rows = 0;
    for (int trial = 0; trial < 8; trial++) {
        // trial: 0 plain, 1 counts past the capacity and negative, 2 bad indices, 3 fewer than eight matches, 4 wild rand() values and SF == 0,
        // 5 NaN keypoints, 6 iterations = 1 and capacity 13, 7 prune with one pair named twice
        const int cap = trial == 6 ? 13 : 70, frames = 4, nPairs = 3, iters = trial == 6 ? 1 : 40;
        // exact-size heap blocks: an access one element past any of them is reported
        std::vector<Keypoint> kps((size_t)frames * cap);
        std::vector<int> nOut(frames), matches((size_t)nPairs * cap), nMatches(nPairs), rnd((size_t)nPairs * iters * 8);
        std::vector<float> p3d((size_t)nPairs * cap * 3, -7.f);
        std::vector<uint8_t> tri((size_t)nPairs * cap, 0xEE);
        std::vector<TwoViewResult> res(nPairs);
        std::vector<float> X((size_t)cap * 3);
        for (int i = 0; i < cap; i++) { X[3 * i] = U(-2.5f, 2.5f); X[3 * i + 1] = U(-1.5f, 1.5f); X[3 * i + 2] = U(4.f, 8.f); }
        for (int f = 0; f < frames; f++) {
            nOut[f] = trial == 1 ? (f == 0 ? cap + 50 : f == 1 ? cap : -3) : cap - f;
            const float yaw = 0.05f * f, c = std::cos(yaw), sn = std::sin(yaw);
            for (int i = 0; i < cap; i++) {
                const float x = c * X[3 * i] + sn * X[3 * i + 2] - 0.6f * f, y = X[3 * i + 1] + 0.05f * f, z = -sn * X[3 * i] + c * X[3 * i + 2] + 0.1f * f;
                Keypoint& k = kps[(size_t)f * cap + i];
                k.x = cam[0] * x / z + cam[2] + U(-0.3f, 0.3f);
                k.y = cam[1] * y / z + cam[3] + U(-0.3f, 0.3f);
                if (trial == 5 && i % 9 == 0) k.x = NAN;
                k.octave = 0; k.angle = 0.f;
            }
        }
        for (int p = 0; p < nPairs; p++) {
            int n = 0;
            for (int i = 0; i < cap; i++) {
                int m = (i % 5 == 4 || i >= cap - 3) ? -1 : i;
                if (trial == 2 && i % 7 == 0) m = p == 0 ? cap + 5 : 2000000000;
                if (trial == 3 && i >= 5 + p) m = -1;
                matches[(size_t)p * cap + i] = m;
                n += m >= 0;
            }
            nMatches[p] = n;
        }
        for (auto& r : rnd) r = trial == 4 ? (int)(rng() & 0xffffffffu) : (int)(rng() & 0x7fffffffu);
        const int f2Step = trial == 7 ? 0 : 1;
        tv_set_zero_f(trial == 4);      // trial 4 also: no F score above 0, the decision meets no F winner
        tv_host(nPairs, 0, 0, 1, f2Step, kps.data(), nOut.data(), cap, matches.data(), nMatches.data(), cam, 1.0f, iters, 1.0f, trial == 6 ? 2 : 20,
                trial % 2 ? 0.4f : 0.5f, rnd.data(), trial == 7, res.data(), p3d.data(), tri.data());
        tv_set_zero_f(0);
        for (int p = 0; p < nPairs; p++) {
            const TwoViewResult& r = res[p];
            if (r.status < 0 || r.status >= kTvStatuses) { std::printf("FAILED: status %d\n", r.status); return 1; }
            const int n1 = max(0, min(nOut[0], cap));
            int flagged = 0;
            for (int i = 0; i < cap; i++) {
                const uint8_t t = tri[(size_t)p * cap + i];
                if (i >= n1) { if (t != 0xEE || p3d[((size_t)p * cap + i) * 3] != -7.f) { std::printf("FAILED: an entry past n was written\n"); return 1; } continue; }
                if (t > 1) { std::printf("FAILED: flag %d\n", t); return 1; }
                if (t && r.status > kTvAcceptedF) { std::printf("FAILED: a rejected pair has a triangulated point\n"); return 1; }
                flagged += t;
            }
            if (r.status <= kTvAcceptedF) {
                accepted++;
                if (flagged > r.nGood[r.chosen]) { std::printf("FAILED: more flags than counted points\n"); return 1; }
            }
            rows++;
        }
        std::printf("trial %d: status %d %d %d, N %d %d %d, model %d, inliers %d, good %d %d %d %d, RH %.3f\n", trial, res[0].status, res[1].status,
                    res[2].status, res[0].nMatches, res[1].nMatches, res[2].nMatches, res[0].model, res[0].nInliers, res[0].nGood[0], res[0].nGood[1],
                    res[0].nGood[2], res[0].nGood[3], res[0].RH);
    }
    if (accepted == 0) { std::printf("FAILED: nothing was accepted at all\n"); return 1; }
    std::printf("two_view_host_check: every access inside its arrays, %ld rows, %ld accepted\n", rows, accepted);
    return 0;
}
#endif
