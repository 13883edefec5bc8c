// new_map_points_host_check.cpp - extractorb_amd/csrc/k_new_map_points.hpp, the statement of k_new_map_points.hip, compiled for the HOST
// (tests/cpp/host_shim stands in for the device vocabulary) and run one lane at a time: a workgroup is every thread's nmpStage into a block
// of exactly the kernel's LDS floats and then every lane's nmpLane - the kernel's own arithmetic, loads, stores and marks around its one
// barrier.  What the kernel does with a ballot and an atomic is a sum here; a workgroup past the list's end is skipped as the kernel leaves it.
// Three uses, all without a GPU:
//   * as a shared library (tests/test_new_map_points.py): nmp_host() over the scenes of the GPU tests, compared with the walk;
//   * nmp_check_cos(): nmpStereoCos's cosine on EVERY float of [pi, 2 pi] (or its negative) against the host libm - the range 2*atan2f
//     reaches beyond the [-pi, pi] tests/test_kb8_math.py holds - and nmp_check_stereo_cos() the whole expression on pseudo-random pairs;
//   * as a stand-alone program (-DNEW_MAP_POINTS_HOST_MAIN) under -fsanitize=address,undefined on exact-size heap blocks: n_matches past
//     the capacity and negative, indices outside the keyframes, NLeft = 0, an empty list, octaves outside the tables, NaN and infinite
//     poses, a monocular call with NULL stereo arrays - every access stays inside its arrays.
#include "host_shim/new_map_points_shim.h"

#include <cstdio>
#include <random>
#include <vector>

#include "../../extractorb_amd/csrc/k_new_map_points.hpp"

using namespace orbx;

namespace {
template <bool TwoEyes>
void runPair(int pair, const int* pairs, const int* nMatches, const float* poses, const Keypoint* kps, const Keypoint* raw, const float* uRight,
             const float* depth, const int* nOut, const NewMapPointsParams& p, uint8_t* exitOut, float* x3d, int* nNew, uint8_t* mark1,
             uint8_t* mark2, int* stats2) {
    const int n = max(0, min(nMatches[pair], p.listCapacity));
    const long long X1 = p.kf1First + (long long)pair * p.kf1Step, X2 = p.kf2First + (long long)pair * p.kf2Step;
    for (int tile = 0; tile < p.tiles && tile * kNmpThreads < n; tile++) {
        std::vector<float> sRig(kNmpLdsFloats, NAN);      // exactly the kernel's LDS; what the one-camera form does not stage stays NaN
        for (int tid = 0; tid < kNmpThreads; tid++) nmpStage<TwoEyes>(tid, poses + X1 * 12, poses + X2 * 12, p, sRig.data());
        for (int tid = 0; tid < kNmpThreads; tid++) {
            const int k = tile * kNmpThreads + tid;
            bool svd = false, stereoBranch = false;
            const bool accepted = nmpLane<TwoEyes>(pair, k, k < n, sRig.data(), pairs, kps, raw, uRight, depth, nOut, p, exitOut, x3d, mark1, mark2, svd, stereoBranch);
            nNew[pair] += accepted ? 1 : 0;
            if (stats2) { stats2[0] += svd ? 1 : 0; stats2[1] += stereoBranch ? 1 : 0; }
        }
    }
}
}  // namespace

extern "C" {

// the arguments of orbx_create_new_map_points_device (twoEyes = 0: cams16[0..3] = fx, fy, cx, cy; kps = mvKeysUn, raw = mvKeys) or
// orbx_create_new_map_points_two_eyes_device (twoEyes = 1: kps = the raw keypoints of both eyes; raw, uRight, depth NULL) on host arrays;
// scale / sigma2: the handle's tables [nlevels]; stats2 (or NULL): SVD branches, UnprojectStereo branches, summed over the pairs
void nmp_host(int twoEyes, int nPairs, int kf1First, int kf1Step, int kf2First, int kf2Step, const int* pairs, const int* nMatches,
              const float* poses, const float* tlr12, const float* cams16, const void* kps, const void* raw, const float* uRight,
              const float* depth, const int* nOut, int capacity, const float* scale, const float* sigma2, int nlevels, float ratioFactor, float mb,
              float mbf, int farPoints, float thFar, uint8_t* exitOut, float* x3d, int* nNew, uint8_t* mark1, uint8_t* mark2, int* stats2) {
    NewMapPointsParams p{};
    for (int i = 0; i < 16; i++) p.cam[i >> 3][i & 7] = cams16[i];
    for (int l = 0; l < kMaxLevels; l++) { p.scale[l] = l < nlevels ? scale[l] : 0.f; p.sigma2[l] = l < nlevels ? sigma2[l] : 0.f; }
    if (tlr12) for (int i = 0; i < 12; i++) p.tlr[i] = tlr12[i];
    p.mb = mb; p.mbf = mbf; p.thFarPoints = thFar; p.ratioFactor = ratioFactor; p.farPoints = farPoints ? 1 : 0;
    p.mono = twoEyes || !uRight ? 1 : 0;
    p.nlevels = max(1, min(nlevels, (int)kMaxLevels));
    p.capacity = capacity; p.listCapacity = twoEyes ? 2 * capacity : capacity;
    p.kf1First = kf1First; p.kf1Step = kf1Step; p.kf2First = kf2First; p.kf2Step = kf2Step;
    p.tiles = (p.listCapacity + kNmpThreads - 1) / kNmpThreads;
    if (stats2) stats2[0] = stats2[1] = 0;
    for (int pr = 0; pr < nPairs; pr++) nNew[pr] = 0;      // k_new_map_points_init
    for (int pr = 0; pr < nPairs; pr++) {
        if (twoEyes) runPair<true>(pr, pairs, nMatches, poses, (const Keypoint*)kps, nullptr, nullptr, nullptr, nOut, p, exitOut, x3d, nNew, mark1, mark2, stats2);
        else runPair<false>(pr, pairs, nMatches, poses, (const Keypoint*)kps, (const Keypoint*)raw, uRight, depth, nOut, p, exitOut, x3d, nNew, mark1, mark2, stats2);
    }
}
int nmp_threads() { return kNmpThreads; }
float nmp_stereo_cos(float mb, float depth) { return nmpStereoCos(mb, depth); }
// kb8SinCos's cosine against cosf on every float of [pi, 2 pi] (negative: of [-2 pi, -pi]); returns the mismatches, *tested the count
long nmp_check_cos(int negative, long* tested) {
    long bad = 0, n = 0;
    for (uint32_t bits = 0x40490fdbu; bits <= 0x40c90fdbu; bits++, n++) {
        const float y = __uint_as_float(bits | (negative ? 0x80000000u : 0u));
        float s, c;
        kb8SinCos(y, &s, &c);
        const float want = cosf(y);
        if (__float_as_uint(c) != __float_as_uint(want)) bad++;
    }
    if (tested) *tested = n;
    return bad;
}
// nmpStereoCos against cosf(2 * atan2f(mb / 2, depth)) on n pseudo-random (mb, depth), depth of either sign, zero and tiny included
long nmp_check_stereo_cos(long n, unsigned long long seed) {
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<float> mbD(0.01f, 1.0f), zD(-50.0f, 50.0f), e(-30.0f, 2.0f);
    long bad = 0;
    for (long i = 0; i < n; i++) {
        const float mb = mbD(rng);
        float z = zD(rng);
        if (i % 7 == 0) z = std::pow(10.0f, e(rng)) * (i % 2 ? -1.f : 1.f);
        if (i % 1001 == 0) z = i % 2 ? 0.0f : -0.0f;
        const float got = nmpStereoCos(mb, z), want = cosf(2 * atan2f(mb / 2, z));
        if (__float_as_uint(got) != __float_as_uint(want)) bad++;
    }
    return bad;
}

}  // extern "C"

#ifdef NEW_MAP_POINTS_HOST_MAIN
int main() {
    std::mt19937 rng(11);
    auto U = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
    const float kb8[16] = {190.97847715128717f, 190.9733070521226f, 254.93170605935475f, 256.8974428996504f, 0.0034823894022493434f,
                           0.0007150348452162257f, -0.0020532361418706202f, 0.00020293673591811182f, 190.44236969414825f, 190.4344384721956f,
                           252.59949716835982f, 254.91723064636983f, 0.0034003170790442797f, 0.001766278153469831f, -0.00266312569781606f,
                           0.0003299517423931039f};
    const float pin[16] = {500.f, 500.f, 320.f, 240.f};
    const float tlr[12] = {1, 0, 0, 0.1f, 0, 1, 0, 0, 0, 0, 1, 0};
    float scale[8], sigma2[8];
    for (int l = 0; l < 8; l++) { scale[l] = std::pow(1.2f, l); sigma2[l] = scale[l] * scale[l]; }
    long accepted = 0, entries = 0;
    for (int twoEyes = 0; twoEyes < 2; twoEyes++)
        for (int trial = 0; trial < 8; trial++) {
            // trial: 0 plain, 1 n_matches past the capacity and negative, 2 indices outside the keyframes, 3 NLeft = 0 / an empty keyframe,
            // 4 octaves outside the tables, 5 a NaN pose, 6 an infinite pose, 7 monocular with NULL stereo arrays / capacity 1
            const int cap = trial == 7 ? 1 : trial % 2 ? 33 : 70, L = twoEyes ? 2 * cap : cap, kfs = 3, B = twoEyes ? 2 * kfs : kfs, nPairs = 3;
            // exact-size heap blocks: an access one element past any of them is reported
            std::vector<Keypoint> kps((size_t)B * cap), raw((size_t)B * cap);
            std::vector<float> uRight((size_t)B * cap), depth((size_t)B * cap), poses(kfs * 12, 0.f), x3d((size_t)nPairs * L * 3, -7.f);
            std::vector<int> nOut(B), pairs((size_t)nPairs * L * 2), nMatches(nPairs), nNew(nPairs, -7);
            std::vector<uint8_t> exitOut((size_t)nPairs * L, 0xEE), mark1((size_t)nPairs * L, 0), mark2((size_t)nPairs * L, 0);
            for (int r = 0; r < kfs; r++) { poses[r * 12] = poses[r * 12 + 5] = poses[r * 12 + 10] = 1.f; poses[r * 12 + 3] = -0.4f * r; poses[r * 12 + 7] = 0.02f * r; }
            if (trial == 5) poses[12 + 6] = NAN;
            if (trial == 6) poses[24 + 3] = INFINITY;
            for (int f = 0; f < B; f++) {
                nOut[f] = trial == 1 ? cap + 50 : cap - (f % 3);
                if (trial == 3 && f == (twoEyes ? 2 : 1)) nOut[f] = 0;
                for (int i = 0; i < cap; i++) {
                    Keypoint& k = kps[(size_t)f * cap + i];
                    const int kf = twoEyes ? f / 2 : f;
                    const float z = 2.f + 0.1f * (i % 17), x = 0.05f * (i % 11) - 0.2f, y = 0.04f * (i % 13) - 0.2f;
                    const float fx = twoEyes ? kb8[0] : pin[0], cx = twoEyes ? kb8[2] : pin[2], cy = twoEyes ? kb8[3] : pin[3];
                    k.x = i == 0 ? cx : i == 1 ? 1e6f : fx * (x - 0.4f * kf - (f & twoEyes ? 0.1f : 0.f)) / z + cx + U(-0.3f, 0.3f);
                    k.y = i == 0 ? cy : fx * (y + 0.02f * kf) / z + cy + U(-0.3f, 0.3f);
                    k.octave = trial == 4 ? (int)U(-6, 30) : (int)U(0, 4); k.angle = 0.f;
                    raw[(size_t)f * cap + i] = k;
                    uRight[(size_t)f * cap + i] = i % 3 == 0 ? -1.f : k.x - 50.f / z;
                    depth[(size_t)f * cap + i] = i % 10 == 4 ? -1.f : z;
                }
            }
            for (int pr = 0; pr < nPairs; pr++) {
                nMatches[pr] = trial == 1 ? (pr == 0 ? L + 1000 : pr == 1 ? -5 : L) : pr == 2 ? 0 : L - 3 * pr;
                for (int k = 0; k < L; k++) {
                    const bool wild = trial == 2 && k % 3 == 0;
                    pairs[((size_t)pr * L + k) * 2] = wild ? (int)U(-2e9f, 2e9f) : (int)U(0, (float)L + (trial == 2 ? 3 : 0));
                    pairs[((size_t)pr * L + k) * 2 + 1] = wild ? (k % 2 ? -1 : 2 * L) : (int)U(0, (float)L);
                }
            }
            const bool mono = trial == 7 && !twoEyes;
            int stats[2];
            nmp_host(twoEyes, nPairs, 0, 0, 0, 1, pairs.data(), nMatches.data(), poses.data(), twoEyes ? tlr : nullptr, twoEyes ? kb8 : pin, kps.data(),
                     twoEyes || mono ? nullptr : raw.data(), twoEyes || mono ? nullptr : uRight.data(), twoEyes || mono ? nullptr : depth.data(),
                     nOut.data(), cap, scale, sigma2, 8, 1.8f, 0.1f, 50.f, trial % 2, 8.f, exitOut.data(), x3d.data(), nNew.data(), mark1.data(),
                     trial % 3 ? mark2.data() : nullptr, stats);
            for (int pr = 0; pr < nPairs; pr++) {
                const int n = max(0, min(nMatches[pr], L));
                int acc = 0;
                for (int k = 0; k < L; k++) {
                    const uint8_t e = exitOut[(size_t)pr * L + k];
                    if (k >= n) { if (e != 0xEE || x3d[((size_t)pr * L + k) * 3] != -7.f) { std::printf("FAILED: an entry past n_matches was written\n"); return 1; } continue; }
                    if (e >= kNmpExits) { std::printf("FAILED: exit %d\n", e); return 1; }
                    acc += e <= kNmpStereo2;
                    entries++;
                }
                if (acc != nNew[pr]) { std::printf("FAILED: d_n_new %d, %d accepting exits\n", nNew[pr], acc); return 1; }
                if ((trial == 5 && pr == 1 && acc) || (trial == 6 && pr == 2 && acc)) { std::printf("FAILED: a NaN or infinite pose made a point\n"); return 1; }
                accepted += acc;
            }
            std::printf("%s trial %d cap %2d: new points %d %d %d, %d SVD branches, %d stereo branches\n", twoEyes ? "two eyes  " : "one camera", trial, cap,
                        nNew[0], nNew[1], nNew[2], stats[0], stats[1]);
        }
    if (accepted == 0) { std::printf("FAILED: nothing was accepted at all\n"); return 1; }
    std::printf("new_map_points_host_check: every access inside its arrays, %ld matches, %ld accepted\n", entries, accepted);
    return 0;
}
#endif
