// triangulation_two_eyes_host_check.cpp - extractorb_amd/csrc/k_triangulate_match_two_eyes.hip compiled for the HOST (tests/cpp/host_shim
// stands in for the device vocabulary; triangulation_two_eyes_shim.h makes a row one lane) and run one thread at a time: a workgroup is every
// thread's triTwoEyesStage, every slot's triTwoEyesLoadSlot and the column copies, every entry's triTwoEyesSegments, every entry's
// triTwoEyesRow - the kernel's own arithmetic and control flow around its barriers - and then the closing scan (histogram removal, vMatchedPairs
// in stacked order), which is restated here sequentially because the kernel's is a workgroup scan.  Two uses, both without a GPU:
//   * as a shared library (tests/test_search_triangulation_two_eyes.py): tri_two_eyes_host() over the scenes of the GPU tests, compared
//     with the walk; tri_two_eyes_relative() is one eye combination as lane `combo` stages it;
//   * as a stand-alone program (-DTRI_TWO_EYES_HOST_MAIN) under -fsanitize=address,undefined: exact-size heap tables, valid and CORRUPT
//     FeatureVectors (indices and counts past the capacity), octaves outside the tables, an empty eye, NLeft = 0, NaN and infinite poses,
//     keypoints at the principal point and far outside the image - every access stays inside its arrays and every row ends.
#include "host_shim/triangulation_two_eyes_shim.h"

#include <cstdio>
#include <random>
#include <vector>

#include "../../extractorb_amd/csrc/k_triangulate_match_two_eyes.hip"

using namespace orbx;

namespace {
struct Args {
    const uint32_t *featNodes, *featIdx;
    const int* nFeat;
    const uint8_t *flags1, *flags2;
    const float* poses;
    const Keypoint* kps;
    const uint8_t* desc;
    const int* nOut;
};

void runPair(const Args& a, const TriMatchTwoEyesParams& p, bool stage, int pair, int* matches12, int* pairs, int* nMatches, int* stats2) {
    const int cap = p.capacity, capA = (cap + 15) & ~15;
    const long long X1 = p.kf1First + (long long)pair * p.kf1Step, X2 = p.kf2First + (long long)pair * p.kf2Step, f1 = 2 * X1, f2 = 2 * X2;
    // one exact-size block, as the kernel's dynamic LDS: the sanitized program sees an access past it (the static tables are blocks of their own)
    std::vector<TriU4> block(((size_t)capA * (62 + (stage ? 64 : 0)) + 15) / 16);
    std::vector<float> sRel(4 * 12), sCam(16);
    std::vector<int> sHist(kHistoLength, 0);
    std::vector<double> sGate(kMaxLevels);
    const TriTwoEyesTables T{(uint8_t*)block.data() + (stage ? 64 * capA : 0), capA};
    int M1[2], M2[2], N1[2], N2[2];
    for (int e = 0; e < 2; e++) {
        M1[e] = max(0, min(a.nFeat[f1 + e], cap)); M2[e] = max(0, min(a.nFeat[f2 + e], cap));
        N1[e] = max(0, min(a.nOut[f1 + e], cap)); N2[e] = max(0, min(a.nOut[f2 + e], cap));
    }
    const Keypoint *kp1 = a.kps + f1 * cap, *kp2 = a.kps + f2 * cap;
    const TriU4 *desc1 = (const TriU4*)(a.desc + f1 * cap * 32), *desc2 = (const TriU4*)(a.desc + f2 * cap * 32);
    for (int tid = 0; tid < 512; tid++) triTwoEyesStage(tid, a.poses + X1 * 12, a.poses + X2 * 12, p, sRel.data(), sCam.data(), sGate.data());
    for (int e = 0; e < 2; e++) {
        const uint32_t *gN1 = a.featNodes + (f1 + e) * cap, *gI1 = a.featIdx + (f1 + e) * cap, *gN2 = a.featNodes + (f2 + e) * cap, *gI2 = a.featIdx + (f2 + e) * cap;
        for (int i = 0; i < M1[e]; i++) { T.segL()[e * capA + i] = gN1[i]; T.idx1()[e * capA + i] = (unsigned short)min(gI1[i], (uint32_t)(cap - 1)); }
        for (int i = 0; i < M2[e]; i++) { T.node2()[e * capA + i] = gN2[i]; T.idx2()[e * capA + i] = (unsigned short)min(gI2[i], (uint32_t)(cap - 1)); }
    }
    for (int s = 0; s < 2 * capA; s++) triTwoEyesLoadSlot(s, T, capA, cap, pair, N2[s >= capA], a.flags1, a.flags2, kp2, p);
    if (stage)
        for (int e = 0; e < 2; e++)
            for (int i = 0; i < 2 * N2[e]; i++) T.desc2()[2 * e * capA + i] = desc2[2LL * e * cap + i];
    for (int s = 0; s < M1[0] + M1[1]; s++) { const int e = s >= M1[0]; triTwoEyesSegments(e * capA + s - e * M1[0], T, capA, M2[0], M2[1]); }
    int nCalls = 0, nWithin = 0;
    if (!p.onlyStereo)
        for (int k = 0; k < M1[0] + M1[1]; k++) {
            if (stage) triTwoEyesRow<true>(k, 0, T, capA, cap, M1[0], N2[0], kp1, kp2, desc1, desc2, p, sRel.data(), sCam.data(), sGate.data(), sHist.data(), nCalls, nWithin);
            else triTwoEyesRow<false>(k, 0, T, capA, cap, M1[0], N2[0], kp1, kp2, desc1, desc2, p, sRel.data(), sCam.data(), sGate.data(), sHist.data(), nCalls, nWithin);
        }
    if (stats2) { stats2[0] += nCalls; stats2[1] += nWithin; }
    // the closing scan, sequentially: ComputeThreeMaxima and the removal (:1174-1193), vMatchedPairs in stacked order (:1195-1203)
    unsigned dropBins = 0u;
    if (p.checkOrientation) {
        const ThreeMaxima top3 = computeThreeMaxima(sHist);
        for (int i = 0; i < kHistoLength; i++)
            if (i != top3.ind1 && i != top3.ind2 && i != top3.ind3) dropBins |= 1u << i;
    }
    int written = 0;
    for (int e = 0; e < 2; e++)
        for (int i = 0; i < cap; i++) {
            int m = i < N1[e] ? T.m12()[e * capA + i] : -1;
            if (m >= 0) { const int bin = T.binOf()[e * capA + i]; if (bin < kHistoLength && ((dropBins >> bin) & 1u)) m = -1; }
            matches12[(2LL * pair + e) * cap + i] = m;
            if (m >= 0) { pairs[4LL * pair * cap + 2 * written] = e ? N1[0] + i : i; pairs[4LL * pair * cap + 2 * written + 1] = m; written++; }
        }
    nMatches[pair] = written;
}

TriMatchTwoEyesParams makeParams(const float* cams16, const float* sigma2, const float* tlr12, int nlevels, int thLow, int checkOrientation,
                                 int onlyStereo, int coarse, int capacity, int kf1First, int kf1Step, int kf2First, int kf2Step) {
    TriMatchTwoEyesParams p{};
    for (int i = 0; i < 16; i++) p.cam[i >> 3][i & 7] = cams16[i];
    for (int l = 0; l < kMaxLevels; l++) p.sigma2[l] = l < nlevels ? sigma2[l] : 0.f;
    for (int i = 0; i < 12; i++) p.tlr[i] = tlr12[i];
    p.nlevels = max(1, min(nlevels, (int)kMaxLevels)); p.thLow = thLow; p.checkOrientation = checkOrientation ? 1 : 0;
    p.onlyStereo = onlyStereo ? 1 : 0; p.coarse = coarse ? 1 : 0; p.capacity = capacity;
    p.kf1First = kf1First; p.kf1Step = kf1Step; p.kf2First = kf2First; p.kf2Step = kf2Step;
    return p;
}
}  // namespace

extern "C" {

// the arguments of orbx_search_for_triangulation_two_eyes_device on host arrays; sigma2: the handle's mvLevelSigma2[nlevels]; stats2 (or
// NULL): triangulations, candidates within th_low, summed over the pairs
void tri_two_eyes_host(int nPairs, int kf1First, int kf1Step, int kf2First, int kf2Step, const uint32_t* featNodes, const uint32_t* featIdx,
                       const int* nFeat, const uint8_t* flags1, const uint8_t* flags2, const float* poses, const float* tlr12, const float* cams16,
                       const void* kps, const uint8_t* desc, const int* nOut, int capacity, const float* sigma2, int nlevels, int onlyStereo,
                       int coarse, int thLow, int checkOrientation, int stage, int* matches12, int* pairs, int* nMatches, int* stats2) {
    const TriMatchTwoEyesParams p = makeParams(cams16, sigma2, tlr12, nlevels, thLow, checkOrientation, onlyStereo, coarse, capacity, kf1First,
                                               kf1Step, kf2First, kf2Step);
    const Args a{featNodes, featIdx, nFeat, flags1, flags2, poses, (const Keypoint*)kps, desc, nOut};
    if (stats2) stats2[0] = stats2[1] = 0;
    for (int pr = 0; pr < nPairs; pr++) runPair(a, p, stage != 0, pr, matches12, pairs, nMatches, stats2);
}
// R12 (9) and t21 (3) of eye combination combo = eye1 * 2 + eye2, as lane `combo` stages them
void tri_two_eyes_relative(const float* pose1, const float* pose2, const float* tlr12, int combo, float* out12) {
    TriMatchTwoEyesParams p{};
    for (int i = 0; i < 12; i++) p.tlr[i] = tlr12[i];
    p.nlevels = 1;
    std::vector<float> sRel(48), sCam(16);
    std::vector<double> sGate(kMaxLevels);
    triTwoEyesStage(combo, pose1, pose2, p, sRel.data(), sCam.data(), sGate.data());
    for (int i = 0; i < 12; i++) out12[i] = sRel[combo * 12 + i];
}
long tri_two_eyes_lds_bytes(int capacity, int stage) { return (long)triMatchTwoEyesLdsBytes(capacity, stage != 0); }

}  // extern "C"

#ifdef TRI_TWO_EYES_HOST_MAIN
int main() {
    std::mt19937 rng(5);
    auto U = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
    const float cams[16] = {190.97847715128717f, 190.9733070521226f, 254.93170605935475f, 256.8974428996504f, 0.0034823894022493434f,
                            0.0007150348452162257f, -0.0020532361418706202f, 0.00020293673591811182f, 190.44236969414825f, 190.4344384721956f,
                            252.59949716835982f, 254.91723064636983f, 0.0034003170790442797f, 0.001766278153469831f, -0.00266312569781606f,
                            0.0003299517423931039f};
    const float tlr[12] = {1, 0, 0, 0.1f, 0, 1, 0, 0, 0, 0, 1, 0};
    float sigma2[8];
    for (int l = 0; l < 8; l++) sigma2[l] = std::pow(1.2f, 2 * l);
    long total = 0;
    for (int trial = 0; trial < 10; trial++) {
        const bool corrupt = trial >= 5;
        const int cap = trial % 5 == 0 ? 33 : trial % 5 == 1 ? 1302 : 97, rigs = 3, B = 2 * rigs, nodes = cap > 200 ? 300 : 9;
        // exact-size heap blocks: an access one element past any of them is reported
        std::vector<Keypoint> kps((size_t)B * cap);
        std::vector<uint8_t> desc((size_t)B * cap * 32), fl1((size_t)2 * 2 * cap), fl2((size_t)2 * 2 * cap);
        std::vector<uint32_t> fn((size_t)B * cap), fi((size_t)B * cap);
        std::vector<int> nout(B), nfeat(B);
        std::vector<float> poses(rigs * 12, 0.f);
        for (int r = 0; r < rigs; r++) { poses[r * 12] = poses[r * 12 + 5] = poses[r * 12 + 10] = 1.f; poses[r * 12 + 3] = 0.3f * r; }
        if (trial % 5 == 3) poses[15] = NAN;                      // a NaN pose of rig 1 (pair 0): every triangulation ends within the sweep cap, no match
        if (trial % 5 == 4) poses[12 + 7] = INFINITY;
        for (int f = 0; f < B; f++) {
            int n = cap - (f & 1 ? 3 : 7);
            if (trial % 5 == 2 && f == 2) n = 0;                  // NLeft = 0 in keyframe 2 of pair 0
            if (trial % 5 == 2 && f == 1) n = 0;                  // an empty right eye
            nout[f] = corrupt ? cap + 40 : n;
            nfeat[f] = corrupt ? cap + 9 : n;
            for (int i = 0; i < cap; i++) {
                Keypoint& k = kps[(size_t)f * cap + i];
                k.x = i == 0 ? cams[2] : i == 1 ? 1e6f : U(0, 511); k.y = i == 0 ? cams[3] : U(0, 511);
                k.angle = corrupt ? U(-1e4f, 1e4f) : U(0, 359.9f); k.octave = corrupt ? (int)U(-5, 30) : (int)U(0, 8);
                fn[(size_t)f * cap + i] = (uint32_t)((long)i * nodes / cap);                     // sorted node column
                fi[(size_t)f * cap + i] = corrupt ? (uint32_t)rng() : (uint32_t)i;
                for (int b = 0; b < 32; b++) desc[((size_t)f * cap + i) * 32 + b] = (uint8_t)(b < 3 ? rng() : 0x5a);      // distances well inside th_low
            }
        }
        for (auto& v : fl1) v = (uint8_t)(rng() % 4 == 0);
        for (auto& v : fl2) v = (uint8_t)(rng() % 4 == 0);
        for (int coarse = 0; coarse < 2; coarse++)
            for (int stage = 0; stage < 2; stage++) {
                if (cap > 200 && (coarse || stage)) continue;
                std::vector<int> m12((size_t)2 * 2 * cap), pairs((size_t)2 * 4 * cap), nm(2);
                int stats[2];
                tri_two_eyes_host(2, 0, 0, 1, 1, fn.data(), fi.data(), nfeat.data(), fl1.data(), fl2.data(), poses.data(), tlr, cams, kps.data(),
                                  desc.data(), nout.data(), cap, sigma2, 8, 0, coarse, 50, 1, stage, m12.data(), pairs.data(), nm.data(), stats);
                std::printf("trial %d cap %d coarse %d stage %d: matches %d %d, triangulations %d of %d within th_low\n", trial, cap, coarse, stage,
                            nm[0], nm[1], stats[0], stats[1]);
                if (trial % 5 == 3 && !coarse && nm[0] != 0) { std::printf("FAILED: a NaN pose matched\n"); return 1; }
                total += nm[0] + nm[1];
            }
    }
    std::printf("triangulation_two_eyes_host_check: every access inside its arrays, %ld matches\n", total);
    return 0;
}
#endif
