// stereo_fisheye_host_check.cpp - extractorb_amd/csrc/k_stereo_fisheye.hip compiled for the HOST (tests/cpp/host_shim stands in for the device
// vocabulary) and run one row at a time: a workgroup is every row's sfScanChunk over the right lapping descriptors in chunks of the
// kernel's kSfChunk, sfRatioPass, and for the rows that pass sfGeometry - the kernel's own arithmetic around its barriers.  What the kernel
// does with ballots and atomics is stated here sequentially: the compaction is the order of the rows, atomicMax a maximum, the counters sums.
// Two uses, both without a GPU:
//   * as a shared library (tests/test_stereo_fisheye.py): stereo_fisheye_host() over the scenes of the GPU tests, compared with the walk;
//   * as a stand-alone program (-DSTEREO_FISHEYE_HOST_MAIN) under -fsanitize=address,undefined on exact-size heap blocks (every staged chunk
//     is a block of exactly its descriptors): zero lapping rows on either side, one right row, mono == N, mono out of range, capacity 1, N
//     past the capacity, octaves outside the table, a NaN transform - every access stays inside its arrays.
#include "host_shim/stereo_fisheye_shim.h"

#include <cstdio>
#include <random>
#include <vector>

#include "../../extractorb_amd/csrc/k_stereo_fisheye.hip"

using namespace orbx;

extern "C" {

// the arguments of orbx_stereo_fisheye_match_device on host arrays; sigma2: the handle's mvLevelSigma2[nlevels]; nDescMatches may be NULL;
// calls (or NULL): sfGeometry calls summed over the rigs
void stereo_fisheye_host(int nRigs, int rigFirst, int rigStep, const void* kpsV, const uint8_t* desc, const int* nOut, const int* monoOut,
                         int capacity, const float* tlr12, const float* cams16, const float* sigma2, int nlevels, int* l2r, int* r2l, float* depth,
                         float* x3d, int* nMatches, int* nDescMatches, int* calls) {
    const Keypoint* kps = (const Keypoint*)kpsV;
    StereoFisheyeParams p{};
    for (int i = 0; i < 16; i++) p.cam[i >> 3][i & 7] = cams16[i];
    for (int l = 0; l < kMaxLevels; l++) p.sigma2[l] = l < nlevels ? sigma2[l] : 0.f;
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) p.R12[3 * r + c] = tlr12[4 * r + c];
        p.t12[r] = tlr12[4 * r + 3];
    }
    p.nlevels = max(1, min(nlevels, (int)kMaxLevels)); p.capacity = capacity; p.rigFirst = rigFirst; p.rigStep = rigStep;
    std::vector<double> sGate(kMaxLevels);
    for (int l = 0; l < kMaxLevels; l++) sGate[l] = 5.991 * (double)p.sigma2[min(l, p.nlevels - 1)];
    const long long cap = capacity;
    if (calls) *calls = 0;
    for (int q = 0; q < nRigs; q++) {
        const long long fL = 2 * (rigFirst + (long long)q * rigStep), fR = fL + 1;
        const SfRig g = sfRig(nOut, monoOut, fL, capacity);
        const int nLap = g.nR - g.monoR;
        for (int i = 0; i < capacity; i++) {                     // k_stereo_fisheye_init and the rows outside the lapping area
            l2r[fL * cap + i] = -1; r2l[fR * cap + i] = -1; depth[fL * cap + i] = -1.0f;
            for (int k = 0; k < 3; k++) x3d[(fL * cap + i) * 3 + k] = 0.0f;
        }
        int accepted = 0, passed = 0;
        const LdsU4 *descL = (const LdsU4*)(desc + fL * cap * 32), *descR = (const LdsU4*)(desc + fR * cap * 32);
        for (int i = g.monoL; i < g.nL; i++) {
            const LdsU4 a = descL[2LL * i], b = descL[2LL * i + 1];
            SfBest best{kSfNoDistance, -1, kSfNoDistance};
            for (int c = 0; c < nLap; c += kSfChunk) {
                const int n = min(kSfChunk, nLap - c);
                std::vector<LdsU4> chunk(descR + 2LL * (g.monoR + c), descR + 2LL * (g.monoR + c + n));      // exactly the staged descriptors
                sfScanChunk(a, b, chunk.data(), n, g.monoR + c, best);
            }
            if (!sfRatioPass(best, nLap)) continue;
            passed++;
            float z, x[3];
            if (!sfGeometry(p, sGate.data(), kps[fL * cap + i], kps[fR * cap + best.i0], z, x)) continue;
            l2r[fL * cap + i] = best.i0; depth[fL * cap + i] = z;
            for (int k = 0; k < 3; k++) x3d[(fL * cap + i) * 3 + k] = x[k];
            r2l[fR * cap + best.i0] = max(r2l[fR * cap + best.i0], i);
            accepted++;
        }
        nMatches[q] = accepted;
        if (nDescMatches) nDescMatches[q] = passed;
        if (calls) *calls += passed;
    }
}
int stereo_fisheye_chunk() { return kSfChunk; }
int stereo_fisheye_tile() { return kSfThreads; }
// the kernel's integer form of the ratio test on a list of two
int stereo_fisheye_ratio(int d0, int d1) { return sfRatioPass(SfBest{d0, 0, d1}, 2) ? 1 : 0; }

}  // extern "C"

#ifdef STEREO_FISHEYE_HOST_MAIN
int main() {
    std::mt19937 rng(7);
    auto U = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
    const float cams[16] = {190.97847715128717f, 190.9733070521226f, 254.93170605935475f, 256.8974428996504f, 0.0034823894022493434f,
                            0.0007150348452162257f, -0.0020532361418706202f, 0.00020293673591811182f, 190.44236969414825f, 190.4344384721956f,
                            252.59949716835982f, 254.91723064636983f, 0.0034003170790442797f, 0.001766278153469831f, -0.00266312569781606f,
                            0.0003299517423931039f};
    float sigma2[8];
    for (int l = 0; l < 8; l++) sigma2[l] = std::pow(1.2f, 2 * l);
    struct Case { const char* name; int cap, nL, nR, monoL, monoR; bool nan; };
    const Case cases[] = {{"plain", 40, 33, 37, 5, 9, false},           {"no left lapping row", 40, 12, 30, 12, 3, false},
                          {"no right lapping row", 40, 30, 12, 3, 12, false}, {"one right row", 40, 30, 8, 2, 7, false},
                          {"two right rows", 40, 30, 9, 2, 7, false},   {"mono == N on both", 40, 20, 20, 20, 20, false},
                          {"mono out of range", 40, 30, 30, -4, 1000, false}, {"mono negative right", 40, 30, 30, 500, -9, false},
                          {"capacity 1", 1, 1, 1, 0, 0, false},         {"N past the capacity", 33, 90, 70, 3, 2, false},
                          {"an empty rig", 16, 0, 0, 0, 0, false},      {"a chunk and one", 160, 20, 135, 4, 6, false},
                          {"a NaN transform", 40, 33, 37, 0, 0, true}};
    long total = 0;
    for (const Case& c : cases) {
        const int rigs = 2, B = 2 * rigs, cap = c.cap;
        float tlr[12] = {1, 0, 0, 0.1f, 0, 1, 0, 0, 0, 0, 1, 0};
        if (c.nan) tlr[7] = NAN;
        // exact-size heap blocks: an access one element past any of them is reported
        std::vector<Keypoint> kps((size_t)B * cap);
        std::vector<uint8_t> desc((size_t)B * cap * 32);
        std::vector<int> nout(B), mono(B), l2r((size_t)B * cap, -7), r2l((size_t)B * cap, -7), nm(rigs), nd(rigs);
        std::vector<float> depth((size_t)B * cap, -7.f), x3d((size_t)B * cap * 3, -7.f);
        for (int f = 0; f < B; f++) {
            nout[f] = f & 1 ? c.nR : c.nL; mono[f] = f & 1 ? c.monoR : c.monoL;
            for (int i = 0; i < cap; i++) {
                Keypoint& k = kps[(size_t)f * cap + i];
                // a grid of points 2 m deep seen by both eyes (disparity 0.1 / 2 * fx), the principal point, far outside, octaves off the table
                k.x = i == 0 ? cams[2] : i == 1 ? 1e6f : 60.f + 11.f * (i % 37) - (f & 1 ? 9.5f : 0.f) + U(-0.2f, 0.2f);
                k.y = i == 0 ? cams[3] : 80.f + 9.f * (i % 41) + U(-0.2f, 0.2f);
                k.angle = 0.f; k.octave = i % 7 == 3 ? (int)U(-5, 30) : (int)U(0, 4);
                for (int b = 0; b < 32; b++) desc[((size_t)f * cap + i) * 32 + b] = (uint8_t)((i * 73 + b * 31) ^ (b < 1 ? rng() & 3 : 0));
            }
        }
        int calls = 0;
        stereo_fisheye_host(rigs, 0, 1, kps.data(), desc.data(), nout.data(), mono.data(), cap, tlr, cams, sigma2, 8, l2r.data(), r2l.data(),
                            depth.data(), x3d.data(), nm.data(), nd.data(), &calls);
        std::printf("%-22s cap %3d: matches %d %d of %d %d rows past the ratio test\n", c.name, cap, nm[0], nm[1], nd[0], nd[1]);
        for (int r = 0; r < rigs; r++) {
            for (int i = 0; i < cap; i++) {
                const int m = l2r[(size_t)(2 * r) * cap + i], back = r2l[(size_t)(2 * r + 1) * cap + i];
                if (m < -1 || m >= cap || back < -1 || back >= cap) { std::printf("FAILED: an index outside the rig\n"); return 1; }
                if (l2r[(size_t)(2 * r + 1) * cap + i] != -7 || r2l[(size_t)(2 * r) * cap + i] != -7 || depth[(size_t)(2 * r + 1) * cap + i] != -7.f) {
                    std::printf("FAILED: a row of the other eye was written\n"); return 1;
                }
            }
            if (c.nan && nm[r] != 0) { std::printf("FAILED: a NaN transform matched\n"); return 1; }
            if ((c.nR - c.monoR < 2 || c.nL - c.monoL < 1) && !(c.monoL < 0 || c.monoR < 0 || c.monoL > c.nL || c.monoR > c.nR) && nd[r] != 0) {
                std::printf("FAILED: a match without two right lapping rows\n"); return 1;
            }
        }
        total += nm[0] + nm[1];
    }
    if (total == 0) { std::printf("FAILED: nothing matched at all\n"); return 1; }
    std::printf("stereo_fisheye_host_check: every access inside its arrays, %ld matches\n", total);
    return 0;
}
#endif
