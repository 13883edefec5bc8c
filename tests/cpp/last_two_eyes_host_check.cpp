// last_two_eyes_host_check.cpp - extractorb_amd/csrc/k_project_last_two_eyes_point.hpp (with k_camera_kb8.hpp) compiled for the HOST
// (tests/cpp/host_shim stands in for the device vocabulary): the front half of the two-camera frame-to-frame projection search, one request
// after the other - what k_project_last_two_eyes does with one thread per request.  Two uses, both without a GPU:
//   * as a shared library (tests/test_last_frame_two_eyes.py): last_two_eyes_host() over the scenes of the GPU tests, compared with the walk;
//   * as a stand-alone program under -fsanitize=address,undefined: exact-size heap buffers, keypoint counts outside [0, capacity],
//     coordinates that are 0, infinite and NaN - every access stays inside its arrays and nothing traps.
#include "host_shim/kb8_shim.h"

#include <cstddef>
#include <cstdio>
#include <random>
#include <vector>

#include "../../extractorb_amd/csrc/k_project_last_two_eyes_point.hpp"

using namespace orbx;

// every pair: 2 * capacity requests, two records each; exits (may be NULL): where each MapPoint left
static void runPairs(const Keypoint* kps, const int* nOut, const uint8_t* mpFlags, const float* world, const float* poses,
                     const ProjectTwoEyesParams& p, int nPairs, ProjQuery* queries, int* exits) {
    for (int pair = 0; pair < nPairs; pair++)
        for (int j = 0; j < 2 * p.capacity; j++) {
            ProjQuery qL, qR;
            const int code = projectLastTwoEyesRequest(kps, nOut, mpFlags, world, poses, p, pair, j, qL, qR);
            ProjQuery* out = queries + ((size_t)pair * 2 * p.capacity + j) * 2;
            out[0] = qL; out[1] = qR;
            if (exits) exits[(size_t)pair * 2 * p.capacity + j] = code;
        }
}

extern "C" int last_two_eyes_host_params_size() { return (int)sizeof(ProjectTwoEyesParams); }
// byte offset of every field of ProjectTwoEyesParams, in declaration order (the test's ctypes mirror must agree field by field)
extern "C" int last_two_eyes_host_params_offsets(int* out, int n) {
    const int off[] = {(int)offsetof(ProjectTwoEyesParams, cam), (int)offsetof(ProjectTwoEyesParams, minX), (int)offsetof(ProjectTwoEyesParams, maxX),
                       (int)offsetof(ProjectTwoEyesParams, minY), (int)offsetof(ProjectTwoEyesParams, maxY), (int)offsetof(ProjectTwoEyesParams, scale),
                       (int)offsetof(ProjectTwoEyesParams, trl), (int)offsetof(ProjectTwoEyesParams, mb), (int)offsetof(ProjectTwoEyesParams, th),
                       (int)offsetof(ProjectTwoEyesParams, mono), (int)offsetof(ProjectTwoEyesParams, capacity), (int)offsetof(ProjectTwoEyesParams, lastFirst),
                       (int)offsetof(ProjectTwoEyesParams, lastStep), (int)offsetof(ProjectTwoEyesParams, curFirst), (int)offsetof(ProjectTwoEyesParams, curStep)};
    const int m = (int)(sizeof(off) / sizeof(off[0]));
    for (int i = 0; i < m && i < n; i++) out[i] = off[i];
    return m;
}
extern "C" void last_two_eyes_host(const void* kps, const int* nOut, const uint8_t* mpFlags, const float* world, const float* poses,
                                   const void* params, int nPairs, void* queries, int* exits) {
    runPairs((const Keypoint*)kps, nOut, mpFlags, world, poses, *(const ProjectTwoEyesParams*)params, nPairs, (ProjQuery*)queries, exits);
}

#ifdef LAST_TWO_EYES_HOST_MAIN
int main() {
    std::mt19937 rng(13);
    auto U = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
    for (int trial = 0; trial < 6; trial++) {
        const int cap = trial < 2 ? 1 : (trial < 4 ? 257 : 333), nPairs = trial & 1 ? 2 : 1;
        const bool wild = trial >= 4;
        const int rigs = nPairs + 1;                      // pair p: last rig p, current rig p + 1
        // exact-size heap blocks: an access one element past any of them is reported
        std::vector<Keypoint> kps((size_t)2 * rigs * cap);
        std::vector<int> nOut(2 * rigs);
        std::vector<uint8_t> fl((size_t)2 * rigs * cap);
        std::vector<float> world((size_t)2 * rigs * cap * 3), poses((size_t)rigs * 12, 0.f);
        std::vector<ProjQuery> queries((size_t)nPairs * 2 * cap * 2);
        std::vector<int> exits((size_t)nPairs * 2 * cap);
        for (int r = 0; r < rigs; r++) {
            float* T = &poses[(size_t)r * 12];
            T[0] = T[5] = T[10] = 1.f; T[3] = U(-.2f, .2f); T[7] = U(-.1f, .1f); T[11] = U(-.5f, .5f);
        }
        for (int f = 0; f < 2 * rigs; f++) {
            nOut[f] = wild ? (f % 3 == 0 ? cap + 9 : (f % 3 == 1 ? -4 : cap)) : cap - (cap > 1 && f % 2);      // counts outside [0, capacity]
            for (int i = 0; i < cap; i++) {
                const size_t a = (size_t)f * cap + i;
                kps[a] = Keypoint{U(0, 640), U(0, 480), 31.f, U(0, 360), 1.f, wild && i % 17 == 0 ? 99 - 200 * (i & 1) : (int)(rng() % 8), -1};
                fl[a] = (uint8_t)(rng() & 3);
                float x = U(-6, 6), y = U(-4, 4), z = U(-1, 8);
                if (wild) {
                    if (i % 7 == 0) z = 0.f;
                    if (i % 7 == 1) { x = 0.f; y = 0.f; }
                    if (i % 11 == 0) x = INFINITY;
                    if (i % 11 == 1) y = -INFINITY;
                    if (i % 13 == 0) z = NAN;
                    if (i % 13 == 1) x = NAN;
                    if (i % 19 == 0) z = INFINITY;
                    if (i % 23 == 0) { x = 3e38f; y = -3e38f; }
                }
                world[a * 3] = x; world[a * 3 + 1] = y; world[a * 3 + 2] = z;
            }
        }
        ProjectTwoEyesParams p{};
        const float k[8] = {190.9785f, 190.9733f, 254.9317f, 256.8974f, 0.0034824f, 0.00071503f, -0.0020532f, 0.00020294f};
        for (int i = 0; i < 8; i++) p.cam[i] = k[i];
        p.minX = 0; p.maxX = 512; p.minY = 0; p.maxY = 512;
        for (int l = 0; l < kMaxLevels; l++) p.scale[l] = std::pow(1.2f, (float)std::min(l, 7));
        const float trl[12] = {0.9998f, 0.01f, -0.017f, -0.1f, -0.0101f, 0.99995f, -0.002f, 0.001f, 0.017f, 0.0022f, 0.99985f, 0.002f};
        for (int i = 0; i < 12; i++) p.trl[i] = trl[i];
        p.mb = trial == 2 ? 0.01f : 0.3f; p.th = 7.f; p.mono = trial == 3; p.capacity = cap;
        p.lastFirst = 0; p.lastStep = 1; p.curFirst = 1; p.curStep = 1;
        runPairs(kps.data(), nOut.data(), fl.data(), world.data(), poses.data(), p, nPairs, queries.data(), exits.data());
        long hist[4] = {};
        for (size_t a = 0; a < exits.size(); a++) {
            hist[exits[a]]++;
            const ProjQuery &L = queries[2 * a], &R = queries[2 * a + 1];
            const bool req = exits[a] == kLastRequest;
            if ((L.flags & 1) != (int)req || (R.flags & 1) != (int)req || (req && (L.u < p.minX || L.u > p.maxX || L.v < p.minY || L.v > p.maxY)) ||
                (req && (L.radius != R.radius || L.minLevel != R.minLevel || L.maxLevel != R.maxLevel || L.minLevel < -1 || L.maxLevel > kMaxLevels)) ||
                (!req && (L.u != 0.f || R.radius != 0.f))) {
                std::printf("trial %d request %zu inconsistent\n", trial, a);
                return 1;
            }
        }
        std::printf("trial %d capacity %d pairs %d wild %d exits %ld %ld %ld %ld\n", trial, cap, nPairs, (int)wild, hist[0], hist[1], hist[2], hist[3]);
    }
    std::printf("clean\n");
    return 0;
}
#endif
