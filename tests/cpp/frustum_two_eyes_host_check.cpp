// frustum_two_eyes_host_check.cpp - extractorb_amd/csrc/k_frustum_two_eyes_point.hpp (with k_camera_kb8.hpp) compiled for the HOST
// (tests/cpp/host_shim stands in for the device vocabulary): the rig invariants, isInFrustumChecks per eye, the far decision and the two
// requests of a slot, one MapPoint after the other, the slots appended in list order and cut at the query capacity - what
// k_frustum_two_eyes_check / _place do with lane pairs, ballots and per-workgroup counts, which is NOT emulated here.  Two uses, both without
// a GPU:
//   * as a shared library (tests/test_frustum_requests_two_eyes.py): frustum_two_eyes_host() over the scenes of the GPU tests, compared with
//     the walk;
//   * as a stand-alone program under -fsanitize=address,undefined: exact-size heap buffers, NULL for the optional pointers, list counts
//     outside [0, capacity], query capacities below the produced count, coordinates that are 0, infinite and NaN - every access stays inside
//     its arrays and nothing traps.
#include "host_shim/kb8_shim.h"

#include <cstddef>
#include <cstdio>
#include <random>
#include <vector>

#include "../../extractorb_amd/csrc/k_frustum_two_eyes_point.hpp"

using namespace orbx;
extern "C" int orbx_predict_scale_breakpoints(float, int, float*);

// one pair: list 0, rig frame 0.  prev, nWanted may be NULL.  Slots past the written ones: all-zero requests, src -1, the descriptor untouched.
static void runList(const float* w, const float* nv, const float* dist, const uint8_t* md, const int* nmp, const uint8_t* fl, const float* prev,
                    const float* pose, const FrustumTwoEyesParams& p, ProjQuery* queries, uint8_t* qdesc, int* qsrc, int* nq, int* nWanted,
                    TrackRecord* track, int* nInView) {
    const int NM = nmp ? std::min(std::max(nmp[0], 0), p.mpCapacity) : p.mpCapacity;
    float eyes[2 * kFrustumEyeFloats];
    frustumTwoEyesRig(pose, p.trl, p.tlr, eyes);
    int total = 0, inView = 0;
    for (int i = 0; i < p.mpCapacity; i++) {
        TrackRecord t[2] = {frustumUntouched(), frustumUntouched()};
        const int flag = i < NM ? fl[i] : 0;
        bool in[2] = {false, false};
        if (flag & 1)
            for (int e = 0; e < 2; e++)
                in[e] = frustumEyeCheck(eyes + e * kFrustumEyeFloats, p.cam[e], w + 3 * i, nv + 3 * i, dist + 3 * i, p, t[e]) == kFrustumRequest;
        const bool any = in[0] || in[1];
        const bool far = any && frustumTwoEyesFar(in[0], t[0].depth, prev ? prev[i] : 0.0f, p);
        for (int e = 0; e < 2; e++) {
            if (in[e] && far) t[e].exit = kFrustumFar;
            track[2 * i + e] = t[e];
        }
        inView += any;
        if (any && !far) {
            if (total < p.queryCapacity) {
                for (int e = 0; e < 2; e++) queries[2 * total + e] = frustumTwoEyesRequest(t[e], e, flag, p);
                qsrc[total] = i;
                std::memcpy(qdesc + (size_t)total * 32, md + (size_t)i * 32, 32);
            }
            total++;
        }
    }
    const int written = std::min(total, p.queryCapacity);
    for (int k = written; k < p.queryCapacity; k++) {
        queries[2 * k] = queries[2 * k + 1] = ProjQuery{0.f, 0.f, 0.f, 0.f, 0, 0, 0, 0.f};
        qsrc[k] = -1;
    }
    *nq = written; *nInView = inView;
    if (nWanted) *nWanted = total;
}

extern "C" int frustum_two_eyes_host_params_size() { return (int)sizeof(FrustumTwoEyesParams); }
// byte offset of every field of FrustumTwoEyesParams, in declaration order (the test's ctypes mirror must agree field by field)
extern "C" int frustum_two_eyes_host_params_offsets(int* out, int n) {
#define OFF(f) (int)offsetof(FrustumTwoEyesParams, f)
    const int off[] = {OFF(cam), OFF(minX), OFF(maxX), OFF(minY), OFF(maxY), OFF(scale), OFF(breaks), OFF(trl), OFF(tlr), OFF(viewCosLimit), OFF(th),
                       OFF(thFarPoints), OFF(nlevels), OFF(farPoints), OFF(mpCapacity), OFF(queryCapacity), OFF(groups), OFF(curFirst), OFF(curStep),
                       OFF(mpFirst), OFF(mpStep)};
#undef OFF
    const int m = (int)(sizeof(off) / sizeof(off[0]));
    for (int i = 0; i < m && i < n; i++) out[i] = off[i];
    return m;
}
extern "C" void frustum_two_eyes_host(const float* w, const float* nv, const float* dist, const uint8_t* md, const int* nmp, const uint8_t* fl,
                                      const float* prev, const float* pose, const void* params, void* queries, uint8_t* qdesc, int* qsrc, int* nq,
                                      int* nWanted, void* track, int* nInView) {
    runList(w, nv, dist, md, nmp, fl, prev, pose, *(const FrustumTwoEyesParams*)params, (ProjQuery*)queries, qdesc, qsrc, nq, nWanted,
            (TrackRecord*)track, nInView);
}
// the thirty rig invariants alone (eye * 15 + {mR 0..8, mt 9..11, twc 12..14})
extern "C" void frustum_two_eyes_host_rig(const float* pose, const float* trl, const float* tlr, float* out30) { frustumTwoEyesRig(pose, trl, tlr, out30); }

#ifdef FRUSTUM_TWO_EYES_HOST_MAIN
int main() {
    std::mt19937 rng(17);
    auto U = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
    for (int trial = 0; trial < 6; trial++) {
        const int cap = trial < 2 ? 1 : (trial < 4 ? 1025 : 333);
        const bool wild = trial >= 4;
        const int qcap = trial == 3 ? 100 : cap;
        // exact-size heap blocks: an access one element past any of them is reported
        std::vector<float> w((size_t)cap * 3), nv((size_t)cap * 3), dist((size_t)cap * 3), prev(cap), pose(12, 0.f);
        std::vector<uint8_t> md((size_t)cap * 32), fl(cap), qdesc((size_t)qcap * 32, 0xA5);
        pose[0] = pose[5] = pose[10] = 1.f; pose[3] = U(-.2f, .2f); pose[7] = U(-.1f, .1f); pose[11] = U(-.2f, .2f);
        for (int i = 0; i < cap; i++) {
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
            w[3 * i] = x; w[3 * i + 1] = y; w[3 * i + 2] = z;
            const float d = std::sqrt(x * x + y * y + z * z);
            for (int c = 0; c < 3; c++) nv[3 * i + c] = w[3 * i + c] / (d + 1e-6f) + U(-.5f, .5f);
            dist[3 * i] = wild ? 0.f : d * U(0.3f, 1.1f); dist[3 * i + 1] = wild ? INFINITY : d * U(0.9f, 3.f); dist[3 * i + 2] = d * U(0.5f, wild ? 1e30f : 4.f);
            if (wild && i % 17 == 0) dist[3 * i + 2] = NAN;
            prev[i] = wild && i % 5 == 0 ? NAN : U(0, 9);
            fl[i] = (uint8_t)(rng() & 3);
            for (int b = 0; b < 32; b++) md[(size_t)i * 32 + b] = (uint8_t)rng();
        }
        std::vector<int> nmp(1, wild ? (trial == 4 ? cap + 9 : -4) : cap - (cap > 1)), qsrc(qcap), nq(1), nw(1), nin(1);
        std::vector<ProjQuery> queries((size_t)qcap * 2);
        std::vector<TrackRecord> track((size_t)cap * 2);
        FrustumTwoEyesParams p{};
        const float kl[8] = {190.9785f, 190.9733f, 254.9317f, 256.8974f, 0.0034824f, 0.00071503f, -0.0020532f, 0.00020294f};
        const float kr[8] = {190.4422f, 190.4344f, 252.5973f, 254.9194f, 0.0034004f, 0.0017663f, -0.0026631f, 0.00032995f};
        for (int i = 0; i < 8; i++) { p.cam[0][i] = kl[i]; p.cam[1][i] = kr[i]; }
        p.minX = 0; p.maxX = 512; p.minY = 0; p.maxY = 512;
        p.nlevels = 8;
        for (int l = 0; l < 8; l++) p.scale[l] = std::pow(1.2f, (float)l);
        orbx_predict_scale_breakpoints(1.2f, 8, p.breaks);
        const float trl[12] = {0.9998f, 0.01f, -0.017f, -0.1f, -0.0101f, 0.99995f, -0.002f, 0.001f, 0.017f, 0.0022f, 0.99985f, 0.002f};
        const float tlr[12] = {0.9998f, -0.0101f, 0.017f, 0.1f, 0.01f, 0.99995f, 0.0022f, -0.001f, -0.017f, -0.002f, 0.99985f, -0.0037f};
        for (int i = 0; i < 12; i++) { p.trl[i] = trl[i]; p.tlr[i] = tlr[i]; }
        p.viewCosLimit = 0.5f; p.th = trial == 2 ? 1.f : 3.f; p.thFarPoints = 5.f; p.farPoints = trial >= 2; p.mpCapacity = cap; p.queryCapacity = qcap;
        // the optional pointers are NULL in turn: no count (trial 3), no earlier depths (odd trials), no wanted count (trial 2)
        runList(w.data(), nv.data(), dist.data(), md.data(), trial == 3 ? nullptr : nmp.data(), fl.data(), trial & 1 ? nullptr : prev.data(), pose.data(), p,
                queries.data(), qdesc.data(), qsrc.data(), nq.data(), trial == 2 ? nullptr : nw.data(), track.data(), nin.data());
        long hist[7] = {};
        for (int i = 0; i < 2 * cap; i++) hist[track[i].exit]++;
        for (int k = 0; k < qcap; k++) {
            const bool used = k < nq[0];
            const ProjQuery &L = queries[2 * k], &R = queries[2 * k + 1];
            if (used != (qsrc[k] >= 0) || (used && k && qsrc[k] <= qsrc[k - 1]) || (used && !((L.flags | R.flags) & 1)) ||
                (used && (L.flags & 1) != (track[2 * qsrc[k]].exit == kFrustumRequest)) ||
                (used && (R.flags & 1) != (track[2 * qsrc[k] + 1].exit == kFrustumRequest)) || (used && (L.minLevel < -1 || L.maxLevel > 8)) ||
                (!used && (L.flags || R.flags || qdesc[(size_t)k * 32] != 0xA5))) {
                std::printf("trial %d slot %d inconsistent\n", trial, k);
                return 1;
            }
        }
        std::printf("trial %d mappoints %d capacity %d wild %d slots %d wanted %d in view %d exits", trial, cap, qcap, (int)wild, nq[0],
                    trial == 2 ? -1 : nw[0], nin[0]);
        for (long h : hist) std::printf(" %ld", h);
        std::printf("\n");
    }
    std::printf("clean\n");
    return 0;
}
#endif
