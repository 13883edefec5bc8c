// frustum_host_check.cpp - extractorb_amd/csrc/k_frustum_point.hpp compiled for the HOST (tests/cpp/host_shim stands in for the device
// vocabulary): frustumPoint over one MapPoint list, one MapPoint after the other, the requests appended in list order - what k_frustum's
// workgroup does with ballots and a scan, which is NOT emulated here.  Two uses, both without a GPU:
//   * as a shared library (tests/test_frustum_requests.py): frustum_host() over the scenes of the GPU tests, compared with the walk;
//   * as a stand-alone program under -fsanitize=address,undefined: exact-size heap buffers, both modes, the pointers each mode may leave NULL,
//     list counts outside [0, capacity], coordinates that overflow to infinity and NaN - every access stays inside its arrays.
#include "host_shim/frustum_shim.h"

#include <cstdio>
#include <random>
#include <vector>

#include "../../extractorb_amd/csrc/k_frustum_point.hpp"

using namespace orbx;
extern "C" int orbx_predict_scale_breakpoints(float, int, float*);

// one pair: list 0, frame 0.  Slots past the requests: an all-zero request, src -1, the descriptor untouched (as the kernel).
static void runList(const float* w, const float* nv, const float* dist, const uint8_t* md, const float* angle, const int* nmp, const uint8_t* fl,
                    const float* pose, const FrustumParams& p, ProjQuery* queries, uint8_t* qdesc, int* qsrc, int* nq, TrackRecord* track,
                    int* nInView) {
    const int NM = nmp ? std::min(std::max(nmp[0], 0), p.mpCapacity) : p.mpCapacity;
    int base = 0, inView = 0;
    for (int i = 0; i < p.mpCapacity; i++) {
        TrackRecord t = frustumUntouched();
        ProjQuery q{};
        int code = kFrustumFlag;
        if (i < NM) code = frustumPoint(pose, w + 3 * i, nv ? nv + 3 * i : nullptr, dist + 3 * i, angle ? angle[i] : 0.0f, fl[i], p, t, q);
        track[i] = t;
        inView += code >= kFrustumFar;
        if (code == kFrustumRequest) {
            queries[base] = q; qsrc[base] = i;
            std::memcpy(qdesc + (size_t)base * 32, md + (size_t)i * 32, 32);
            base++;
        }
    }
    for (int k = base; k < p.mpCapacity; k++) { queries[k] = ProjQuery{0.f, 0.f, 0.f, 0.f, 0, 0, 0, 0.f}; qsrc[k] = -1; }
    *nq = base; *nInView = inView;
}

extern "C" int frustum_host_params_size() { return (int)sizeof(FrustumParams); }
extern "C" void frustum_host(const float* w, const float* nv, const float* dist, const uint8_t* md, const float* angle, const int* nmp,
                             const uint8_t* fl, const float* pose, const void* params, void* queries, uint8_t* qdesc, int* qsrc, int* nq,
                             void* track, int* nInView) {
    runList(w, nv, dist, md, angle, nmp, fl, pose, *(const FrustumParams*)params, (ProjQuery*)queries, qdesc, qsrc, nq, (TrackRecord*)track, nInView);
}

#ifdef FRUSTUM_HOST_MAIN
int main() {
    std::mt19937 rng(11);
    auto U = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
    for (int trial = 0; trial < 6; trial++) {
        const int mode = trial & 1, cap = trial < 2 ? 1 : (trial < 4 ? 1025 : 333);
        const bool wild = trial >= 4;
        // exact-size heap blocks: an access one element past any of them is reported
        std::vector<float> w((size_t)cap * 3), nv((size_t)cap * 3), dist((size_t)cap * 3), angle(cap), pose(12, 0.f);
        std::vector<uint8_t> md((size_t)cap * 32), fl(cap), qdesc((size_t)cap * 32, 0xA5);
        pose[0] = pose[5] = pose[10] = 1.f; pose[3] = U(-.2f, .2f); pose[11] = U(-.2f, .2f);
        for (int i = 0; i < cap; i++) {
            const float z = wild && i % 7 == 0 ? 0.f : U(-1, 8), u = U(-50, 700), v = U(-50, 530);
            w[3 * i] = (u - 320) / 450 * (z == 0.f ? 1.f : z); w[3 * i + 1] = (v - 240) / 450 * z; w[3 * i + 2] = z;
            if (wild && i % 11 == 0) w[3 * i] = i % 22 ? 3e38f : NAN;
            const float d = std::sqrt(w[3 * i] * w[3 * i] + w[3 * i + 1] * w[3 * i + 1] + z * z);
            for (int c = 0; c < 3; c++) nv[3 * i + c] = w[3 * i + c] / (d + 1e-6f) + U(-.5f, .5f);
            dist[3 * i] = wild ? 0.f : d * U(0.3f, 1.1f); dist[3 * i + 1] = wild ? INFINITY : d * U(0.9f, 3.f); dist[3 * i + 2] = d * U(0.5f, wild ? 1e30f : 4.f);
            if (wild && i % 13 == 0) dist[3 * i + 2] = NAN;
            angle[i] = U(0, 360); fl[i] = (uint8_t)(rng() & 3);
            for (int b = 0; b < 32; b++) md[(size_t)i * 32 + b] = (uint8_t)rng();
        }
        std::vector<int> nmp(1, wild ? (trial == 4 ? cap + 9 : -4) : cap - (cap > 1)), qsrc(cap), nq(1), nin(1);
        std::vector<ProjQuery> queries(cap);
        std::vector<TrackRecord> track(cap);
        FrustumParams p{};
        p.fx = p.fy = 450; p.cx = 320; p.cy = 240; p.minX = 0; p.maxX = 640; p.minY = 0; p.maxY = 480;
        p.nlevels = 8;
        for (int l = 0; l < 8; l++) p.scale[l] = std::pow(1.2f, (float)l);
        orbx_predict_scale_breakpoints(1.2f, 8, p.breaks);
        p.mbf = 40.f; p.viewCosLimit = 0.5f; p.th = trial == 2 ? 1.f : 3.f; p.thFarPoints = 5.f; p.farPoints = trial >= 2; p.mode = mode; p.mpCapacity = cap;
        // the pointers a mode does not read are NULL; trial 3 passes no count
        runList(w.data(), mode == 0 ? nv.data() : nullptr, dist.data(), md.data(), mode == 1 ? angle.data() : nullptr, trial == 3 ? nullptr : nmp.data(),
                fl.data(), pose.data(), p, queries.data(), qdesc.data(), qsrc.data(), nq.data(), track.data(), nin.data());
        long hist[7] = {};
        for (int i = 0; i < cap; i++) hist[track[i].exit]++;
        for (int k = 0; k < cap; k++) {
            const bool used = k < nq[0];
            if (used != (qsrc[k] >= 0) || (used && track[qsrc[k]].exit != kFrustumRequest) || (used && k && qsrc[k] <= qsrc[k - 1]) ||
                (used && (queries[k].minLevel < -1 || queries[k].maxLevel > 8)) || (!used && qdesc[(size_t)k * 32] != 0xA5)) {
                std::printf("trial %d slot %d inconsistent\n", trial, k);
                return 1;
            }
        }
        std::printf("trial %d mode %d mappoints %d wild %d requests %d in view %d exits", trial, mode, cap, (int)wild, nq[0], nin[0]);
        for (long h : hist) std::printf(" %ld", h);
        std::printf("\n");
    }
    std::printf("clean\n");
    return 0;
}
#endif
