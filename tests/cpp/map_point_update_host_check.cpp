// map_point_update_host_check.cpp - extractorb_amd/csrc/k_map_point_update.hpp, the statement of k_map_point_update.hip, compiled for the
// HOST (tests/cpp/host_shim stands in for the device vocabulary) and run one point at a time: every listed MapPoint goes through
// mpuPointSerial, which is the kernel's own entry check, centre, product, bisection and finish in list order.  What the kernel deals to
// lanes (who stages which entry, who walks which row, DPP sums and minima) is not emulated: a count is a loop here.
// Two uses, both without a GPU:
//   * as a shared library (tests/test_map_point_update.py, tests/test_map_point_update_gpu.py): mpu_host() over the scenes of the GPU
//     tests, compared byte for byte with the walk, and the reference of the working-size GPU test;
//   * as a stand-alone program (-DMAP_POINT_UPDATE_HOST_MAIN) under -fsanitize=address,undefined on exact-size heap blocks: frames and rows
//     outside the batch, a reference entry outside the list, negative offsets and slots, lists of 0, 1024 and 1025 entries, octaves
//     outside the table, every `what` - every access stays inside its arrays and a refused point writes no table row.
#include "host_shim/map_point_update_shim.h"

#include <cstdio>
#include <random>
#include <vector>

#include "../../extractorb_amd/csrc/k_map_point_update.hpp"

using namespace orbx;

extern "C" {

// the arguments of orbx_update_map_points_device (twoEyes = 0; nFrames batch frames) or orbx_update_map_points_two_eyes_device
// (twoEyes = 1; nFrames = 2 * rigs) on host arrays; scale: the handle's mvScaleFactors [nlevels]
void mpu_host(int twoEyes, int nPoints, const int* obsOff, const int* obs, const uint8_t* obsFlags, const int* ref, const int* slot,
              const float* mpWorld, const float* poses, const float* tlr12, int nFrames, const void* kps, const uint8_t* desc, const int* nOut,
              int capacity, const float* scale, int nlevels, int what, uint8_t* mpDesc, float* mpNormal, float* mpDist, int* best,
              int* bestMedian, uint8_t* status) {
    MapPointUpdateParams p{};
    for (int l = 0; l < nlevels && l < kMaxLevels; l++) p.scale[l] = scale[l];
    if (tlr12) for (int i = 0; i < 12; i++) p.tlr[i] = tlr12[i];
    p.nlevels = nlevels; p.capacity = capacity; p.nFrames = nFrames; p.nPoints = nPoints; p.what = what;
    const MapPointUpdateArrays a{obsOff, obs, obsFlags, ref, slot, mpWorld, poses, (const Keypoint*)kps, desc, nOut,
                                 mpDesc, mpNormal, mpDist, best, bestMedian, status};
    for (long long m = 0; m < nPoints; m++) {
        if (twoEyes) mpuPointSerial<true>(a, p, m);
        else mpuPointSerial<false>(a, p, m);
    }
}
int mpu_max_observations() { return kMpuMaxObservations; }

}  // extern "C"

#ifdef MAP_POINT_UPDATE_HOST_MAIN
int main() {
    std::mt19937 rng(21);
    auto U = [&](int a, int b) { return std::uniform_int_distribution<int>(a, b)(rng); };
    auto F = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
    const float tlr[12] = {0.8f, 0.f, 0.6f, 0.4f, 0.f, 1.f, 0.f, -0.2f, -0.6f, 0.f, 0.8f, 0.1f};
    float scale[8];
    for (int l = 0; l < 8; l++) scale[l] = std::pow(1.2f, (float)l);
    long points = 0, ok = 0;
    for (int twoEyes = 0; twoEyes < 2; twoEyes++)
        for (int trial = 0; trial < 6; trial++) {
            // trial: 0 plain, 1 wild frames and rows, 2 wild d_ref / offsets / slots, 3 octaves outside the table, 4 all flagged / no flags, 5 long lists
            const int cap = trial % 2 ? 7 : 33, kfs = 3, B = twoEyes ? 2 * kfs : kfs, nPoints = trial == 5 ? 6 : 40, slots = nPoints + 5;
            std::vector<int> lens(nPoints);
            for (int m = 0; m < nPoints; m++) lens[m] = trial == 5 ? (m == 0 ? 1024 : m == 1 ? 1025 : m == 2 ? 0 : U(60, 300)) : U(0, 20);
            std::vector<int> off(nPoints + 1, 0);
            for (int m = 0; m < nPoints; m++) off[m + 1] = off[m] + lens[m];
            const int total = off[nPoints];
            // exact-size heap blocks: an access one element past any of them is reported
            std::vector<int> obs((size_t)2 * total), ref(nPoints), slot(nPoints), nOut(B), best(nPoints, -7), bestMedian(nPoints, -7);
            std::vector<uint8_t> flags(total), desc((size_t)B * cap * 32), mpDesc((size_t)slots * 32, 0xEE), status(nPoints, 0xEE);
            std::vector<float> world((size_t)slots * 3), poses((size_t)kfs * 12, 0.f), mpNormal((size_t)slots * 3, -7.f), mpDist((size_t)slots * 3, -7.f);
            std::vector<Keypoint> kps((size_t)B * cap);
            for (auto& b : desc) b = (uint8_t)U(0, 255);
            for (auto& w : world) w = F(-3.f, 3.f);
            for (int r = 0; r < kfs; r++) { poses[r * 12] = poses[r * 12 + 5] = poses[r * 12 + 10] = 1.f; poses[r * 12 + 3] = -0.4f * r; poses[r * 12 + 11] = 5.f; }
            for (int f = 0; f < B; f++) nOut[f] = trial == 1 && f == 0 ? cap + 50 : cap - (f % 3);
            for (auto& k : kps) { k = Keypoint{}; k.octave = trial == 3 ? U(-6, 30) : U(0, 7); }
            for (int o = 0; o < total; o++) {
                const bool wild = trial == 1 && o % 5 == 0;
                obs[2 * o] = wild ? U(-3, B + 2) : U(0, B - 1);
                obs[2 * o + 1] = wild ? U(-3, cap + 3) : U(0, cap - 3);
                flags[o] = trial == 4 ? 1 : (uint8_t)(U(0, 3) == 0);
            }
            for (int m = 0; m < nPoints; m++) {
                ref[m] = trial == 2 && m % 3 == 0 ? U(-2, lens[m] + 1) : lens[m] ? U(0, lens[m] - 1) : 0;
                slot[m] = trial == 2 && m % 7 == 0 ? -1 - m : (m * 7) % slots;
            }
            if (trial == 2) { off[0] = -3; }      // (point 0 then owns three entries in front of d_obs: refused, never read)
            for (int what = 1; what <= 3; what++) {
                mpu_host(twoEyes, nPoints, off.data(), obs.data(), trial == 4 && what == 2 ? nullptr : flags.data(), ref.data(),
                         trial == 0 ? nullptr : slot.data(), world.data(), poses.data(), twoEyes ? tlr : nullptr, B, kps.data(), desc.data(),
                         nOut.data(), cap, scale, 8, what, mpDesc.data(), mpNormal.data(), mpDist.data(), best.data(), bestMedian.data(),
                         status.data());
                for (int m = 0; m < nPoints; m++, points++) {
                    if (status[m] > kMpuTooLong) { std::printf("FAILED: status %d\n", status[m]); return 1; }
                    const bool skew = trial == 2 && m == 0;      // its list starts in front of d_obs: refused, never read
                    if (skew ? status[m] != kMpuBadIndex : (lens[m] == 0) != (status[m] == kMpuEmpty)) { std::printf("FAILED: EMPTY / BAD_INDEX\n"); return 1; }
                    if ((lens[m] > 1024) != (status[m] == kMpuTooLong)) { std::printf("FAILED: TOO_LONG\n"); return 1; }
                    if ((best[m] >= 0) != (status[m] == kMpuOk && (what & 1))) { std::printf("FAILED: best %d beside status %d\n", best[m], status[m]); return 1; }
                    ok += status[m] == kMpuOk;
                }
            }
            std::printf("%s trial %d: %d points, %d entries\n", twoEyes ? "two eyes  " : "one camera", trial, nPoints, total);
        }
    if (ok == 0) { std::printf("FAILED: no point was updated at all\n"); return 1; }
    std::printf("map_point_update_host_check: every access inside its arrays, %ld points, %ld updated\n", points, ok);
    return 0;
}
#endif
