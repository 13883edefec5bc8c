// sim3_host_check.cpp - extractorb_amd/csrc/k_project_sim3.hip compiled for the HOST (tests/cpp/host_shim stands in for the device
// vocabulary).  k_sim3_window runs one thread at a time; the settling is EMULATED in rounds with the kernel's own per-request step
// (sim3RoundStep -> sim3Decide of k_sim3_decide.hpp, and the re-scan): all requests of a round decide against the previous round's closedBy,
// closedBy is rebuilt, until no decision changes - what k_sim3_settle does with a workgroup.  Two uses, both without a GPU:
//   * as a shared library (tests/test_sim3_projection.py): sim3_host() over the scenes of the GPU tests, compared with the walk;
//   * as a stand-alone program under -fsanitize=address,undefined: exact-size heap buffers, valid and CORRUPT grids (garbage offsets and
//     indices, counts above the capacities, octaves outside the tables), a negative radius - every access stays inside its arrays.
#include "host_shim/sim3_shim.h"

#include <climits>
#include <cstdio>
#include <random>
#include <vector>

#include "../../extractorb_amd/csrc/k_project_sim3.hip"

using namespace orbx;
extern "C" int orbx_predict_scale_breakpoints(float, int, float*);

// stats2: [0] rounds of the last pair, [1] requests of all pairs whose final decision came from a re-scan
static void runAll(const float* w, const float* nv, const float* dist, const uint8_t* md, const int* nmp, const uint8_t* fl, const float* poses,
                   const Keypoint* kps, const uint8_t* desc, const int* nout, const int* off, const int* idx, const uint8_t* occ,
                   const Sim3SearchParams& p, int* matches, int* mi, int* mdist, uint8_t* ex, int* nm, int pairs, int* stats2) {
    const size_t total = (size_t)pairs * p.mpCapacity;
    std::vector<Sim3Record> rec(total);
    for (int pr = 0; pr < pairs; pr++)
        for (int b = 0; b < (p.mpCapacity + 255) / 256; b++)
            for (int t = 0; t < 256; t++) {
                blockIdx = dim3(b, pr); threadIdx = dim3(t);
                k_sim3_window(w, nv, dist, md, nmp, fl, poses, kps, desc, nout, off, idx, occ, p, rec.data(), ex);
            }
    stats2[0] = stats2[1] = 0;
    for (int pr = 0; pr < pairs; pr++) {
        const long long f = p.kfFirst + (long long)pr * p.kfStep;
        std::vector<int> closedBy(p.capacity, INT_MAX), dec(p.mpCapacity, kSim3NoKey), next(p.mpCapacity);
        int rounds = 0, rescans = 0;
        for (int round = 1; round <= p.mpCapacity + 1; round++) {
            bool changed = false;
            rescans = 0;
            for (int i = 0; i < p.mpCapacity; i++) {
                bool rescanned;
                next[i] = sim3RoundStep(i, pr, dec[i], md, kps, desc, nout, off, idx, occ, p, rec.data(), closedBy.data(), &rescanned);
                rescans += rescanned;
                changed |= next[i] != dec[i] && !(sim3IsNone(next[i]) && sim3IsNone(dec[i]));
            }
            dec = next;
            rounds = round;
            if (!changed) break;
            std::fill(closedBy.begin(), closedBy.end(), INT_MAX);
            for (int i = 0; i < p.mpCapacity; i++)
                if (!sim3IsNone(dec[i])) closedBy[sim3Slot(dec[i])] = std::min(closedBy[sim3Slot(dec[i])], i);
        }
        int* out = matches + (size_t)pr * p.capacity;
        for (int s = 0; s < p.capacity; s++) out[s] = -1;
        int n = 0;
        for (int i = 0; i < p.mpCapacity; i++) {
            const size_t o = (size_t)pr * p.mpCapacity + i;
            if (sim3IsNone(dec[i])) { mi[o] = -1; mdist[o] = 256; continue; }
            const int g = std::min(std::max(idx[f * p.capacity + sim3Slot(dec[i])], 0), p.capacity - 1);
            out[g] = i; mi[o] = g; mdist[o] = sim3Dist(dec[i]);
            if (ex) ex[o] = 7;
            n++;
        }
        nm[pr] = n;
        stats2[0] = rounds; stats2[1] += rescans;
    }
}

extern "C" int sim3_host_params_size() { return (int)sizeof(Sim3SearchParams); }
extern "C" int sim3_host_list_length() { return kSim3Top; }
extern "C" void sim3_host(const float* w, const float* nv, const float* dist, const uint8_t* md, const int* nmp, const uint8_t* fl, const float* poses,
                          const void* kps, const uint8_t* desc, const int* nout, const int* off, const int* idx, const uint8_t* occ,
                          const void* params, int* matches, int* mi, int* mdist, uint8_t* ex, int* nm, int pairs, int* stats2) {
    runAll(w, nv, dist, md, nmp, fl, poses, (const Keypoint*)kps, desc, nout, off, idx, occ, *(const Sim3SearchParams*)params, matches, mi, mdist, ex,
           nm, pairs, stats2);
}

#ifdef SIM3_HOST_MAIN
int main() {
    std::mt19937 rng(7);
    auto U = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
    for (int trial = 0; trial < 6; trial++) {
        const bool corrupt = trial >= 3;
        const int cap = trial % 3 == 0 ? 97 : 1302, mpCap = trial % 3 == 1 ? 5000 : 333, pairs = 3, B = 3;
        // exact-size heap blocks: an access one element past any of them is reported
        std::vector<Keypoint> kps((size_t)B * cap);
        std::vector<uint8_t> desc((size_t)B * cap * 32), occ((size_t)pairs * cap);
        std::vector<float> poses(pairs * 12, 0.f);
        std::vector<int> nout(B), off((size_t)B * 3073), idx((size_t)B * cap);
        for (int q = 0; q < pairs; q++) { poses[q * 12 + 0] = poses[q * 12 + 5] = poses[q * 12 + 10] = 1.f; poses[q * 12 + 3] = U(-.2f, .2f); }
        // few distinct descriptors: many MapPoints want the same keypoints, windows hold more equal candidates than a key list
        std::vector<std::vector<uint8_t>> words(5, std::vector<uint8_t>(32));
        for (auto& wd : words) for (auto& b : wd) b = (uint8_t)rng();
        for (int f = 0; f < B; f++) {
            nout[f] = corrupt ? cap + 50 : cap - 5;
            std::vector<std::vector<int>> cells(64 * 48);
            for (int i = 0; i < cap; i++) {
                Keypoint& k = kps[(size_t)f * cap + i];
                k.x = U(0, 634); k.y = U(0, 474); k.octave = corrupt ? (int)U(-3, 20) : (int)U(0, 3);
                const std::vector<uint8_t>& wd = words[rng() % 5];
                std::copy(wd.begin(), wd.end(), desc.begin() + ((size_t)f * cap + i) * 32);
                if (i < cap - 5) cells[(int)std::round(k.x * .1f) * 48 + (int)std::round(k.y * .1f)].push_back(i);
            }
            int s = 0;
            for (int c = 0; c < 64 * 48; c++) { off[(size_t)f * 3073 + c] = s; for (int i : cells[c]) idx[(size_t)f * cap + s++] = i; }
            off[(size_t)f * 3073 + 64 * 48] = s;
            if (corrupt) {
                if (trial != 4) for (int c = 0; c <= 64 * 48; c++) off[(size_t)f * 3073 + c] = (int)U(-1e6f, 1e6f);      // (trial 4: valid offsets over garbage indices)
                for (int i = 0; i < cap; i++) idx[(size_t)f * cap + i] = (int)U(-1e6f, 1e6f);
            }
        }
        for (auto& o : occ) o = rng() % 4 == 0;
        std::vector<float> w((size_t)mpCap * 3), nv((size_t)mpCap * 3), dist((size_t)mpCap * 3);
        std::vector<uint8_t> md((size_t)mpCap * 32), fl((size_t)pairs * mpCap);
        for (int i = 0; i < mpCap; i++) {
            const float z = U(-1, 8), u = U(-50, 700), v = U(-50, 530);
            w[3 * i] = (u - 320) / 450 * z; w[3 * i + 1] = (v - 240) / 450 * z; w[3 * i + 2] = z;
            const float d = std::sqrt(w[3 * i] * w[3 * i] + w[3 * i + 1] * w[3 * i + 1] + z * z);
            for (int c = 0; c < 3; c++) nv[3 * i + c] = w[3 * i + c] / (d + 1e-6f);
            dist[3 * i] = 0; dist[3 * i + 1] = 1e9f; dist[3 * i + 2] = d * U(0.5f, corrupt ? 1e30f : 1.6f);
            const std::vector<uint8_t>& wd = words[rng() % 5];
            std::copy(wd.begin(), wd.end(), md.begin() + (size_t)i * 32);
        }
        for (auto& x : fl) x = rng() % 8 != 0;
        std::vector<int> nmp(1, corrupt ? mpCap + 9 : mpCap - 3), matches((size_t)pairs * cap), mi((size_t)pairs * mpCap), mdist((size_t)pairs * mpCap), nm(pairs, 0);
        std::vector<uint8_t> ex((size_t)pairs * mpCap);
        Sim3SearchParams p{};
        p.fx = p.fy = 450; p.cx = 320; p.cy = 240; p.minX = 0; p.maxX = 640; p.minY = 0; p.maxY = 480; p.wInv = 0.1f; p.hInv = 0.1f;
        p.nlevels = 8;
        for (int l = 0; l < 8; l++) p.scale[l] = std::pow(1.2f, (float)l);
        orbx_predict_scale_breakpoints(1.2f, 8, p.breaks);
        p.th = trial == 2 ? -300.f : (corrupt ? 40.f : 12.f); p.maxDist = trial == 1 ? 255 : 75; p.projection = trial & 1; p.capacity = cap; p.mpCapacity = mpCap;
        p.kfFirst = 1; p.kfStep = trial == 0 ? 0 : 1; p.mpFirst = 0; p.mpStep = 0;
        const int usedPairs = trial == 0 ? 3 : 2;      // (kfStep 1 from keyframe 1: keyframes 1, 2)
        int stats2[2];
        runAll(w.data(), nv.data(), dist.data(), md.data(), nmp.data(), fl.data(), poses.data(), kps.data(), desc.data(), nout.data(), off.data(),
               idx.data(), trial == 4 ? nullptr : occ.data(), p, matches.data(), mi.data(), mdist.data(), trial == 5 ? nullptr : ex.data(), nm.data(),
               usedPairs, stats2);
        long hist[8] = {};
        if (trial != 5) for (size_t i = 0; i < (size_t)usedPairs * mpCap; i++) hist[ex[i] & 7]++;
        std::printf("trial %d capacity %d mappoints %d corrupt %d rounds %d rescans %d matches %d exits", trial, cap, mpCap, (int)corrupt, stats2[0],
                    stats2[1], nm[0]);
        for (long h : hist) std::printf(" %ld", h);
        std::printf("\n");
    }
    std::printf("clean\n");
    return 0;
}
#endif
