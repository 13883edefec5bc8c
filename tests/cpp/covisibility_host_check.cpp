// covisibility_host_check.cpp - extractorb_amd/csrc/k_covisibility.hpp, the statement of k_covisibility.hip, compiled for the HOST
// (tests/cpp/host_shim stands in for the device vocabulary): cvRank runs frame by frame, cvVote and rdKeyFrame subject by subject, a
// workgroup being one lane, on arrays of exactly the entries' sizes - the rank tables and the "LDS" block of a subject included.  Two uses,
// both without a GPU:
//   * as a shared library (tests/test_covisibility.py): cv_host() / rd_host() over the scenes of the GPU tests, compared with the walk byte
//     for byte; the entries' rejections and launch-time bounds; cv_time() / rd_time() for tools/covisibility_rate.py;
//   * as a stand-alone program (-DCOVISIBILITY_HOST_MAIN) under -fsanitize=address,undefined on exact-size heap blocks: indices outside
//     every table, negative and oversized counts, CSR offsets that decrease, empty everything; and the entries' rejections
//     (orbx_entry.hpp: covisBadArgument, covisUnsupported, redundancyBadArgument, redundancyUnsupported), one bad argument each.
#include "host_shim/covisibility_shim.h"

#include <chrono>
#include <cstdio>
#include <random>
#include <vector>

#include "../../extractorb_amd/csrc/k_covisibility.hpp"
#include "../../extractorb_amd/csrc/orbx_entry.hpp"

using namespace orbx;

extern "C" {

int cv_result_bytes() { return (int)sizeof(CovisResult); }
int rd_result_bytes() { return (int)sizeof(RedundancyResult); }
int cv_statuses() { return kCvStatuses; }
int rd_statuses() { return kRdStatuses; }
int cv_max_frames() { return kCvMaxFrames; }
int rd_max_capacity() { return kRdMaxCapacity; }
long cv_vote_lds_bytes(int nFrames) { return (long)cvVoteLdsBytes(nFrames); }
long rd_lds_bytes(int capacity) { return (long)rdLdsBytes(capacity); }
int cv_unsupported(int nFrames) { return covisUnsupported(nFrames) ? 1 : 0; }
int rd_unsupported(int capacity) { return redundancyUnsupported(capacity) ? 1 : 0; }
// the entries' refusals as orbx_entry.hpp states them.  ptrs (vote): d_obs_off, d_obs, d_mp_flags, d_kf_flags, d_kf_map_id, d_kf_key,
// d_subject_mp, d_subject_n, d_subject_kf, d_subject_map_id, d_counter_kf, d_counter_w, d_ordered_kf, d_ordered_w, d_result (15 pointers)
int cv_bad_argument(const void* const* q, int mode, int nPoints, int nFrames, int nSubjects, int capacity, int connCapacity) {
    return covisBadArgument(mode, nPoints, q[0], q[1], q[2], nFrames, q[3], q[4], q[5], nSubjects, q[6], q[7], capacity, q[8], q[9], connCapacity, q[10],
                            q[11], q[12], q[13], q[14]) ? 1 : 0;
}
// ptrs (redundancy): d_obs_off, d_obs, d_mp_flags, d_kf_flags, d_kps_un, d_n_out, d_depth, d_th_depth, d_subject_mp, d_subject_n,
// d_subject_kf, d_result (12 pointers)
int rd_bad_argument(const void* const* q, int nPoints, int nFrames, int nSubjects, int capacity, int monocular, float redundantTh) {
    return redundancyBadArgument(nPoints, q[0], q[1], q[2], nFrames, q[3], q[4], q[5], q[6], q[7], nSubjects, q[8], q[9], capacity, q[10], monocular,
                                 redundantTh, q[11]) ? 1 : 0;
}

// the arguments of orbx_covisibility_device on host arrays (without the handle)
void cv_host(int mode, int nPoints, const int* obsOff, const int* obs, const uint8_t* mpFlags, int nFrames, const uint8_t* kfFlags, const int* kfMap,
             const uint64_t* kfKey, int nSubjects, const int* subjectMp, const int* subjectN, int capacity, const int* subjectKf, const int* subjectMap,
             int th, int connCapacity, int* counterKf, int* counterW, int* orderedKf, int* orderedW, void* result) {
    const bool update = mode == kCvUpdateConnections;
    CovisParams p{};
    p.mode = mode; p.nPoints = nPoints; p.nFrames = nFrames; p.nSubjects = nSubjects; p.capacity = capacity; p.th = th; p.connCapacity = connCapacity;
    // exact-size heap blocks: an access one element past any of them is reported
    std::vector<int> rank(nFrames), byRank(nFrames), dupWords(cvRankBlocks(nFrames), 0);
    CovisArrays a{};
    a.obsOff = obsOff; a.obs = obs; a.mpFlags = mpFlags; a.kfFlags = kfFlags; a.kfMap = kfMap; a.kfKey = kfKey; a.subjectMp = subjectMp;
    a.subjectN = subjectN; a.subjectKf = update ? subjectKf : nullptr; a.subjectMap = update ? subjectMap : nullptr; a.counterKf = counterKf;
    a.counterW = counterW; a.orderedKf = update ? orderedKf : nullptr; a.orderedW = update ? orderedW : nullptr; a.result = result;
    a.wsRank = rank.data(); a.wsByRank = byRank.data(); a.wsDup = dupWords.data();
    for (int f = 0; f < nFrames; f++) {                       // k_covis_rank
        bool dup;
        const int r = cvRank(0, f, kfKey, nFrames, dup);
        rank[f] = r; byRank[r] = f;
        if (dup) dupWords[f / kCvRankBlock] = 1;
    }
    std::vector<uint64_t> lds((cvVoteLdsBytes(nFrames) + 7) / 8);
    for (int s = 0; s < nSubjects; s++) cvVote(0, s, a, p, (uint8_t*)lds.data());
}

// the arguments of orbx_keyframe_redundancy_device on host arrays (without the handle)
void rd_host(int nPoints, const int* obsOff, const int* obs, const uint8_t* mpFlags, const int* mpNobs, int nFrames, const uint8_t* kfFlags,
             const void* kpsUn, const int* nOut, const float* depth, const float* thDepth, int nSubjects, const int* subjectMp, const int* subjectN,
             int capacity, const int* subjectKf, int monocular, int thObs, float redundantTh, void* result, uint8_t* slotState) {
    CovisParams p{};
    p.nPoints = nPoints; p.nFrames = nFrames; p.nSubjects = nSubjects; p.capacity = capacity; p.monocular = monocular ? 1 : 0; p.thObs = thObs;
    p.redundantTh = redundantTh;
    CovisArrays a{};
    a.obsOff = obsOff; a.obs = obs; a.mpFlags = mpFlags; a.mpNobs = mpNobs; a.kfFlags = kfFlags; a.kpsUn = (const Keypoint*)kpsUn; a.nOut = nOut;
    a.depth = monocular ? nullptr : depth; a.thDepth = monocular ? nullptr : thDepth; a.subjectMp = subjectMp; a.subjectN = subjectN;
    a.subjectKf = subjectKf; a.result = result; a.slotState = slotState;
    std::vector<uint32_t> lds(rdLdsBytes(capacity) / 4);
    for (int s = 0; s < nSubjects; s++) rdKeyFrame(0, s, a, p, (uint8_t*)lds.data());
}

// seconds per call, the best of `repeats`, on one thread (tools/covisibility_rate.py)
double cv_time(int repeats, int mode, int nPoints, const int* obsOff, const int* obs, const uint8_t* mpFlags, int nFrames, const uint8_t* kfFlags,
               const int* kfMap, const uint64_t* kfKey, int nSubjects, const int* subjectMp, const int* subjectN, int capacity, const int* subjectKf,
               const int* subjectMap, int th, int connCapacity, int* counterKf, int* counterW, int* orderedKf, int* orderedW, void* result) {
    double best = 1e30;
    for (int r = 0; r < repeats; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        cv_host(mode, nPoints, obsOff, obs, mpFlags, nFrames, kfFlags, kfMap, kfKey, nSubjects, subjectMp, subjectN, capacity, subjectKf, subjectMap, th,
                connCapacity, counterKf, counterW, orderedKf, orderedW, result);
        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        best = dt < best ? dt : best;
    }
    return best;
}
double rd_time(int repeats, int nPoints, const int* obsOff, const int* obs, const uint8_t* mpFlags, const int* mpNobs, int nFrames, const uint8_t* kfFlags,
               const void* kpsUn, const int* nOut, int nSubjects, const int* subjectMp, const int* subjectN, int capacity, const int* subjectKf,
               void* result) {
    double best = 1e30;
    for (int r = 0; r < repeats; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        rd_host(nPoints, obsOff, obs, mpFlags, mpNobs, nFrames, kfFlags, kpsUn, nOut, nullptr, nullptr, nSubjects, subjectMp, subjectN, capacity, subjectKf, 1,
                3, 0.9f, result, nullptr);
        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        best = dt < best ? dt : best;
    }
    return best;
}

}  // extern "C"

#ifdef COVISIBILITY_HOST_MAIN
int main() {
    std::mt19937 rng(34);
    auto U = [&](int a, int b) { return std::uniform_int_distribution<int>(a, b)(rng); };
    long rows = 0, answered = 0, refused = 0;
    for (int trial = 0; trial < 10; trial++) {
        // trial: 0 plain, 1 MapPoint indices outside [-1, n_points), 2 frames outside [0, n_frames), 3 CSR offsets that decrease or leave the table,
        // 4 subject counts negative and past the capacity, 5 subject frames outside the table, 6 empty everything (no MapPoint, no observation,
        // no slot), 7 keypoint rows outside [0, N_f), N_f negative / past the capacity, conn_capacity 1, 8 one frame and conn_capacity 0, 9 duplicate keys
        const int nPoints = trial == 6 ? 0 : 90, nFrames = trial == 8 ? 1 : 37, nSub = 5, cap = 41, cc = trial == 8 ? 0 : trial == 7 ? 1 : trial == 0 ? 3 : 37;
        std::vector<int> obsOff(nPoints + 1, 0);
        for (int m = 0; m < nPoints; m++) obsOff[m + 1] = obsOff[m] + U(0, 9);
        const int nObs = obsOff[nPoints];
        std::vector<int> obs((size_t)2 * nObs), mpNobs(nPoints), kfMap(nFrames), nOut(nFrames), subjectMp((size_t)nSub * cap), subjectN(nSub), subjectKf(nSub),
            subjectMap(nSub);
        std::vector<uint8_t> mpFlags(nPoints), kfFlags(nFrames);
        std::vector<uint64_t> key(nFrames);
        std::vector<Keypoint> kps((size_t)nFrames * cap);
        std::vector<float> depth((size_t)nFrames * cap), thDepth(nFrames);
        for (int o = 0; o < nObs; o++) {
            obs[2 * o] = trial == 2 && o % 5 == 0 ? (o % 2 ? nFrames + U(0, 3) : -1 - U(0, 3)) : U(0, nFrames - 1);
            obs[2 * o + 1] = trial == 7 && o % 4 == 0 ? (o % 8 ? cap + U(0, 5) : -1 - U(0, 5)) : U(0, cap - 1);
        }
        if (trial == 3)
            for (int m = 1; m < nPoints; m += 7) obsOff[m] = m % 2 ? obsOff[m + 1] + 3 : m % 3 ? -4 : nObs + 11;
        for (int m = 0; m < nPoints; m++) { mpFlags[m] = U(0, 9) == 0; mpNobs[m] = U(0, 12); }
        for (int f = 0; f < nFrames; f++) {
            kfFlags[f] = (U(0, 9) == 0) | (f == 3 ? 2 : 0); kfMap[f] = f % 11 == 5; key[f] = trial == 9 ? (uint64_t)(f % 30) : 0xffffffff00000000ull - 7919ull * f;
            nOut[f] = trial == 7 ? (f % 3 == 0 ? -2 : f % 3 == 1 ? cap + 9 : cap) : cap;
            thDepth[f] = 3.f;
            for (int i = 0; i < cap; i++) { kps[(size_t)f * cap + i] = Keypoint{0, 0, 0, 0, 0, U(0, 7), -1}; depth[(size_t)f * cap + i] = (float)U(-1, 5); }
        }
        for (int s = 0; s < nSub; s++) {
            subjectN[s] = trial == 4 ? (s % 2 ? -3 : cap + 1000) : trial == 6 ? 0 : U(0, cap);
            subjectKf[s] = trial == 5 ? (s % 2 ? nFrames + s : -2 - s) : U(0, nFrames - 1);
            subjectMap[s] = s == 4;
            for (int i = 0; i < cap; i++)
                subjectMp[(size_t)s * cap + i] = nPoints == 0 ? -1 : trial == 1 && i % 6 == 0 ? (i % 12 ? nPoints + U(0, 4) : -2 - U(0, 4)) : U(-1, nPoints - 1);
        }
        for (int mode = 0; mode < 2; mode++) {
            std::vector<int> cKf((size_t)nSub * cc, -77), cW((size_t)nSub * cc, -77), oKf((size_t)nSub * cc, -77), oW((size_t)nSub * cc, -77);
            std::vector<CovisResult> res(nSub);
            cv_host(mode, nPoints, obsOff.data(), obs.data(), mpFlags.data(), nFrames, kfFlags.data(), kfMap.data(), key.data(), nSub, subjectMp.data(),
                    subjectN.data(), cap, subjectKf.data(), subjectMap.data(), 3, cc, cKf.data(), cW.data(), oKf.data(), oW.data(), res.data());
            for (int s = 0; s < nSub; s++) {
                const CovisResult& r = res[s];
                if (r.status < 0 || r.status >= kCvStatuses) { std::printf("FAILED: status %d\n", r.status); return 1; }
                const bool lists = r.status == kCvOk || r.status == kCvTruncated;
                if (!lists && (r.nCounter || r.nOrdered || r.nmax || r.kfMax != -1)) { std::printf("FAILED: a refused row holds counts\n"); return 1; }
                if (r.nCounter > nFrames || r.nOrdered > nFrames) { std::printf("FAILED: the counts\n"); return 1; }
                for (int i = 0; i < cc; i++) {
                    const int v = cKf[(size_t)s * cc + i], w = oKf[(size_t)s * cc + i];
                    if (i < r.nCounter ? (v < 0 || v >= nFrames) : v != -77) { std::printf("FAILED: counter entry %d of subject %d is %d\n", i, s, v); return 1; }
                    if (i < r.nOrdered ? (w < 0 || w >= nFrames) : w != -77) { std::printf("FAILED: ordered entry %d of subject %d is %d\n", i, s, w); return 1; }
                }
                if (trial == 9 && r.status != kCvDuplicateKey) { std::printf("FAILED: duplicate keys went unnoticed\n"); return 1; }
                if (trial >= 1 && trial <= 3 && r.status == kCvBadIndex) refused++;
                if (lists || r.status == kCvEmpty) answered++;
                rows++;
            }
            std::printf("trial %d vote mode %d: status %d %d %d %d %d, counter %d %d %d %d %d, ordered %d %d %d %d %d\n", trial, mode, res[0].status, res[1].status,
                        res[2].status, res[3].status, res[4].status, res[0].nCounter, res[1].nCounter, res[2].nCounter, res[3].nCounter, res[4].nCounter,
                        res[0].nOrdered, res[1].nOrdered, res[2].nOrdered, res[3].nOrdered, res[4].nOrdered);
        }
        for (int mono = 0; mono < 2; mono++) {
            std::vector<uint8_t> state((size_t)nSub * cap, 0x77);
            std::vector<RedundancyResult> res(nSub);
            rd_host(nPoints, obsOff.data(), obs.data(), mpFlags.data(), trial % 2 ? mpNobs.data() : nullptr, nFrames, kfFlags.data(), kps.data(), nOut.data(),
                    depth.data(), thDepth.data(), nSub, subjectMp.data(), subjectN.data(), cap, subjectKf.data(), mono, 3, mono ? 0.9f : 0.5f, res.data(),
                    trial % 3 ? state.data() : nullptr);
            for (int s = 0; s < nSub; s++) {
                const RedundancyResult& r = res[s];
                if (r.status < 0 || r.status >= kRdStatuses) { std::printf("FAILED: status %d\n", r.status); return 1; }
                if (r.nRedundant > r.nMps || r.nMps > cap || (r.status != kRdOk && (r.nMps || r.redundant))) { std::printf("FAILED: the redundancy counts\n"); return 1; }
                const int N = cvClamp(subjectN[s], cap);
                int counted = 0, red = 0;
                for (int i = 0; i < cap; i++) {
                    const int v = state[(size_t)s * cap + i];
                    if (trial % 3 && r.status == kRdOk && i < N ? v > 2 : v != 0x77) { std::printf("FAILED: slot state %d of subject %d is %d\n", i, s, v); return 1; }
                    counted += v == 1 || v == 2; red += v == 2;
                }
                if (trial % 3 && r.status == kRdOk && (counted != r.nMps || red != r.nRedundant)) { std::printf("FAILED: the states do not add up\n"); return 1; }
                if ((trial == 5) != (r.status == kRdBadIndex) && trial != 1 && trial != 2 && trial != 3 && trial != 7) { std::printf("FAILED: subject frame check\n"); return 1; }
                if (r.status == kRdBadIndex) refused++;
                if (r.status == kRdOk) answered++;
                rows++;
            }
            std::printf("trial %d redundancy mono %d: status %d %d %d %d %d, n_mps %d %d %d %d %d\n", trial, mono, res[0].status, res[1].status, res[2].status,
                        res[3].status, res[4].status, res[0].nMps, res[1].nMps, res[2].nMps, res[3].nMps, res[4].nMps);
        }
    }
    {   // the entries' rejections: one bad argument each on a call that is otherwise accepted
        int dummy = 0, wrong = 0;
        const void* good[15];
        for (int k = 0; k < 15; k++) good[k] = &dummy;
        struct Call { int mode, nPoints, nFrames, nSubjects, capacity, connCapacity; };
        const Call ok{0, 90, 37, 5, 41, 37};
        auto bad = [&](const void* const* q, Call c) { return cv_bad_argument(q, c.mode, c.nPoints, c.nFrames, c.nSubjects, c.capacity, c.connCapacity); };
        wrong += bad(good, ok) != 0;
        for (int k = 0; k < 15; k++) {
            const void* q[15];
            for (int j = 0; j < 15; j++) q[j] = j == k ? nullptr : good[j];
            Call c = ok;
            wrong += bad(q, c) != 1;                             // UPDATE_CONNECTIONS needs every pointer
            c.mode = 1;                                          // LOCAL_KEYFRAMES: no map ids, no subject frames, no ordered block
            wrong += bad(q, c) != (k == 4 || k == 8 || k == 9 || k == 12 || k == 13 ? 0 : 1);
            c = ok; c.connCapacity = 0;                          // no list blocks at all
            wrong += bad(q, c) != (k >= 10 && k <= 13 ? 0 : 1);
        }
        const Call bads[] = {{2, 90, 37, 5, 41, 37}, {-1, 90, 37, 5, 41, 37}, {0, -1, 37, 5, 41, 37}, {0, 90, 0, 5, 41, 37}, {0, 90, 37, 0, 41, 37},
                             {0, 90, 37, 65536, 41, 37}, {0, 90, 37, 5, 0, 37}, {0, 90, 37, 5, 41, -1}, {0, 90, 37, 65535, 32769, 37}, {0, 90, 37, 65535, 41, 32769}};
        for (const Call& b : bads) wrong += bad(good, b) != 1;
        wrong += bad(good, Call{1, 0, 8192, 65535, 32767, 32767}) != 0;      // the largest call
        wrong += cv_unsupported(kCvMaxFrames) != 0;
        wrong += cv_unsupported(kCvMaxFrames + 1) != 1;
        wrong += cv_unsupported(0x7fffffff) != 1;
        struct RCall { int nPoints, nFrames, nSubjects, capacity, monocular; float th; };
        const RCall rok{90, 37, 5, 41, 0, 0.9f};
        auto rbad = [&](const void* const* q, RCall c) { return rd_bad_argument(q, c.nPoints, c.nFrames, c.nSubjects, c.capacity, c.monocular, c.th); };
        wrong += rbad(good, rok) != 0;
        for (int k = 0; k < 12; k++) {
            const void* q[12];
            for (int j = 0; j < 12; j++) q[j] = j == k ? nullptr : good[j];
            RCall c = rok;
            wrong += rbad(q, c) != 1;
            c.monocular = 1;                                     // no depth arrays
            wrong += rbad(q, c) != (k == 6 || k == 7 ? 0 : 1);
        }
        const RCall rbads[] = {{-1, 37, 5, 41, 0, 0.9f}, {90, 0, 5, 41, 0, 0.9f}, {90, 37, 0, 41, 0, 0.9f}, {90, 37, 65536, 41, 0, 0.9f}, {90, 37, 5, 0, 0, 0.9f},
                               {90, 37, 5, 41, 0, NAN}, {90, 37, 65535, 32769, 0, 0.9f}};
        for (const RCall& b : rbads) wrong += rbad(good, b) != 1;
        wrong += rd_unsupported(kRdMaxCapacity) != 0;
        wrong += rd_unsupported(kRdMaxCapacity + 1) != 1;
        wrong += rd_unsupported(0x7fffffff) != 1;
        if (wrong) { std::printf("FAILED: %d of the entries' rejections\n", wrong); return 1; }
    }
    if (answered == 0 || refused == 0) { std::printf("FAILED: nothing was answered, or nothing refused, at all\n"); return 1; }
    std::printf("covisibility_host_check: every access inside its arrays, %ld rows, %ld answered, %ld refused for an index\n", rows, answered, refused);
    return 0;
}
#endif
