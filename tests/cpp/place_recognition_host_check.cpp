// place_recognition_host_check.cpp - extractorb_amd/csrc/k_place_recognition.hpp, the statement of k_place_recognition.hip, compiled for the
// HOST (tests/cpp/host_shim stands in for the device vocabulary): prPair runs pair by pair and prQuery query by query, a wave and a workgroup
// being one lane, on arrays of exactly the entry's sizes - the workspace and the "LDS" block of a query included.  Two uses, both without a
// GPU:
//   * as a shared library (tests/test_place_recognition.py): pr_host() over the scenes of the GPU tests, compared with the walk byte for
//     byte; pr_fits() for the entry's launch-time bounds; pr_time() for tools/place_recognition_rate.py;
//   * as a stand-alone program (-DPLACE_RECOGNITION_HOST_MAIN) under -fsanitize=address,undefined on exact-size heap blocks: neighbour indices
//     outside [-1, n_db), n_words past the capacity and negative, unsorted and repeated word ids, NaN weights, n_candidates 0, n_db 0, a
//     cand_capacity of 0; and the entry's rejections (orbx_entry.hpp: placeBadArgument, placeUnsupported), one bad argument each.
#include "host_shim/place_recognition_shim.h"

#include <chrono>
#include <cstdio>
#include <random>
#include <vector>

#include "../../extractorb_amd/csrc/k_place_recognition.hpp"
#include "../../extractorb_amd/csrc/orbx_entry.hpp"

using namespace orbx;

extern "C" {

int pr_result_bytes() { return (int)sizeof(PlaceResult); }
int pr_statuses() { return kPrStatuses; }
int pr_max_db() { return kPrMaxDb; }
int pr_max_query_words() { return kPrMaxQueryWords; }
int pr_fits(int nDb, int qCapacity) { return placeFits(nDb, qCapacity) ? 1 : 0; }
// the entry's two refusals as orbx_entry.hpp states them: ptrs = v, the six database arrays, the four query arrays, d_score, d_result,
// d_loop, d_merge, d_cand in the entry's order (16 pointers)
int pr_bad_argument(const void* const* ptrs, int mode, int nDb, int capacity, int nQueries, int qFirst, int qStep, int qCapacity, int nCandidates,
                    int candCapacity) {
    return placeBadArgument(ptrs[0], mode, nDb, ptrs[1], ptrs[2], ptrs[3], capacity, ptrs[4], ptrs[5], ptrs[6], nQueries, qFirst, qStep, ptrs[7], ptrs[8],
                            ptrs[9], qCapacity, ptrs[10], nCandidates, ptrs[11], ptrs[12], ptrs[13], ptrs[14], ptrs[15], candCapacity) ? 1 : 0;
}
int pr_unsupported(int scoring, int nDb, int qCapacity) { return placeUnsupported(scoring, nDb, qCapacity) ? 1 : 0; }
long pr_pair_lds_bytes(int qCapacity) { return (long)prPairLdsBytes(qCapacity); }
long pr_query_lds_bytes(int nDb) { return (long)prQueryLdsBytes(nDb); }

// the arguments of orbx_detect_candidates_device on host arrays (without the handle and the vocabulary)
void pr_host(int mode, int nDb, const uint32_t* dbIds, const double* dbW, const int* dbN, int capacity, const int* dbMap, const uint8_t* dbFlags,
             const int* dbCovis, int nQueries, int qFirst, int qStep, const uint32_t* qIds, const double* qW, const int* qN, int qCapacity,
             const int* qMap, const uint8_t* connected, int nCandidates, float* score, void* result, int* loop, int* merge, int* cand,
             int candCapacity, int* commonWords) {
    const bool nBest = mode == kPrNBest;
    const PlaceParams p{mode, nDb, capacity, nQueries, qFirst, qStep, qCapacity, nBest ? nCandidates : 0, nBest ? 0 : candCapacity, prPairRows(nDb, nQueries)};
    const size_t pairs = (size_t)nQueries * (size_t)nDb;
    // exact-size heap blocks: an access one element past any of them is reported
    std::vector<int> wsWords(pairs);
    std::vector<uint32_t> wsFirst(pairs);
    std::vector<float> wsScore(pairs);
    const PlaceArrays a{dbIds, dbW, dbN, dbMap, dbFlags, dbCovis, qIds, qW, qN, qMap, nBest ? connected : nullptr, score, result, loop, merge, cand,
                        commonWords, wsWords.data(), wsFirst.data(), wsScore.data()};
    for (int q = 0; q < nQueries; q++) {
        const long long frame = qFirst + (long long)q * qStep;
        const int nq = prClampWords(qN[frame], qCapacity);
        // the staged query, as k_place_pairs lays it out
        std::vector<uint64_t> stage((prPairLdsBytes(qCapacity) + 7) / 8);
        double* sW = (double*)stage.data();
        uint32_t* sIds = (uint32_t*)((uint8_t*)stage.data() + (size_t)8 * qCapacity);
        for (int i = 0; i < nq; i++) { sW[i] = qW[frame * qCapacity + i]; sIds[i] = qIds[frame * qCapacity + i]; }
        for (int k = 0; k < nDb; k++) {
            int words; uint32_t first; float sc;
            prPair(0, sIds, sW, nq, dbIds + (size_t)k * capacity, dbW + (size_t)k * capacity, prClampWords(dbN[k], capacity), words, first, sc);
            const size_t at = (size_t)q * nDb + k;
            wsWords[at] = words; wsFirst[at] = first; wsScore[at] = sc;
            if (commonWords) commonWords[at] = words;
        }
        std::vector<uint64_t> lds((prQueryLdsBytes(nDb) + 7) / 8);
        prQuery(0, q, a, p, (uint8_t*)lds.data());
    }
}

// seconds per call of pr_host, the best of `repeats`, on one thread (tools/place_recognition_rate.py)
double pr_time(int repeats, int mode, int nDb, const uint32_t* dbIds, const double* dbW, const int* dbN, int capacity, const int* dbMap,
               const uint8_t* dbFlags, const int* dbCovis, int nQueries, const uint32_t* qIds, const double* qW, const int* qN, int qCapacity,
               const int* qMap, int nCandidates, float* score, void* result, int* loop, int* merge, int* cand, int candCapacity) {
    double best = 1e30;
    for (int r = 0; r < repeats; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        pr_host(mode, nDb, dbIds, dbW, dbN, capacity, dbMap, dbFlags, dbCovis, nQueries, 0, 1, qIds, qW, qN, qCapacity, qMap, nullptr, nCandidates, score,
                result, loop, merge, cand, candCapacity, nullptr);
        const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        best = dt < best ? dt : best;
    }
    return best;
}

}  // extern "C"

#ifdef PLACE_RECOGNITION_HOST_MAIN
int main() {
    std::mt19937 rng(31);
    auto U = [&](int a, int b) { return std::uniform_int_distribution<int>(a, b)(rng); };
    auto F = [&]() { return std::uniform_real_distribution<double>(0.0, 1.0)(rng); };
    long rows = 0, answered = 0;
    for (int trial = 0; trial < 10; trial++) {
        // trial: 0 plain, 1 neighbour indices outside [-1, n_db), 2 n_words past the capacity and negative, 3 unsorted and repeated word ids,
        // 4 NaN weights, 5 n_candidates 0 / cand_capacity 0, 6 n_db 0, 7 every row bad, 8 one row, 9 a database of 300 rows
        for (int mode = 0; mode < 2; mode++) {
            const int nDb = trial == 6 ? 0 : trial == 8 ? 1 : trial == 9 ? 300 : 70, cap = trial == 9 ? 5 : 37, qCap = 41, nQ = 3, qFirst = 4, qStep = -2;
            const int nCand = trial == 5 ? 0 : 3, candCap = trial == 5 ? 0 : 4;
            std::vector<uint32_t> dbIds((size_t)nDb * cap), qIds((size_t)5 * qCap);
            std::vector<double> dbW((size_t)nDb * cap), qW((size_t)5 * qCap);
            std::vector<int> dbN(nDb), dbMap(nDb), covis((size_t)nDb * kPrCovis), qN(5), qMap(nQ), loop((size_t)nQ * nCand, -77), merge((size_t)nQ * nCand, -77),
                cand((size_t)nQ * candCap, -77), common((size_t)nQ * nDb, -77);
            std::vector<uint8_t> flags(nDb), conn((size_t)nQ * nDb);
            std::vector<float> score((size_t)nQ * nDb);
            std::vector<PlaceResult> res(nQ);
            auto fill = [&](uint32_t* ids, double* w, int n, int vocab) {
                uint32_t id = 0;
                for (int j = 0; j < n; j++) {
                    id += 1 + (uint32_t)U(0, vocab);
                    ids[j] = trial == 3 ? (uint32_t)U(0, 8) : id;
                    w[j] = trial == 4 && j % 3 == 0 ? NAN : F();
                }
            };
            for (int k = 0; k < nDb; k++) {
                fill(&dbIds[(size_t)k * cap], &dbW[(size_t)k * cap], cap, 3);
                dbN[k] = trial == 2 ? (k % 3 == 0 ? cap + 1000 : k % 3 == 1 ? -5 : cap) : U(0, cap);
                dbMap[k] = k % 4 == 1; flags[k] = trial == 7 ? 1 : (k % 9 == 4) | ((k % 4 == 1 && k % 8 == 1) ? 2 : 0);
                for (int j = 0; j < kPrCovis; j++)
                    covis[(size_t)k * kPrCovis + j] = trial == 1 ? (j % 3 == 0 ? nDb + U(0, 5) : j % 3 == 1 ? -2 - U(0, 5) : 2000000000) : U(-1, nDb - 1);
                for (int q = 0; q < nQ; q++) { conn[(size_t)q * nDb + k] = U(0, 5) == 0; score[(size_t)q * nDb + k] = (float)F(); }
            }
            for (int f = 0; f < 5; f++) {
                fill(&qIds[(size_t)f * qCap], &qW[(size_t)f * qCap], qCap, 3);
                qN[f] = trial == 2 ? (f == 0 ? -1 : qCap + 7) : U(1, qCap);
            }
            for (int q = 0; q < nQ; q++) qMap[q] = q == 1;
            pr_host(mode, nDb, dbIds.data(), dbW.data(), dbN.data(), cap, dbMap.data(), flags.data(), covis.data(), nQ, qFirst, qStep, qIds.data(), qW.data(),
                    qN.data(), qCap, qMap.data(), conn.data(), nCand, score.data(), res.data(), loop.data(), merge.data(), cand.data(), candCap,
                    trial % 2 ? common.data() : nullptr);
            for (int q = 0; q < nQ; q++) {
                const PlaceResult& r = res[q];
                if (r.status < 0 || r.status >= kPrStatuses) { std::printf("FAILED: status %d\n", r.status); return 1; }
                if (r.nScored > r.nSharing || r.nSharing > nDb) { std::printf("FAILED: the counts\n"); return 1; }
                const int nl = mode == kPrNBest ? nCand : candCap;
                const int* first = mode == kPrNBest ? loop.data() : cand.data();
                for (int i = 0; i < nl; i++) {
                    const int v = first[(size_t)q * nl + i];
                    if (i < r.nLoop ? (v < 0 || v >= nDb) : v != -77) { std::printf("FAILED: candidate %d of query %d is %d\n", i, q, v); return 1; }
                }
                if (mode == kPrNBest)
                    for (int i = 0; i < nCand; i++) {
                        const int v = merge[(size_t)q * nCand + i];
                        if (i < r.nMerge ? (v < 0 || v >= nDb) : v != -77) { std::printf("FAILED: merge candidate %d of query %d is %d\n", i, q, v); return 1; }
                    }
                if (r.status == kPrOk || r.status == kPrTruncated || r.status == kPrBadKeyFrame) answered++;
                rows++;
            }
            std::printf("trial %d mode %d: status %d %d %d, sharing %d %d %d, scored %d %d %d, candidates %d+%d %d+%d %d+%d\n", trial, mode, res[0].status,
                        res[1].status, res[2].status, res[0].nSharing, res[1].nSharing, res[2].nSharing, res[0].nScored, res[1].nScored, res[2].nScored,
                        res[0].nLoop, res[0].nMerge, res[1].nLoop, res[1].nMerge, res[2].nLoop, res[2].nMerge);
        }
    }
    {   // the entry's rejections: one bad argument each on a call that is otherwise accepted
        int dummy = 0;
        const void* good[16];
        for (int k = 0; k < 16; k++) good[k] = &dummy;
        struct Call { int mode, nDb, capacity, nQueries, qFirst, qStep, qCapacity, nCandidates, candCapacity; };
        const Call ok{0, 70, 37, 3, 4, -2, 41, 3, 4};
        auto bad = [&](const void* const* p, Call c) { return pr_bad_argument(p, c.mode, c.nDb, c.capacity, c.nQueries, c.qFirst, c.qStep, c.qCapacity, c.nCandidates, c.candCapacity); };
        int wrong = bad(good, ok) != 0;
        for (int k = 0; k < 16; k++) {                       // every required pointer; d_cand is not read in N_BEST mode, d_loop / d_merge not in the other
            const void* p[16];
            for (int j = 0; j < 16; j++) p[j] = j == k ? nullptr : good[j];
            Call c = ok;
            c.mode = k == 15;
            wrong += bad(p, c) != 1;
            c.nDb = 0;                                       // an empty database has no arrays and no score row
            wrong += bad(p, c) != ((k >= 1 && k <= 6) || k == 11 ? 0 : 1);
        }
        const void* none[16];
        for (int j = 0; j < 16; j++) none[j] = j == 13 || j == 14 || j == 15 ? nullptr : good[j];
        Call c = ok; c.nCandidates = 0; wrong += bad(none, c) != 0;                      // no candidates: no candidate arrays
        c = ok; c.mode = 1; c.candCapacity = 0; wrong += bad(none, c) != 0;
        const Call bads[] = {{2, 70, 37, 3, 4, -2, 41, 3, 4}, {-1, 70, 37, 3, 4, -2, 41, 3, 4}, {0, -1, 37, 3, 4, -2, 41, 3, 4}, {0, 70, 0, 3, 4, -2, 41, 3, 4},
                             {0, 70, 37, 0, 4, -2, 41, 3, 4}, {0, 70, 37, 65536, 0, 1, 41, 3, 4}, {0, 70, 37, 3, -1, 1, 41, 3, 4}, {0, 70, 37, 3, 3, -2, 41, 3, 4},
                             {0, 70, 37, 3, 4, -2, 0, 3, 4}, {0, 70, 37, 3, 4, -2, 41, -1, 4}, {0, 70, 37, 3, 4, -2, 41, 0x40000000, 4}, {1, 70, 37, 3, 4, -2, 41, 3, -1},
                             {0, 70, 37, 65535, 0, 1, 41, 32769, 4}, {1, 70, 37, 65535, 0, 1, 41, 3, 32769}, {0, 8192, 37, 65535, 0, 1, 41, 3, 4} /* the largest call: 65535 * 8192 pairs, accepted */};
        for (const Call& b : bads) wrong += bad(good, b) != (b.nDb == 8192 ? 0 : 1);
        wrong += pr_unsupported(0, kPrMaxDb, kPrMaxQueryWords) != 0;
        wrong += pr_unsupported(1, 70, 41) != 1;
        wrong += pr_unsupported(5, 70, 41) != 1;
        wrong += pr_unsupported(0, kPrMaxDb + 1, 41) != 1;
        wrong += pr_unsupported(0, 70, kPrMaxQueryWords + 1) != 1;
        if (wrong) { std::printf("FAILED: %d of the entry's rejections\n", wrong); return 1; }
    }
    if (pr_fits(kPrMaxDb, kPrMaxQueryWords) != 1 || pr_fits(kPrMaxDb + 1, 1) != 0 || pr_fits(1, kPrMaxQueryWords + 1) != 0) { std::printf("FAILED: the bounds\n"); return 1; }
    if (answered == 0) { std::printf("FAILED: nothing was answered at all\n"); return 1; }
    std::printf("place_recognition_host_check: every access inside its arrays, %ld rows, %ld answered\n", rows, answered);
    return 0;
}
#endif
