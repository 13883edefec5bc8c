// k_place_recognition.hpp - KeyFrameDatabase::DetectNBestCandidates (reference src/KeyFrameDatabase.cc:612-780, loop closing) and
// KeyFrameDatabase::DetectRelocalizationCandidates (:783-895, relocalisation) for a batch of independent queries against one database of
// keyframe BoW vectors.  k_place_recognition.hip holds the two kernels around prPair and prQuery; everything they compute is stated here, and
// tests/place_recognition_walk.py states it a second time with the reference's own structures (an inverted file, lists, a set).
//   pairs        the reference walks an inverted file; the device scores PAIRS: one wave per (query, database row) searches the row's word
//                ids in the query's ids (staged once per workgroup in LDS), compacts the hits in ascending order by ballot - the count, the
//                SMALLEST shared word id, the terms - and adds the terms by a sequential chain;
//   list order   lKFsSharingWords is in order of first encounter: the query's words ascending, each word's inverted list in `add` order, which
//                is the row order.  A row is first met at its smallest shared word, so the list is the rows in order of (smallest shared word
//                id, row); lScoreAndMatch and lAccScoreAndMatch keep it.  RELOCALIZATION never sorts: it IS the output order.  N_BEST's
//                list::sort(compFirst) is stable on a.first > b.first: descending accumulated score, ties in list order;
//   connected    (N_BEST, :635-645) a row of pKF->GetConnectedKeyFrames() never enters the list and never takes the query's id: it does not
//                count towards maxCommonWords, is never scored, and as a covisibility neighbour it is skipped (:704).  RELOCALIZATION has
//                no such test;
//   threshold    int minCommonWords = maxCommonWords*0.8f is a FLOAT product truncated to int; a row is scored when words > minCommonWords;
//   score        L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68): from a double 0, for every common word in ascending id,
//                score += (fabs(vi - wi) - fabs(vi)) - fabs(wi) with vi the query's weight - three roundings, one sequential sum, no tree -
//                then (float)(-score / 2.0);
//   stale score  mPlaceRecognitionScore / mRelocScore is written only for the rows that pass the threshold (:681, :834) and read for every
//                neighbour that carries the query's id (:707-711, :860-864) - rows that share a word but did not pass included.  For them
//                the reference reads what an earlier query left, so d_score is STATE, one row per query: read, overwritten only where a
//                row is scored, the rest left byte for byte.  Assumed: no row carries the query's id before the call;
//   neighbours   accScore is a float sum in neighbour order; pBestKF is the first neighbour with a strictly greater score; bestAccScore
//                starts at 0 and takes every strictly greater accScore (a NaN never);
//   selection    RELOCALIZATION keeps accScore > 0.75f*bestAccScore (a float product), skips another map's keyframe BEFORE the duplicate set,
//                then drops duplicates of pBestKF.  N_BEST walks the sorted list while either output is short: a keyframe not yet in the set
//                is a loop candidate (same map, list short) or else a merge candidate (other map, list short, map not bad), and enters the
//                set either way; `if(pKFi->isBad()) continue;` (:735-736) advances nothing - the reference never returns once a bad keyframe
//                reaches the front of the walk.  The device stops there, writes what was collected and names the exit;
//   early exits  n_db == 0, a query without words, no sharing keyframe (:655, :808), none scored (:686, :839; unreachable: the row that
//                holds maxCommonWords passes its own threshold, kept as a name).
// The host build (ORBX_HOST_ROW, tests/cpp/host_shim) runs the same functions with a wave and a workgroup of ONE lane: ballots are the lane's
// own bit, barriers are nothing, atomics are plain.
#pragma once
#include "orbx_device.hpp"
#include "orbx_params.hpp"

namespace orbx {

// == orbx_place_mode / orbx_place_status
enum { kPrNBest = 0, kPrRelocalization = 1 };
enum { kPrOk = 0, kPrNoSharing, kPrNoneScored, kPrEmptyDatabase, kPrEmptyQuery, kPrBadKeyFrame, kPrTruncated, kPrStatuses };
constexpr int kPrCovis = 10;                              // GetBestCovisibilityKeyFrames(10)
#ifdef ORBX_HOST_ROW
constexpr int kPrLanes = 1, kPrThreads = 1;
#else
constexpr int kPrLanes = 64, kPrThreads = 256;
#endif

// == orbx_place_result
struct PlaceResult { int status, nSharing, maxCommonWords, minCommonWords, nScored; float bestAccScore; int nLoop, nMerge; };
static_assert(sizeof(PlaceResult) == 32, "orbx_place_result layout");

// ---- the vocabulary of a lane ------------------------------------------------------------------------------------------------------------
#ifdef ORBX_HOST_ROW
static inline void prSync() {}
static inline unsigned long long prBallot(bool c) { return c ? 1ull : 0ull; }
static inline uint32_t prLaneU32(uint32_t v, int) { return v; }
static inline double prLaneF64(double v, int) { return v; }
static inline void prAtomicAdd(int* p, int v) { *p += v; }
static inline int prAtomicInc(int* p) { return (*p)++; }
static inline void prAtomicMax(int* p, int v) { if (v > *p) *p = v; }
static inline void prAtomicMin(int* p, int v) { if (v < *p) *p = v; }
static inline uint32_t prFloatBits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static inline float prBitsFloat(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
#else
__device__ __forceinline__ void prSync() { __threadfence_block(); __syncthreads(); }
__device__ __forceinline__ unsigned long long prBallot(bool c) { return __ballot(c); }
// a cross-lane read from a lane every lane names alike (the first set bit of a ballot): v_readlane, no trip through the LDS crossbar
__device__ __forceinline__ uint32_t prLaneU32(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, __builtin_amdgcn_readfirstlane(lane)); }
__device__ __forceinline__ double prLaneF64(double v, int lane) {
    const int l = __builtin_amdgcn_readfirstlane(lane);
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}
__device__ __forceinline__ void prAtomicAdd(int* p, int v) { atomicAdd(p, v); }
__device__ __forceinline__ int prAtomicInc(int* p) { return atomicAdd(p, 1); }
__device__ __forceinline__ void prAtomicMax(int* p, int v) { atomicMax(p, v); }
__device__ __forceinline__ void prAtomicMin(int* p, int v) { atomicMin(p, v); }
__device__ __forceinline__ uint32_t prFloatBits(float f) { return __float_as_uint(f); }
__device__ __forceinline__ float prBitsFloat(uint32_t u) { return __uint_as_float(u); }
#endif

__device__ __forceinline__ int prClampWords(int n, int capacity) { return n < 0 ? 0 : n > capacity ? capacity : n; }
// ascending in the float's order; -0 and +0 are one key, as they compare
__device__ __forceinline__ uint32_t prOrderable(float f) {
    const uint32_t u = prFloatBits(f + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// ---- one (query, database row) pair by one wave: mnPlaceRecognitionWords, the smallest shared word id, L1Scoring::score -----------------
// qIds / qW: the query's nq words (ascending ids); rIds / rW: the row's nr words.  Every lane returns the same three values.
__device__ __forceinline__ void prPair(int lane, const uint32_t* qIds, const double* qW, int nq, const uint32_t* rIds, const double* rW, int nr,
                                       int& words, uint32_t& first, float& score) {
    words = 0; first = 0xffffffffu;
    double sum = 0.0;
    for (int base = 0; base < nr; base += kPrLanes) {
        const int j = base + lane;
        bool hit = false;
        double term = 0.0;
        uint32_t id = 0;
        if (j < nr) {
            id = rIds[j];
            int lo = 0, hi = nq;                                  // lower_bound
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (qIds[mid] < id) lo = mid + 1; else hi = mid;
            }
            if (lo < nq && qIds[lo] == id) {
                const double vi = qW[lo], wi = rW[j];
                hit = true;
                term = (fabs(vi - wi) - fabs(vi)) - fabs(wi);
            }
        }
        unsigned long long m = prBallot(hit);
        if (m && words == 0) first = prLaneU32(id, __builtin_ctzll(m));
        words += __builtin_popcountll(m);
        while (m) {                                               // the sequential sum, in ascending word id
            sum = sum + prLaneF64(term, __builtin_ctzll(m));
            m &= m - 1;
        }
    }
    score = (float)(-sum / 2.0);
}

// ---- a workgroup's ordered count: the flagged threads before this one, and all of them ----------------------------------------------------
__device__ __forceinline__ int prExclusive(bool flag, int tid, int* waveTotals, int& total) {
#ifdef ORBX_HOST_ROW
    (void)tid; (void)waveTotals;
    total = flag ? 1 : 0;
    return 0;
#else
    const unsigned long long m = __ballot(flag);
    const int lane = tid & 63, w = tid >> 6;
    const int within = __popcll(m & ((1ull << lane) - 1ull));
    __syncthreads();                                              // the totals of the previous use have been read
    if (lane == 0) waveTotals[w] = __popcll(m);
    __syncthreads();
    int before = 0;
    total = 0;
    for (int x = 0; x < kPrThreads / 64; x++) {
        const int t = waveTotals[x];
        if (x < w) before += t;
        total += t;
    }
    return before + within;
#endif
}

// ascending bitonic sort of P2 (a power of two) keys
__device__ __forceinline__ void prSort(unsigned long long* keys, int P2, int tid) {
    for (int k = 2; k <= P2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P2; i += kPrThreads) {
                const int l = i ^ j;
                if (l > i) {
                    const unsigned long long a = keys[i], b = keys[l];
                    if ((a > b) == ((i & k) == 0)) { keys[i] = b; keys[l] = a; }
                }
            }
            prSync();
        }
}

// ---- one query by one workgroup: everything behind the pairs -------------------------------------------------------------------------------
// lds: prQueryLdsBytes(p.nDb) bytes.  a.wsWords / a.wsFirst / a.wsScore hold the pairs of all queries.
__device__ __forceinline__ void prQuery(int tid, int q, const PlaceArrays& a, const PlaceParams& p, uint8_t* lds) {
    const int nDb = p.nDb, P = prPow2(nDb);
    unsigned long long* keys = (unsigned long long*)lds;
    int* best = (int*)(lds + (size_t)8 * P);
    int* owner = best + P;
    int* scr = owner + nDb;      // 0 nSharing, 1 maxWords, 2 nScored, 3 bestAcc bits, 4 first bad, 5 loop full at, 6 merge full at, 7 nLoop, 8 nMerge; 9 .. 12 and 13 .. 16 the wave totals of two ordered counts
    PlaceResult* res = (PlaceResult*)a.result + q;
    const size_t row = (size_t)q * (size_t)nDb;
    const bool nBest = p.mode == kPrNBest;
    const uint8_t* conn = nBest && a.connected ? a.connected + row : nullptr;
    float* score = a.score + row;
    PlaceResult r{};
    if (nDb == 0) {
        r.status = kPrEmptyDatabase;
        if (tid == 0) *res = r;
        return;
    }
    const int nq = prClampWords(a.qN[p.qFirst + (long long)q * p.qStep], p.qCapacity);
    const int qMap = a.qMap[q];
    if (tid == 0) {
        for (int k = 0; k < kPrScratchInts; k++) scr[k] = 0;
        scr[4] = scr[5] = scr[6] = 0x7fffffff;
    }
    prSync();
    {   // lKFsSharingWords: its size and maxCommonWords
        int n = 0, mx = 0;
        for (int k = tid; k < nDb; k += kPrThreads) {
            owner[k] = 0x7fffffff;
            const int w = a.wsWords[row + k];
            if (w > 0 && !(conn && conn[k])) { n++; mx = w > mx ? w : mx; }
        }
        prAtomicAdd(scr + 0, n);
        prAtomicMax(scr + 1, mx);
    }
    prSync();
    r.nSharing = scr[0]; r.maxCommonWords = scr[1];
    if (r.nSharing == 0) {
        r.status = nq == 0 ? kPrEmptyQuery : kPrNoSharing;
        if (tid == 0) *res = r;
        return;
    }
    r.minCommonWords = (int)((float)r.maxCommonWords * 0.8f);
    // lScoreAndMatch: the rows that pass, their score written back, keyed by (smallest shared word, row)
    for (int k = tid; k < nDb; k += kPrThreads) {
        const int w = a.wsWords[row + k];
        if (w > 0 && !(conn && conn[k]) && w > r.minCommonWords) {
            score[k] = a.wsScore[row + k];
            keys[prAtomicInc(scr + 2)] = ((unsigned long long)a.wsFirst[row + k] << 32) | (unsigned)k;
        }
    }
    prSync();
    const int n = r.nScored = scr[2];
    if (n == 0) {
        r.status = kPrNoneScored;
        if (tid == 0) *res = r;
        return;
    }
    const int P2 = prPow2(n);
    for (int i = n + tid; i < P2; i += kPrThreads) keys[i] = ~0ull;
    prSync();
    prSort(keys, P2, tid);
    // lAccScoreAndMatch: the covisibility neighbours that carry the query's id add their score, stale or fresh
    for (int i = tid; i < n; i += kPrThreads) {
        const int k = (int)(unsigned)keys[i];
        float bestScore = score[k], acc = bestScore;
        int bestK = k;
        for (int j = 0; j < kPrCovis; j++) {
            const int nb = a.dbCovis[(size_t)k * kPrCovis + j];
            if (nb < 0 || nb >= nDb) continue;
            if (!(a.wsWords[row + nb] > 0) || (conn && conn[nb])) continue;      // mnPlaceRecognitionQuery != pKF->mnId
            const float s2 = score[nb];
            acc = acc + s2;
            if (s2 > bestScore) { bestK = nb; bestScore = s2; }
        }
        best[i] = bestK;
        if (acc > 0.f) prAtomicMax(scr + 3, (int)prFloatBits(acc));      // positive floats order as their bits
        keys[i] = ((unsigned long long)(nBest ? ~prOrderable(acc) : prFloatBits(acc)) << 32) | (unsigned)i;
    }
    prSync();
    r.bestAccScore = prBitsFloat((uint32_t)scr[3]);
    if (!nBest) {
        const float minScoreToRetain = 0.75f * r.bestAccScore;
        auto kept = [&](int i) { return prBitsFloat((uint32_t)(keys[i] >> 32)) > minScoreToRetain && a.dbMap[best[i]] == qMap; };
        for (int i = tid; i < n; i += kPrThreads)
            if (kept(i)) prAtomicMin(owner + best[i], i);
        prSync();
        int base = 0;
        for (int i0 = 0; i0 < n; i0 += kPrThreads) {
            const int i = i0 + tid;
            const bool out = i < n && kept(i) && owner[best[i]] == i;
            int total;
            const int pos = base + prExclusive(out, tid, scr + 9, total);
            if (out && pos < p.candCapacity) a.cand[(size_t)q * p.candCapacity + pos] = best[i];
            base += total;
        }
        r.nLoop = base;
        r.status = base > p.candCapacity ? kPrTruncated : kPrOk;
        if (tid == 0) *res = r;
        return;
    }
    for (int i = n + tid; i < P2; i += kPrThreads) keys[i] = ~0ull;
    prSync();
    prSort(keys, P2, tid);
    // the walk over the sorted list: first occurrences of pBestKF, the first bad keyframe
    for (int s = tid; s < n; s += kPrThreads) {
        const int b = best[(int)(unsigned)keys[s]];
        prAtomicMin(owner + b, s);
        if (a.dbFlags[b] & 1) prAtomicMin(scr + 4, s);
    }
    prSync();
    int lBase = 0, mBase = 0;
    for (int s0 = 0; s0 < n; s0 += kPrThreads) {
        const int s = s0 + tid;
        int b = 0;
        bool lf = false, mf = false;
        if (s < n) {
            b = best[(int)(unsigned)keys[s]];
            const bool fresh = owner[b] == s, same = a.dbMap[b] == qMap;
            lf = fresh && same;
            mf = fresh && !same && !(a.dbFlags[b] & 2);
        }
        int lTotal, mTotal;
        const int lPos = lBase + prExclusive(lf, tid, scr + 9, lTotal), mPos = mBase + prExclusive(mf, tid, scr + 13, mTotal);
        lBase += lTotal; mBase += mTotal;
        int kind = 0, pos = 0;
        if (lf && lPos < p.nCandidates) { kind = 1; pos = lPos; if (lPos == p.nCandidates - 1) scr[5] = s; }
        if (mf && mPos < p.nCandidates) { kind = 2; pos = mPos; if (mPos == p.nCandidates - 1) scr[6] = s; }
        if (s < n) keys[s] = ((unsigned long long)kind << 62) | ((unsigned long long)(unsigned)pos << 32) | (unsigned)b;
    }
    prSync();
    // the walk ends behind the entry that fills the second list, or at the end of the list; a bad keyframe in front of that end stops it
    const int firstBad = scr[4];
    const int end = p.nCandidates == 0 ? 0 : (scr[5] != 0x7fffffff && scr[6] != 0x7fffffff) ? (scr[5] > scr[6] ? scr[5] : scr[6]) + 1 : n;
    for (int s = tid; s < n && s < firstBad; s += kPrThreads) {
        const unsigned long long c = keys[s];
        const int kind = (int)(c >> 62), pos = (int)((c >> 32) & 0x3fffffffu);
        if (kind == 1) { a.loop[(size_t)q * p.nCandidates + pos] = (int)(unsigned)c; prAtomicAdd(scr + 7, 1); }
        if (kind == 2) { a.merge[(size_t)q * p.nCandidates + pos] = (int)(unsigned)c; prAtomicAdd(scr + 8, 1); }
    }
    prSync();
    r.nLoop = scr[7]; r.nMerge = scr[8];
    r.status = firstBad < end ? kPrBadKeyFrame : kPrOk;
    if (tid == 0) *res = r;
}

}  // namespace orbx
