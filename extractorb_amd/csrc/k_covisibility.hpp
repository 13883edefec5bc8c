// k_covisibility.hpp - the double walk "a row of MapPoints, each MapPoint's observations" of the reference, in its three places, for
// one-camera keyframes (NLeft == -1) and a batch of independent subjects:
//   KeyFrame::UpdateConnections (src/KeyFrame.cc:388-511)                          cvVote, mode kCvUpdateConnections
//   the voting half of Tracking::UpdateLocalKeyFrames (src/Tracking.cc:3030-3102)  cvVote, mode kCvLocalKeyFrames
//   the test inside LocalMapping::KeyFrameCulling's loop (src/LocalMapping.cc:977-1043)   rdKeyFrame
// k_covisibility.hip holds the three kernels around cvRank, cvVote and rdKeyFrame; everything they compute is stated here, and
// tests/covisibility_walk.py states it a second time with the reference's own structures (a std::map in key order, a vector of pairs).
// All of it is integers but one float product.
//   key order    std::map<KeyFrame*,int> iterates in ADDRESS order and std::sort on pair<int,KeyFrame*> breaks equal weights by address:
//                the order of d_kf_key is part of the result.  cvRank turns the keys into ranks once per call (frame f's rank is the
//                number of smaller keys); the counters of a subject are indexed by RANK, so that walking them in index order is walking
//                the map.  Two frames with one key have no order: the call says so in every subject's row and writes nothing else;
//   the vote     every slot i < N is visited, a MapPoint that stands in two slots votes twice (:401).  Skipped: -1, a bad MapPoint; in
//                UpdateConnections an observer that is the subject itself, is bad or lives in another map (:415).  UpdateLocalKeyFrames
//                has none of the three tests: a bad observer IS counted and is skipped when the map is walked (:3091) - it is not
//                listed and cannot be pKFmax;
//   nmax         the FIRST strictly greater count in key order (:440, :3094): the largest count and, among its holders, the smallest rank;
//   the lists    the counter block is the whole map in key order (mConnectedKeyFrameWeights; mvpLocalKeyFrames before the neighbour
//                expansion).  The ordered block (UpdateConnections only) is every count >= th, or else the single pair (nmax, pKFmax)
//                (:452-456), after sort ascending on (weight, key) and push_front: weight DESCENDING and, among equal weights, key
//                DESCENDING - one descending sort of weight << 32 | rank;
//   empty        KFcounter.empty() returns before anything is assigned (:423): kCvEmpty, no list entry is written;
//   redundancy   per slot: NULL and bad MapPoints are skipped, then (not monocular) depth > th || depth < 0 as written - a NaN depth is
//                counted; nMPs++; only if Observations() > thObs the observers OTHER than the subject whose octave is <= octave_i + 1 are
//                counted (no isBad test); the slot is redundant when that count is > thObs (the break changes nothing).  The keyframe is
//                redundant when (float)nRedundant > redundant_th * (float)nMPs: ONE float product and a float compare.
// An index outside its table (a MapPoint, a CSR offset, a frame, a keypoint row, the subject's own frame) is kCvBadIndex / kRdBadIndex for
// that subject, found before anything of the subject is written: the counters live in LDS, the slot states are held back in LDS.
// The host build (ORBX_HOST_ROW, tests/cpp/host_shim) runs the same functions with a workgroup of ONE lane; the lane vocabulary (prSync,
// prAtomic*, prExclusive, prSort) is k_place_recognition.hpp's.  Nothing of k_small_math.hpp or k_match_helpers.hpp is needed: there is no
// arithmetic here but counts, compares and the one product.
#pragma once
#include "k_place_recognition.hpp"

namespace orbx {

// == orbx_covis_mode / orbx_covis_status / orbx_redundancy_status
enum { kCvUpdateConnections = 0, kCvLocalKeyFrames = 1 };
enum { kCvOk = 0, kCvEmpty, kCvTruncated, kCvBadIndex, kCvDuplicateKey, kCvStatuses };
enum { kRdOk = 0, kRdSkipped, kRdBadIndex, kRdStatuses };
constexpr int kCvThreads = kPrThreads;

// == orbx_covis_result / orbx_redundancy_result
struct CovisResult { int status, nCounter, nOrdered, nmax, kfMax; };
struct RedundancyResult { int status, nMps, nRedundant, redundant; };
static_assert(sizeof(CovisResult) == 20 && sizeof(RedundancyResult) == 16, "orbx_covis_result / orbx_redundancy_result layout");

__device__ __forceinline__ int cvClamp(int n, int capacity) { return n < 0 ? 0 : n > capacity ? capacity : n; }
// MapPoint m's entries [o0, o1) of d_obs: inside [0, total], not decreasing
__device__ __forceinline__ bool cvListOk(const int* obsOff, int m, int total, int& o0, int& o1) {
    o0 = obsOff[m]; o1 = obsOff[m + 1];
    return o0 >= 0 && o1 >= o0 && o1 <= total;
}

// ---- frame f's rank in key order, and whether another frame holds its key, by one wave: every lane returns the same two values -----------
__device__ __forceinline__ int cvRank(int lane, int f, const uint64_t* key, int nFrames, bool& dup) {
    const uint64_t k = key[f];
    int rank = 0;
    dup = false;
    for (int base = 0; base < nFrames; base += kPrLanes) {
        const int g = base + lane;
        const bool in = g < nFrames;
        const uint64_t kg = in ? key[g] : 0;
        rank += __builtin_popcountll(prBallot(in && kg < k));
        dup |= prBallot(in && kg == k && g != f) != 0;
    }
    return rank;
}

// ---- one subject's vote by one workgroup ---------------------------------------------------------------------------------------------------
// lds: cvVoteLdsBytes(p.nFrames) bytes
__device__ __forceinline__ void cvVote(int tid, int s, const CovisArrays& a, const CovisParams& p, uint8_t* lds) {
    const int nF = p.nFrames, cc = p.connCapacity;
    unsigned long long* keys = (unsigned long long*)lds;
    int* counter = (int*)(lds + (size_t)8 * prPow2(nF));      // by RANK
    int* scr = counter + nF;      // 0 a bad index, 1 counts >= th, 2 nmax, 3 the smallest rank that holds it, 4 .. 7 the wave totals of the ordered count, 8 two keys are equal
    CovisResult* res = (CovisResult*)a.result + s;
    CovisResult r{kCvOk, 0, 0, 0, -1};
    const bool update = p.mode == kCvUpdateConnections;
    for (int k = tid; k < nF; k += kCvThreads) counter[k] = 0;
    if (tid == 0) { scr[0] = scr[1] = scr[2] = scr[8] = 0; scr[3] = 0x7fffffff; }
    prSync();
    {
        bool dupKeys = false;
        for (int b = tid; b < cvRankBlocks(nF); b += kCvThreads) dupKeys |= a.wsDup[b] != 0;
        if (dupKeys) scr[8] = 1;
    }
    {   // KFcounter[mit->first]++ / keyframeCounter[it->first]++
        const int N = cvClamp(a.subjectN[s], p.capacity), total = a.obsOff[p.nPoints];
        const int self = update ? a.subjectKf[s] : -1, myMap = update ? a.subjectMap[s] : 0;
        bool bad = self < -1 || self >= nF;
        for (int i = tid; i < N; i += kCvThreads) {
            const int m = a.subjectMp[(size_t)s * p.capacity + i];
            if (m == -1) continue;
            if (m < 0 || m >= p.nPoints) { bad = true; continue; }
            if (a.mpFlags[m] & 1) continue;
            int o0, o1;
            if (!cvListOk(a.obsOff, m, total, o0, o1)) { bad = true; continue; }
            for (int o = o0; o < o1; o++) {
                const int f = a.obs[2 * (size_t)o];
                if (f < 0 || f >= nF) { bad = true; continue; }
                if (update && (f == self || (a.kfFlags[f] & 1) || a.kfMap[f] != myMap)) continue;
                prAtomicAdd(counter + a.wsRank[f], 1);
            }
        }
        if (bad) scr[0] = 1;
    }
    prSync();
    if (scr[8] || scr[0]) {                                       // (with two equal keys the ranks collide, inside the counters)
        r.status = scr[8] ? kCvDuplicateKey : kCvBadIndex;
        if (tid == 0) *res = r;
        return;
    }
    // the walk over the map: its entries in key order, nmax, the counts that reach th
    int base = 0;
    for (int k0 = 0; k0 < nF; k0 += kCvThreads) {
        const int k = k0 + tid;
        int w = 0, f = -1;
        bool listed = false;
        if (k < nF && (w = counter[k]) > 0) {
            f = a.wsByRank[k];
            listed = update || !(a.kfFlags[f] & 1);               // :3091
            if (!listed) counter[k] = 0;                          // ... and so not pKFmax
        }
        int total;
        const int pos = base + prExclusive(listed, tid, scr + 4, total);
        base += total;
        if (listed) {
            if (pos < cc) { a.counterKf[(size_t)s * cc + pos] = f; a.counterW[(size_t)s * cc + pos] = w; }
            prAtomicMax(scr + 2, w);
            if (update && w >= p.th) keys[prAtomicInc(scr + 1)] = ~(((unsigned long long)(unsigned)w << 32) | (unsigned)k);
        }
    }
    prSync();
    r.nCounter = base;
    if (base == 0) {
        r.status = update ? kCvEmpty : kCvOk;                     // :423; UpdateLocalKeyFrames goes on with an empty list and pKFmax NULL
        if (tid == 0) *res = r;
        return;
    }
    r.nmax = scr[2];
    for (int k = tid; k < nF; k += kCvThreads)
        if (counter[k] == r.nmax) prAtomicMin(scr + 3, k);
    prSync();
    r.kfMax = a.wsByRank[scr[3]];
    if (update) {
        const int n = scr[1];
        if (n == 0) {                                             // :452-456
            r.nOrdered = 1;
            if (tid == 0 && cc >= 1) { a.orderedKf[(size_t)s * cc] = r.kfMax; a.orderedW[(size_t)s * cc] = r.nmax; }
        } else {
            const int P2 = prPow2(n);
            for (int i = n + tid; i < P2; i += kCvThreads) keys[i] = ~0ull;
            prSync();
            prSort(keys, P2, tid);                                // ascending in the complement: weight descending, then key descending
            for (int i = tid; i < n && i < cc; i += kCvThreads) {
                const unsigned long long e = ~keys[i];
                a.orderedKf[(size_t)s * cc + i] = a.wsByRank[(unsigned)e];
                a.orderedW[(size_t)s * cc + i] = (int)(e >> 32);
            }
            r.nOrdered = n;
        }
    }
    r.status = r.nCounter > cc || r.nOrdered > cc ? kCvTruncated : kCvOk;
    if (tid == 0) *res = r;
}

// ---- one keyframe's redundancy by one workgroup -------------------------------------------------------------------------------------------
// a lane per slot: groups of 4 and 8 lanes that share a slot's observations were 1.4 x and 2 x slower (profiles/r34_covisibility.md)
// lds: rdLdsBytes(p.capacity) bytes
__device__ __forceinline__ void rdKeyFrame(int tid, int s, const CovisArrays& a, const CovisParams& p, uint8_t* lds) {
    uint8_t* state = lds;
    int* scr = (int*)(lds + (((size_t)p.capacity + 3) & ~(size_t)3));      // 0 a bad index, 1 nMPs, 2 nRedundantObservations
    RedundancyResult* res = (RedundancyResult*)a.result + s;
    RedundancyResult r{kRdOk, 0, 0, 0};
    const int kf = a.subjectKf[s];
    if (kf < 0 || kf >= p.nFrames) {
        r.status = kRdBadIndex;
        if (tid == 0) *res = r;
        return;
    }
    if (a.kfFlags[kf] & 3) {                                      // :977
        r.status = kRdSkipped;
        if (tid == 0) *res = r;
        return;
    }
    if (tid == 0) scr[0] = scr[1] = scr[2] = 0;
    prSync();
    const int N = cvClamp(a.subjectN[s], p.capacity), total = a.obsOff[p.nPoints];
    const size_t row0 = (size_t)kf * p.capacity;
    {
        bool bad = false;
        int nMps = 0, nRed = 0;
        for (int i = tid; i < N; i += kCvThreads) {
            int st = 0;
            const int m = a.subjectMp[(size_t)s * p.capacity + i];
            if (m != -1 && (m < 0 || m >= p.nPoints)) bad = true;
            else if (m != -1 && !(a.mpFlags[m] & 1)) {
                bool skip = false;
                if (!p.monocular) {
                    const float d = a.depth[row0 + i];
                    skip = d > a.thDepth[kf] || d < 0.f;          // :994
                }
                int o0, o1;
                if (skip) {
                } else if (!cvListOk(a.obsOff, m, total, o0, o1)) bad = true;
                else {
                    st = 1;
                    if ((a.mpNobs ? a.mpNobs[m] : o1 - o0) > p.thObs) {      // pMP->Observations() > thObs
                        const long long level = (long long)a.kpsUn[row0 + i].octave + 1;
                        int nObs = 0;
                        for (int o = o0; o < o1; o++) {
                            const int f = a.obs[2 * (size_t)o], row = a.obs[2 * (size_t)o + 1];
                            if (f < 0 || f >= p.nFrames || row < 0 || row >= cvClamp(a.nOut[f], p.capacity)) { bad = true; continue; }
                            if (f == kf) continue;
                            nObs += (long long)a.kpsUn[(size_t)f * p.capacity + row].octave <= level ? 1 : 0;
                        }
                        if (nObs > p.thObs) st = 2;
                    }
                }
            }
            state[i] = (uint8_t)st;
            nMps += st >= 1; nRed += st == 2;
        }
        if (bad) scr[0] = 1;
        prAtomicAdd(scr + 1, nMps);
        prAtomicAdd(scr + 2, nRed);
    }
    prSync();
    if (scr[0]) {
        r.status = kRdBadIndex;
        if (tid == 0) *res = r;
        return;
    }
    if (a.slotState)
        for (int i = tid; i < N; i += kCvThreads) a.slotState[(size_t)s * p.capacity + i] = state[i];
    r.nMps = scr[1]; r.nRedundant = scr[2];
    r.redundant = (float)r.nRedundant > __fmul_rn(p.redundantTh, (float)r.nMps) ? 1 : 0;      // :1043
    if (tid == 0) *res = r;
}

}  // namespace orbx
