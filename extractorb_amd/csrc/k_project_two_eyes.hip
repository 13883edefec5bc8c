// k_project_two_eyes.hip — ORBmatcher::SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) for TWO-CAMERA frames
// (F.Nleft != -1: reference src/ORBmatcher.cc:44-213, caller Tracking::SearchLocalPoints, src/Tracking.cc:2986), with
// Frame::GetFeaturesInArea over the left eye's mGrid / the right eye's mGridRight and the RAW keypoints mvKeys / mvKeysRight
// (src/Frame.cc:655-724).  The one-eye form (Nleft == -1) is k_search_proj in k_project.hip.
//
// The reference walks the MapPoints in order; MapPoint i runs a left sub-search (L, :62-140) and then a right one (R, :145-207).  Both
// take best and second best over the keypoints of their window that are not closed, i.e. whose CURRENT holder (mvpMapPoints[idx])
// has Observations() > 0.  An accepted sub-search writes its keypoint and, through mvLeftToRightMatch / mvRightToLeftMatch, the paired
// keypoint of the other eye ("pairing write", which checks nothing).  So, unlike the one-eye form,
//   * closure crosses eyes, also into the same MapPoint's own R;
//   * a MapPoint without observations that a pairing write puts on a closed keypoint opens it again;
//   * an L rejected by the ratio test (`continue`, :127) suppresses the MapPoint's R;
//   * a pairing write may land on a keypoint outside the grid.
// ONE WORKGROUP PER PAIR, the parallel fixed point of k_search_proj over a chain of 2*NQ sub-searches (j = 2i: L, j = 2i + 1: R):
//   * every keypoint of both eyes is staged into one slot space: the left eye's mGrid CSR slots, then its keypoints outside the grid,
//     then (from capA on) the same for the right eye; a per-eye keypoint -> slot table turns the pairing maps into a partner slot per slot;
//   * every round, every MapPoint decides L and then R against closedBy[s] = the first sub-search that writes s with a MapPoint that
//     has observations (the one-eye closure, "closed stays closed"); sub-search j's decision depends on decisions < j only (R's activity
//     on its L's), so by induction the fixed point is the sequential result of that closure model, within 2*NQ + 1 rounds;
//   * that model is the reference's exactly unless some pairing write of a MapPoint WITHOUT observations lands on a slot closed
//     before it (reopen).  Up to the first such write the two models agree, so checking the converged decisions for one decides it:
//     none -> the decisions are the reference's; one -> the pair is settled again by a walk of wave 0 (one sub-search after the other,
//     a true holder per slot), the rare corner (local-map MapPoints have observations in practice).
// Descriptors stay in LDS and every round re-scans its windows (no best-key lists: two eyes of 1302 keypoints and 4096 sub-searches
// leave no room for them in 160 KB).  LDS per pair: 50 B per slot (2 * capacity rounded up to 4), 4 B per sub-search, 12 KB of cell offsets.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orbx_lds_pollute.hpp"
#include "k_match_helpers.hpp"
#include "k_wave_min.hpp"
#include "orbx_device.hpp"
#include "orbx_params.hpp"

namespace orbx {

namespace {
constexpr int kCellTab = kGridCells + 2;                  // cell offsets per eye (kGridCells + 1 used)
constexpr int kNoneKey = (256 << 16) | 0xFFFF;            // bestDist = 256, no slot
constexpr unsigned kNoDecision = 0xFFFFFFFFu;             // inactive, no candidate or best above the bound (the MapPoint's R still runs)
constexpr unsigned kRatioReject = 0xFFFFFFFEu;            // rejected by the ratio test (:127 / :191): an L so rejected suppresses its R
constexpr unsigned short kNoSlot = 0xFFFF;
constexpr int kOpen = 0x7fffffff;
constexpr int kThreads = 1024;
}  // namespace

size_t twoEyesSearchLdsBytes(int capacity, int queryCapacity) {
    const size_t s = 2 * (size_t)((capacity + 3) & ~3);
    return s * (32 + 8 + 4 + 2 + 2 + 1 + 1) + (size_t)queryCapacity * 2 * 4 + 8 * sizeof(int) + 2 * kCellTab * sizeof(unsigned short) + 64;
}
__device__ int g_twoEyesStats[4];      // diagnostics: pair 0's rounds, pair 0 settled by the walk, pairs settled by the walk (since the last read), pair 0's ticks
extern "C" int orbx_debug_two_eyes_search_stats(int* out4) {
    if (!out4) return -2;                                  // ORBX_ERR_BAD_ARGUMENT
    hipError_t e = hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_twoEyesStats), sizeof(int) * 4);
    const int zero = 0;
    if (e == hipSuccess) e = hipMemcpyToSymbol(HIP_SYMBOL(g_twoEyesStats), &zero, sizeof(int), 2 * sizeof(int));
    return e == hipSuccess ? 0 : -6;                       // ORBX_ERR_HIP
}

// grid: n_pairs; kThreads threads.  Pair q: left eye = frame 2*(pairFirst + q*pairStep), right eye = the next frame.
__global__ __launch_bounds__(kThreads) void k_search_proj_two_eyes(const ProjQuery* __restrict__ queries, const uint8_t* __restrict__ qdesc,
                                                                   const int* __restrict__ nQueries, const Keypoint* __restrict__ kps,
                                                                   const uint8_t* __restrict__ desc, const int* __restrict__ nOut,
                                                                   const int* __restrict__ gridOff, const int* __restrict__ gridIdx,
                                                                   const int* __restrict__ leftToRight, const int* __restrict__ rightToLeft,
                                                                   uint8_t* __restrict__ occupied, TwoEyesSearchParams p,
                                                                   int* __restrict__ matches, int* __restrict__ nMatches) {
    extern __shared__ __align__(16) uint8_t smem[];
    const int cap = p.capacity, capA = (cap + 3) & ~3, S = 2 * capA;
    uint4* d2 = (uint4*)smem;                              // [S][2] descriptor of slot s
    float2* xy = (float2*)(d2 + 2 * S);                    // [S] raw keypoint position
    int* closedBy = (int*)(xy + S);                        // [S] first sub-search that closes slot s (-1: closed on entry, kOpen: nobody);
                                                           //     after the search: last writer + 1 << 1 | closed
    unsigned* dec = (unsigned*)(closedBy + S);             // [2 * queryCapacity] decision of every sub-search: slot | closes << 16, kNoDecision, kRatioReject
    int* flags = (int*)(dec + 2 * p.queryCapacity);        // [8] "a decision changed" (two alternating slots), writes, reopen seen, outside counters (2)
    unsigned short* cellOff = (unsigned short*)(flags + 8);      // [2][kCellTab] slot range of every grid cell, per eye
    unsigned short* pairSlot = cellOff + 2 * kCellTab;     // [S] slot of the paired keypoint in the other eye, kNoSlot = none
    unsigned short* kp2slot = pairSlot + S;                // [2][capA] slot of keypoint i of an eye
    uint8_t* oct = (uint8_t*)(kp2slot + S);                // [S] octave
    uint8_t* occ = oct + S;                                // [S] holds a MapPoint with Observations() > 0 on entry
    int* lastW = (int*)d2;                                 // (after the rounds, over the then dead descriptors) last sub-search that writes the slot

    const int pair = blockIdx.x, tid = threadIdx.x;
    const int fL = 2 * (p.pairFirst + pair * p.pairStep), fR = fL + 1;
    const int NL = min(max(nOut[fL], 0), cap), NR = min(max(nOut[fR], 0), cap);
    const int nInL = min(max(gridOff[(long long)fL * (kGridCells + 1) + kGridCells], 0), NL);
    const int nInR = min(max(gridOff[(long long)fR * (kGridCells + 1) + kGridCells], 0), NR);
    const ProjQuery* Q = queries + (long long)pair * p.queryCapacity * 2;
    const uint32_t* QD = (const uint32_t*)(qdesc + (long long)(p.descFirst + pair * p.descStep) * p.queryCapacity * 32);
    const int NQ = nQueries ? min(max(nQueries[pair], 0), p.queryCapacity) : p.queryCapacity;

    // ---- stage both eyes: grid keypoints in CSR order, then the keypoints outside the grid (written by pairing writes only) ----
    const unsigned long long tStart = __builtin_amdgcn_s_memrealtime();
    for (int t = tid; t < S; t += kThreads) { kp2slot[t] = kNoSlot; pairSlot[t] = kNoSlot; occ[t] = 0; }
    if (tid < 8) flags[tid] = 0;
    __syncthreads();
    for (int t = tid; t < S; t += kThreads) {
        const int e = t >= capA, pos = t - e * capA;
        if (pos >= (e ? nInR : nInL)) continue;
        const int f = fL + e, i = min(max(gridIdx[(long long)f * cap + pos], 0), (e ? NR : NL) - 1);      // (clamped: a corrupt grid must not index past the frame)
        const Keypoint k = kps[(long long)f * cap + i];
        xy[t] = make_float2(k.x, k.y);
        oct[t] = (uint8_t)min(max(k.octave, 0), 255);
        occ[t] = occupied ? occupied[(long long)(2 * pair + e) * cap + i] : (uint8_t)0;
        kp2slot[e * capA + i] = (unsigned short)t;
        const uint32_t* D = (const uint32_t*)(desc + ((long long)f * cap + i) * 32);
        d2[2 * t] = *(const uint4*)D; d2[2 * t + 1] = *(const uint4*)(D + 4);
    }
    for (int c = tid; c < 2 * kCellTab; c += kThreads) {
        const int e = c >= kCellTab, cc = c - e * kCellTab, nIn = e ? nInR : nInL;
        const int o = cc <= kGridCells ? gridOff[(long long)(fL + e) * (kGridCells + 1) + cc] : nIn;
        cellOff[c] = (unsigned short)(e * capA + min(max(o, 0), nIn));
    }
    for (int j = tid; j < 2 * NQ; j += kThreads) dec[j] = kNoDecision;
    __syncthreads();
    for (int t = tid; t < S; t += kThreads) {
        const int e = t >= capA, i = t - e * capA;
        if (i >= (e ? NR : NL) || kp2slot[t] != kNoSlot) continue;
        const int pos = (e ? nInR : nInL) + atomicAdd(&flags[4 + e], 1);
        if (pos >= capA) continue;                         // (only a grid that lists a keypoint twice gets here)
        const int s = e * capA + pos;
        kp2slot[t] = (unsigned short)s;
        occ[s] = occupied ? occupied[(long long)(2 * pair + e) * cap + i] : (uint8_t)0;
    }
    __syncthreads();
    for (int t = tid; t < S; t += kThreads) {
        const int e = t >= capA, i = t - e * capA;
        const unsigned short s = kp2slot[t];
        if (i < (e ? NR : NL) && s != kNoSlot) {
            int m = -1;                                    // mvLeftToRightMatch / mvRightToLeftMatch; outside [0, N of the other eye): none
            if (e == 0) { if (leftToRight) m = leftToRight[(long long)fL * cap + i]; }
            else if (rightToLeft) m = rightToLeft[(long long)fR * cap + i];
            if (m >= 0 && m < (e ? NL : NR)) pairSlot[s] = kp2slot[(1 - e) * capA + m];
        }
        closedBy[t] = occ[t] ? -1 : kOpen;
    }
    __syncthreads();

    // does slot s pass GetFeaturesInArea's level filter (:690, :705-712) and box test (:717)?
    auto inArea = [&](const ProjQuery& q, int s) -> bool {
        const bool checkLevels = q.minLevel > 0 || q.maxLevel >= 0;
        const int lv = oct[s];
        const float2 pt = xy[s];
        return (!checkLevels || (lv >= q.minLevel && (q.maxLevel < 0 || lv <= q.maxLevel))) && fabsf(__fsub_rn(pt.x, q.u)) < q.radius &&
               fabsf(__fsub_rn(pt.y, q.v)) < q.radius;
    };
    // the acceptance tests on the smallest and second smallest key (distance << 16 | slot: slots ascend in traversal order, so this is
    // the reference's running best / second with its strict "<"): :115-127 / :179-191
    auto judge = [&](int key, int second, int qflags) -> unsigned {
        const int bestDist = key >> 16, bs = key & 0xFFFF;
        if (key == kNoneKey || bestDist > p.maxDist) return kNoDecision;
        const int bestDist2 = second >> 16;
        const int bestLevel = oct[bs], bestLevel2 = bestDist2 < 256 ? (int)oct[second & 0xFFFF] : -1;
        if (bestLevel == bestLevel2 && (float)bestDist > __fmul_rn(p.nnRatio, (float)bestDist2)) return kRatioReject;
        return (unsigned)bs | (((unsigned)qflags >> 1) & 1u) << 16;      // accepted: slot, bit 16 = the MapPoint closes what it writes
    };
    // sub-search j against the current closure (closedBy[s] < j, or s == alsoClosed)
    auto decide = [&](int j, const ProjQuery& q, const uint4& dlo, const uint4& dhi, int alsoClosed) -> unsigned {
        if (!(q.flags & 1)) return kNoDecision;
        int minCX, maxCX, minCY, maxCY;
        if (!frameCellWindow(q.u, q.v, q.radius, p, minCX, maxCX, minCY, maxCY)) return kNoDecision;
        const int cb = (j & 1) * kCellTab;
        int key = kNoneKey, second = kNoneKey;
        for (int cx = minCX; cx <= maxCX; cx++) {          // ascending cells, push_back order inside a cell = ascending slots
            const int sEnd = cellOff[cb + cx * kGridRows + maxCY + 1];
            for (int s = cellOff[cb + cx * kGridRows + minCY]; s < sEnd; s++) {
                if (closedBy[s] < j || s == alsoClosed || !inArea(q, s)) continue;      // :89-91 / :158-160
                const int k = (hamming256(dlo, dhi, d2[2 * s], d2[2 * s + 1]) << 16) | s;
                if (k < key) { second = key; key = k; } else if (k < second) second = k;
            }
        }
        return judge(key, second, q.flags);
    };
    // MapPoint i: L, then R unless L was rejected by the ratio test; R already sees what L's own pairing write closes
    auto decideMapPoint = [&](int i) -> bool {
        const uint4 dlo = *(const uint4*)(QD + (long long)i * 8), dhi = *(const uint4*)(QD + (long long)i * 8 + 4);
        const unsigned dL = decide(2 * i, Q[2 * i], dlo, dhi, -1);
        int also = -1;
        if (dL < kRatioReject && (dL >> 16)) { const unsigned short ps = pairSlot[dL & 0xFFFFu]; if (ps != kNoSlot) also = ps; }
        const unsigned dR = dL == kRatioReject ? kNoDecision : decide(2 * i + 1, Q[2 * i + 1], dlo, dhi, also);
        const bool changed = dL != dec[2 * i] || dR != dec[2 * i + 1];
        dec[2 * i] = dL; dec[2 * i + 1] = dR;
        return changed;
    };

    for (int i = tid; i < NQ; i += kThreads) decideMapPoint(i);
    __syncthreads();
    int rounds = 1;
    for (int round = 1; round <= 2 * NQ + 1; round++, rounds++) {
        for (int j = tid; j < 2 * NQ; j += kThreads) {     // closedBy[s] = first sub-search that closes slot s under the current decisions
            const unsigned d = dec[j];
            if (d < kRatioReject && (d >> 16)) {
                atomicMin(&closedBy[d & 0xFFFFu], j);
                const unsigned short ps = pairSlot[d & 0xFFFFu];
                if (ps != kNoSlot) atomicMin(&closedBy[ps], j);
            }
        }
        __syncthreads();
        bool mineChanged = false;
        for (int i = tid; i < NQ; i += kThreads) mineChanged |= decideMapPoint(i);
        if (mineChanged) flags[round & 1] = 1;
        __syncthreads();
        const bool any = flags[round & 1] != 0;
        if (tid == 0) flags[(round & 1) ^ 1] = 0;          // the other slot is read again only after the next barriers
        if (!any) break;
        for (int s = tid; s < S; s += kThreads) closedBy[s] = occ[s] ? -1 : kOpen;
        __syncthreads();
    }
    // closedBy now belongs to the converged decisions: does a pairing write of a MapPoint without observations land on a slot closed before it?
    for (int j = tid; j < 2 * NQ; j += kThreads) {
        const unsigned d = dec[j];
        if (d < kRatioReject && !(d >> 16)) {
            const unsigned short ps = pairSlot[d & 0xFFFFu];
            if (ps != kNoSlot && closedBy[ps] < j) flags[3] = 1;
        }
    }
    __syncthreads();
    const bool walk = p.forceWalk || flags[3] != 0;

    if (walk) {
        // ---- the walk (wave 0): one sub-search after the other, a true holder per slot: bit 0 = closed, bits 1.. = last writer + 1 ----
        if (tid < 64) {
            const int lane = tid;
            for (int s = lane; s < S; s += 64) closedBy[s] = occ[s];
            __builtin_amdgcn_wave_barrier();
            int writes = 0;
            bool ratioL = false;
            for (int j = 0; j < 2 * NQ; j++) {
                if ((j & 1) && ratioL) continue;
                const ProjQuery q = Q[j];
                int minCX, maxCX, minCY, maxCY;
                unsigned d = kNoDecision;
                if ((q.flags & 1) && frameCellWindow(q.u, q.v, q.radius, p, minCX, maxCX, minCY, maxCY)) {
                    const uint4 dlo = *(const uint4*)(QD + (long long)(j >> 1) * 8), dhi = *(const uint4*)(QD + (long long)(j >> 1) * 8 + 4);
                    const int cb = (j & 1) * kCellTab;
                    int key = kNoneKey, second = kNoneKey;
                    for (int cx = minCX; cx <= maxCX; cx++) {
                        const int sEnd = cellOff[cb + cx * kGridRows + maxCY + 1];
                        for (int s = cellOff[cb + cx * kGridRows + minCY] + lane; s < sEnd; s += 64) {
                            if ((closedBy[s] & 1) || !inArea(q, s)) continue;
                            const int k = (hamming256(dlo, dhi, d2[2 * s], d2[2 * s + 1]) << 16) | s;
                            if (k < key) { second = key; key = k; } else if (k < second) second = k;
                        }
                    }
                    const int best = waveMin(key);         // keys are unique: exactly one lane held the best, it offers its second
                    if (key == best) key = second;
                    d = judge(best, waveMin(key), q.flags);
                }
                if (!(j & 1)) ratioL = d == kRatioReject;
                if (d < kRatioReject) {
                    const int bs = (int)(d & 0xFFFFu);
                    const unsigned short ps = pairSlot[bs];
                    const int v = ((j + 1) << 1) | (int)(d >> 16);
                    closedBy[bs] = v;
                    if (ps != kNoSlot) closedBy[ps] = v;
                    writes += 1 + (ps != kNoSlot);
                }
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
                __builtin_amdgcn_wave_barrier();
            }
            if (lane == 0) flags[2] = writes;
        }
    } else {
        // ---- the tables of the converged decisions: last writer of every slot (a later write replaces an earlier one), every write counts ----
        for (int s = tid; s < S; s += kThreads) lastW[s] = -1;
        __syncthreads();
        int writes = 0;
        for (int j = tid; j < 2 * NQ; j += kThreads) {
            const unsigned d = dec[j];
            if (d >= kRatioReject) continue;
            atomicMax(&lastW[d & 0xFFFFu], j);
            const unsigned short ps = pairSlot[d & 0xFFFFu];
            if (ps != kNoSlot) atomicMax(&lastW[ps], j);
            writes += 1 + (ps != kNoSlot);
        }
        if (writes) atomicAdd(&flags[2], writes);
        __syncthreads();
        for (int s = tid; s < S; s += kThreads) closedBy[s] = ((lastW[s] + 1) << 1) | (int)(closedBy[s] != kOpen);
    }
    __syncthreads();
    for (int t = tid; t < 2 * cap; t += kThreads) {
        const int e = t >= cap, i = t - e * cap;
        int m = -1;
        if (i < (e ? NR : NL)) {
            const unsigned short s = kp2slot[e * capA + i];
            if (s != kNoSlot) {
                const int w = closedBy[s], j = (w >> 1) - 1;
                m = j >= 0 ? j >> 1 : -1;                  // the MapPoint of the last writer
                if (occupied) occupied[(long long)(2 * pair + e) * cap + i] = (uint8_t)(w & 1);
            }
        }
        matches[(long long)(2 * pair + e) * cap + i] = m;
    }
    if (tid == 0) {
        nMatches[pair] = flags[2];
        if (walk) atomicAdd(&g_twoEyesStats[2], 1);
        if (pair == 0) {
            g_twoEyesStats[0] = rounds; g_twoEyesStats[1] = walk ? 1 : 0;
            g_twoEyesStats[3] = (int)(__builtin_amdgcn_s_memrealtime() - tStart);
        }
    }
}

void launchSearchProjTwoEyes(hipStream_t st, const ProjQuery* queries, const uint8_t* qdesc, const int* nQueries, const Keypoint* kps,
                             const uint8_t* desc, const int* nOut, const int* gridOff, const int* gridIdx, const int* leftToRight,
                             const int* rightToLeft, uint8_t* occupied, const TwoEyesSearchParams& p, int* matches, int* nMatches, int nPairs, LdsPolluter pollute) {
    pollute(st);
    hipLaunchKernelGGL(k_search_proj_two_eyes, dim3(nPairs), dim3(kThreads), twoEyesSearchLdsBytes(p.capacity, p.queryCapacity), st, queries, qdesc,
                       nQueries, kps, desc, nOut, gridOff, gridIdx, leftToRight, rightToLeft, occupied, p, matches, nMatches);
}

}  // namespace orbx
