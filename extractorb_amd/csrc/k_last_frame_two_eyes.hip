// k_last_frame_two_eyes.hip — ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) for TWO-CAMERA frames
// (CurrentFrame.Nleft != -1: reference src/ORBmatcher.cc:1961-2177, caller Tracking::TrackWithMotionModel), with KannalaBrandt8::project
// (src/CameraModels/KannalaBrandt8.cpp:28-44, k_camera_kb8.hpp), Frame::GetFeaturesInArea over the left eye's mGrid / the right eye's
// mGridRight and the RAW keypoints mvKeys / mvKeysRight (src/Frame.cc:655-724).  The one-camera form is k_project_last / k_search_proj in
// k_project.hip.  Three kernels:
//   k_kb8_project            KannalaBrandt8::project over a point list (callers' own isInFrustum on such rigs);
//   k_project_last_two_eyes  the front half, one thread per MapPoint of the last rig (k_project_last_two_eyes_point.hpp);
//   k_search_last_two_eyes   the matching, ONE WORKGROUP PER PAIR, the parallel fixed point of k_search_proj.
//
// Why the fixed point carries over.  MapPoint j of the last rig runs a left sub-search (L, :2013-2082) and then a right one (R, :2083-2149).
// An accepted L writes mvpMapPoints[bestIdx2], an accepted R writes mvpMapPoints[bestIdx2 + Nleft]; there are NO pairing writes here
// (mvLeftToRightMatch is not read), so L only ever touches left keypoints and R only right ones, and a keypoint is closed to later
// requests exactly when a MapPoint with Observations() > 0 has been written to it (:2036-2038, :2111-2113): closed stays closed, as in the
// one-camera form.  The walk is therefore TWO INDEPENDENT sequential chains, the L chain over the left eye and the R chain over the right
// eye, coupled by exactly two things:
//   * an L whose GetFeaturesInArea result is empty `continue`s (:2024) and so suppresses the R of its MapPoint.  That result depends on the
//     cell window, the level range and the box test only - never on closure - so it is known before the first round.  (An L whose best
//     is above TH_HIGH does NOT suppress R; nor does an L all of whose candidates are closed: vIndices2 is not empty then.)
//   * ONE rotation histogram over both eyes (:2155-2174): the three maxima are taken over the joint counts, and every entry of a dropped
//     bin clears its keypoint and takes one off nmatches.
// So each chain settles as k_search_proj's does: every sub-search decides in parallel against closedBy[s] = the first request of its chain
// that closes slot s under the current decisions, closedBy is rebuilt, and the round repeats until no decision changes; by induction the
// decisions of requests 0..k are final after round k + 1, so the fixed point IS the sequential result.  Two launches of k_search_proj
// cannot express this entry: neither the suppression rule nor the joint histogram.
// Both eyes are staged into one slot space in CSR order (left eye's mGrid slots from 0, right eye's mGridRight slots from capA), descriptors
// in LDS, every round re-scans its windows (no best-key lists: two eyes of 1302 keypoints and 5208 sub-searches leave no room for them).
// LDS per pair: 48 B per slot (2 * capacity rounded up to 4), 3 B per sub-search (4 * capacity of them), 12 KB of cell offsets.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orbx_lds_pollute.hpp"
#include "k_camera_kb8.hpp"
#include "k_match_helpers.hpp"
#include "k_project_last_two_eyes_point.hpp"
#include "orbx_device.hpp"
#include "orbx_params.hpp"

namespace orbx {

namespace {
constexpr int kCellTab = kGridCells + 2;                  // cell offsets per eye (kGridCells + 1 used)
constexpr int kNoneKey = (256 << 16) | 0xFFFF;            // bestDist = 256, no slot
constexpr unsigned short kNoDecision = 0xFFFF;            // inactive, suppressed, no candidate or best above the bound
constexpr int kOpen = 0x7fffffff;
constexpr int kThreads = 1024;
constexpr int kRuns = 1, kObs = 2, kAny = 4;              // qstat bits: the sub-search runs, its MapPoint has observations, its area result is not empty
struct Kb8Cam { float k[8]; };
}  // namespace

size_t lastTwoEyesLdsBytes(int capacity) {
    const size_t s = 2 * (size_t)((capacity + 3) & ~3);
    return s * (32 + 8 + 4 + 2 + 1 + 1) + (size_t)capacity * 4 * (2 + 1) + (kHistoLength + 4) * sizeof(int) + 2 * kCellTab * sizeof(unsigned short) + 64;
}
__device__ int g_lastTwoEyesStats[4];      // diagnostics of the last launch's pair 0: rounds, ticks (100 MHz) of staging, of the first scan, of the rounds
extern "C" int orbx_debug_last_frame_two_eyes_stats(int* out4) {
    if (!out4) return -2;                                  // ORBX_ERR_BAD_ARGUMENT
    return hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_lastTwoEyesStats), sizeof(int) * 4) == hipSuccess ? 0 : -6;      // ORBX_ERR_HIP
}

// grid: ceil(n / 256)
__global__ __launch_bounds__(256) void k_kb8_project(const float* __restrict__ xyz, Kb8Cam cam, int n, float* __restrict__ uv) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float u, v;
    kb8Project(cam.k, xyz[3LL * i], xyz[3LL * i + 1], xyz[3LL * i + 2], u, v);
    uv[2LL * i] = u; uv[2LL * i + 1] = v;
}

// grid (ceil(2 * capacity / 256), n_pairs)
__global__ __launch_bounds__(256) void k_project_last_two_eyes(const Keypoint* __restrict__ kps, const int* __restrict__ nOut,
                                                               const uint8_t* __restrict__ mpFlags, const float* __restrict__ world,
                                                               const float* __restrict__ poses, ProjectTwoEyesParams p,
                                                               ProjQuery* __restrict__ queries) {
    const int pair = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= 2 * p.capacity) return;
    ProjQuery qL, qR;
    projectLastTwoEyesRequest(kps, nOut, mpFlags, world, poses, p, pair, j, qL, qR);
    ProjQuery* out = queries + ((long long)pair * 2 * p.capacity + j) * 2;
    out[0] = qL; out[1] = qR;
}

// grid: n_pairs; kThreads threads.  Pair q: left eye = frame 2*(curFirst + q*curStep), right eye = the next frame.
__global__ __launch_bounds__(kThreads) void k_search_last_two_eyes(const ProjQuery* __restrict__ queries, const uint8_t* __restrict__ qdesc,
                                                                   const Keypoint* __restrict__ kps, const uint8_t* __restrict__ desc,
                                                                   const int* __restrict__ nOut, const int* __restrict__ gridOff,
                                                                   const int* __restrict__ gridIdx, uint8_t* __restrict__ occupied,
                                                                   LastTwoEyesSearchParams p, int* __restrict__ matches, int* __restrict__ nMatches) {
    extern __shared__ __align__(16) uint8_t smem[];
    const int cap = p.capacity, capA = (cap + 3) & ~3, S = 2 * capA, NQ = 2 * cap, T = 2 * NQ;
    uint4* d2 = (uint4*)smem;                              // [S][2] descriptor of slot s
    float2* xy = (float2*)(d2 + 2 * S);                    // [S] raw keypoint position
    int* closedBy = (int*)(xy + S);                        // [S] first request of the eye's chain that closes slot s (-1: closed on entry, kOpen: nobody)
    int* hist = closedBy + S;                              // [30] rotHist sizes, both eyes
    int* flags = hist + kHistoLength;                      // [4] "a decision changed" (two alternating slots), number of accepted sub-searches
    unsigned short* dec = (unsigned short*)(flags + 4);    // [T] decision of sub-search t = 2 * request + eye: slot | closes << 15, or kNoDecision
    unsigned short* cellOff = dec + T;                     // [2][kCellTab] slot range of every grid cell, per eye
    unsigned short* idx2 = cellOff + 2 * kCellTab;         // [S] keypoint index in its eye
    uint8_t* oct = (uint8_t*)(idx2 + S);                   // [S] octave
    uint8_t* occ = oct + S;                                // [S] holds a MapPoint with Observations() > 0 on entry
    uint8_t* qstat = occ + S;                              // [T] kRuns | kObs | kAny
    int* m2q = (int*)d2;                                   // (after the rounds, over the then dead descriptors) request whose MapPoint the keypoint holds, -1 = none
    unsigned* binMask = (unsigned*)(m2q + S);              // (same) rotHist bins the keypoint was pushed to

    const int pair = blockIdx.x, tid = threadIdx.x;
    const int fL = 2 * (p.curFirst + pair * p.curStep);
    const int N0 = min(max(nOut[fL], 0), cap), N1 = min(max(nOut[fL + 1], 0), cap);
    const int nIn0 = min(max(gridOff[(long long)fL * (kGridCells + 1) + kGridCells], 0), N0);
    const int nIn1 = min(max(gridOff[(long long)(fL + 1) * (kGridCells + 1) + kGridCells], 0), N1);
    const ProjQuery* Q = queries + (long long)pair * T;
    const uint32_t* QD = (const uint32_t*)(qdesc + (long long)pair * NQ * 32);
    uint8_t* occIO = occupied ? occupied + (long long)pair * 2 * cap : nullptr;
    int* out = matches + (long long)pair * 2 * cap;

    // ---- stage both eyes in grid order ----
    const unsigned long long tStart = __builtin_amdgcn_s_memrealtime();
    for (int t = tid; t < S; t += kThreads) {
        const int e = t >= capA, pos = t - e * capA, nE = e ? N1 : N0;
        if (pos >= (e ? nIn1 : nIn0)) continue;
        const int f = fL + e, i = min(max(gridIdx[(long long)f * cap + pos], 0), nE - 1);      // (clamped: a corrupt grid must not index past the frame)
        const Keypoint k = kps[(long long)f * cap + i];
        xy[t] = make_float2(k.x, k.y);
        oct[t] = (uint8_t)min(max(k.octave, 0), 255);      // one byte per slot: an octave outside [0, 255] (no extractor writes one) counts as 0 / 255 (include/orbx.h)
        occ[t] = occIO ? occIO[e * cap + i] : (uint8_t)0;
        idx2[t] = (unsigned short)i;
        const uint32_t* D = (const uint32_t*)(desc + ((long long)f * cap + i) * 32);
        d2[2 * t] = *(const uint4*)D; d2[2 * t + 1] = *(const uint4*)(D + 4);
        closedBy[t] = occ[t] ? -1 : kOpen;
    }
    for (int c = tid; c < 2 * kCellTab; c += kThreads) {
        const int e = c >= kCellTab, cc = c - e * kCellTab, nIn = e ? nIn1 : nIn0;
        const int o = cc <= kGridCells ? gridOff[(long long)(fL + e) * (kGridCells + 1) + cc] : nIn;
        cellOff[c] = (unsigned short)(e * capA + min(max(o, 0), nIn));
    }
    for (int i = tid; i < 2 * cap; i += kThreads) out[i] = -1;      // keypoints outside the grid can never match
    if (tid < kHistoLength) hist[tid] = 0;
    if (tid < 4) flags[tid] = 0;
    __syncthreads();
    const unsigned long long tStaged = __builtin_amdgcn_s_memrealtime();

    // Sub-search t against the current closure: the smallest key (distance << 16 | slot; slots ascend in GetFeaturesInArea's traversal order, so
    // this is the reference's running best with its strict "<") among the keypoints of the window that pass the level filter (Frame.cc:690,
    // :705-712) and the box test (:717) and are not closed for request t >> 1.  `any`: the area result is not empty, closed keypoints included.
    auto decide = [&](int t, const ProjQuery& q, bool& any) -> unsigned short {
        any = false;
        int minCX, maxCX, minCY, maxCY;
        if (!frameCellWindow(q.u, q.v, q.radius, p, minCX, maxCX, minCY, maxCY)) return kNoDecision;
        const int j = t >> 1, cb = (t & 1) * kCellTab;
        const bool checkLevels = q.minLevel > 0 || q.maxLevel >= 0;
        const int loLv = checkLevels ? max(q.minLevel, 0) : 0, hiLv = checkLevels && q.maxLevel >= 0 ? min(q.maxLevel, 255) : 255;
        const uint4 dlo = *(const uint4*)(QD + (long long)j * 8), dhi = *(const uint4*)(QD + (long long)j * 8 + 4);
        int key = kNoneKey;
        for (int cx = minCX; cx <= maxCX; cx++) {          // ascending cells, push_back order inside a cell = ascending slots
            const int sEnd = cellOff[cb + cx * kGridRows + maxCY + 1];
            for (int s = cellOff[cb + cx * kGridRows + minCY]; s < sEnd; s++) {
                const int lv = oct[s];
                const float2 pt = xy[s];
                if (lv < loLv || lv > hiLv || !(fabsf(__fsub_rn(pt.x, q.u)) < q.radius) || !(fabsf(__fsub_rn(pt.y, q.v)) < q.radius)) continue;
                any = true;
                if (closedBy[s] < j) continue;                                                              // :2036-2038 / :2111-2113
                key = min(key, (hamming256(dlo, dhi, d2[2 * s], d2[2 * s + 1]) << 16) | s);
            }
        }
        if (key == kNoneKey || (key >> 16) > p.maxDist) return kNoDecision;                                  // :2059 / :2126
        return (unsigned short)((key & 0xFFFF) | ((q.flags >> 1) & 1) << 15);      // accepted: slot, bit 15 = the MapPoint closes it
    };

    // round 0: every sub-search scans its window once; what the area result holds is settled here for good
    for (int t = tid; t < T; t += kThreads) {
        const ProjQuery q = Q[t];
        bool any = false;
        unsigned short d = kNoDecision;
        if (q.flags & 1) d = decide(t, q, any);
        qstat[t] = (uint8_t)((q.flags & 1 ? kRuns : 0) | (q.flags & 2 ? kObs : 0) | (any ? kAny : 0));
        dec[t] = d;
    }
    __syncthreads();
    for (int j = tid; j < NQ; j += kThreads) {             // :2024: an L with an empty area result skips the rest of its MapPoint, R included
        const uint8_t sl = qstat[2 * j];
        if ((sl & kRuns) && !(sl & kAny)) { qstat[2 * j + 1] &= (uint8_t)~kRuns; dec[2 * j + 1] = kNoDecision; }
    }
    __syncthreads();
    const unsigned long long tScanned = __builtin_amdgcn_s_memrealtime();
    int rounds = 1;
    for (int round = 1; round <= NQ + 1; round++, rounds++) {
        for (int t = tid; t < T; t += kThreads) {          // closedBy[s] = first request that closes slot s under the current decisions
            const unsigned short d = dec[t];
            if (d != kNoDecision && (d & 0x8000)) atomicMin(&closedBy[d & 0x7FFF], t >> 1);
        }
        __syncthreads();
        bool mineChanged = false;
        for (int t = tid; t < T; t += kThreads) {
            if ((qstat[t] & (kRuns | kAny)) != (kRuns | kAny)) continue;
            bool any;
            const unsigned short d = decide(t, Q[t], any);
            if (d != dec[t]) { dec[t] = d; mineChanged = true; }
        }
        if (mineChanged) flags[round & 1] = 1;
        __syncthreads();
        const bool changed = flags[round & 1] != 0;
        if (tid == 0) flags[(round & 1) ^ 1] = 0;          // the other slot is read again only after the next barriers
        if (!changed) break;
        for (int s = tid; s < S; s += kThreads) {
            const int e = s >= capA;
            if (s - e * capA < (e ? nIn1 : nIn0)) closedBy[s] = occ[s] ? -1 : kOpen;
        }
        __syncthreads();
    }
    if (tid == 0 && pair == 0) {
        g_lastTwoEyesStats[0] = rounds; g_lastTwoEyesStats[1] = (int)(tStaged - tStart); g_lastTwoEyesStats[2] = (int)(tScanned - tStaged);
        g_lastTwoEyesStats[3] = (int)(__builtin_amdgcn_s_memrealtime() - tScanned);
    }

    // ---- the tables the walk would have left: mvpMapPoints[bestIdx2] = pMP is overwritten by every later accepted request, nmatches and the
    //      ONE rotHist count every acceptance of either eye ----
    for (int s = tid; s < S; s += kThreads) { m2q[s] = -1; binMask[s] = 0u; }      // (nobody reads the descriptor words any more)
    __syncthreads();
    int nm = 0;
    for (int t = tid; t < T; t += kThreads) {
        const unsigned short d = dec[t];
        if (d == kNoDecision) continue;
        const int bs = d & 0x7FFF;
        atomicMax(&m2q[bs], t >> 1);
        nm++;
        if (p.checkOrientation) {                                                                                    // :2064-2081 / :2130-2146
            const int e = bs >= capA;
            const int bin = rotationBin(Q[t].angle, kps[(long long)(fL + e) * cap + idx2[bs]].angle);
            atomicOr(&binMask[bs], 1u << bin);
            atomicAdd(&hist[bin], 1);
        }
    }
    if (nm) atomicAdd(&flags[2], nm);
    __syncthreads();

    unsigned dropBins = 0u;
    int droppedCount = 0;
    if (p.checkOrientation) {                                                                                        // :2155-2174
        const ThreeMaxima top3 = computeThreeMaxima(hist);
        for (int i = 0; i < kHistoLength; i++)
            if (i != top3.ind1 && i != top3.ind2 && i != top3.ind3) { dropBins |= 1u << i; droppedCount += hist[i]; }      // one nmatches-- per entry
    }
    for (int s = tid; s < S; s += kThreads) {
        const int e = s >= capA;
        if (s - e * capA >= (e ? nIn1 : nIn0)) continue;
        const bool dropped = (binMask[s] & dropBins) != 0u;
        out[e * cap + idx2[s]] = dropped ? -1 : m2q[s];
        if (occIO) occIO[e * cap + idx2[s]] = dropped ? (uint8_t)0 : (uint8_t)(closedBy[s] != kOpen);
    }
    if (tid == 0) nMatches[pair] = flags[2] - droppedCount;
}

void launchKb8Project(hipStream_t st, const float* xyz, const float* cam8, int n, float* uv, LdsPolluter pollute) {
    Kb8Cam c;
    for (int i = 0; i < 8; i++) c.k[i] = cam8[i];
    pollute(st);
    hipLaunchKernelGGL(k_kb8_project, dim3((n + 255) / 256), dim3(256), 0, st, xyz, c, n, uv);
}

void launchProjectLastTwoEyes(hipStream_t st, const Keypoint* kps, const int* nOut, const uint8_t* mpFlags, const float* world,
                              const float* poses, const ProjectTwoEyesParams& p, ProjQuery* queries, int nPairs, LdsPolluter pollute) {
    pollute(st);
    hipLaunchKernelGGL(k_project_last_two_eyes, dim3((2 * p.capacity + 255) / 256, nPairs), dim3(256), 0, st, kps, nOut, mpFlags, world, poses, p, queries);
}

void launchSearchLastTwoEyes(hipStream_t st, const ProjQuery* queries, const uint8_t* qdesc, const Keypoint* kps, const uint8_t* desc,
                             const int* nOut, const int* gridOff, const int* gridIdx, uint8_t* occupied, const LastTwoEyesSearchParams& p,
                             int* matches, int* nMatches, int nPairs, LdsPolluter pollute) {
    pollute(st);
    hipLaunchKernelGGL(k_search_last_two_eyes, dim3(nPairs), dim3(kThreads), lastTwoEyesLdsBytes(p.capacity), st, queries, qdesc, kps, desc, nOut,
                       gridOff, gridIdx, occupied, p, matches, nMatches);
}

}  // namespace orbx
