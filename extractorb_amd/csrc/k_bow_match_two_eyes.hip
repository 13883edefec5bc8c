// k_bow_match_two_eyes.hip — ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vpMapPointMatches) for TWO-CAMERA frames (reference
// src/ORBmatcher.cc:269-471 with F.Nleft != -1: the else branch :340-367 and :373-433), on what ComputeBoW wrote PER EYE.
//
// A pair X is batch frame 2X (left eye: mvKeys, the first Nleft rows of mDescriptors) and 2X + 1 (right eye: mvKeysRight, the other rows).
// The reference's mFeatVec of the concatenated descriptors is not built: FeatureVector::addFeature appends in feature order and every left
// index precedes every right one, so node n's list is the left eye's list of n followed by the right eye's list of n (+ Nleft).  For a
// keyframe feature of a node both concatenated vectors hold, the reference keeps best / second best and the first index of the best
// separately for the frame's left (index < Nleft) and right candidates, and then (:373-433)
//     if (bestDist1 <= TH_LOW) { if (left ratio test) write left;  if (bestDist1R <= TH_LOW) write right; }
// so nothing happens without an open LEFT candidate within TH_LOW, the right write has no ratio test (`|| true`, :403) and does not depend
// on the left one, and one keyframe feature can hand its MapPoint to two keypoints.  Only nodes of the FRAME'S LEFT EYE can therefore match.
//   k_search_bow_two_eyes: one workgroup per search; the four node columns in LDS; the starts of the node segments of the frame's left eye
//   are collected (any order: a feature lies in one node, so nodes are independent), each 16-lane row takes segments: three binary searches
//   (keyframe left / right, frame right), then for the keyframe's left features of the node and after them its right ones, in list order,
//   the row's lanes share the frame's open candidates: left eye two smallest (distance << 16 | position) keys per lane and a DPP row
//   minimum for best and second best, right eye the smallest only.  Both eyes push into one rotation histogram (:446-468).
//   STAGE: the frame pair's descriptors (read once per keyframe feature of their node) are copied to LDS; a keyframe descriptor is read
//   once, from L2, one feature ahead of its use.  The staged block is addressed by a template parameter, never through a generic pointer.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orbx_lds_pollute.hpp"
#include "k_match_helpers.hpp"
#include "k_wave_min.hpp"
#include "orbx_device.hpp"
#include "orbx_params.hpp"

namespace orbx {

namespace {
constexpr unsigned kNoneKey = (256u << 16) | 0xFFFFu;     // bestDist = 256, no position
constexpr int kThreads = 1024;                            // 64 rows of 16 lanes
// the match table is read by 16 lanes and written by one: volatile, and typed as LDS so that no access becomes a FLAT one
typedef __attribute__((address_space(3))) volatile int LdsVolatileInt;
// [lo, hi) of `node` in a sorted node column of n entries (the maps' lower_bound walk, :432-439, meets exactly the common keys)
__device__ __forceinline__ void segmentOf(const uint32_t* col, int n, uint32_t node, int& s0, int& s1) {
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (col[mid] < node) lo = mid + 1; else hi = mid; }
    s0 = lo;
    while (lo < n && col[lo] == node) lo++;
    s1 = lo;
}
}  // namespace

// per slot of the capacity rounded up to 16: four node columns (16), the segment list (4), two match tables (8), four index columns (8),
// two bin tables (2), two flag tables (2); staged, the frame pair's descriptors (2 x 32)
size_t bowTwoEyesLdsBytes(int capacity, bool stage) { return (size_t)((capacity + 15) & ~15) * (40 + (stage ? 64 : 0)) + 64; }

// grid n_pairs; 1024 threads; dynamic LDS bowTwoEyesLdsBytes(capacity, STAGE)
template <bool STAGE>
__global__ __launch_bounds__(kThreads) void k_search_bow_two_eyes(const uint32_t* __restrict__ featNodes, const uint32_t* __restrict__ featIdx,
                                                                  const int* __restrict__ nFeat, const uint8_t* __restrict__ kfFlags,
                                                                  const Keypoint* __restrict__ kps, const uint8_t* __restrict__ desc,
                                                                  const int* __restrict__ nOut, BowTwoEyesParams p, int* __restrict__ matches,
                                                                  int* __restrict__ nMatches) {
    extern __shared__ __align__(16) uint8_t smem[];
    __shared__ int sSeg, sHist[kHistoLength], sCount;
    const int cap = p.capacity, capA = (cap + 15) & ~15, pair = blockIdx.x, tid = threadIdx.x, sub = tid & 15, row = tid >> 4;
    const long long fK = 2LL * (p.kfFirst + (long long)pair * p.kfStep), fC = 2LL * (p.curFirst + (long long)pair * p.curStep);      // left eyes; right = + 1
    uint4* sDesc = (uint4*)smem;                                     // (STAGE) [2][capA][2] the frame pair's descriptors, eye-major
    uint32_t* nodeCol = (uint32_t*)(sDesc + (STAGE ? 4 * capA : 0));  // [4][capA] node columns: keyframe left, right, frame left, right
    int* segList = (int*)(nodeCol + 4 * capA);                       // [capA] first entry of every node segment of the frame's left eye
    LdsVolatileInt* takenBy = (LdsVolatileInt*)(segList + capA);     // [2][capA] frame keypoint (eye-major) -> concatenated keyframe index whose MapPoint it got
    unsigned short* idxCol = (unsigned short*)(segList + 3 * capA);  // [4][capA] feature-index columns, as nodeCol
    uint8_t* binOf = (uint8_t*)(idxCol + 4 * capA);                  // [2][capA] rotHist bin the frame keypoint was pushed to
    uint8_t* sFlag = binOf + 2 * capA;                               // [2][capA] the keyframe pair's MapPoint flags
    const uint32_t *nodeKL = nodeCol, *nodeKR = nodeCol + capA, *nodeCL = nodeCol + 2 * capA, *nodeCR = nodeCol + 3 * capA;
    const unsigned short *idxKL = idxCol, *idxKR = idxCol + capA, *idxCL = idxCol + 2 * capA, *idxCR = idxCol + 3 * capA;
    int M[4], N[4];      // FeatureVector entries and keypoints of: keyframe left, right, frame left, right
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const long long f = (t < 2 ? fK : fC) + (t & 1);
        M[t] = max(0, min(nFeat[f], cap)); N[t] = max(0, min(nOut[f], cap));
    }
    const int NleftKF = N[0];
    const uint4 *descK = (const uint4*)(desc + fK * cap * 32), *descC = (const uint4*)(desc + fC * cap * 32);      // [2][cap][2]: the right eye follows the left
    const Keypoint *kpK = kps + fK * cap, *kpC = kps + fC * cap;                                                   // [2][cap]
    if (tid == 0) { sSeg = 0; sCount = 0; }
    if (tid < kHistoLength) sHist[tid] = 0;
#pragma unroll
    for (int t = 0; t < 4; t++) {      // (indices clamped: a corrupt FeatureVector must not index past the tables)
        const long long f = (t < 2 ? fK : fC) + (t & 1);
        const uint32_t *gNode = featNodes + f * cap, *gIdx = featIdx + f * cap;
        for (int i = tid; i < M[t]; i += kThreads) {
            nodeCol[t * capA + i] = gNode[i];
            idxCol[t * capA + i] = (unsigned short)min(gIdx[i], (uint32_t)(cap - 1));
        }
    }
    for (int i = tid; i < 2 * capA; i += kThreads) {
        const int e = i >= capA, j = i - e * capA;
        // (an index at or above its eye's count names no feature: closed as a candidate, without a MapPoint as a key)
        takenBy[i] = j < N[2 + e] ? -1 : -2; binOf[i] = 255;
        sFlag[i] = j < N[e] ? kfFlags[(2LL * pair + e) * cap + j] : (uint8_t)0;
    }
    if constexpr (STAGE) {
#pragma unroll
        for (int e = 0; e < 2; e++)
            for (int i = tid; i < 2 * N[2 + e]; i += kThreads) sDesc[2 * e * capA + i] = descC[2LL * e * cap + i];
    }
    __syncthreads();
    for (int i = tid; i < M[2]; i += kThreads)
        if (i == 0 || nodeCL[i] != nodeCL[i - 1]) segList[atomicAdd(&sSeg, 1)] = i;      // (any order: nodes are independent)
    __syncthreads();
    const int nSeg = sSeg;
    for (int s = row; s < nSeg; s += kThreads / 16) {
        const int cl0 = segList[s];
        const uint32_t node = nodeCL[cl0];
        int cl1 = cl0 + 1;
        while (cl1 < M[2] && nodeCL[cl1] == node) cl1++;
        int kl0, kl1, kr0, kr1, cr0, cr1;
        segmentOf(nodeKL, M[0], node, kl0, kl1);
        segmentOf(nodeKR, M[1], node, kr0, kr1);
        const int nKL = kl1 - kl0, nK = nKL + kr1 - kr0;
        if (nK == 0) continue;
        segmentOf(nodeCR, M[3], node, cr0, cr1);
        // vIndicesKF in list order (:297): entry t of the concatenated list is the left eye's for t < nKL, then the right eye's
        auto kfEntry = [&](int t, int& eye, int& idx) { eye = t >= nKL; idx = eye ? (int)idxKR[kr0 + t - nKL] : (int)idxKL[kl0 + t]; };
        int eyeK, idxK;
        kfEntry(0, eyeK, idxK);
        uint4 a = descK[2 * ((long long)eyeK * cap + idxK)], b = descK[2 * ((long long)eyeK * cap + idxK) + 1];
        for (int t = 0; t < nK; t++) {
            const int eye = eyeK, realIdx = idxK;
            const uint4 da = a, db = b;
            if (t + 1 < nK) {      // the next keyframe descriptor travels while this one is matched
                kfEntry(t + 1, eyeK, idxK);
                a = descK[2 * ((long long)eyeK * cap + idxK)]; b = descK[2 * ((long long)eyeK * cap + idxK) + 1];
            }
            if (!(sFlag[eye * capA + realIdx] & 1)) continue;                                   // no MapPoint, or a bad one (:303-307)
            unsigned key = kNoneKey, second = kNoneKey, keyR = kNoneKey;
            for (int c = cl0 + sub; c < cl1; c += 16) {                                         // realIdxF < F.Nleft (:347-354)
                const int f = (int)idxCL[c];
                if (takenBy[f] != -1) continue;                                                 // :343-344
                uint4 x, y;
                if constexpr (STAGE) { x = sDesc[2 * f]; y = sDesc[2 * f + 1]; }
                else { x = descC[2 * f]; y = descC[2 * f + 1]; }
                const unsigned kk = ((unsigned)hamming256(da, db, x, y) << 16) | (unsigned)(c - cl0);   // positions ascend per lane: a later equal distance never displaces
                if (kk < key) { second = key; key = kk; }
                else if (kk < second) second = kk;
            }
            for (int c = cr0 + sub; c < cr1; c += 16) {                                         // realIdxF >= F.Nleft (:356-363); bestDist2R is dead
                const int f = (int)idxCR[c];
                if (takenBy[capA + f] != -1) continue;
                uint4 x, y;
                if constexpr (STAGE) { x = sDesc[2 * (capA + f)]; y = sDesc[2 * (capA + f) + 1]; }
                else { x = descC[2 * ((long long)cap + f)]; y = descC[2 * ((long long)cap + f) + 1]; }
                const unsigned kk = ((unsigned)hamming256(da, db, x, y) << 16) | (unsigned)(c - cr0);
                if (kk < keyR) keyR = kk;
            }
            const unsigned best = rowMin16(key);
            const int bestDist1 = (int)(best >> 16);
            if (bestDist1 > p.thLow) continue;                                                  // :373 (thLow <= 255: an open left candidate exists)
            const unsigned best2 = rowMin16(key == best ? second : key), bestR = rowMin16(keyR);
            const int bestDist2 = (int)(best2 >> 16), bestDist1R = (int)(bestR >> 16);
            const bool left = (float)bestDist1 < __fmul_rn(p.nnRatio, (float)bestDist2), right = bestDist1R <= p.thLow;   // :375, :403
            if (sub == 0 && (left || right)) {
                const int from = eye ? NleftKF + realIdx : realIdx;                             // the index space of pKF->GetMapPointMatches()
                const float angleK = kpK[(long long)eye * cap + realIdx].angle;
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    if (!(e ? right : left)) continue;
                    const int f = e ? (int)idxCR[cr0 + (int)(bestR & 0xFFFFu)] : (int)idxCL[cl0 + (int)(best & 0xFFFFu)];
                    takenBy[e * capA + f] = from;                                               // vpMapPointMatches[bestIdxF / bestIdxFR] = pMP
                    if (p.checkOrientation) {                                                   // :384-401, :411-428
                        int bin = rotationBin(angleK, kpC[(long long)e * cap + f].angle);
                        bin = min(max(bin, 0), kHistoLength - 1);                               // (the reference asserts it; an angle outside [0, 360) must not index past the table)
                        binOf[e * capA + f] = (uint8_t)bin;
                        atomicAdd(&sHist[bin], 1);
                    }
                }
            }
            __builtin_amdgcn_wave_barrier();      // the row's next keyframe feature must see the closed keypoints (same wave: LDS is in order)
        }
    }
    __syncthreads();
    unsigned dropBins = 0u;
    if (p.checkOrientation) {                                                                   // ComputeThreeMaxima (:2303-2344), then :446-468
        const ThreeMaxima top3 = computeThreeMaxima(sHist);
        for (int i = 0; i < kHistoLength; i++)
            if (i != top3.ind1 && i != top3.ind2 && i != top3.ind3) dropBins |= 1u << i;
    }
    int mine = 0;
#pragma unroll
    for (int e = 0; e < 2; e++) {
        int* out = matches + (2LL * pair + e) * cap;
        for (int i = tid; i < cap; i += kThreads) {
            int m = i < N[2 + e] ? takenBy[e * capA + i] : -1;
            const int bin = binOf[e * capA + i];
            if (m >= 0 && bin < kHistoLength && ((dropBins >> bin) & 1u)) m = -1;
            out[i] = m;
            mine += m >= 0;
        }
    }
    if (mine) atomicAdd(&sCount, mine);
    __syncthreads();
    if (tid == 0) nMatches[pair] = sCount;
}

void launchSearchBowTwoEyes(hipStream_t st, const uint32_t* featNodes, const uint32_t* featIdx, const int* nFeat, const uint8_t* kfFlags,
                            const Keypoint* kps, const uint8_t* desc, const int* nOut, const BowTwoEyesParams& p, bool stage, int* matches,
                            int* nMatches, int nPairs, LdsPolluter pollute) {
    pollute(st);
    if (stage)
        hipLaunchKernelGGL(k_search_bow_two_eyes<true>, dim3(nPairs), dim3(kThreads), bowTwoEyesLdsBytes(p.capacity, true), st, featNodes, featIdx,
                           nFeat, kfFlags, kps, desc, nOut, p, matches, nMatches);
    else
        hipLaunchKernelGGL(k_search_bow_two_eyes<false>, dim3(nPairs), dim3(kThreads), bowTwoEyesLdsBytes(p.capacity, false), st, featNodes, featIdx,
                           nFeat, kfFlags, kps, desc, nOut, p, matches, nMatches);
}

}  // namespace orbx
