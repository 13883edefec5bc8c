// k_triangulate_match.hip — the mapping thread's matcher: ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo,
// bCoarse) (reference src/ORBmatcher.cc:965-1206; LocalMapping::CreateNewMapPoints, src/LocalMapping.cc:456-463, once per neighbour keyframe)
// for one-camera keyframes (NLeft == -1, no mpCamera2 on either side) with Pinhole::epipolarConstrain (src/CameraModels/Pinhole.cpp:122-144),
// on what ComputeBoW, the Frame finishing and the stereo matching left on the device.
//
// The two FeatureVectors are walked in step and only features of a common vocabulary node meet (:1025-1172).  A keyframe-1 feature WITHOUT a
// MapPoint (:1033-1039) scans keyframe 2's features of the node in list order; a candidate is dropped if it holds a MapPoint (:1067), by the
// stereo filter (:1070-1074), if dist > TH_LOW or dist > bestDist with bestDist starting AT TH_LOW (:1057, :1080), inside the epipole's disc
// when neither feature is stereo (:1089-1097), and if it misses the epipolar line unless bCoarse (:1132).  vbMatched2 is created (:1011) and
// tested (:1067) but NEVER SET here (compare :911 of SearchByBoW): no keyframe-1 feature closes a candidate for another one, and none of the
// filters but the running bestDist depends on the scan.  So every keyframe-1 feature is a search of its own whose result is, among the
// candidates that pass the filters with dist <= TH_LOW, the smallest distance and of equal smallest distances the LAST in list order (:1080
// lets an equal distance replace the holder: the opposite tie rule of k_search_bow).  Several features may choose the same keypoint of keyframe 2.
//   k_search_triangulation: one workgroup per keyframe pair; the node and index columns of both FeatureVectors, both flag tables and keyframe
//   2's positions and octaves in LDS.  A thread per keyframe-1 entry finds keyframe 2's segment of its node (two binary searches; the range
//   replaces the node in place).  Then a 16-lane row per keyframe-1 FEATURE (not per node segment: there is no chain to respect): its lanes
//   share the node's candidates, Hamming distance by v_bcnt, geometry only for candidates within th_low, ONE (distance << 16 | 0xFFFF - position)
//   key per lane and one 16-lane DPP minimum per feature.  The rotation histogram (:1147-1157) is 30 LDS counters, ComputeThreeMaxima and
//   the removal (:1174-1193) close the search, and vMatchedPairs (:1195-1203) is compacted in keypoint order by a workgroup scan.
//   STAGE: keyframe 2's descriptors (each read once per keyframe-1 feature of its node) are copied to LDS; keyframe 1's are read once from global.
//   Every LDS table is typed as LDS: no generic pointer, no FLAT instruction.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orbx_lds_pollute.hpp"
#include "k_match_helpers.hpp"
#include "k_wave_min.hpp"
#include "orbx_device.hpp"
#include "orbx_params.hpp"

namespace orbx {

namespace {
constexpr unsigned kNoneKey = 0xFFFFFFFFu;                // no candidate passed
constexpr int kThreads = 1024;                            // 64 rows of 16 lanes
constexpr int kWaves = kThreads / 64;
typedef uint32_t U4 __attribute__((ext_vector_type(4)));      // (the compiler's own vectors: HIP's uint4 / float2 classes cannot live behind an address space)
typedef float F2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) U4 LdsU4;
typedef __attribute__((address_space(3))) F2 LdsF2;
typedef __attribute__((address_space(3))) uint32_t LdsU32;
typedef __attribute__((address_space(3))) int LdsInt;
typedef __attribute__((address_space(3))) unsigned short LdsU16;
typedef __attribute__((address_space(3))) uint8_t LdsU8;
}  // namespace

// per slot of the capacity rounded up to 16: keyframe 2's positions (8), two node columns (8; keyframe 1's becomes the segment ranges), the
// match table (4), two index columns (4), two flag tables, keyframe 2's octaves and the bins (4); staged, keyframe 2's descriptors (32)
size_t triMatchLdsBytes(int capacity, bool stage) { return (size_t)((capacity + 15) & ~15) * (28 + (stage ? 32 : 0)) + 64; }

// grid n_pairs; 1024 threads; dynamic LDS triMatchLdsBytes(capacity, STAGE)
template <bool STAGE>
__global__ __launch_bounds__(kThreads) void k_search_triangulation(const uint32_t* __restrict__ featNodes, const uint32_t* __restrict__ featIdx,
                                                                   const int* __restrict__ nFeat, const uint8_t* __restrict__ mpFlags1,
                                                                   const uint8_t* __restrict__ mpFlags2, const Keypoint* __restrict__ kps,
                                                                   const float* __restrict__ uRight, const uint8_t* __restrict__ desc,
                                                                   const int* __restrict__ nOut, const float* __restrict__ f12,
                                                                   const float* __restrict__ epipole, TriMatchParams p,
                                                                   int* __restrict__ matches12, int* __restrict__ pairs, int* __restrict__ nMatches) {
    extern __shared__ __align__(16) uint8_t smem[];
    __shared__ int sHist[kHistoLength], sWave[kWaves];
    __shared__ float sDisc[kMaxLevels];       // 100 * mvScaleFactors[octave] (:1093)
    __shared__ double sGate[kMaxLevels];      // 3.84 * mvLevelSigma2[octave], in double (Pinhole.cpp:143)
    const int cap = p.capacity, capA = (cap + 15) & ~15, pair = blockIdx.x, tid = threadIdx.x, sub = tid & 15, row = tid >> 4;
    const long long f1 = p.kf1First + (long long)pair * p.kf1Step, f2 = p.kf2First + (long long)pair * p.kf2Step;
    LdsU4* sDesc2 = (LdsU4*)smem;                                   // (STAGE) [capA][2] keyframe 2's descriptors
    LdsF2* sPos2 = (LdsF2*)(sDesc2 + (STAGE ? 2 * capA : 0));       // [capA] keyframe 2's mvKeysUn[i].pt
    LdsU32* segK = (LdsU32*)(sPos2 + capA);                         // [capA] node column of keyframe 1's FeatureVector, then c0 | c1 << 16 of keyframe 2's segment
    LdsU32* nodeC = segK + capA;                                    // [capA] node column of keyframe 2's FeatureVector
    LdsInt* m12 = (LdsInt*)(nodeC + capA);                          // [capA] vMatches12
    LdsU16* idxK = (LdsU16*)(m12 + capA);                           // [capA] feature-index column of keyframe 1's FeatureVector
    LdsU16* idxC = idxK + capA;                                     // [capA] ... of keyframe 2's
    LdsU8* flag1 = (LdsU8*)(idxC + capA);                           // [capA] bit 0: holds a MapPoint, bit 1: mvuRight >= 0
    LdsU8* flag2 = flag1 + capA;                                    // [capA] ... of keyframe 2
    LdsU8* oct2 = flag2 + capA;                                     // [capA] keyframe 2's octaves, clamped to the tables
    LdsU8* binOf = oct2 + capA;                                     // [capA] rotHist bin keyframe 1's keypoint was pushed to
    const int M1 = max(0, min(nFeat[f1], cap)), M2 = max(0, min(nFeat[f2], cap));
    const int N1 = max(0, min(nOut[f1], cap)), N2 = max(0, min(nOut[f2], cap));
    const uint32_t *gNode1 = featNodes + f1 * cap, *gNode2 = featNodes + f2 * cap, *gIdx1 = featIdx + f1 * cap, *gIdx2 = featIdx + f2 * cap;
    const U4 *desc1 = (const U4*)(desc + f1 * cap * 32), *desc2 = (const U4*)(desc + f2 * cap * 32);
    const Keypoint *kp1 = kps + f1 * cap, *kp2 = kps + f2 * cap;
    const float* F = f12 + (long long)pair * 9;
    const float F00 = F[0], F01 = F[1], F02 = F[2], F10 = F[3], F11 = F[4], F12 = F[5], F20 = F[6], F21 = F[7], F22 = F[8];
    const float epx = epipole[2LL * pair], epy = epipole[2LL * pair + 1];
    if (tid < kHistoLength) sHist[tid] = 0;
    if (tid < kMaxLevels) {
        const int l = min(tid, p.nlevels - 1);
        sDisc[tid] = __fmul_rn(100.0f, p.scale[l]);
        sGate[tid] = 3.84 * (double)p.sigma2[l];
    }
    // (indices clamped: a corrupt FeatureVector must not index past the tables)
    for (int i = tid; i < M1; i += kThreads) { segK[i] = gNode1[i]; idxK[i] = (unsigned short)min(gIdx1[i], (uint32_t)(cap - 1)); }
    for (int i = tid; i < M2; i += kThreads) { nodeC[i] = gNode2[i]; idxC[i] = (unsigned short)min(gIdx2[i], (uint32_t)(cap - 1)); }
    for (int i = tid; i < capA; i += kThreads) {
        m12[i] = -1; binOf[i] = 255;
        // (an index at or above the frame's count names no feature: it reads as "holds a MapPoint", which skips a key entry and drops a candidate)
        flag1[i] = i < N1 ? (uint8_t)((mpFlags1[(long long)pair * cap + i] & 1) | (uRight && uRight[f1 * cap + i] >= 0.0f ? 2 : 0)) : (uint8_t)1;
        flag2[i] = i < N2 ? (uint8_t)((mpFlags2[(long long)pair * cap + i] & 1) | (uRight && uRight[f2 * cap + i] >= 0.0f ? 2 : 0)) : (uint8_t)1;
        F2 pt = {0.0f, 0.0f};
        int o = 0;
        if (i < N2) { pt.x = kp2[i].x; pt.y = kp2[i].y; o = min(max(kp2[i].octave, 0), p.nlevels - 1); }
        sPos2[i] = pt; oct2[i] = (uint8_t)o;
    }
    if constexpr (STAGE)
        for (int i = tid; i < 2 * N2; i += kThreads) sDesc2[i] = desc2[i];
    __syncthreads();
    // keyframe 2's segment [c0, c1) of every keyframe-1 entry's node (the maps' walk in step, :1025-1172, meets exactly the common keys)
    for (int i = tid; i < M1; i += kThreads) {
        const uint32_t node = segK[i];
        int lo = 0, hi = M2;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (nodeC[mid] < node) lo = mid + 1; else hi = mid; }
        const int c0 = lo;
        hi = M2;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (nodeC[mid] <= node) lo = mid + 1; else hi = mid; }
        segK[i] = (uint32_t)c0 | ((uint32_t)lo << 16);
    }
    __syncthreads();
    for (int k = row; k < M1; k += kThreads / 16) {
        const int idx1 = (int)idxK[k];
        const unsigned fl1 = flag1[idx1], range = segK[k];
        const int c0 = (int)(range & 0xFFFFu), c1 = (int)(range >> 16);
        if ((fl1 & 1u) || c0 == c1) continue;                                                   // holds a MapPoint (:1033-1039)
        const bool stereo1 = fl1 & 2u;
        if (p.onlyStereo && !stereo1) continue;                                                 // :1041-1045
        const U4 da = desc1[2 * idx1], db = desc1[2 * idx1 + 1];
        const float x1 = kp1[idx1].x, y1 = kp1[idx1].y;
        // the epipolar line in keyframe 2, l = x1' F12 (Pinhole.cpp:130-136): every product and sum rounded on its own
        const float la = __fadd_rn(__fadd_rn(__fmul_rn(x1, F00), __fmul_rn(y1, F10)), F20);
        const float lb = __fadd_rn(__fadd_rn(__fmul_rn(x1, F01), __fmul_rn(y1, F11)), F21);
        const float lc = __fadd_rn(__fadd_rn(__fmul_rn(x1, F02), __fmul_rn(y1, F12)), F22);
        const float den = __fadd_rn(__fmul_rn(la, la), __fmul_rn(lb, lb));
        unsigned key = kNoneKey;
        for (int c = c0 + sub; c < c1; c += 16) {                                               // f2it->second in list order (:1060)
            const int idx2 = (int)idxC[c];
            const unsigned fl2 = flag2[idx2];
            if (fl2 & 1u) continue;                                                             // holds a MapPoint (:1067; vbMatched2 is never set)
            const bool stereo2 = fl2 & 2u;
            if (p.onlyStereo && !stereo2) continue;                                             // :1070-1074
            U4 x, y;
            if constexpr (STAGE) { x = sDesc2[2 * idx2]; y = sDesc2[2 * idx2 + 1]; }
            else { x = desc2[2 * idx2]; y = desc2[2 * idx2 + 1]; }
            const int dist = hamming256(da, db, x, y);
            if (dist > p.thLow) continue;                                                       // :1080 (dist > bestDist is the minimum below)
            const F2 pt = sPos2[idx2];
            const int o = oct2[idx2];
            if (!stereo1 && !stereo2) {                                                         // :1089-1097
                const float ex = __fsub_rn(epx, pt.x), ey = __fsub_rn(epy, pt.y);
                if (__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)) < sDisc[o]) continue;
            }
            if (!p.coarse) {                                                                    // :1132, Pinhole.cpp:134-143
                const float num = __fadd_rn(__fadd_rn(__fmul_rn(la, pt.x), __fmul_rn(lb, pt.y)), lc);
                if (den == 0.0f) continue;
                const float dsqr = __fdiv_rn(__fmul_rn(num, num), den);
                if (!((double)dsqr < sGate[o])) continue;
            }
            const unsigned kk = ((unsigned)dist << 16) | (0xFFFFu - (unsigned)(c - c0));        // of equal distances the LAST position wins (:1080)
            key = kk < key ? kk : key;
        }
        const unsigned best = rowMin16(key);
        if (best == kNoneKey || sub != 0) continue;
        const int bestIdx2 = (int)idxC[c0 + (int)(0xFFFFu - (best & 0xFFFFu))];
        m12[idx1] = bestIdx2;                                                                   // :1144
        if (p.checkOrientation) {                                                               // :1147-1157
            int bin = rotationBin(kp1[idx1].angle, kp2[bestIdx2].angle);
            bin = min(max(bin, 0), kHistoLength - 1);                                           // (the reference asserts it; an angle outside [0, 360) must not index past the table)
            binOf[idx1] = (uint8_t)bin;
            atomicAdd(&sHist[bin], 1);
        }
    }
    __syncthreads();
    unsigned dropBins = 0u;
    if (p.checkOrientation) {                                                                   // ComputeThreeMaxima (:2303-2344), then :1174-1193
        const ThreeMaxima top3 = computeThreeMaxima(sHist);
        for (int i = 0; i < kHistoLength; i++)
            if (i != top3.ind1 && i != top3.ind2 && i != top3.ind3) dropBins |= 1u << i;
    }
    // vMatches12 and vMatchedPairs in increasing keypoint index (:1195-1203): a ballot inside the wave, the waves' counts through LDS
    int* out = matches12 + (long long)pair * cap;
    int* outPairs = pairs + 2LL * pair * cap;
    const int wave = tid >> 6, lane = tid & 63;
    int written = 0;
    for (int base = 0; base < cap; base += kThreads) {
        const int i = base + tid;
        int m = i < N1 ? m12[i] : -1;
        if (m >= 0) { const int bin = binOf[i]; if (bin < kHistoLength && ((dropBins >> bin) & 1u)) m = -1; }
        if (i < cap) out[i] = m;
        const unsigned long long vote = __ballot(m >= 0);
        if (lane == 0) sWave[wave] = __popcll(vote);
        __syncthreads();
        int before = written, all = written;
        for (int w = 0; w < kWaves; w++) { const int n = sWave[w]; all += n; before += w < wave ? n : 0; }
        if (m >= 0) {
            const int slot = before + __popcll(vote & ((1ull << lane) - 1ull));
            outPairs[2 * slot] = i; outPairs[2 * slot + 1] = m;
        }
        written = all;
        __syncthreads();
    }
    if (tid == 0) nMatches[pair] = written;
}

void launchSearchTriangulation(hipStream_t st, const uint32_t* featNodes, const uint32_t* featIdx, const int* nFeat, const uint8_t* mpFlags1,
                               const uint8_t* mpFlags2, const Keypoint* kps, const float* uRight, const uint8_t* desc, const int* nOut,
                               const float* f12, const float* epipole, const TriMatchParams& p, bool stage, int* matches12, int* pairs,
                               int* nMatches, int nPairs, LdsPolluter pollute) {
    pollute(st);
    if (stage)
        hipLaunchKernelGGL(k_search_triangulation<true>, dim3(nPairs), dim3(kThreads), triMatchLdsBytes(p.capacity, true), st, featNodes, featIdx,
                           nFeat, mpFlags1, mpFlags2, kps, uRight, desc, nOut, f12, epipole, p, matches12, pairs, nMatches);
    else
        hipLaunchKernelGGL(k_search_triangulation<false>, dim3(nPairs), dim3(kThreads), triMatchLdsBytes(p.capacity, false), st, featNodes, featIdx,
                           nFeat, mpFlags1, mpFlags2, kps, uRight, desc, nOut, f12, epipole, p, matches12, pairs, nMatches);
}

}  // namespace orbx
