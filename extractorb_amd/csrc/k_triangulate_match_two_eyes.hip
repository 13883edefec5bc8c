// k_triangulate_match_two_eyes.hip - ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, bCoarse) for TWO-CAMERA
// keyframes (reference src/ORBmatcher.cc:965-1206 with mpCamera2 on both sides: :994-1004 and :1099-1129; a KannalaBrandt8 pair), the twin of
// k_triangulate_match.hip, and the two kernels that expose its camera math on its own (k_kb8_unproject, k_kb8_triangulate).  What differs from
// the one-camera search:
//   * a keyframe X is batch frames 2X (left eye: mvKeys, the first NLeft rows of mDescriptors) and 2X + 1 (right eye: mvKeysRight), with the
//     FeatureVectors ComputeBoW wrote PER EYE, as k_bow_match_two_eyes.hip: a node's list of the stacked mFeatVec is the left eye's list
//     followed by the right eye's (+ NLeft), a node is common when either eye of keyframe 1 and either eye of keyframe 2 hold it, and every
//     index that leaves the kernel is in the stacked numbering;
//   * kp1 / kp2 are the RAW keypoints of the eye the index falls in (:1048-1050, :1083-1085), bRight is idx >= NLeft;
//   * bStereo1 and bStereo2 are false by construction (:1041, :1070: `!mpCamera2 && ...`): bOnlyStereo = true skips every keyframe-1 feature
//     and the search returns no match; the epipole's disc (:1089) is not tested; F12 and the epipole are not inputs;
//   * the geometric test is pCamera1->epipolarConstrain(pCamera2, kp1, kp2, R12, t12, sigma1, sigma2) = KannalaBrandt8::TriangulateMatches
//     (...) > 0.0001f (k_camera_kb8_unproject.hpp) with the cameras and (R12, t12) of the eye combination (:995-1003).  pCamera1 / pCamera2 /
//     R12 / t12 are REASSIGNED on every candidate (:1099-1129): that they persist across iterations changes nothing; bCoarse accepts without
//     the test (:1132).
// As there, vbMatched2 is never set: every keyframe-1 feature is a search of its own whose result is, among the candidates without a MapPoint
// that pass the test with dist <= TH_LOW, the smallest distance and of equal distances the LAST in list order.
//   k_search_triangulation_two_eyes: one workgroup per keyframe pair, every table typed as LDS (no FLAT).
//   STAGING, behind one barrier: lanes 0 .. 3 each compute one eye combination - the two eyes' (R, t) from the keyframes' poses and mTlr
//   (fuseTwoEyesRigElement of k_rig_two_eyes.hpp, shared with Fuse), R12 = R1*R2.t() and t12 = R1*(-R2.t()*t2) + t1 as gemmRow rows in the
//   reference's association order, then R21 = R12.t() and t21 = -R21*t12 ONCE per combination; sixteen lanes copy the cameras, sixteen the
//   5.991 * mvLevelSigma2[l] gates (double); every keypoint of keyframe 2 is UNPROJECTED ONCE with its eye's camera into LDS (8 bytes per
//   slot) beside the FeatureVector columns and the flags.  A second barrier follows the segment searches, as in the one-camera kernel.
//   SEARCH: a 16-lane row per keyframe-1 feature; its ray is unprojected once per row.  The lanes share the node's candidates (keyframe 2's
//   left list, then its right list) and rank them by the (distance << 16 | 0xFFFF - position) key FIRST; the geometry is evaluated only in
//   increasing key order: in each round every lane tests its own best untested candidate that is still better than the row's best PASSING
//   key, the row's minimum over the passing lanes (rowMin16) tightens that bound, and the row ends when no lane holds a better untested
//   candidate.  Sixteen tests run side by side at the cost of one and the result is the smallest passing key: the reference's.  In the
//   FIRST round every lane tests its best candidate whatever the other lanes hold, so a candidate worse than one that passes in the same
//   round IS triangulated; only from the second round on does the bound skip anything.  With lists of at most 16 candidates that is nearly
//   every candidate within th_low: the counter (g_triTwoEyesStats, a debug option) does not favour this form over the strictly sequential
//   order in calls, only in rounds (docs/history/r18_two_eyes_triangulation.md).
//   Histogram, ComputeThreeMaxima, removal and the compaction of vMatchedPairs (stacked numbering, increasing) as the one-camera kernel.
// The statement is four functions, triTwoEyesStage, triTwoEyesLoadSlot, triTwoEyesSegments and triTwoEyesRow; the kernel is the four around
// its barriers, with the column copies and the closing scan.  The
// CPU suite compiles them for the HOST (tests/cpp/triangulation_two_eyes_host_check.cpp behind tests/cpp/host_shim/
// triangulation_two_eyes_shim.h, which defines ORBX_HOST_ROW: a row is one lane there and LDS is memory).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orbx_lds_pollute.hpp"
#include "k_camera_kb8_unproject.hpp"
#include "k_lds_vec.hpp"
#include "k_match_helpers.hpp"
#include "k_rig_two_eyes.hpp"
#include "orbx_device.hpp"
#include "orbx_params.hpp"

#ifdef ORBX_HOST_ROW
namespace orbx { typedef LdsU4 TriU4; constexpr int kTriRowLanes = 1; }
#else
#include "k_wave_min.hpp"
namespace orbx { typedef LdsU4 TriU4; constexpr int kTriRowLanes = 16; }
#endif

namespace orbx {

namespace {
constexpr unsigned kTriNoneKey = 0xFFFFFFFFu;             // no candidate
constexpr int kTriThreads = 512;                          // 32 rows of 16 lanes (the triangulation's registers: two waves per SIMD)
constexpr int kTriWaves = kTriThreads / 64;
constexpr int kTriRelFloats = 12;                         // one eye combination: R12 (row-major) at 0..8, t21 at 9..11
}  // namespace

// The LDS tables of a keyframe pair, as ONE base and the rounded capacity (eleven table pointers kept live across the row loop cost eleven
// scalar registers; an offset that is a multiple of capA costs none).  `base` is the first byte after the staged descriptors; eye e of a
// table is at [e * capA + i].
struct TriTwoEyesTables {
    ORBX_LDS uint8_t* base;
    int capA;
    __device__ ORBX_LDS TriU4* desc2() const { return (ORBX_LDS TriU4*)(base - 64 * capA); }                 // (STAGE) [2][capA][2] keyframe 2's descriptors
    __device__ ORBX_LDS float* ray2() const { return (ORBX_LDS float*)base; }                                // [2][capA][2] keyframe 2's rays (x, y; z = 1)
    // [2][capA] node column of keyframe 1's FeatureVectors, then c0 | c1 << 16 of the node in keyframe 2's LEFT column / RIGHT column
    __device__ ORBX_LDS uint32_t* segL() const { return (ORBX_LDS uint32_t*)(base + 16 * capA); }
    __device__ ORBX_LDS uint32_t* segR() const { return (ORBX_LDS uint32_t*)(base + 24 * capA); }
    __device__ ORBX_LDS uint32_t* node2() const { return (ORBX_LDS uint32_t*)(base + 32 * capA); }           // [2][capA] node columns of keyframe 2's FeatureVectors
    __device__ ORBX_LDS int* m12() const { return (ORBX_LDS int*)(base + 40 * capA); }                       // [2][capA] vMatches12 (stacked index of keyframe 2)
    __device__ ORBX_LDS unsigned short* idx1() const { return (ORBX_LDS unsigned short*)(base + 48 * capA); }      // [2][capA] feature-index columns of keyframe 1's FeatureVectors
    __device__ ORBX_LDS unsigned short* idx2() const { return (ORBX_LDS unsigned short*)(base + 52 * capA); }      // ... of keyframe 2's
    __device__ ORBX_LDS uint8_t* flag1() const { return base + 56 * capA; }                                  // [2][capA] bit 0: holds a MapPoint
    __device__ ORBX_LDS uint8_t* flag2() const { return base + 58 * capA; }
    __device__ ORBX_LDS uint8_t* binOf() const { return base + 60 * capA; }                                  // [2][capA] rotHist bin keyframe 1's keypoint was pushed to
};

// LDS of a pair, capacity counted over BOTH eyes: per slot of the per-eye capacity rounded up to 16 and per eye, keyframe 2's ray (8), three
// node / segment columns (12), the match table (4), two index columns (4), two flag tables and the bins (3) = 31; staged, keyframe 2's
// descriptors (32).  1024 covers the static tables (four eye combinations, cameras, gates, histogram, scan counts).
//   62 * ((capacity + 15) & ~15) + 1024 <= 163 328  (capacity <= 2608 per eye; 2 x 1302 fit);  staged: 126 * ... (capacity <= 1280 per eye)
size_t triMatchTwoEyesLdsBytes(int capacity, bool stage) { return (size_t)((capacity + 15) & ~15) * 2 * (31 + (stage ? 32 : 0)) + 1024; }

// before the first barrier: the four eye combinations (lanes 0 .. 3), the cameras (64 .. 79), the gates (128 .. 128 + kMaxLevels)
//   sRel[4 * kTriRelFloats]: combination c = eye1 * 2 + eye2;  sCam[16];  sGate[kMaxLevels]
__device__ __forceinline__ void triTwoEyesStage(int tid, const float* T1, const float* T2, const TriMatchTwoEyesParams& p, float* sRel,
                                                float* sCam, double* sGate) {
    if (tid < 4) {
        const int eye1 = tid >> 1, eye2 = tid & 1;
        float E1[12], E2[12];      // mR | mt of the eye: GetRotation / GetTranslation or GetRightRotation / GetRightTranslation
        for (int j = 0; j < 12; j++) {
            E1[j] = fuseTwoEyesRigElement(T1, p.tlr, eye1 * kRigEyeFloats + j);
            E2[j] = fuseTwoEyesRigElement(T2, p.tlr, eye2 * kRigEyeFloats + j);
        }
        const float t2[3] = {E2[9], E2[10], E2[11]};
        float R12[9], inner[3], t12[3];
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) {                                                     // R1 * R2.t() (:995-998)
                const float col[3] = {E2[3 * c], E2[3 * c + 1], E2[3 * c + 2]};
                R12[3 * r + c] = gemmRow(E1[3 * r], E1[3 * r + 1], E1[3 * r + 2], col, 1.0, 0.f, false);
            }
        for (int r = 0; r < 3; r++) inner[r] = gemmRow(E2[r], E2[3 + r], E2[6 + r], t2, -1.0, 0.f, false);          // -R2.t() * t2
        for (int r = 0; r < 3; r++) t12[r] = gemmRow(E1[3 * r], E1[3 * r + 1], E1[3 * r + 2], inner, 1.0, E1[9 + r], true);      // R1 * (...) + t1 (:1000-1003)
        Kb8Relative q;
        kb8RelativeFrom(R12, t12, q);
        for (int j = 0; j < 9; j++) sRel[tid * kTriRelFloats + j] = q.R12[j];
        for (int j = 0; j < 3; j++) sRel[tid * kTriRelFloats + 9 + j] = q.t21[j];
    } else if (tid >= 64 && tid < 80) {
        sCam[tid - 64] = p.cam[(tid - 64) >> 3][tid & 7];
    } else if (tid >= 128 && tid < 128 + kMaxLevels) {
        sGate[tid - 128] = 5.991 * (double)p.sigma2[min(tid - 128, p.nlevels - 1)];            // the float promoted, the product in double
    }
}

// before the first barrier: slot s = e * capA + i of the per-keypoint tables (flags, the empty match table, keyframe 2's ray); n2 = keyframe
// 2's keypoints in eye e.  An index at or above the eye's count names no feature: a candidate with one reads as "holds a MapPoint" and is
// dropped (keyframe 1's side of the rule is the kernel's, behind this call: the signature is the host check's)
__device__ __forceinline__ void triTwoEyesLoadSlot(int s, const TriTwoEyesTables& T, int capA, int cap, int pair, int n2,
                                                   const uint8_t* __restrict__ mpFlags1, const uint8_t* __restrict__ mpFlags2,
                                                   const Keypoint* __restrict__ kp2, const TriMatchTwoEyesParams& p) {
    const int e = s >= capA, i = s - e * capA;
    T.m12()[s] = -1; T.binOf()[s] = 255;
    T.flag1()[s] = i < cap ? (uint8_t)(mpFlags1[(2LL * pair + e) * cap + i] & 1) : (uint8_t)1;
    T.flag2()[s] = i < n2 ? (uint8_t)(mpFlags2[(2LL * pair + e) * cap + i] & 1) : (uint8_t)1;
    float rx = 0.0f, ry = 0.0f;
    if (i < n2 && !p.coarse) {                                                                  // pCamera2->unproject(kp2.pt), once per keypoint
        float k2[8];
#pragma unroll
        for (int a = 0; a < 8; a++) k2[a] = e ? p.cam[1][a] : p.cam[0][a];
        kb8Unproject(k2, kp2[(long long)e * cap + i].x, kp2[(long long)e * cap + i].y, rx, ry);
    }
    T.ray2()[2 * s] = rx; T.ray2()[2 * s + 1] = ry;
}

// between the barriers: entry i of eye e of keyframe 1's FeatureVectors finds its node's segments in keyframe 2's two columns
__device__ __forceinline__ void triTwoEyesSegments(int slot, const TriTwoEyesTables& T, int capA, int M2L, int M2R) {
    const uint32_t node = T.segL()[slot];
    uint32_t out[2];
    for (int e = 0; e < 2; e++) {
        const ORBX_LDS uint32_t* col = T.node2() + e * capA;
        const int M = e ? M2R : M2L;
        int lo = 0, hi = M;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (col[mid] < node) lo = mid + 1; else hi = mid; }
        const int c0 = lo;
        hi = M;
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (col[mid] <= node) lo = mid + 1; else hi = mid; }
        out[e] = (uint32_t)c0 | ((uint32_t)lo << 16);
    }
    T.segL()[slot] = out[0]; T.segR()[slot] = out[1];
}

// after the second barrier: lane `sub` of the row of entry k (0 .. M1L + M1R: the left eye's entries, then the right eye's) of keyframe 1.
// kp1 / kp2 / desc1 / desc2g: the keyframe's two eyes, [2][cap].  nCalls / nWithin: this lane's triangulations and candidates within th_low.
template <bool STAGE>
__device__ __forceinline__ void triTwoEyesRow(int k, int sub, const TriTwoEyesTables& T, int capA, int cap, int M1L, int nLeft2,
                                              const Keypoint* __restrict__ kp1, const Keypoint* __restrict__ kp2,
                                              const TriU4* __restrict__ desc1, const TriU4* __restrict__ desc2g, const TriMatchTwoEyesParams& p,
                                              const float* sRel, const float* sCam, const double* sGate, int* sHist, int& nCalls, int& nWithin) {
    const int eye1 = k >= M1L, slot = eye1 * capA + (k - eye1 * M1L);
    const int idx1 = (int)T.idx1()[slot];
    const unsigned rangeL = T.segL()[slot], rangeR = T.segR()[slot];
    const int a0 = (int)(rangeL & 0xFFFFu), nL = (int)(rangeL >> 16) - a0, b0 = (int)(rangeR & 0xFFFFu), nC = nL + (int)(rangeR >> 16) - b0;
    if ((T.flag1()[eye1 * capA + idx1] & 1u) || nC == 0) return;                                  // holds a MapPoint (:1033-1039)
    const TriU4 da = desc1[2 * ((long long)eye1 * cap + idx1)], db = desc1[2 * ((long long)eye1 * cap + idx1) + 1];
    const Keypoint& K1 = kp1[(long long)eye1 * cap + idx1];                                     // mvKeys or mvKeysRight (:1048-1050)
    const float u1 = K1.x, v1 = K1.y;
    float k1[8], r1x = 0.f, r1y = 0.f;
    double gate1 = 0.0;
    if (!p.coarse) {
#pragma unroll
        for (int a = 0; a < 8; a++) k1[a] = sCam[eye1 * 8 + a];
        kb8Unproject(k1, u1, v1, r1x, r1y);                                                     // once per row
        gate1 = sGate[min(max(K1.octave, 0), p.nlevels - 1)];
    }
    // position t of the node's list in keyframe 2: the left eye's entries, then the right eye's
    auto candidate = [&](int t, int& eye2, int& idx2) { eye2 = t >= nL; idx2 = (int)T.idx2()[eye2 ? capA + b0 + t - nL : a0 + t]; };
    unsigned bestPass = kTriNoneKey, lowBound = 1u;
    bool first = true;
    for (;;) {
        // this lane's smallest key not yet tested (f2it->second in list order, :1060; of equal distances the LAST position wins, :1080)
        unsigned next = kTriNoneKey;
        if (lowBound != kTriNoneKey)
            for (int t = sub; t < nC; t += kTriRowLanes) {
                int eye2, idx2;
                candidate(t, eye2, idx2);
                if (T.flag2()[eye2 * capA + idx2] & 1u) continue;                                 // holds a MapPoint (:1067; vbMatched2 is never set)
                TriU4 x, y;
                if constexpr (STAGE) { x = T.desc2()[2 * (eye2 * capA + idx2)]; y = T.desc2()[2 * (eye2 * capA + idx2) + 1]; }
                else { x = desc2g[2 * ((long long)eye2 * cap + idx2)]; y = desc2g[2 * ((long long)eye2 * cap + idx2) + 1]; }
                const int dist = hamming256(da, db, x, y);
                if (dist > p.thLow) continue;                                                   // :1080
                if (first) nWithin++;
                const unsigned kk = ((unsigned)dist << 16) | (0xFFFFu - (unsigned)t);
                if (kk >= lowBound && kk < next) next = kk;
            }
        first = false;
        const bool active = next < bestPass;
        if (rowMin16(active ? next : kTriNoneKey) == kTriNoneKey) break;                        // no lane holds a better untested candidate
        bool pass = active;                                                                // bCoarse accepts without the test (:1132)
        if (active && !p.coarse) {
            int eye2, idx2;
            candidate((int)(0xFFFFu - (next & 0xFFFFu)), eye2, idx2);
            const float* rel = sRel + (eye1 * 2 + eye2) * kTriRelFloats;                             // R12, t12 of :1099-1129
            Kb8Relative q;
#pragma unroll
            for (int r = 0; r < 3; r++) {
#pragma unroll
                for (int c = 0; c < 3; c++) { q.R12[3 * r + c] = rel[3 * r + c]; q.R21[3 * c + r] = rel[3 * r + c]; }
                q.t21[r] = rel[9 + r];
            }
            float k2[8], x3D[3];
#pragma unroll
            for (int a = 0; a < 8; a++) k2[a] = sCam[eye2 * 8 + a];
            const Keypoint& K2 = kp2[(long long)eye2 * cap + idx2];                         // mvKeys or mvKeysRight (:1083-1085)
            const float r2x = T.ray2()[2 * (eye2 * capA + idx2)], r2y = T.ray2()[2 * (eye2 * capA + idx2) + 1];
            int why;
            const float z = kb8TriangulateMatches(k1, k2, r1x, r1y, r2x, r2y, u1, v1, K2.x, K2.y, q, gate1,
                                                  sGate[min(max(K2.octave, 0), p.nlevels - 1)], x3D, why);
            pass = z > 0.0001f;                                                             // epipolarConstrain (KannalaBrandt8.cpp:237-240)
            nCalls++;
        }
        lowBound = active ? next + 1u : kTriNoneKey;                                            // (bestPass only falls: an inactive lane is done)
        bestPass = min(bestPass, rowMin16(pass ? next : kTriNoneKey));
    }
    if (bestPass == kTriNoneKey || sub != 0) return;
    int eye2, idx2;
    candidate((int)(0xFFFFu - (bestPass & 0xFFFFu)), eye2, idx2);
    T.m12()[eye1 * capA + idx1] = eye2 ? nLeft2 + idx2 : idx2;                                    // :1144, the stacked numbering
    if (p.checkOrientation) {                                                                   // :1147-1157
        int bin = rotationBin(K1.angle, kp2[(long long)eye2 * cap + idx2].angle);
        bin = min(max(bin, 0), kHistoLength - 1);                                               // (an angle outside [0, 360) must not index past the table)
        T.binOf()[eye1 * capA + idx1] = (uint8_t)bin;
        atomicAdd(&sHist[bin], 1);
    }
}

// the lane of k_kb8_triangulate: both unprojections, TriangulateMatches
__device__ __forceinline__ float kb8TriangulateLane(const Kb8TriangulateParams& p, const Kb8Relative& q, float u1, float v1, float u2, float v2,
                                                    float (&x3D)[3]) {
    float r1x, r1y, r2x, r2y;
    int why;
    kb8Unproject(p.cam1, u1, v1, r1x, r1y);
    kb8Unproject(p.cam2, u2, v2, r2x, r2y);
    return kb8TriangulateMatches(p.cam1, p.cam2, r1x, r1y, r2x, r2y, u1, v1, u2, v2, q, 5.991 * (double)p.sigma1, 5.991 * (double)p.sigma2, x3D, why);
}

#ifndef ORBX_HOST_ROW

// Diagnostics, OFF unless orbx_debug_search_triangulation_two_eyes_enable(1) was called: a launch then zeroes the two counters and its
// workgroups add their kb8TriangulateMatches calls and their candidates with dist <= th_low.  A production launch pays nothing for them.
__device__ int g_triTwoEyesStats[2];
static bool g_triTwoEyesStatsOn = false;
extern "C" int orbx_debug_search_triangulation_two_eyes_enable(int on) { g_triTwoEyesStatsOn = on != 0; return 0; }
extern "C" int orbx_debug_search_triangulation_two_eyes_stats(int* out2) {
    if (!out2) return -2;                                  // ORBX_ERR_BAD_ARGUMENT
    if (hipDeviceSynchronize() != hipSuccess) return -6;   // (the handle's stream may be a non-blocking one: the copy below would not wait for it)
    return hipMemcpyFromSymbol(out2, HIP_SYMBOL(g_triTwoEyesStats), sizeof(int) * 2) == hipSuccess ? 0 : -6;      // ORBX_ERR_HIP
}

// grid n_pairs; kTriThreads threads; dynamic LDS triMatchTwoEyesLdsBytes(capacity, STAGE) - 1024
template <bool STAGE>
__global__ __launch_bounds__(kTriThreads) void k_search_triangulation_two_eyes(
    const uint32_t* __restrict__ featNodes, const uint32_t* __restrict__ featIdx, const int* __restrict__ nFeat, const uint8_t* __restrict__ mpFlags1,
    const uint8_t* __restrict__ mpFlags2, const float* __restrict__ poses, const Keypoint* __restrict__ kps, const uint8_t* __restrict__ desc,
    const int* __restrict__ nOut, TriMatchTwoEyesParams p, int* __restrict__ matches12, int* __restrict__ pairs, int* __restrict__ nMatches) {
    extern __shared__ __align__(16) uint8_t smem[];
    __shared__ int sHist[kHistoLength], sWave[kTriWaves], sStat[2];
    __shared__ float sRel[4 * kTriRelFloats], sCam[16];
    __shared__ double sGate[kMaxLevels];
    const int cap = p.capacity, capA = (cap + 15) & ~15, pair = blockIdx.x, tid = threadIdx.x, sub = tid & 15, row = tid >> 4;
    const long long X1 = p.kf1First + (long long)pair * p.kf1Step, X2 = p.kf2First + (long long)pair * p.kf2Step, f1 = 2 * X1, f2 = 2 * X2;
    const TriTwoEyesTables T{(ORBX_LDS uint8_t*)smem + (STAGE ? 64 * capA : 0), capA};
    int M1[2], M2[2], N1[2], N2[2];
#pragma unroll
    for (int e = 0; e < 2; e++) {
        M1[e] = max(0, min(nFeat[f1 + e], cap)); M2[e] = max(0, min(nFeat[f2 + e], cap));
        N1[e] = max(0, min(nOut[f1 + e], cap)); N2[e] = max(0, min(nOut[f2 + e], cap));
    }
    const Keypoint *kp1 = kps + f1 * cap, *kp2 = kps + f2 * cap;                                // [2][cap]: the right eye follows the left
    const TriU4 *desc1 = (const TriU4*)(desc + f1 * cap * 32), *desc2 = (const TriU4*)(desc + f2 * cap * 32);
    if (tid < kHistoLength) sHist[tid] = 0;
    if (tid < 2) sStat[tid] = 0;
    triTwoEyesStage(tid, poses + X1 * 12, poses + X2 * 12, p, sRel, sCam, sGate);
    // (indices clamped: a corrupt FeatureVector must not index past the tables)
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const uint32_t *gN1 = featNodes + (f1 + e) * cap, *gI1 = featIdx + (f1 + e) * cap, *gN2 = featNodes + (f2 + e) * cap, *gI2 = featIdx + (f2 + e) * cap;
        for (int i = tid; i < M1[e]; i += kTriThreads) { T.segL()[e * capA + i] = gN1[i]; T.idx1()[e * capA + i] = (unsigned short)min(gI1[i], (uint32_t)(cap - 1)); }
        for (int i = tid; i < M2[e]; i += kTriThreads) { T.node2()[e * capA + i] = gN2[i]; T.idx2()[e * capA + i] = (unsigned short)min(gI2[i], (uint32_t)(cap - 1)); }
    }
    for (int s = tid; s < 2 * capA; s += kTriThreads) {
        triTwoEyesLoadSlot(s, T, capA, cap, pair, N2[s >= capA], mpFlags1, mpFlags2, kp2, p);
        if (s - (s >= capA) * capA >= N1[s >= capA]) T.flag1()[s] = 1;      // a key entry whose index names no feature is skipped before it searches or votes
    }
    if constexpr (STAGE) {
#pragma unroll
        for (int e = 0; e < 2; e++)
            for (int i = tid; i < 2 * N2[e]; i += kTriThreads) T.desc2()[2 * e * capA + i] = desc2[2LL * e * cap + i];
    }
    __syncthreads();
    for (int s = tid; s < M1[0] + M1[1]; s += kTriThreads) {
        const int e = s >= M1[0];
        triTwoEyesSegments(e * capA + s - e * M1[0], T, capA, M2[0], M2[1]);
    }
    __syncthreads();
    int nCalls = 0, nWithin = 0;
    if (!p.onlyStereo)                                                                          // bStereo1 is false for every feature (:1041-1045)
        for (int k = row; k < M1[0] + M1[1]; k += kTriThreads / 16)
            triTwoEyesRow<STAGE>(k, sub, T, capA, cap, M1[0], N2[0], kp1, kp2, desc1, desc2, p, sRel, sCam, sGate, sHist, nCalls, nWithin);
    if (p.countStats) {
        if (nCalls) atomicAdd(&sStat[0], nCalls);
        if (nWithin) atomicAdd(&sStat[1], nWithin);
    }
    __syncthreads();
    if (p.countStats && tid < 2 && sStat[tid]) atomicAdd(&g_triTwoEyesStats[tid], sStat[tid]);
    unsigned dropBins = 0u;
    if (p.checkOrientation) {                                                                   // ComputeThreeMaxima (:2303-2344), then :1174-1193
        const ThreeMaxima top3 = computeThreeMaxima(sHist);
        for (int i = 0; i < kHistoLength; i++)
            if (i != top3.ind1 && i != top3.ind2 && i != top3.ind3) dropBins |= 1u << i;
    }
    // vMatches12 per eye and vMatchedPairs in increasing stacked index (:1195-1203): the left eye, then the right eye + NLeft
    int* outPairs = pairs + 4LL * pair * cap;
    const int wave = tid >> 6, lane = tid & 63;
    int written = 0;
    for (int e = 0; e < 2; e++) {
        int* out = matches12 + (2LL * pair + e) * cap;
        for (int base0 = 0; base0 < cap; base0 += kTriThreads) {
            const int i = base0 + tid;
            int m = i < N1[e] ? T.m12()[e * capA + i] : -1;
            if (m >= 0) { const int bin = T.binOf()[e * capA + i]; if (bin < kHistoLength && ((dropBins >> bin) & 1u)) m = -1; }
            if (i < cap) out[i] = m;
            const unsigned long long vote = __ballot(m >= 0);
            if (lane == 0) sWave[wave] = __popcll(vote);
            __syncthreads();
            int before = written, all = written;
            for (int w = 0; w < kTriWaves; w++) { const int n = sWave[w]; all += n; before += w < wave ? n : 0; }
            if (m >= 0) {
                const int slot = before + __popcll(vote & ((1ull << lane) - 1ull));
                outPairs[2 * slot] = e ? N1[0] + i : i; outPairs[2 * slot + 1] = m;
            }
            written = all;
            __syncthreads();
        }
    }
    if (tid == 0) nMatches[pair] = written;
}

// grid: ceil(n / 256)
__global__ __launch_bounds__(256) void k_kb8_unproject(const float* __restrict__ uv, Kb8UnprojectParams p, float* __restrict__ rays) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    float rx, ry;
    kb8Unproject(p.k, uv[2LL * i], uv[2LL * i + 1], rx, ry);
    rays[3LL * i] = rx; rays[3LL * i + 1] = ry; rays[3LL * i + 2] = 1.0f;
}

// grid: ceil(n / 256)
__global__ __launch_bounds__(256) void k_kb8_triangulate(const float* __restrict__ kp1, const float* __restrict__ kp2, Kb8TriangulateParams p,
                                                         float* __restrict__ z, float* __restrict__ x3d) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    Kb8Relative q;
    kb8RelativeFrom(p.R12, p.t12, q);
    float x[3];
    z[i] = kb8TriangulateLane(p, q, kp1[2LL * i], kp1[2LL * i + 1], kp2[2LL * i], kp2[2LL * i + 1], x);
    x3d[3LL * i] = x[0]; x3d[3LL * i + 1] = x[1]; x3d[3LL * i + 2] = x[2];
}

void launchSearchTriangulationTwoEyes(hipStream_t st, const uint32_t* featNodes, const uint32_t* featIdx, const int* nFeat, const uint8_t* mpFlags1,
                                      const uint8_t* mpFlags2, const float* poses, const Keypoint* kps, const uint8_t* desc, const int* nOut,
                                      const TriMatchTwoEyesParams& params, bool stage, int* matches12, int* pairs, int* nMatches, int nPairs, LdsPolluter pollute) {
    TriMatchTwoEyesParams p = params;
    p.countStats = g_triTwoEyesStatsOn ? 1 : 0;
    void* stats = nullptr;
    if (p.countStats && hipGetSymbolAddress(&stats, HIP_SYMBOL(g_triTwoEyesStats)) == hipSuccess) (void)hipMemsetAsync(stats, 0, sizeof(int) * 2, st);
    const size_t lds = triMatchTwoEyesLdsBytes(p.capacity, stage) - 1024;
    pollute(st);
    if (stage)
        hipLaunchKernelGGL(k_search_triangulation_two_eyes<true>, dim3(nPairs), dim3(kTriThreads), lds, st, featNodes, featIdx, nFeat, mpFlags1,
                           mpFlags2, poses, kps, desc, nOut, p, matches12, pairs, nMatches);
    else
        hipLaunchKernelGGL(k_search_triangulation_two_eyes<false>, dim3(nPairs), dim3(kTriThreads), lds, st, featNodes, featIdx, nFeat, mpFlags1,
                           mpFlags2, poses, kps, desc, nOut, p, matches12, pairs, nMatches);
}

void launchKb8Unproject(hipStream_t st, const float* uv, const float* cam8, int n, float* rays, LdsPolluter pollute) {
    Kb8UnprojectParams p;
    for (int i = 0; i < 8; i++) p.k[i] = cam8[i];
    p.n = n;
    pollute(st);
    hipLaunchKernelGGL(k_kb8_unproject, dim3((n + 255) / 256), dim3(256), 0, st, uv, p, rays);
}

void launchKb8Triangulate(hipStream_t st, const float* kp1, const float* kp2, const Kb8TriangulateParams& p, float* z, float* x3d, LdsPolluter pollute) {
    pollute(st);
    hipLaunchKernelGGL(k_kb8_triangulate, dim3((p.n + 255) / 256), dim3(256), 0, st, kp1, kp2, p, z, x3d);
}

#endif  // ORBX_HOST_ROW

}  // namespace orbx
