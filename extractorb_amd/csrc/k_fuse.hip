// k_fuse.hip — the search half of ORBmatcher::Fuse, the matcher of LocalMapping::SearchInNeighbors (reference src/LocalMapping.cc:729-837):
//   reprojCheck 1: Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, th, bRight = false)   reference src/ORBmatcher.cc:1399-1609
//   reprojCheck 0: Fuse(KeyFrame* pKF, cv::Mat Scw, vpPoints, th, vpReplacePoint) (LoopClosing)    reference src/ORBmatcher.cc:1611-1733
// for keyframes with NLeft == -1 and the Pinhole model, with KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:770-814: NOT Frame's - no level
// filter, four early returns), KeyFrame::IsInImage (:816-819, upper bounds strict), MapPoint::PredictScale (src/MapPoint.cc:514-529),
// Pinhole::project (src/CameraModels/Pinhole.cpp:30-33) and ORBmatcher::DescriptorDistance (:2349-2365).
//
// Everything up to bestIdx / bestDist (:1455-1570, :1643-1712) reads the MapPoint's position, normal, distance bounds and descriptor and the
// keyframe's pose, keypoints, grid, mvuRight and descriptors - no map state.  Only the tail (:1573-1592, :1715-1729: Replace / AddObservation /
// AddMapPoint) touches the map, and unlike SearchByProjection it closes no keypoint for a later MapPoint.  So every (keyframe, MapPoint) is a
// search of its own: ONE THREAD PER MAPPOINT, grid (ceil(mpCapacity / 256), pairs); the caller replays the tail on the host in list order.
// One thing the tail does change that a LATER KEYFRAME's search reads: Replace ends with ComputeDistinctiveDescriptors() on the survivor
// (src/MapPoint.cc:296-298), so a list entry that survived a Replace may have a new descriptor.  The caller searches such entries again for
// the later keyframes (include/orbx.h); this kernel is a pure function of what it is given.
// minX .. maxY arrive TRUNCATED (KeyFrame's const int mnMinX .. mnMaxY), wInv / hInv from the float bounds (orbx_fuse_device).
// The window of a MapPoint (th = 3: a radius of 3 to 11 px against cells of ~10 x 10 px) holds a handful of keypoints, so the front end
// dominates; the keyframe's grid, keypoints and descriptors are read through L2 (62 KB per keyframe at capacity 1302): no LDS table, no
// capacity bound.  Cells are visited with ix outer and iy inner and push_back order inside a cell (KeyFrame.cc:794-811): a window is one
// slot range of mGrid's CSR order per cell column, and the strict "<" of :1565 keeps the FIRST of equal distances in that order.
// PredictScale's ceil(log(ratio) / mfLogScaleFactor) is a monotone step function of ratio: the host finds the steps by bisection with the
// same libm expression (orbx_predict_scale_breakpoints) and the level is the number of breakpoints <= ratio - no logarithm here.
// Arithmetic: every operation rounded on its own (-ffp-contract=off and the __f*_rn / __d*_rn intrinsics), cv::Mat products as gemmRow.
// The front end - pose, projection, IsInImage, distance and normal tests, PredictScale, the cell window (:1455-1509) - is projectIntoKeyFrame of
// k_keyframe_project.hpp, shared with the Sim3 projection search (k_project_sim3.hip): one statement, two users.
// This file is also compiled for the HOST by the CPU suite (tests/cpp/fuse_host_check.cpp includes it behind tests/cpp/host_shim/hip/
// hip_runtime.h, a hand-written stand-in for the device vocabulary used here).  An intrinsic, builtin or vector type this kernel or that header gains must
// get its stand-in there in the same change, or the CPU suite no longer builds; the wave-wide count into nFused is not emulated there.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_keyframe_project.hpp"
#include "k_match_helpers.hpp"
#include "orbx_device.hpp"
#include "orbx_params.hpp"

namespace orbx {

namespace {
enum { kExitFlag = 0, kExitNegDepth, kExitNotInImage, kExitDistance, kExitNormal, kExitEmptyWindow, kExitAboveThLow, kExitFused };      // == ORBX_FUSE_*
}  // namespace

__global__ __launch_bounds__(256) void k_fuse(const float* __restrict__ mpWorld, const float* __restrict__ mpNormal,
                                              const float* __restrict__ mpDist, const uint8_t* __restrict__ mpDesc,
                                              const int* __restrict__ nMp, const uint8_t* __restrict__ mpFlags,
                                              const float* __restrict__ poses, const Keypoint* __restrict__ kpsUn,
                                              const float* __restrict__ uRight, const uint8_t* __restrict__ desc,
                                              const int* __restrict__ nOut, const int* __restrict__ gridOff,
                                              const int* __restrict__ gridIdx, FuseParams p, int* __restrict__ bestIdxOut,
                                              int* __restrict__ bestDistOut, uint8_t* __restrict__ exitOut, int* __restrict__ nFused) {
    const int pair = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const long long f = p.kfFirst + (long long)pair * p.kfStep, list = p.mpFirst + (long long)pair * p.mpStep;
    int code = kExitFlag, bestDist = 256, bestIdx = -1;
    if (i < p.mpCapacity) {
        const long long m = list * p.mpCapacity + i, o = (long long)pair * p.mpCapacity + i;
        const int NM = nMp ? min(max(nMp[list], 0), p.mpCapacity) : p.mpCapacity;
        do {
            if (i >= NM || !(mpFlags[o] & 1)) break;                                         // :1435-1452 / :1639
            // the pose, the projection, IsInImage, the distance and normal tests, PredictScale and the cell window: k_keyframe_project.hpp,
            // shared with the Sim3 projection search; its exits 1 .. 5 are kExitNegDepth .. kExitEmptyWindow
            KfProjection q;
            code = projectIntoKeyFrame(poses + f * 12, mpWorld + 3 * m, mpNormal + 3 * m, mpDist + 3 * m, p, kProjectPinhole, q);
            if (code != kFrontPassed) break;
            code = kExitEmptyWindow;
            const float u = q.u, v = q.v, r = q.r;
            const int level = q.level, minCX = q.minCX, maxCX = q.maxCX, minCY = q.minCY, maxCY = q.maxCY;
            const float ur = __fsub_rn(u, __fmul_rn(p.mbf, q.invz));                         // :1479
            // a candidate's kpLevel is level or level - 1 (:1530): the two mvInvLevelSigma2 it can need
            const float invHi = p.invSigma2[level], invLo = p.invSigma2[max(level - 1, 0)];
            const int N = min(max(nOut[f], 0), p.capacity);
            const int* off = gridOff + f * (kGridCells + 1);
            const int* gi = gridIdx + f * p.capacity;
            const Keypoint* K = kpsUn + f * p.capacity;
            const float* UR = uRight ? uRight + f * p.capacity : nullptr;
            const uint4* D = (const uint4*)(desc + f * p.capacity * 32);
            const int nIn = min(max(off[kGridCells], 0), N);                                     // (clamped: a corrupt grid must not index past the frame)
            const uint4 dlo = *(const uint4*)(mpDesc + m * 32), dhi = *(const uint4*)(mpDesc + m * 32 + 16);
            bool any = false;
            for (int cx = minCX; cx <= maxCX; cx++) {
                if (minCY > maxCY) break;
                const int sEnd = min(max(off[cx * kGridRows + maxCY + 1], 0), nIn);
                for (int s = min(max(off[cx * kGridRows + minCY], 0), nIn); s < sEnd; s++) {
                    const int idx = min(max(gi[s], 0), p.capacity - 1);
                    const float kx = K[idx].x, ky = K[idx].y;
                    if (!(fabsf(__fsub_rn(kx, u)) < r && fabsf(__fsub_rn(ky, v)) < r)) continue;      // KeyFrame.cc:804-808
                    any = true;
                    const int lv = K[idx].octave;
                    if (lv < level - 1 || lv > level) continue;                              // :1530
                    if (p.reprojCheck) {
                        const float inv = lv == level ? invHi : invLo;      // mvInvLevelSigma2[kpLevel]; level - 1 = -1 reads entry 0 (the reference would index past the table)
                        const float kr = UR ? UR[idx] : -1.0f;
                        const float ex = __fsub_rn(u, kx), ey = __fsub_rn(v, ky);
                        const float e2m = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
                        if (kr >= 0.0f) {                                                    // :1533-1546
                            const float er = __fsub_rn(ur, kr);
                            if ((double)__fmul_rn(__fadd_rn(e2m, __fmul_rn(er, er)), inv) > 7.8) continue;
                        } else if ((double)__fmul_rn(e2m, inv) > 5.99) continue;             // :1547-1557
                    }
                    const uint4 e = D[2 * idx], g = D[2 * idx + 1];
                    const int dist = hamming256(dlo, dhi, e, g);
                    if (dist < bestDist) { bestDist = dist; bestIdx = idx; }                 // :1565, strict: the first of equals stays
                }
            }
            if (!any) break;                                                                 // vIndices.empty() (:1509)
            code = bestIdx >= 0 && bestDist <= p.thLow ? kExitFused : kExitAboveThLow;       // :1573
        } while (false);
        bestIdxOut[o] = code == kExitFused ? bestIdx : -1;
        bestDistOut[o] = bestDist;
        if (exitOut) exitOut[o] = (uint8_t)code;
    }
    const unsigned long long fused = __ballot(code == kExitFused);
    if ((threadIdx.x & 63) == 0 && fused) atomicAdd(&nFused[pair], __popcll(fused));
}

void launchFuse(hipStream_t st, const float* mpWorld, const float* mpNormal, const float* mpDist, const uint8_t* mpDesc, const int* nMp,
                const uint8_t* mpFlags, const float* poses, const Keypoint* kpsUn, const float* uRight, const uint8_t* desc, const int* nOut,
                const int* gridOff, const int* gridIdx, const FuseParams& p, int* bestIdx, int* bestDist, uint8_t* exitCode, int* nFused,
                int nPairs) {
    hipLaunchKernelGGL(k_fuse, dim3((p.mpCapacity + 255) / 256, nPairs), dim3(256), 0, st, mpWorld, mpNormal, mpDist, mpDesc, nMp, mpFlags, poses,
                       kpsUn, uRight, desc, nOut, gridOff, gridIdx, p, bestIdx, bestDist, exitCode, nFused);
}

}  // namespace orbx
