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
// capacity bound.  The strict "<" of :1565 keeps the FIRST of equal distances in the order of GetFeaturesInArea's visit (KeyFrame.cc:794-811).
// PredictScale's ceil(log(ratio) / mfLogScaleFactor) is a monotone step function of ratio: the host finds the steps by bisection with the
// same libm expression (orbx_predict_scale_breakpoints) and the level is the number of breakpoints <= ratio - no logarithm here.
// Arithmetic: every operation rounded on its own (-ffp-contract=off and the __f*_rn / __d*_rn intrinsics), cv::Mat products as gemmRow.
// Stated here: the lane's bookkeeping (pair, MapPoint, flag) and the wave-wide count into nFused.  From k_keyframe_project.hpp, shared with
// k_fuse_two_eyes.hip and the Sim3 projection search (k_project_sim3.hip): the front end (projectIntoKeyFrame, :1455-1509), the keyframe's tables
// with their clamps (keyFrameView), the window's visit with Fuse's candidate tests - here with mvuRight - and the strict minimum
// (fuseBest<true>), the thLow decision, the result stores and the exit codes (fuseFinish, kFuse*).
// This file is also compiled for the HOST by the CPU suite (tests/cpp/fuse_host_check.cpp includes it behind tests/cpp/host_shim/hip/
// hip_runtime.h, a hand-written stand-in for the device vocabulary used here).  An intrinsic, builtin or vector type this kernel or that header gains must
// get its stand-in there in the same change, or the CPU suite no longer builds; the wave-wide count into nFused is not emulated there.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orbx_lds_pollute.hpp"
#include "k_keyframe_project.hpp"
#include "k_match_helpers.hpp"
#include "orbx_device.hpp"
#include "orbx_params.hpp"

namespace orbx {

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
    int code = kFuseFlag, bestDist = 256, bestIdx = -1;
    if (i < p.mpCapacity) {
        const long long m = list * p.mpCapacity + i, o = (long long)pair * p.mpCapacity + i;
        const int NM = nMp ? min(max(nMp[list], 0), p.mpCapacity) : p.mpCapacity;
        do {
            if (i >= NM || !(mpFlags[o] & 1)) break;                                         // :1435-1452 / :1639
            KfProjection q;
            code = projectIntoKeyFrame(poses + f * 12, mpWorld + 3 * m, mpNormal + 3 * m, mpDist + 3 * m, p, kProjectPinhole, q);
            if (code != kFrontPassed) break;
            const KeyFrameView kf = keyFrameView(f, kpsUn, desc, nOut, gridOff, gridIdx, p.capacity);
            const float* UR = uRight ? uRight + f * p.capacity : nullptr;
            const uint4 dlo = *(const uint4*)(mpDesc + m * 32), dhi = *(const uint4*)(mpDesc + m * 32 + 16);
            if (!fuseBest<true>(kf, q, UR, dlo, dhi, p, bestDist, bestIdx)) code = kFrontEmptyWindow;      // vIndices.empty() (:1509)
        } while (false);
        code = fuseFinish(code, bestIdx, bestDist, p, o, bestIdxOut, bestDistOut, exitOut);
    }
    const unsigned long long fused = __ballot(code == kFuseFused);
    if ((threadIdx.x & 63) == 0 && fused) atomicAdd(&nFused[pair], __popcll(fused));
}

void launchFuse(hipStream_t st, const float* mpWorld, const float* mpNormal, const float* mpDist, const uint8_t* mpDesc, const int* nMp,
                const uint8_t* mpFlags, const float* poses, const Keypoint* kpsUn, const float* uRight, const uint8_t* desc, const int* nOut,
                const int* gridOff, const int* gridIdx, const FuseParams& p, int* bestIdx, int* bestDist, uint8_t* exitCode, int* nFused,
                int nPairs, LdsPolluter pollute) {
    pollute(st);
    hipLaunchKernelGGL(k_fuse, dim3((p.mpCapacity + 255) / 256, nPairs), dim3(256), 0, st, mpWorld, mpNormal, mpDist, mpDesc, nMp, mpFlags, poses,
                       kpsUn, uRight, desc, nOut, gridOff, gridIdx, p, bestIdx, bestDist, exitCode, nFused);
}

}  // namespace orbx
