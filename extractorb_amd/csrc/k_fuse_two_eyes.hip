// k_fuse_two_eyes.hip - the search half of ORBmatcher::Fuse for TWO-CAMERA keyframes (NLeft != -1, a KannalaBrandt8 pair):
//   Fuse(pKF, vpMapPoints, th, bRight = false) and Fuse(pKF, vpMapPoints, th, bRight = true)   reference src/ORBmatcher.cc:1399-1609,
//   as LocalMapping::SearchInNeighbors calls them one after the other (src/LocalMapping.cc:787-788, :816-817), and the loop-closing overload
//   (:1611-1733, reprojCheck 0) on such a keyframe, which has a left form only.  k_fuse.hip is the one-camera form; what differs here:
//   * the right eye has a pose of its own, from KeyFrame's getters (src/KeyFrame.cc:1232-1262), which derive it from mTlr ALONE:
//       Rrl = mTlr.R.t();  Rrw = Rrl*Rlw;  trl = -Rrl*mTlr.t (one gemm, alpha = -1);  trw = Rrl*tlw + trl (one gemm with the addend);
//       twr = Rwl*mTlr.t + Ow (one gemm with the float Ow as addend)
//     (Frame holds mTrl beside mTlr and isInFrustumChecks takes both, k_frustum_two_eyes_point.hpp: not so here);
//   * uv = KannalaBrandt8::project with the eye's own camera (mpCamera / mpCamera2, :1409, :1416): kb8Project of k_camera_kb8.hpp.  z == 0 does
//     NOT leave by itself as it does under the pinhole model: atan2f(r, 0) is pi / 2, the projection is finite and may be inside the image, and
//     the MapPoint goes on through the distance and normal tests like any other (z = -0.0f is not < 0.0f either);
//   * KeyFrame::GetFeaturesInArea(u, v, r, bRight) reads that eye's grid (mGrid / mGridRight) and its RAW keypoints (mvKeys / mvKeysRight,
//     KeyFrame.cc:801-803), and :1524-1528 take position and octave from the same: device frames 2r (left) and 2r + 1 (right) of rig r, the
//     layout of orbx_frame_finish_two_eyes_device;
//   * the reprojection test is always the monocular one (:1547-1557): fuseBest<false>, where k_keyframe_project.hpp says why;
//   * bestIdx is in the KEYFRAME's numbering (:1559): a right keypoint i is NLeft + i; its descriptor is row i of device frame 2r + 1.
// From k_keyframe_project.hpp, shared with k_fuse and / or the Sim3 projection search: everything after (u, v) up to the cell window
// (keyFrameIsInImage + keyFrameWindow), the eye's tables (keyFrameView of device frame 2r + eye), the visit of the window with Fuse's
// candidate tests and strict minimum (fuseBest), the thLow decision, the result stores and the exit codes (fuseFinish, kFuse*).  The tables
// are read through L2: no LDS table, no capacity bound.
// LAUNCH SHAPE: one lane per (MapPoint, eye), as k_frustum_two_eyes_check.  With both eyes asked for the eye is the lane's parity; with one eye
// asked for every lane takes that eye and a workgroup covers twice the MapPoints (no lane idles for an eye nobody wants).  Either way the eye
// is a run-time index into LDS, never a template or a loop: the KannalaBrandt8 code (two software atan2f, a sincos, the polynomial) is
// instantiated once, and the eye's pose, centre and camera are read from LDS by eye index into statically indexed registers.  The thirty rig
// invariants (mR | mt | centre per eye) are dealt to thirty lanes once per workgroup, each straight from the pose and mTlr (at most two
// dependent gemm rows), so ONE barrier separates staging and search.  One thread per MapPoint looping over the eyes was not built, for
// k_frustum_two_eyes.hip's reasons: half the lanes per point at the same cost per point, and both eyes' invariants in registers at once.
// nFused[pair * 2 + eye]: a wave ballot, split by eye, and at most one atomic per eye and wave, as k_fuse.
// The statement is two functions, fuseTwoEyesStage (before the barrier) and fuseTwoEyesLane (after it); the kernel is the two around the
// barrier.  The CPU suite compiles this file for the HOST (tests/cpp/fuse_two_eyes_host_check.cpp behind tests/cpp/host_shim) and runs a
// workgroup as "every thread's stage, then every thread's lane", one thread at a time.  A device word this file gains needs its stand-in in
// tests/cpp/host_shim/fuse_two_eyes_shim.h; the wave-wide count into nFused is not emulated there.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orbx_lds_pollute.hpp"
#include "k_camera_kb8.hpp"
#include "k_keyframe_project.hpp"
#include "k_match_helpers.hpp"
#include "k_rig_two_eyes.hpp"
#include "orbx_device.hpp"
#include "orbx_params.hpp"

namespace orbx {

namespace {
constexpr int kFuse2Threads = 256;
constexpr int kFuse2EyeFloats = kRigEyeFloats;      // one eye of a rig keyframe (k_rig_two_eyes.hpp)
}  // namespace

// before the barrier: thirty lanes compute the rig's invariants, sixteen others copy the two cameras.  sEye[2 * kFuse2EyeFloats], sCam[16]
__device__ __forceinline__ void fuseTwoEyesStage(const float* __restrict__ poses, const FuseTwoEyesParams& p, float* sEye, float* sCam) {
    const int pair = blockIdx.y, tid = threadIdx.x;
    const long long rig = p.kfFirst + (long long)pair * p.kfStep;
    if (tid < 2 * kFuse2EyeFloats) sEye[tid] = fuseTwoEyesRigElement(poses + rig * 12, p.tlr, tid);
    else if (tid >= 64 && tid < 80) sCam[tid - 64] = p.cam[(tid - 64) >> 3][tid & 7];
}

// after the barrier: one (MapPoint, eye)
__device__ __forceinline__ void fuseTwoEyesLane(const float* __restrict__ mpWorld, const float* __restrict__ mpNormal,
                                                const float* __restrict__ mpDist, const uint8_t* __restrict__ mpDesc,
                                                const int* __restrict__ nMp, const uint8_t* __restrict__ mpFlags,
                                                const Keypoint* __restrict__ kps, const uint8_t* __restrict__ desc, const int* __restrict__ nOut,
                                                const int* __restrict__ gridOff, const int* __restrict__ gridIdx, const FuseTwoEyesParams& p,
                                                const float* sEye, const float* sCam, int* __restrict__ bestIdxOut, int* __restrict__ bestDistOut,
                                                uint8_t* __restrict__ exitOut, int* __restrict__ nFused) {
    const int pair = blockIdx.y;
    const long long slot = (long long)blockIdx.x * kFuse2Threads + threadIdx.x;
    const bool both = p.eyes == 3;
    const int eye = both ? (int)(slot & 1) : p.eyes - 1;
    const long long i = both ? slot >> 1 : slot;
    const long long rig = p.kfFirst + (long long)pair * p.kfStep, list = p.mpFirst + (long long)pair * p.mpStep;
    int code = kFuseFlag, bestDist = 256, bestIdx = -1;
    if (i < p.mpCapacity) {
        const long long m = list * p.mpCapacity + i, o = ((long long)pair * 2 + eye) * p.mpCapacity + i;
        const int NM = nMp ? min(max(nMp[list], 0), p.mpCapacity) : p.mpCapacity;
        do {
            if (i >= NM || !(mpFlags[(long long)pair * p.mpCapacity + i] & 1)) break;        // :1435-1452 / :1639; one flag serves both eyes
            float e[kFuse2EyeFloats], k[8];
#pragma unroll
            for (int a = 0; a < kFuse2EyeFloats; a++) e[a] = sEye[eye * kFuse2EyeFloats + a];
#pragma unroll
            for (int a = 0; a < 8; a++) k[a] = sCam[eye * 8 + a];
            const float xw[3] = {mpWorld[3 * m], mpWorld[3 * m + 1], mpWorld[3 * m + 2]};
            float xc[3];
            for (int r = 0; r < 3; r++) xc[r] = gemmRow(e[3 * r], e[3 * r + 1], e[3 * r + 2], xw, 1.0, e[9 + r], true);      // Rcw*p3Dw+tcw (:1456)
            code = kFrontNegDepth;
            if (xc[2] < 0.0f) break;                                                         // :1459 (z == 0 and z == -0 go on)
            float u, v;
            kb8Project(k, xc[0], xc[1], xc[2], u, v);                                        // pCamera->project (:1470)
            code = kFrontNotInImage;
            if (!keyFrameIsInImage(u, v, p)) break;                                          // :1473
            const float Ow[3] = {e[12], e[13], e[14]};
            KfProjection q;
            code = keyFrameWindow(u, v, xw, Ow, mpNormal + 3 * m, mpDist + 3 * m, p, q);     // kFrontDistance .. kFrontEmptyWindow, or passed
            if (code != kFrontPassed) break;
            const long long f = 2 * rig + eye;                                               // mvKeys / mGrid or mvKeysRight / mGridRight
            const KeyFrameView kf = keyFrameView(f, kps, desc, nOut, gridOff, gridIdx, p.capacity);
            const int nLeft = min(max(nOut[2 * rig], 0), p.capacity);                        // pKF->NLeft
            const uint4 dlo = *(const uint4*)(mpDesc + m * 32), dhi = *(const uint4*)(mpDesc + m * 32 + 16);
            if (!fuseBest<false>(kf, q, nullptr, dlo, dhi, p, bestDist, bestIdx)) code = kFrontEmptyWindow;      // vIndices.empty() (:1509); nullptr: <false> never reads UR
            if (eye && bestIdx >= 0) bestIdx += nLeft;                                       // :1559: the keyframe's numbering
        } while (false);
        code = fuseFinish(code, bestIdx, bestDist, p, o, bestIdxOut, bestDistOut, exitOut);
    }
    // the lanes of a wave hold the left eye (both: the even lanes; eyes == 1: all), the right eye (the odd lanes; eyes == 2: all)
    const unsigned long long fused = __ballot(code == kFuseFused);
    const unsigned long long leftLanes = both ? 0x5555555555555555ull : p.eyes == 1 ? ~0ull : 0ull;
    if ((threadIdx.x & 63) == 0) {
        if (fused & leftLanes) atomicAdd(&nFused[pair * 2], __popcll(fused & leftLanes));
        if (fused & ~leftLanes) atomicAdd(&nFused[pair * 2 + 1], __popcll(fused & ~leftLanes));
    }
}

// grid (ceil(mpCapacity * (eyes == 3 ? 2 : 1) / kFuse2Threads), pairs)
__global__ __launch_bounds__(kFuse2Threads) void k_fuse_two_eyes(const float* __restrict__ mpWorld, const float* __restrict__ mpNormal,
                                                                 const float* __restrict__ mpDist, const uint8_t* __restrict__ mpDesc,
                                                                 const int* __restrict__ nMp, const uint8_t* __restrict__ mpFlags,
                                                                 const float* __restrict__ poses, const Keypoint* __restrict__ kps,
                                                                 const uint8_t* __restrict__ desc, const int* __restrict__ nOut,
                                                                 const int* __restrict__ gridOff, const int* __restrict__ gridIdx,
                                                                 FuseTwoEyesParams p, int* __restrict__ bestIdxOut, int* __restrict__ bestDistOut,
                                                                 uint8_t* __restrict__ exitOut, int* __restrict__ nFused) {
    __shared__ float sEye[2 * kFuse2EyeFloats], sCam[16];
    fuseTwoEyesStage(poses, p, sEye, sCam);
    __syncthreads();
    fuseTwoEyesLane(mpWorld, mpNormal, mpDist, mpDesc, nMp, mpFlags, kps, desc, nOut, gridOff, gridIdx, p, sEye, sCam, bestIdxOut, bestDistOut,
                    exitOut, nFused);
}

int fuseTwoEyesGroups(int mpCapacity, int eyes) {
    return (int)(((long long)mpCapacity * (eyes == 3 ? 2 : 1) + kFuse2Threads - 1) / kFuse2Threads);
}

void launchFuseTwoEyes(hipStream_t st, const float* mpWorld, const float* mpNormal, const float* mpDist, const uint8_t* mpDesc, const int* nMp,
                       const uint8_t* mpFlags, const float* poses, const Keypoint* kps, const uint8_t* desc, const int* nOut, const int* gridOff,
                       const int* gridIdx, const FuseTwoEyesParams& p, int* bestIdx, int* bestDist, uint8_t* exitCode, int* nFused, int nPairs, LdsPolluter pollute) {
    pollute(st);
    hipLaunchKernelGGL(k_fuse_two_eyes, dim3(fuseTwoEyesGroups(p.mpCapacity, p.eyes), nPairs), dim3(kFuse2Threads), 0, st, mpWorld, mpNormal, mpDist,
                       mpDesc, nMp, mpFlags, poses, kps, desc, nOut, gridOff, gridIdx, p, bestIdx, bestDist, exitCode, nFused);
}

}  // namespace orbx
