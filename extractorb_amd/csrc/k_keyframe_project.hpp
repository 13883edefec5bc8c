// k_keyframe_project.hpp - the front end of the searches that project a MapPoint into a KEYFRAME with a Sim3-decomposed (or plain) pose:
// from the pose load to the predicted level and the four cell-window bounds.  ONE statement with two users:
//   k_fuse.hip          both ORBmatcher::Fuse overloads                       (reference src/ORBmatcher.cc:1455-1509, :1643-1700)
//   k_project_sim3.hip  the two Sim3 ORBmatcher::SearchByProjection overloads  (reference src/ORBmatcher.cc:504-547, :620-664)
// The arithmetic is the reference's x86-64 build, every operation rounded on its own (-ffp-contract=off and the __f*_rn / __d*_rn intrinsics):
// p3Dc and Ow as cv::gemm (products and sums in double, one rounding to float), KeyFrame::IsInImage on the truncated bounds with strict upper
// bounds, cv::norm and Mat::dot in double, MapPoint::PredictScale as a count of breakpoints, KeyFrame::GetFeaturesInArea's cell window with
// its four early returns (src/KeyFrame.cc:778-792).  The only thing the callers differ in is how (u, v) is formed:
//   kProjectPinhole  pKF->mpCamera->project (src/CameraModels/Pinhole.cpp:30-33):  u = fx*x/z + cx
//   kProjectInvZ     the second Sim3 overload's own lines (:631-636):              invz = 1/z; x = X*invz; u = fx*x + cx
// which differ in the last bit.  What follows (u, v) - IsInImage, the distance and normal tests, PredictScale, the cell window - is
// keyFrameIsInImage + keyFrameWindow, stated apart so that a third user takes it as it is:
//   k_fuse_two_eyes.hip  Fuse on a two-camera keyframe (NLeft != -1): its own pose per eye and KannalaBrandt8::project in front, then these two.
// Takes gemmRow, dot3Double (cv::norm, Mat::dot) and the cell window from k_match_helpers.hpp.
// Also compiled for the HOST by the CPU suite (tests/cpp/host_shim): a device word this header gains needs its stand-in there.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_match_helpers.hpp"
#include "orbx_device.hpp"

namespace orbx {

enum { kProjectPinhole = 0, kProjectInvZ = 1 };
// where the front end leaves a MapPoint: == ORBX_FUSE_* / ORBX_SIM3_SEARCH_* 1 .. 5; kFrontPassed = it reached the window scan
enum { kFrontNegDepth = 1, kFrontNotInImage = 2, kFrontDistance = 3, kFrontNormal = 4, kFrontEmptyWindow = 5, kFrontPassed = 6 };

struct KfProjection {
    float u, v, invz, r;      // the projection, 1/z (Fuse's ur needs it), the search radius th * mvScaleFactors[level]
    int level;                // MapPoint::PredictScale
    int minCX, maxCX, minCY, maxCY;
};

// MapPoint::PredictScale as a count of breakpoints (ascending; NaN is above none, +inf above all).  P: nlevels, breaks[].
// Shared with the frustum test of k_frustum_point.hpp.
template <class P>
__device__ __forceinline__ int predictScaleLevel(float ratio, const P& p) {
    int level = 0;
#pragma unroll
    for (int k = 1; k < kMaxLevels; k++) level += k < p.nlevels && ratio >= p.breaks[k - 1] ? 1 : 0;
    return level;
}

// KeyFrame::IsInImage (KeyFrame.cc:816-819) on the truncated bounds, upper bounds strict; a NaN is outside.  P: minX .. maxY (truncated).
template <class P>
__device__ __forceinline__ bool keyFrameIsInImage(float u, float v, const P& p) {
    return u >= p.minX && u < p.maxX && v >= p.minY && v < p.maxY;
}

// From a projection (u, v) inside the image to the predicted level and the cell window (:1479-1509, :524-547): xw the MapPoint's position, Ow
// the centre of the camera that sees it, nrm / dst its normal and (min, max invariance, mfMaxDistance).  Fills all of `o` but invz.
// P: minX, minY (truncated), wInv, hInv (from the float bounds), scale[], breaks[], th, nlevels.
// Returns kFrontDistance, kFrontNormal, kFrontEmptyWindow or kFrontPassed.
template <class P>
__device__ __forceinline__ int keyFrameWindow(float u, float v, const float (&xw)[3], const float (&Ow)[3], const float* __restrict__ nrm,
                                              const float* __restrict__ dst, const P& p, KfProjection& o) {
    float PO[3];
    for (int r = 0; r < 3; r++) PO[r] = __fsub_rn(xw[r], Ow[r]);                     // :1483, :528
    // cv::norm of CV_32F: squares accumulated in double in element order, one square root, then float
    const double n2 = dot3Double(PO[0], PO[1], PO[2], PO[0], PO[1], PO[2]);
    const float dist3D = (float)__dsqrt_rn(n2);
    const float minDistance = dst[0], maxDistance = dst[1];
    if (dist3D < minDistance || dist3D > maxDistance) return kFrontDistance;         // :1487, :531
    const double dot = dot3Double(PO[0], PO[1], PO[2], nrm[0], nrm[1], nrm[2]);
    if (dot < __dmul_rn(0.5, (double)dist3D)) return kFrontNormal;                   // :1496, :537
    const float ratio = __fdiv_rn(dst[2], dist3D);                                   // mfMaxDistance itself, not 1.2f * it (MapPoint.cc:519)
    const int level = predictScaleLevel(ratio, p);
    const float r = __fmul_rn(p.th, p.scale[level]);                                 // :1505, :543
    // KeyFrame::GetFeaturesInArea's cell window with its four early returns (KeyFrame.cc:778-792)
    const int minCX = cellWindowMin(u, p.minX, r, p.wInv);
    if (minCX >= kGridCols) return kFrontEmptyWindow;
    const int maxCX = cellWindowMax(u, p.minX, r, p.wInv, kGridCols);
    if (maxCX < 0) return kFrontEmptyWindow;
    const int minCY = cellWindowMin(v, p.minY, r, p.hInv);
    if (minCY >= kGridRows) return kFrontEmptyWindow;
    const int maxCY = cellWindowMax(v, p.minY, r, p.hInv, kGridRows);
    if (maxCY < 0) return kFrontEmptyWindow;
    o.u = u; o.v = v; o.r = r; o.level = level;
    o.minCX = minCX; o.maxCX = maxCX; o.minCY = minCY; o.maxCY = maxCY;
    return kFrontPassed;
}

// P: keyFrameWindow's block with fx, fy, cx, cy and maxX, maxY (truncated) beside it.
// T: the 12 floats of the pose (Rcw | tcw rows); xw / nrm / dst: the MapPoint's position, normal and (min, max invariance, mfMaxDistance).
// Returns the exit (kFrontNegDepth .. kFrontEmptyWindow) or kFrontPassed with `o` filled.
template <class P>
__device__ __forceinline__ int projectIntoKeyFrame(const float* __restrict__ T, const float* __restrict__ xwp, const float* __restrict__ nrm,
                                                   const float* __restrict__ dst, const P& p, int projection, KfProjection& o) {
    const float R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
    const float tcw[3] = {T[3], T[7], T[11]};
    const float xw[3] = {xwp[0], xwp[1], xwp[2]};
    float xc[3];
    for (int r = 0; r < 3; r++) xc[r] = gemmRow(R[3 * r], R[3 * r + 1], R[3 * r + 2], xw, 1.0, tcw[r], true);      // Rcw*p3Dw+tcw (:1456, :508)
    if (xc[2] < 0.0f) return kFrontNegDepth;                                         // :1459, :511
    const float invz = __fdiv_rn(1.0f, xc[2]);                                       // :1465, :631, a float division
    float u, v;
    if (projection == kProjectInvZ) {                                                // :632-636
        u = __fadd_rn(__fmul_rn(p.fx, __fmul_rn(xc[0], invz)), p.cx);
        v = __fadd_rn(__fmul_rn(p.fy, __fmul_rn(xc[1], invz)), p.cy);
    } else {                                                                         // Pinhole::project
        u = __fadd_rn(__fdiv_rn(__fmul_rn(p.fx, xc[0]), xc[2]), p.cx);
        v = __fadd_rn(__fdiv_rn(__fmul_rn(p.fy, xc[1]), xc[2]), p.cy);
    }
    if (!keyFrameIsInImage(u, v, p)) return kFrontNotInImage;                        // (z == 0: inf / NaN fail here)
    float Ow[3];
    for (int r = 0; r < 3; r++) Ow[r] = gemmRow(R[r], R[3 + r], R[6 + r], tcw, -1.0, 0.f, false);      // -Rcw.t()*tcw (KeyFrame.cc:118, :1624, :487)
    o.invz = invz;
    return keyFrameWindow(u, v, xw, Ow, nrm, dst, p, o);
}

}  // namespace orbx
