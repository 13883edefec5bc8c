// k_keyframe_project.hpp - the searches that project a MapPoint into a KEYFRAME with a Sim3-decomposed (or plain) pose, front end and back end:
// from the pose load to the predicted level and the four cell-window bounds, then KeyFrame::GetFeaturesInArea's visit of that window, then
// Fuse's choice among the visited keypoints.  ONE statement of each, three users:
//   k_fuse.hip           both ORBmatcher::Fuse overloads                       (reference src/ORBmatcher.cc:1455-1609, :1643-1733)
//   k_fuse_two_eyes.hip  Fuse on a two-camera keyframe (NLeft != -1): its own pose per eye and KannalaBrandt8::project in front
//   k_project_sim3.hip   the two Sim3 ORBmatcher::SearchByProjection overloads  (reference src/ORBmatcher.cc:504-580, :620-697)
// FRONT END.  The arithmetic is the reference's x86-64 build, every operation rounded on its own (-ffp-contract=off and the __f*_rn / __d*_rn
// intrinsics): p3Dc and Ow as cv::gemm (products and sums in double, one rounding to float), KeyFrame::IsInImage on the truncated bounds with
// strict upper bounds, cv::norm and Mat::dot in double, MapPoint::PredictScale as a count of breakpoints, KeyFrame::GetFeaturesInArea's cell
// window with its four early returns (src/KeyFrame.cc:778-792).  projectIntoKeyFrame is all of it for the two pinhole users, which differ only
// in how (u, v) is formed:
//   kProjectPinhole  pKF->mpCamera->project (src/CameraModels/Pinhole.cpp:30-33):  u = fx*x/z + cx
//   kProjectInvZ     the second Sim3 overload's own lines (:631-636):              invz = 1/z; x = X*invz; u = fx*x + cx
// (the last bit differs).  What follows (u, v) - IsInImage, the distance and normal tests, PredictScale, the cell window - is keyFrameIsInImage +
// keyFrameWindow, stated apart: the two-camera Fuse takes them as they are behind its own projection.
// BACK END.  keyFrameView: a keyframe as the visit reads it, the only statement of the clamps that keep a corrupt grid inside the frame
// (k_sim3_settle, short of registers, takes keyFrameSlotsInGrid alone).  keyFrameVisitArea: GetFeaturesInArea's visit of a KfProjection's
// window with the area test; what a search does with a keypoint inside is its body's (sim3Scan of k_project_sim3.hip is one).  fuseBest and
// fuseFinish: Fuse's candidate tests, strict minimum, thLow decision and result stores for both Fuse kernels, under one exit enum.
// Takes gemmRow, dot3Double (cv::norm, Mat::dot), the cell window and hamming256 from k_match_helpers.hpp.
// Also compiled for the HOST by the CPU suite (tests/cpp/host_shim): a device word this header gains needs its stand-in there.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_match_helpers.hpp"
#include "orbx.h"
#include "orbx_device.hpp"

namespace orbx {

enum { kProjectPinhole = 0, kProjectInvZ = 1 };
// where the front end leaves a MapPoint: == ORBX_FUSE_* / ORBX_SIM3_SEARCH_* 1 .. 5; kFrontPassed = it reached the window scan
enum { kFrontNegDepth = 1, kFrontNotInImage = 2, kFrontDistance = 3, kFrontNormal = 4, kFrontEmptyWindow = 5, kFrontPassed = 6 };
// Fuse's own exits beside those; all eight == ORBX_FUSE_* of include/orbx.h
enum { kFuseFlag = 0, kFuseAboveThLow = 6, kFuseFused = 7 };
static_assert(kFuseFlag == ORBX_FUSE_FLAG && kFrontNegDepth == ORBX_FUSE_NEG_DEPTH && kFrontNotInImage == ORBX_FUSE_NOT_IN_IMAGE &&
              kFrontDistance == ORBX_FUSE_DISTANCE && kFrontNormal == ORBX_FUSE_NORMAL && kFrontEmptyWindow == ORBX_FUSE_EMPTY_WINDOW &&
              kFuseAboveThLow == ORBX_FUSE_ABOVE_TH_LOW && kFuseFused == ORBX_FUSE_FUSED, "Fuse's exit codes are the header's");

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

// The keyframe of device frame f as the visit reads it: the grid's CSR offsets and slot -> keypoint table, the keypoints, the descriptors
struct KeyFrameView {
    const int* off; const int* gi; const Keypoint* K; const uint4* D; int nIn, capacity;
};

// The slots of frame f's grid that a scan may read: mGrid's total, cut to the frame's count, cut to the capacity (a corrupt grid must not
// index past the frame - or past k_sim3_settle's closedBy)
__device__ __forceinline__ int keyFrameSlotsInGrid(long long f, const int* __restrict__ nOut, const int* __restrict__ gridOff, int capacity) {
    const int N = min(max(nOut[f], 0), capacity);
    const int* off = gridOff + f * (kGridCells + 1);
    return min(max(off[kGridCells], 0), N);
}

__device__ __forceinline__ KeyFrameView keyFrameView(long long f, const Keypoint* __restrict__ kps, const uint8_t* __restrict__ desc,
                                                     const int* __restrict__ nOut, const int* __restrict__ gridOff,
                                                     const int* __restrict__ gridIdx, int capacity) {
    KeyFrameView k;
    k.off = gridOff + f * (kGridCells + 1); k.gi = gridIdx + f * capacity; k.K = kps + f * capacity;
    k.D = (const uint4*)(desc + f * capacity * 32);
    k.nIn = keyFrameSlotsInGrid(f, nOut, gridOff, capacity);
    k.capacity = capacity;
    return k;
}

// KeyFrame::GetFeaturesInArea's visit (src/KeyFrame.cc:794-811) of q's window: body(s, idx, kx, ky) for every keypoint inside the area (CSR slot,
// index, position) in the reference's order - ix outer, iy inner, push order in a cell: one slot range per cell column.  Ranges are clamped to
// [0, nIn], indices to the frame.  Returns whether any keypoint was inside: vIndices is not empty.
template <class Body>
__device__ __forceinline__ bool keyFrameVisitArea(const KeyFrameView& kf, const KfProjection& q, Body&& body) {
    bool any = false;
    for (int cx = q.minCX; cx <= q.maxCX; cx++) {
        if (q.minCY > q.maxCY) break;
        const int sEnd = min(max(kf.off[cx * kGridRows + q.maxCY + 1], 0), kf.nIn);
        for (int s = min(max(kf.off[cx * kGridRows + q.minCY], 0), kf.nIn); s < sEnd; s++) {
            const int idx = min(max(kf.gi[s], 0), kf.capacity - 1);
            const float kx = kf.K[idx].x, ky = kf.K[idx].y;
            if (!(fabsf(__fsub_rn(kx, q.u)) < q.r && fabsf(__fsub_rn(ky, q.v)) < q.r)) continue;      // KeyFrame.cc:804-808
            any = true;
            body(s, idx, kx, ky);
        }
    }
    return any;
}

// Fuse's candidate tests and strict minimum over q's window (:1511-1570, :1702-1712): bestDist / bestIdx (256 / -1 on entry) of the keypoints of
// level q.level - 1 .. q.level that pass the reprojection test (p.reprojCheck; the loop-closing overload has none).  Returns the visit's `any`.
// kStereo chooses at compile time whether a keypoint can have a right coordinate (UR[idx] >= 0, UR may be NULL: the 7.8 test on (u, v, ur),
// :1533-1546) or not (the 5.99 test on (u, v), :1547-1557).  A two-camera keyframe (NLeft != -1) is never stereo: its mvuRight has Nleft
// entries, all -1 (src/Frame.cc:1150), so ur, invz and mbf have no observable effect and its kernel carries no code for them.  (The
// reference indexes that mvuRight with the right eye's own index, :1533 before :1559: past the array where Nright > Nleft.  -1 is taken.)
// P: invSigma2[], reprojCheck, and with kStereo mbf.
template <bool kStereo, class P>
__device__ __forceinline__ bool fuseBest(const KeyFrameView& kf, const KfProjection& q, const float* UR, const uint4& dlo, const uint4& dhi,
                                         const P& p, int& bestDist, int& bestIdx) {
    float ur = 0.f;
    if constexpr (kStereo) ur = __fsub_rn(q.u, __fmul_rn(p.mbf, q.invz));                    // :1479
    // a candidate's kpLevel is level or level - 1 (:1530): the two mvInvLevelSigma2 it can need
    const float invHi = p.invSigma2[q.level], invLo = p.invSigma2[max(q.level - 1, 0)];
    return keyFrameVisitArea(kf, q, [&](int, int idx, float kx, float ky) {
        const int lv = kf.K[idx].octave;
        if (lv < q.level - 1 || lv > q.level) return;                                        // :1530
        if (p.reprojCheck) {
            const float inv = lv == q.level ? invHi : invLo;      // mvInvLevelSigma2[kpLevel]; level - 1 = -1 reads entry 0 (the reference would index past the table)
            const float ex = __fsub_rn(q.u, kx), ey = __fsub_rn(q.v, ky);
            const float e2m = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
            float kr = -1.0f;
            if constexpr (kStereo) kr = UR ? UR[idx] : -1.0f;
            if (kr >= 0.0f) {                                                                // :1533-1546
                const float er = __fsub_rn(ur, kr);
                if ((double)__fmul_rn(__fadd_rn(e2m, __fmul_rn(er, er)), inv) > 7.8) return;
            } else if ((double)__fmul_rn(e2m, inv) > 5.99) return;                           // :1547-1557
        }
        const uint4 e = kf.D[2 * idx], g = kf.D[2 * idx + 1];
        const int dist = hamming256(dlo, dhi, e, g);
        if (dist < bestDist) { bestDist = dist; bestIdx = idx; }                             // :1565, strict: the first of equals stays
    });
}

// Fuse's tail for result o.  code: the exit that ended the search (kFuseFlag, the front end's 1 .. 5; kFrontEmptyWindow also where fuseBest
// found the area empty, :1509) or kFrontPassed: bestIdx / bestDist stand, bestIdx in the KEYFRAME's numbering.  Returns the exit.  P: thLow.
template <class P>
__device__ __forceinline__ int fuseFinish(int code, int bestIdx, int bestDist, const P& p, long long o, int* __restrict__ bestIdxOut,
                                          int* __restrict__ bestDistOut, uint8_t* __restrict__ exitOut) {
    if (code == kFrontPassed) code = bestIdx >= 0 && bestDist <= p.thLow ? kFuseFused : kFuseAboveThLow;      // :1573
    bestIdxOut[o] = code == kFuseFused ? bestIdx : -1;
    bestDistOut[o] = bestDist;
    if (exitOut) exitOut[o] = (uint8_t)code;
    return code;
}

}  // namespace orbx
