// k_frustum_two_eyes_point.hpp - what the tracker does to ONE MapPoint of the local map on a TWO-CAMERA rig (Nleft != -1, a KannalaBrandt8
// pair) between "the local map exists" and "the matcher has its two search requests":
//   Frame::isInFrustum's else branch (reference src/Frame.cc:571-581) = Frame::isInFrustumChecks once per eye (:1181-1254), called from the
//   loop of Tracking::SearchLocalPoints (src/Tracking.cc:2941-2959), plus the prelude of ORBmatcher::SearchByProjection(F, vpMapPoints, th,
//   bFarPoints, thFarPoints) for F.Nleft != -1 (src/ORBmatcher.cc:50-73, :145-151) with RadiusByViewingCos (:216-222).
// The one-camera statement is frustumPoint of k_frustum_point.hpp.  What differs, beyond the camera model and the second eye:
//   * a check that returns false assigns NOTHING (no mTrackProjX = uv.x in front of the distance test as at :526-527, no invz): the record
//     of an eye that is not in view is -1, -1, 0, 0, 0, -1 whatever test it left by (-1 is the level :574-575 leave);
//   * the right eye has its own pose (mR = Rrl*Rcw, mt = Rrl*tcw + trl), its own centre (twc = mRwc*mTlr.col(3) + mOw) and its own camera
//     (mpCamera2, :1210) - unlike the frame-to-frame search, which projects both eyes with mpCamera;
//   * the far test (:56) reads mTrackDepth, the LEFT eye's Pc_dist, also for a MapPoint only the right eye sees: then nothing assigned it in
//     this frame and the reference reads what an earlier frame left there, which the caller passes in (prevDepth);
//   * the left radius takes th (:69-70), the right one does not (:148).
// Every operation is rounded on its own, in the forms the tree already has: gemmRow / gemmMat3 (cv::gemm, k_match_helpers.hpp), cv::norm and
// Mat::dot accumulated in double in element order (dot3Double, k_match_helpers.hpp; the norm: one __dsqrt_rn, then float), predictScaleLevel
// (k_keyframe_project.hpp), kb8Project (k_camera_kb8.hpp).  The cv::Mat roundings are parity unpinned, as Fuse's.
// Plain arithmetic only, nothing that talks to other lanes: also compiled for the HOST by the CPU suite (tests/cpp/frustum_two_eyes_host_check.cpp
// behind tests/cpp/host_shim/kb8_shim.h).  A device word this header gains needs its stand-in there.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_camera_kb8.hpp"
#include "k_frustum_point.hpp"
#include "k_match_helpers.hpp"
#include "orbx_device.hpp"
#include "orbx_params.hpp"

namespace orbx {

// what isInFrustumChecks works with for one eye, as fifteen floats: mR (row-major) at 0..8, mt at 9..11, twc at 12..14.  Invariants of the rig
// frame: computed once per pair, not per MapPoint.
constexpr int kFrustumEyeFloats = 15;

// T: the rig frame's pose (3x4 row-major, Rcw | tcw); trl / tlr: Frame::mTrl / mTlr (3x4 row-major) - both as the Frame holds them, neither is
// derived from the other.  eye[0]: mR = mRcw, mt = mtcw, twc = mOw = -mRcw.t()*mtcw (Frame.cc:466-472, :1194-1196).  eye[1] (:1187-1191):
// mR = Rrl*mRcw, a 3x3 product; mt = Rrl*mtcw + trl, ONE gemm with the addend; twc = mRwc*mTlr.col(3) + mOw, one gemm of the transposed
// mRcw with the float mOw as addend.
// Stated per ELEMENT j = eye * kFrustumEyeFloats + k of the two records, so that the kernel can deal the thirty elements to thirty lanes (at
// most two dependent gemm rows each) and the host build walks the same lines.
__device__ __forceinline__ float frustumTwoEyesRigElement(const float* T, const float* trl, const float* tlr, int j) {
    const int eye = j >= kFrustumEyeFloats, k = j - eye * kFrustumEyeFloats;
    const float tcw[3] = {T[3], T[7], T[11]};
    if (k < 9) {                                                                     // mR
        const int r = k / 3, c = k - 3 * r;
        return eye ? gemmMat3Element(trl, 4, T, 4, r, c) : T[4 * r + c];
    }
    if (k < 12) {                                                                    // mt
        const int r = k - 9;
        return eye ? gemmRow(trl[4 * r], trl[4 * r + 1], trl[4 * r + 2], tcw, 1.0, trl[4 * r + 3], true) : tcw[r];
    }
    const int r = k - 12;                                                            // twc
    const float ow = gemmRow(T[r], T[4 + r], T[8 + r], tcw, -1.0, 0.f, false);
    if (!eye) return ow;
    const float tlr3[3] = {tlr[3], tlr[7], tlr[11]};
    return gemmRow(T[r], T[4 + r], T[8 + r], tlr3, 1.0, ow, true);
}
__device__ __forceinline__ void frustumTwoEyesRig(const float* T, const float* trl, const float* tlr, float* eyes) {      // eyes[2 * kFrustumEyeFloats]
    for (int j = 0; j < 2 * kFrustumEyeFloats; j++) eyes[j] = frustumTwoEyesRigElement(T, trl, tlr, j);
}

// Frame::isInFrustumChecks for one eye (e: that eye's mR / mt / twc as 15 floats, k: that eye's camera).  Returns the test it left by
// (kFrustumNegDepth .. kFrustumViewCos) with t untouched, or kFrustumRequest with t = (uv, 0, Pc_dist, viewCos, level): in view - what the
// matcher's far test makes of it comes afterwards.  P: minX .. maxY, viewCosLimit, nlevels, breaks[].
template <class P>
__device__ __forceinline__ int frustumEyeCheck(const float* __restrict__ e, const float (&k)[8], const float* __restrict__ xwp,
                                               const float* __restrict__ nrm, const float* __restrict__ dst, const P& p, TrackRecord& t) {
    t = frustumUntouched();
    const float xw[3] = {xwp[0], xwp[1], xwp[2]};
    float xc[3];
    for (int r = 0; r < 3; r++) xc[r] = gemmRow(e[3 * r], e[3 * r + 1], e[3 * r + 2], xw, 1.0, e[9 + r], true);      // Pc = mR*P+mt (:1200)
    const double c2 = dot3Double(xc[0], xc[1], xc[2], xc[0], xc[1], xc[2]);
    const float depth = (float)__dsqrt_rn(c2);                                       // Pc_dist = cv::norm(Pc) (:1201)
    if (xc[2] < 0.0f) return t.exit = kFrustumNegDepth;                              // :1205 (z == 0 goes on)
    float u, v;
    kb8Project(k, xc[0], xc[1], xc[2], u, v);                                        // :1210-1211
    if (u < p.minX || u > p.maxX) return t.exit = kFrustumNotInImage;                // :1213-1216, the reference's own form: both ends pass and
    if (v < p.minY || v > p.maxY) return t.exit = kFrustumNotInImage;                //   a NaN passes every one of the four, as it does there
    float PO[3];
    for (int r = 0; r < 3; r++) PO[r] = __fsub_rn(xw[r], e[12 + r]);                 // PO = P - twc (:1221)
    const double n2 = dot3Double(PO[0], PO[1], PO[2], PO[0], PO[1], PO[2]);
    const float dist = (float)__dsqrt_rn(n2);                                        // :1222
    if (dist < dst[0] || dist > dst[1]) return t.exit = kFrustumDistance;            // :1224, both ends pass
    const double dot = dot3Double(PO[0], PO[1], PO[2], nrm[0], nrm[1], nrm[2]);
    const float viewCos = (float)__ddiv_rn(dot, (double)dist);                       // :1230: a double quotient stored to float
    if (viewCos < p.viewCosLimit) return t.exit = kFrustumViewCos;                   // :1232
    const float ratio = __fdiv_rn(dst[2], dist);                                     // mfMaxDistance itself (MapPoint.cc:519)
    t.level = predictScaleLevel(ratio, p);                                           // :1236
    t.projX = u; t.projY = v; t.depth = depth; t.viewCos = viewCos;                  // :1238-1251; proj_xr stays 0
    return t.exit = kFrustumRequest;
}

// ORBmatcher.cc:56 for a MapPoint some eye sees: bFarPoints && mTrackDepth > thFarPoints.  mTrackDepth is the LEFT eye's Pc_dist when the left
// check passed in this frame, else what an earlier frame left in the MapPoint (prevDepth; 0 when the caller has none: never far).
template <class P>
__device__ __forceinline__ bool frustumTwoEyesFar(bool leftInView, float leftDepth, float prevDepth, const P& p) {
    return p.farPoints && (leftInView ? leftDepth : prevDepth) > p.thFarPoints;
}

// The request of one eye, from its track record alone (it holds everything: u, v, view_cos, level) and the MapPoint's input flag.  An eye in
// view of a MapPoint that is not far has exit == kFrustumRequest; every other eye's request is all zero apart from bit 1 of the flag.
// mnTrackScaleLevelR != -1 (:147) is always true for a right eye in view - isInFrustumChecks assigns the level whenever it returns true - so
// there is no test for it.  P: th, scale[].
template <class P>
__device__ __forceinline__ ProjQuery frustumTwoEyesRequest(const TrackRecord& t, int eye, int flag, const P& p) {
    if (t.exit != kFrustumRequest) return ProjQuery{0.f, 0.f, 0.f, 0.f, 0, 0, flag & 2, 0.f};
    // RadiusByViewingCos (:216-222): the float against the double literal 0.998, which is viewCos >= 0.998f (k_frustum_point.hpp)
    float r = (double)t.viewCos > 0.998 ? 2.5f : 4.0f;
    if (eye == 0 && p.th != 1.0f) r = __fmul_rn(r, p.th);                            // bFactor (:48, :69-70): the LEFT request only; :148 has no th
    return ProjQuery{t.projX, t.projY, 0.f, __fmul_rn(r, p.scale[t.level]), t.level - 1, t.level, 1 | (flag & 2), 0.f};      // :73 / :151
}

}  // namespace orbx
