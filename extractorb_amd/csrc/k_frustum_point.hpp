// k_frustum_point.hpp - what the tracker does to ONE MapPoint between "the local map exists" and "the matcher has a search request":
//   kFrustumLocalMap        Frame::isInFrustum, the Nleft == -1 branch (reference src/Frame.cc:493-570; caller Tracking::SearchLocalPoints,
//                           src/Tracking.cc:2941-2959) plus the prelude of ORBmatcher::SearchByProjection(F, vpMapPoints, th, bFarPoints,
//                           thFarPoints) (src/ORBmatcher.cc:50-73) with RadiusByViewingCos (:216-222)
//   kFrustumRelocalization  the front half of ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)
//                           (src/ORBmatcher.cc:2183-2230)
// It is a statement of its own and NOT projectIntoKeyFrame of k_keyframe_project.hpp: the bounds are Frame's FLOAT mnMinX .. mnMaxY with
// NON-STRICT tests (uv.x < mnMinX || uv.x > mnMaxX, src/Frame.cc:520-523, src/ORBmatcher.cc:2209-2212), not KeyFrame's truncated, strict
// ones; there is no cell window; the viewing-angle test has another form (below); the relocalisation path has no depth test at all.  What
// is shared: gemmRow (cv::gemm) and dot3Double (cv::norm / Mat::dot) of k_match_helpers.hpp, and predictScaleLevel
// (MapPoint::PredictScale as a count of breakpoints, k_keyframe_project.hpp).
// The arithmetic is the reference's x86-64 build, every operation rounded on its own (-ffp-contract=off and the __f*_rn / __d*_rn
// intrinsics).  Where the forms matter:
//   * Pc_dist, dist = cv::norm of CV_32F: squares summed in double in element order, one square root, then float;
//   * invz = 1.0f / PcZ is a FLOAT division (src/Frame.cc:512) and z == 0 is not rejected: it goes on to Pinhole::project
//     (fx*x/z + cx, src/CameraModels/Pinhole.cpp:30-33), and +-inf leaves by the bounds because the comparisons keep the reference's form;
//   * viewCos = PO.dot(Pn) / dist (src/Frame.cc:545): Mat::dot returns a double accumulated in element order, dist is promoted, the quotient
//     is a DOUBLE division stored to float, and THAT float is compared with viewingCosLimit.  Fuse's normal test (dot < 0.5 * dist in
//     double, src/ORBmatcher.cc:1496) is another predicate: a quotient just below 0.5 that rounds to 0.5f passes here and fails there.
//   * RadiusByViewingCos compares the float with the DOUBLE literal 0.998 (src/ORBmatcher.cc:218).
// Also compiled for the HOST by the CPU suite (tests/cpp/frustum_host_check.cpp behind tests/cpp/host_shim/frustum_shim.h): a device word
// this header gains needs its stand-in there.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_keyframe_project.hpp"
#include "orbx_device.hpp"
#include "orbx_params.hpp"

namespace orbx {

enum { kFrustumLocalMap = 0, kFrustumRelocalization = 1 };                                        // == ORBX_FRUSTUM_LOCAL_MAP / _RELOCALIZATION
enum { kFrustumFlag = 0, kFrustumNegDepth, kFrustumNotInImage, kFrustumDistance, kFrustumViewCos, kFrustumFar, kFrustumRequest };      // == orbx_frustum_exit

// what a MapPoint that is not looked at carries (bit 0 of its flag clear, or beyond the list): every byte defined
__device__ __forceinline__ TrackRecord frustumUntouched() { return TrackRecord{-1.0f, -1.0f, 0.0f, 0.0f, 0.0f, -1, kFrustumFlag}; }

// T: the 12 floats of the frame's pose (Rcw | tcw rows); xwp / nrm / dst: the MapPoint's position, normal (read in the local-map mode only)
// and (min invariance, max invariance, mfMaxDistance); angle: pKF->mvKeysUn[i].angle (relocalisation only); flag: bit 0 = look at it, bit 1
// = Observations() > 0.  Returns the exit; t is what isInFrustum leaves in the MapPoint, q the request (all zero unless the exit is
// kFrustumRequest).
template <class P>
__device__ __forceinline__ int frustumPoint(const float* __restrict__ T, const float* __restrict__ xwp, const float* __restrict__ nrm,
                                            const float* __restrict__ dst, float angle, int flag, const P& p, TrackRecord& t, ProjQuery& q) {
    t = frustumUntouched();                                                          // Frame.cc:497-499: mTrackProjX = mTrackProjY = -1
    q = ProjQuery{0.f, 0.f, 0.f, 0.f, 0, 0, 0, 0.f};
    if (!(flag & 1)) return kFrustumFlag;                                            // Tracking.cc:2945-2948 / ORBmatcher.cc:2199-2201
    const bool local = p.mode == kFrustumLocalMap;
    const float R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
    const float tcw[3] = {T[3], T[7], T[11]};
    const float xw[3] = {xwp[0], xwp[1], xwp[2]};
    float xc[3];
    for (int r = 0; r < 3; r++) xc[r] = gemmRow(R[3 * r], R[3 * r + 1], R[3 * r + 2], xw, 1.0, tcw[r], true);      // mRcw*P+mtcw (Frame.cc:507, ORBmatcher.cc:2205)
    float depth = 0.f, invz = 0.f;
    if (local) {
        const double c2 = dot3Double(xc[0], xc[1], xc[2], xc[0], xc[1], xc[2]);
        depth = (float)__dsqrt_rn(c2);                                               // Pc_dist = cv::norm(Pc) (:508)
        invz = __fdiv_rn(1.0f, xc[2]);                                               // :512, a float division, in front of the test
        if (xc[2] < 0.0f) return t.exit = kFrustumNegDepth;                          // :513 (z == 0 goes on).  The relocalisation path has NO depth test.
    }
    const float u = __fadd_rn(__fdiv_rn(__fmul_rn(p.fx, xc[0]), xc[2]), p.cx);       // Pinhole::project
    const float v = __fadd_rn(__fdiv_rn(__fmul_rn(p.fy, xc[1]), xc[2]), p.cy);
    if (u < p.minX || u > p.maxX) return t.exit = kFrustumNotInImage;                // :520-523 / :2209-2212, the reference's own form: both ends pass
    if (v < p.minY || v > p.maxY) return t.exit = kFrustumNotInImage;
    t.projX = u; t.projY = v;                                                        // :526-527, kept when a later test fails
    float Ow[3], PO[3];
    for (int r = 0; r < 3; r++) Ow[r] = gemmRow(R[r], R[3 + r], R[6 + r], tcw, -1.0, 0.f, false);      // mOw = -mRcw.t()*mtcw (Frame.cc:466-472, ORBmatcher.cc:2185)
    for (int r = 0; r < 3; r++) PO[r] = __fsub_rn(xw[r], Ow[r]);                     // :532 / :2215
    const double n2 = dot3Double(PO[0], PO[1], PO[2], PO[0], PO[1], PO[2]);
    const float dist = (float)__dsqrt_rn(n2);                                        // :533 / :2216
    if (dist < dst[0] || dist > dst[1]) return t.exit = kFrustumDistance;            // :535 / :2222, both ends pass
    float viewCos = 0.f;
    if (local) {
        const double dot = dot3Double(PO[0], PO[1], PO[2], nrm[0], nrm[1], nrm[2]);
        viewCos = (float)__ddiv_rn(dot, (double)dist);                               // :545: a double quotient stored to float
        if (viewCos < p.viewCosLimit) return t.exit = kFrustumViewCos;               // :547
    }
    const float ratio = __fdiv_rn(dst[2], dist);                                     // mfMaxDistance itself (MapPoint.cc:519)
    const int level = predictScaleLevel(ratio, p);                                   // :551 / :2225
    t.level = level;
    if (!local) {
        q = ProjQuery{u, v, 0.f, __fmul_rn(p.th, p.scale[level]), level - 1, level + 1, 3, angle};      // :2228-2230
        return t.exit = kFrustumRequest;
    }
    t.projXR = __fsub_rn(u, __fmul_rn(p.mbf, invz));                                 // :558
    t.depth = depth;                                                                 // :560
    t.viewCos = viewCos;                                                             // :565
    if (p.farPoints && depth > p.thFarPoints) return t.exit = kFrustumFar;           // ORBmatcher.cc:56: mbTrackInView, counted, but not searched
    // RadiusByViewingCos (:216-222) compares the float with the double literal 0.998.  (double)0.998f = 0.998000026 lies above it and the
    // float below 0.998f lies below it, so the test is viewCos >= 0.998f - NOT "> 0.998f".
    float r = (double)viewCos > 0.998 ? 2.5f : 4.0f;
    if (p.th != 1.0f) r = __fmul_rn(r, p.th);                                        // bFactor (:48, :69-70)
    q = ProjQuery{u, v, t.projXR, __fmul_rn(r, p.scale[level]), level - 1, level, 1 | (flag & 2), 0.f};      // :73; ur = mTrackProjXR
    return t.exit = kFrustumRequest;
}

}  // namespace orbx
