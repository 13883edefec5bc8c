// k_project_last_two_eyes_point.hpp - one request of the front half of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono)
// for two-camera frames (reference src/ORBmatcher.cc:1971-2023 and :2084-2101 with CurrentFrame.Nleft != -1): MapPoint j of the last rig
// (j = eye * capacity + i: the left eye's keypoints, then the right eye's, the reference's order i < Nleft, i >= Nleft) becomes a left and a
// right search request under the current rig's pose.  One thread per request in k_project_last_two_eyes; plain arithmetic, so the CPU suite
// compiles it for the host (tests/cpp/last_two_eyes_host_check.cpp behind tests/cpp/host_shim) and walks it under the sanitizers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_camera_kb8.hpp"
#include "k_match_helpers.hpp"
#include "orbx_device.hpp"
#include "orbx_params.hpp"

namespace orbx {

enum LastTwoEyesExit { kLastNoMapPoint = 0, kLastNegDepth = 1, kLastOutside = 2, kLastRequest = 3 };

// poses: one 3x4 row-major mTcw per RIG frame; kps, nOut, mpFlags, world: per device frame (2r: left eye, 2r + 1: right eye).
// Writes both requests (all zero where the reference `continue`s) and returns where the MapPoint left.
__device__ __forceinline__ int projectLastTwoEyesRequest(const Keypoint* kps, const int* nOut, const uint8_t* mpFlags, const float* world,
                                                         const float* poses, const ProjectTwoEyesParams& p, int pair, int j, ProjQuery& qL,
                                                         ProjQuery& qR) {
    qL = ProjQuery{0.f, 0.f, 0.f, 0.f, 0, 0, 0, 0.f};
    qR = qL;
    const int eye = j >= p.capacity, i = j - eye * p.capacity;
    const int rl = p.lastFirst + pair * p.lastStep, rc = p.curFirst + pair * p.curStep;
    const long long f = 2LL * rl + eye;
    const int NE = min(max(nOut[f], 0), p.capacity);       // Nleft / Nright of the last rig
    const uint8_t fl8 = i < NE ? mpFlags[f * p.capacity + i] : (uint8_t)0;
    if (!(fl8 & 1)) return kLastNoMapPoint;                                       // ORBmatcher.cc:1987-1990
    const float* C = poses + (long long)rc * 12;
    const float* L = poses + (long long)rl * 12;
    const float tcw[3] = {C[3], C[7], C[11]};
    float twc[3], tlc[3];
    for (int r = 0; r < 3; r++) twc[r] = gemmRow(C[r], C[4 + r], C[8 + r], tcw, -1.0, 0.f, false);      // -Rcw.t()*tcw (:1974)
    for (int r = 0; r < 3; r++) tlc[r] = gemmRow(L[4 * r], L[4 * r + 1], L[4 * r + 2], twc, 1.0, L[4 * r + 3], true);   // Rlw*twc+tlw (:1979)
    const bool bForward = tlc[2] > p.mb && !p.mono, bBackward = -tlc[2] > p.mb && !p.mono;                // :1981-1982
    const float* X = world + (f * p.capacity + i) * 3;
    const float xw[3] = {X[0], X[1], X[2]};
    float xc[3], xr[3];
    for (int r = 0; r < 3; r++) xc[r] = gemmRow(C[4 * r], C[4 * r + 1], C[4 * r + 2], xw, 1.0, C[4 * r + 3], true);   // Rcw*x3Dw+tcw (:1993)
    const float invzc = (float)__ddiv_rn(1.0, (double)xc[2]);                     // :1997
    if (invzc < 0) return kLastNegDepth;
    float u, v;
    kb8Project(p.cam, xc[0], xc[1], xc[2], u, v);                                 // CurrentFrame.mpCamera->project(x3Dc) (:2002)
    if (u < p.minX || u > p.maxX || v < p.minY || v > p.maxY) return kLastOutside;   // :2004-2007
    const Keypoint kp = kps[f * p.capacity + i];                                  // mvKeys[i] / mvKeysRight[i - Nleft], RAW (:2009-2010, :2066-2068)
    const int oct = min(max(kp.octave, 0), kMaxLevels - 1);
    qL.u = u; qL.v = v;
    qL.radius = __fmul_rn(p.th, p.scale[oct]);                                    // :2013
    if (bForward) { qL.minLevel = oct; qL.maxLevel = -1; }                        // :2017-2022
    else if (bBackward) { qL.minLevel = 0; qL.maxLevel = oct; }
    else { qL.minLevel = oct - 1; qL.maxLevel = oct + 1; }
    qL.angle = kp.angle;
    qL.flags = 1 | (fl8 & 2);
    // the right eye (:2084-2101): mTrl * x3Dc as a cv::Mat product, projected with the LEFT camera's parameters (mpCamera, not mpCamera2),
    // no depth test and no bounds test; same radius and level range
    for (int r = 0; r < 3; r++) xr[r] = gemmRow(p.trl[4 * r], p.trl[4 * r + 1], p.trl[4 * r + 2], xc, 1.0, p.trl[4 * r + 3], true);
    qR = qL;
    kb8Project(p.cam, xr[0], xr[1], xr[2], qR.u, qR.v);
    return kLastRequest;
}

}  // namespace orbx
