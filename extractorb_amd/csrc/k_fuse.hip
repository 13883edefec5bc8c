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
// This file is also compiled for the HOST by the CPU suite (tests/cpp/fuse_host_check.cpp includes it behind tests/cpp/host_shim/hip/
// hip_runtime.h, a hand-written stand-in for the device vocabulary used here).  An intrinsic, builtin or vector type this kernel gains must
// get its stand-in there in the same change, or the CPU suite no longer builds; the wave-wide count into nFused is not emulated there.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orbx_device.hpp"

namespace orbx {

struct FuseParams {      // == orbx_internal.hpp
    float fx, fy, cx, cy, minX, maxX, minY, maxY, wInv, hInv;
    float scale[kMaxLevels], invSigma2[kMaxLevels];      // mvScaleFactors, mvInvLevelSigma2 of the handle
    float breaks[kMaxLevels];                            // [k - 1]: smallest ratio whose predicted level is >= k (k = 1 .. nlevels - 1)
    float mbf, th;
    int nlevels, thLow, reprojCheck, capacity, mpCapacity, kfFirst, kfStep, mpFirst, mpStep;
};

namespace {
constexpr int kCols = 64, kRows = 48, kCells = kCols * kRows;
enum { kExitFlag = 0, kExitNegDepth, kExitNotInImage, kExitDistance, kExitNormal, kExitEmptyWindow, kExitAboveThLow, kExitFused };      // == ORBX_FUSE_*

// one row of cv::gemm on 3x3 * 3x1 float data: products and sums in double (each rounded), scaled, C added, rounded to float once
__device__ __forceinline__ float gemmRow(float a0, float a1, float a2, const float (&b)[3], double alpha, float c, bool hasC) {
    double s = __dmul_rn((double)a0, (double)b[0]);
    s = __dadd_rn(s, __dmul_rn((double)a1, (double)b[1]));
    s = __dadd_rn(s, __dmul_rn((double)a2, (double)b[2]));
    s = __dmul_rn(s, alpha);
    if (hasC) s = __dadd_rn(s, (double)c);
    return (float)s;
}
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
            const float* T = poses + f * 12;
            const float R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
            const float tcw[3] = {T[3], T[7], T[11]};
            const float xw[3] = {mpWorld[3 * m], mpWorld[3 * m + 1], mpWorld[3 * m + 2]};
            float xc[3];
            for (int r = 0; r < 3; r++) xc[r] = gemmRow(R[3 * r], R[3 * r + 1], R[3 * r + 2], xw, 1.0, tcw[r], true);      // Rcw*p3Dw+tcw (:1456)
            code = kExitNegDepth;
            if (xc[2] < 0.0f) break;                                                         // :1459
            const float invz = __fdiv_rn(1.0f, xc[2]);                                       // :1465, a float division
            const float u = __fadd_rn(__fdiv_rn(__fmul_rn(p.fx, xc[0]), xc[2]), p.cx);       // Pinhole::project
            const float v = __fadd_rn(__fdiv_rn(__fmul_rn(p.fy, xc[1]), xc[2]), p.cy);
            code = kExitNotInImage;
            if (!(u >= p.minX && u < p.maxX && v >= p.minY && v < p.maxY)) break;            // KeyFrame::IsInImage (z == 0: inf / NaN fail here)
            const float ur = __fsub_rn(u, __fmul_rn(p.mbf, invz));                           // :1479
            float Ow[3], PO[3];
            for (int r = 0; r < 3; r++) Ow[r] = gemmRow(R[r], R[3 + r], R[6 + r], tcw, -1.0, 0.f, false);      // -Rcw.t()*tcw (KeyFrame.cc:118, :1624)
            for (int r = 0; r < 3; r++) PO[r] = __fsub_rn(xw[r], Ow[r]);                     // :1483
            // cv::norm of CV_32F: squares accumulated in double in element order, one square root, then float
            const double n2 = __dadd_rn(__dadd_rn(__dmul_rn((double)PO[0], (double)PO[0]), __dmul_rn((double)PO[1], (double)PO[1])),
                                        __dmul_rn((double)PO[2], (double)PO[2]));
            const float dist3D = (float)__dsqrt_rn(n2);
            const float minDistance = mpDist[3 * m], maxDistance = mpDist[3 * m + 1];
            code = kExitDistance;
            if (dist3D < minDistance || dist3D > maxDistance) break;                         // :1487
            const double dot = __dadd_rn(__dadd_rn(__dmul_rn((double)PO[0], (double)mpNormal[3 * m]), __dmul_rn((double)PO[1], (double)mpNormal[3 * m + 1])),
                                         __dmul_rn((double)PO[2], (double)mpNormal[3 * m + 2]));
            code = kExitNormal;
            if (dot < __dmul_rn(0.5, (double)dist3D)) break;                                 // :1496
            // MapPoint::PredictScale as a count of breakpoints (ascending; NaN is above none, +inf above all)
            const float ratio = __fdiv_rn(mpDist[3 * m + 2], dist3D);                        // mfMaxDistance itself, not 1.2f * it (MapPoint.cc:519)
            int level = 0;
#pragma unroll
            for (int k = 1; k < kMaxLevels; k++) level += k < p.nlevels && ratio >= p.breaks[k - 1] ? 1 : 0;
            // a candidate's kpLevel is level or level - 1 (:1530): the two mvInvLevelSigma2 it can need
            const float invHi = p.invSigma2[level], invLo = p.invSigma2[max(level - 1, 0)];
            const float r = __fmul_rn(p.th, p.scale[level]);                                 // :1505
            // KeyFrame::GetFeaturesInArea's cell window with its four early returns (KeyFrame.cc:778-792)
            code = kExitEmptyWindow;
            const int minCX = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(u, p.minX), r), p.wInv)));
            if (minCX >= kCols) break;
            const int maxCX = min(kCols - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(u, p.minX), r), p.wInv)));
            if (maxCX < 0) break;
            const int minCY = max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(v, p.minY), r), p.hInv)));
            if (minCY >= kRows) break;
            const int maxCY = min(kRows - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(v, p.minY), r), p.hInv)));
            if (maxCY < 0) break;
            const int N = min(max(nOut[f], 0), p.capacity);
            const int* off = gridOff + f * (kCells + 1);
            const int* gi = gridIdx + f * p.capacity;
            const Keypoint* K = kpsUn + f * p.capacity;
            const float* UR = uRight ? uRight + f * p.capacity : nullptr;
            const uint4* D = (const uint4*)(desc + f * p.capacity * 32);
            const int nIn = min(max(off[kCells], 0), N);                                     // (clamped: a corrupt grid must not index past the frame)
            const uint4 dlo = *(const uint4*)(mpDesc + m * 32), dhi = *(const uint4*)(mpDesc + m * 32 + 16);
            bool any = false;
            for (int cx = minCX; cx <= maxCX; cx++) {
                if (minCY > maxCY) break;
                const int sEnd = min(max(off[cx * kRows + maxCY + 1], 0), nIn);
                for (int s = min(max(off[cx * kRows + minCY], 0), nIn); s < sEnd; s++) {
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
                    const int dist = __popc(dlo.x ^ e.x) + __popc(dlo.y ^ e.y) + __popc(dlo.z ^ e.z) + __popc(dlo.w ^ e.w) + __popc(dhi.x ^ g.x) +
                                     __popc(dhi.y ^ g.y) + __popc(dhi.z ^ g.z) + __popc(dhi.w ^ g.w);
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
