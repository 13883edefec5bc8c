// k_match_helpers.hpp - the lines of the reference that every matcher kernel restates, stated ONCE: ORBmatcher::DescriptorDistance,
// Frame / KeyFrame::GetFeaturesInArea's cell window, the rotation-histogram bin, ORBmatcher::ComputeThreeMaxima, the sorted best-key list,
// cv::gemm on 3x3 data and Mat::dot / cv::norm on three floats (dot3Double, which the geometry entries take through k_small_math.hpp).  Their exact rounding and tie order are the reference's; a correction here reaches every kernel.  A new matcher entry
// uses these and adds what it shares to this file.
// Plain arithmetic only - nothing that talks to other lanes (that is k_wave_min.hpp) - so the kernels the CPU suite compiles for the HOST
// (k_fuse.hip, k_project_sim3.hip, k_frustum_point.hpp behind tests/cpp/host_shim) can include it, and tests/cpp/match_helpers_check.cpp
// tests these statements directly.  A device word this header gains needs its stand-in in the shim.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orbx_device.hpp"

namespace orbx {

constexpr int kHistoLength = 30;      // HISTO_LENGTH, ORBmatcher.cc:38

// ORBmatcher::DescriptorDistance (:2349-2365): 256-bit Hamming distance of the descriptors (a, b) and (x, y), each two 128-bit halves.
// V: HIP's uint4 or a compiler vector of four uint32_t (k_triangulate_match.hip's, which can live behind an address space).
// By reference: callers hand over LDS lvalues, and by value k_search_proj_two_eyes came out different and measurably slower.
template <class V>
__device__ __forceinline__ int hamming256(const V& a, const V& b, const V& x, const V& y) {
    return __popc(a.x ^ x.x) + __popc(a.y ^ x.y) + __popc(a.z ^ x.z) + __popc(a.w ^ x.w) + __popc(b.x ^ y.x) + __popc(b.y ^ y.y) +
           __popc(b.z ^ y.z) + __popc(b.w ^ y.w);
}

// GetFeaturesInArea's cell window along one axis (Frame.cc:666-688, KeyFrame.cc:778-792) for a request at c with radius r: lo = mnMinX / mnMinY,
// inv = mfGridElementWidthInv / HeightInv, cells = FRAME_GRID_COLS / ROWS.  The callers keep the order of the reference's early returns.
__device__ __forceinline__ int cellWindowMin(float c, float lo, float r, float inv) {
    return max(0, (int)floorf(__fmul_rn(__fsub_rn(__fsub_rn(c, lo), r), inv)));
}
__device__ __forceinline__ int cellWindowMax(float c, float lo, float r, float inv, int cells) {
    return min(cells - 1, (int)ceilf(__fmul_rn(__fadd_rn(__fsub_rn(c, lo), r), inv)));
}
// Frame::GetFeaturesInArea's window of a request at (u, v); false: empty, no candidates.  P: minX, minY, wInv, hInv.
template <class P>
__device__ __forceinline__ bool frameCellWindow(float u, float v, float r, const P& p, int& minCX, int& maxCX, int& minCY, int& maxCY) {
    minCX = cellWindowMin(u, p.minX, r, p.wInv);
    maxCX = cellWindowMax(u, p.minX, r, p.wInv, kGridCols);
    minCY = cellWindowMin(v, p.minY, r, p.hInv);
    maxCY = cellWindowMax(v, p.minY, r, p.hInv, kGridRows);
    return !(minCX >= kGridCols || maxCX < 0 || minCY >= kGridRows || maxCY < 0 || minCX > maxCX || minCY > maxCY);
}

// rotHist's bin of a match (ORBmatcher.cc:773-783 and its copies in every search): rot = angle1 - angle2, 360 added once if negative,
// round(rot * factor) with factor = 1.0f / HISTO_LENGTH as the reference has it (angles in [0, 360) reach bins 0 .. 12), bin 30 wraps to 0
__device__ __forceinline__ int rotationBin(float angle1, float angle2) {
    const float factor = 1.0f / kHistoLength;
    float rot = __fsub_rn(angle1, angle2);
    if (rot < 0.0f) rot = __fadd_rn(rot, 360.0f);
    int bin = (int)roundf(__fmul_rn(rot, factor));
    if (bin == kHistoLength) bin = 0;
    return bin;
}

// ORBmatcher::ComputeThreeMaxima (:2303-2344) over the kHistoLength bin sizes: the bins of the three largest counts (strict ">": of equal counts
// the lower bin takes the higher rank), -1 for a second / third below a tenth of the first.  An empty histogram leaves all three -1.
struct ThreeMaxima { int ind1, ind2, ind3; };
template <class Hist>
__device__ __forceinline__ ThreeMaxima computeThreeMaxima(const Hist& hist) {
    int ind1 = -1, ind2 = -1, ind3 = -1, max1 = 0, max2 = 0, max3 = 0;
    for (int i = 0; i < kHistoLength; i++) {
        const int s = hist[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
        else if (s > max3) { max3 = s; ind3 = i; }
    }
    if ((float)max2 < __fmul_rn(0.1f, (float)max1)) { ind2 = -1; ind3 = -1; }
    else if ((float)max3 < __fmul_rn(0.1f, (float)max1)) ind3 = -1;
    return ThreeMaxima{ind1, ind2, ind3};
}

// Insert key k into the ascending list keys[N], dropping the largest.  Keys are (distance << 16 | slot) with slots ascending in the reference's
// traversal order, so of equal distances the first visited stays in front (the strict "<" of the reference's running minimum).
// (k_search_proj's window scan in k_project.hip has these three statements written out: called from there the search measured 3 % slower.)
template <int N>
__device__ __forceinline__ void sortedInsert(int (&keys)[N], int k) {
#pragma unroll
    for (int t = 0; t < N; t++) { const int lo = min(keys[t], k); k = max(keys[t], k); keys[t] = lo; }
}

// one row of cv::gemm on 3x3 * 3x1 float data: products and sums in double (each rounded), scaled, C added, rounded to float once
__device__ __forceinline__ float gemmRow(float a0, float a1, float a2, const float (&b)[3], double alpha, float c, bool hasC) {
    double s = __dmul_rn((double)a0, (double)b[0]);
    s = __dadd_rn(s, __dmul_rn((double)a1, (double)b[1]));
    s = __dadd_rn(s, __dmul_rn((double)a2, (double)b[2]));
    s = __dmul_rn(s, alpha);
    if (hasC) s = __dadd_rn(s, (double)c);
    return (float)s;
}

// A 3x3 * 3x3 cv::Mat product of float data (Rrl * mRcw of Frame::isInFrustumChecks): every element is one gemmRow of a row of A and a column
// of B, no addend.  A and B are row-major with row strides sa / sb (3 for a 3x3 block, 4 for the rotation of a 3x4 pose); out is 3x3 row-major.
// Parity unpinned, as the other cv::Mat roundings of the matchers: a later pin against the reference's cv::gemm changes this one place.
__device__ __forceinline__ float gemmMat3Element(const float* A, int sa, const float* B, int sb, int r, int c) {
    const float col[3] = {B[c], B[sb + c], B[2 * sb + c]};
    return gemmRow(A[sa * r], A[sa * r + 1], A[sa * r + 2], col, 1.0, 0.f, false);
}
__device__ __forceinline__ void gemmMat3(const float* A, int sa, const float* B, int sb, float* out) {
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) out[3 * r + c] = gemmMat3Element(A, sa, B, sb, r, c);
}

// Mat::dot / cv::norm's sum on CV_32F data: three products and two sums in binary64, in element order
__device__ __forceinline__ double dot3Double(float a0, float a1, float a2, float b0, float b1, float b2) {
    return __dadd_rn(__dadd_rn(__dmul_rn((double)a0, (double)b0), __dmul_rn((double)a1, (double)b1)), __dmul_rn((double)a2, (double)b2));
}

}  // namespace orbx
