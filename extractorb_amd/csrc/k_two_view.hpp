// k_two_view.hpp - TwoViewReconstruction::Reconstruct (reference src/TwoViewReconstruction.cc:39-125) behind Pinhole::ReconstructWithTwoViews
// (src/CameraModels/Pinhole.cpp:105-113): the monocular initialisation on the vnMatches12 that SearchForInitialization left in HBM.
// k_two_view.hip holds the three kernels around the three functions at the end of this file; everything they compute is stated here.
// The reference's own loops and orders are kept; what is OpenCV's (cv::SVD, cv::Mat kernels) is the project's definition, "parity unpinned"
// (DESIGN.md section 2), each stated ONCE, here or in k_small_svd.hpp:
//   matches      mvMatches12 = the (i, vMatches12[i]) with vMatches12[i] >= 0 in ascending i (:53-62); N = their count;
//   sets         mvSets[it][j] from the CALLER'S raw rand() values r (ints of [0, 2^31 - 1]): randi = int(((double)r / 2147483648.0) * (N - j))
//                (DUtils/Random.cpp:47-50), idx = avail[randi], avail[randi] = avail[N - j - 1] (:83-95) - at most eight displaced slots
//                of the identity, kept in registers (drawSet<8>, k_small_math.hpp).  randi is clamped into [0, N - j - 1]: a value outside [0, 2^31 - 1] is the
//                caller's error and must not index outside the list;
//   Normalize    :752-798 over ALL n keypoints of a frame, not the matched ones: four left-to-right binary32 sums, meanX / N a float
//                division, sX = 1.0 / meanDevX in double rounded once; T = [sX 0 -meanX*sX; 0 sY -meanY*sY; 0 0 1]; T2inv = inv3(T2);
//   ComputeH21   :229-269, A in binary32 as written, vt.row(8) = nullVector9<16>;  ComputeF21 :271-306, nullVector9<8>, svd3, w[2] = 0,
//                u * diag(w) * vt two gemm3;
//   products     T2inv*Hn*T1, T2t*Fn*T1, K.t()*F21*K, invK*H21*K, s*U*Rp*Vt: left to right, one gemm3 per product (s is the first one's alpha);
//   scores       CheckHomography :308-391, CheckFundamental :393-471 in binary32 with 1.0 / (float) in double rounded once; the score is
//                the reference's left-to-right sum: every lane computes the two terms of its match, the terms of a rejected distance are 0
//                (adding 0 is exact: the score is never -0), and ONE chain adds them in match order (tvChainAdd);
//   best         the first hypothesis with a strictly greater score, from 0: ties go to the lower iteration, a NaN score never wins;
//   RH           SH + SF == 0 rejects (:111); RH = SH / (SH + SF) in binary32; RH > rhThreshold takes H;
//   ReconstructF :473-574 with DecomposeE :912-932;  ReconstructH :576-735;  CheckRT :801-910;  Triangulate :737-750 is the row form of
//                k_new_map_points.hpp's A (float(p * P.row(2)[c]) - P.row(r)[c]) and nullVector4, skipped by a wave in which no lane has an
//                inlier (waveAny).  t / cv::norm(t) is fmul(t[c], (float)(1.0 / norm)) with the norm in double;
//   mixed precision   invZ = 1.0 / z in double rounded once; 4.0 * mSigma2 a double narrowed to float; d1 / d2 < 1.00001,
//                cosParallax < 0.99998, 0.9 * N, 0.7 * maxGood, 0.75 * bestGood compare in double; normal1.dot(normal2) and cv::norm in
//                double, dist narrowed to float, dist1 * dist2 a float product under a double division;
//   parallax     acos(vCosParallax[idx]) * 180 / CV_PI: acosFloat32 (k_acosf.hpp), a float product, a double division, narrowed.  idx =
//                min(50, size - 1) of the sorted list is a k-th smallest, taken by rank counting (ties do not change the value).  A NaN
//                cosine counts as larger than everything; when the rank falls on one the parallax is NaN (the reference's std::sort on
//                NaN is undefined).  A cosine above 1 gives NaN, on which :528's > and :724's >= are false.
// One workgroup is ONE WAVE everywhere (kTvLanes lanes); the host build (ORBX_HOST_ROW, tests/cpp/host_shim) runs the same functions
// with a wave of one lane: ballots are the lane's own bit, the chain adds one match at a time - the same order.
// Takes acosFloat32 from k_acosf.hpp, the null vectors / svd3 / det3 / inv3 / gemm3 from k_small_svd.hpp, drawSet / sqrtFloat32 / quietNaN /
// canonNaN / waveAny from k_small_math.hpp, gemmRow / dot3Double from k_match_helpers.hpp, the parameter blocks from orbx_params.hpp.
#pragma once
#include "k_acosf.hpp"
#include "k_lds_vec.hpp"
#include "k_match_helpers.hpp"
#include "k_small_math.hpp"
#include "k_small_svd.hpp"
#include "orbx_device.hpp"
#include "orbx_params.hpp"

namespace orbx {

// == orbx_two_view_status
enum {
    kTvAcceptedH = 0, kTvAcceptedF, kTvTooFewMatches, kTvBadIndex, kTvZeroScores, kTvHDegenerate, kTvHAmbiguous, kTvHLowParallax, kTvHFewPoints,
    kTvHBelowInlierShare, kTvFFewPoints, kTvFAmbiguous, kTvFLowParallax, kTvStatuses
};
constexpr int kTvRunning = -1;                            // TvPrep::status while no exit has been taken

// == orbx_two_view_result
struct TwoViewResult {
    int status, model, nMatches, bestItH, bestItF, nInliers, chosen;
    float SH, SF, RH;
    float H21[9], F21[9], R21[9], t21[3];
    int nGood[8];
    float parallax[8];
};

#ifdef ORBX_HOST_ROW
constexpr int kTvLanes = 1;
__device__ __forceinline__ float tvChainAdd(float score, float t1, float t2) { return __fadd_rn(__fadd_rn(score, t1), t2); }
#else
constexpr int kTvLanes = 64;
// score += t1[0]; score += t2[0]; score += t1[1]; ... over the lanes in order: one dependent add per term, uniform on every lane
__device__ __forceinline__ float tvChainAdd(float score, float t1, float t2) {
#pragma unroll 8
    for (int l = 0; l < kTvLanes; l++) {
        score = __fadd_rn(score, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t1), l)));
        score = __fadd_rn(score, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t2), l)));
    }
    return score;
}
#endif

constexpr int kTvHypLdsFloats = 2 * 16 * 9 + 81 + 18;    // the hypothesis wave: W, A0, V, then M21 | M12
constexpr int kTvMotionFloats = 27;                       // R[9] t[3] P2[12] O2[3]
constexpr int kTvDecideLdsFloats = 8 * kTvMotionFloats + 8 + 12;     // the motions, their parallaxes, then as ints a status and the motions' counts

__device__ __forceinline__ bool tvFinite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
__device__ __forceinline__ float tvInvDouble(float x) { return (float)__ddiv_rn(1.0, (double)x); }      // `1.0 / x` assigned to a float

// Normalize's two chains of one coordinate (comp 0: x, 1: y) over the n keypoints of a frame: the mean and the scale
__device__ __forceinline__ void tvNormalizeChain(const Keypoint* __restrict__ kps, int n, int comp, float& mean, float& s) {
    float sum = 0.0f;
    for (int i = 0; i < n; i++) sum = __fadd_rn(sum, comp ? kps[i].y : kps[i].x);
    mean = __fdiv_rn(sum, (float)n);
    float dev = 0.0f;
    for (int i = 0; i < n; i++) dev = __fadd_rn(dev, fabsf(__fsub_rn(comp ? kps[i].y : kps[i].x, mean)));
    s = tvInvDouble(__fdiv_rn(dev, (float)n));
}
__device__ __forceinline__ void tvNormalizeT(const float* norm4, float (&T)[9]) {
    T[0] = norm4[1]; T[1] = 0.0f; T[2] = __fmul_rn(-norm4[0], norm4[1]);
    T[3] = 0.0f; T[4] = norm4[3]; T[5] = __fmul_rn(-norm4[2], norm4[3]);
    T[6] = 0.0f; T[7] = 0.0f; T[8] = 1.0f;
}

// the null vector of a hypothesis to M21 | M12: T2inv*Hn*T1 and its inverse, or T2t*(rank-2 Fn)*T1 and zeros
__device__ __forceinline__ void tvDenormalise(int model, const float (&n9)[9], const TvPrep& pr, float (&m)[18]) {
    float T1[9], tmp[9], M21[9], M12[9];
#pragma unroll
    for (int c = 0; c < 9; c++) { T1[c] = pr.T1[c]; M12[c] = 0.0f; }
    if (model == 0) {
        float T2inv[9];
#pragma unroll
        for (int c = 0; c < 9; c++) T2inv[c] = pr.T2inv[c];
        gemm3(T2inv, n9, 1.0, tmp);
        gemm3(tmp, T1, 1.0, M21);
        inv3(M21, M12);
    } else {
        float U[9], w[3], Vt[9], T2t[9], Fn[9];
        svd3(n9, U, w, Vt);
        const float D[9] = {w[0], 0.f, 0.f, 0.f, w[1], 0.f, 0.f, 0.f, 0.0f};      // w.at<float>(2) = 0
        gemm3(U, D, 1.0, tmp);
        gemm3(tmp, Vt, 1.0, Fn);
#pragma unroll
        for (int c = 0; c < 9; c++) T2t[c] = pr.T2t[c];
        gemm3(T2t, Fn, 1.0, tmp);
        gemm3(tmp, T1, 1.0, M21);
    }
#pragma unroll
    for (int c = 0; c < 9; c++) { m[c] = M21[c]; m[9 + c] = M12[c]; }
}

// One hypothesis on ONE lane (:151-164 / :202-215): the set's normalised points, A, the null vector, the denormalised matrix and for H its
// inverse.  sW, sA0 (16 * 9 floats each) and sV (81) are the lane's memory; out18 = M21 | M12 (M12 zeros for F).
__device__ __forceinline__ void tvHypothesis(int model, const int (&idx)[8], const TvPrep& pr, const int* __restrict__ first,
                                             const int* __restrict__ second, const Keypoint* __restrict__ k1, const Keypoint* __restrict__ k2,
                                             ORBX_LDS float* sW, ORBX_LDS float* sA0, ORBX_LDS float* sV, ORBX_LDS float* out18) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const Keypoint a = k1[first[idx[j]]], b = k2[second[idx[j]]];
        const float u1 = __fmul_rn(__fsub_rn(a.x, pr.norm[0]), pr.norm[1]), v1 = __fmul_rn(__fsub_rn(a.y, pr.norm[2]), pr.norm[3]);
        const float u2 = __fmul_rn(__fsub_rn(b.x, pr.norm[4]), pr.norm[5]), v2 = __fmul_rn(__fsub_rn(b.y, pr.norm[6]), pr.norm[7]);
        if (model == 0) {
            const float row0[9] = {0.f, 0.f, 0.f, -u1, -v1, -1.f, __fmul_rn(v2, u1), __fmul_rn(v2, v1), v2};
            const float row1[9] = {u1, v1, 1.f, 0.f, 0.f, 0.f, __fmul_rn(-u2, u1), __fmul_rn(-u2, v1), -u2};
#pragma unroll
            for (int c = 0; c < 9; c++) { sW[18 * j + c] = sA0[18 * j + c] = row0[c]; sW[18 * j + 9 + c] = sA0[18 * j + 9 + c] = row1[c]; }
        } else {
            const float row[9] = {__fmul_rn(u2, u1), __fmul_rn(u2, v1), u2, __fmul_rn(v2, u1), __fmul_rn(v2, v1), v2, u1, v1, 1.f};
#pragma unroll
            for (int c = 0; c < 9; c++) sW[9 * j + c] = sA0[9 * j + c] = row[c];
        }
    }
    float n9[9], m[18];
    if (model == 0) nullVector9<16>(sW, sA0, sV, n9);
    else nullVector9<8>(sW, sA0, sV, n9);
    tvDenormalise(model, n9, pr, m);
#pragma unroll
    for (int c = 0; c < 18; c++) out18[c] = m[c];
}

#ifndef ORBX_HOST_ROW
// The same hypothesis with the ROWS OF A OVER THE LANES (nullVector9Wave): every lane draws the set and normalises the eight points
// (uniform), lane k builds row k of A, the null vector comes out uniform, and every lane denormalises it - no LDS, nothing to broadcast.
template <int M>
__device__ __forceinline__ void tvHypothesisSpread(const int (&idx)[8], const TvPrep& pr, const int* __restrict__ first,
                                                   const int* __restrict__ second, const Keypoint* __restrict__ k1, const Keypoint* __restrict__ k2,
                                                   float (&m)[18]) {
    constexpr int model = M == 16 ? 0 : 1;
    const int lane = (int)threadIdx.x, mine = model == 0 ? lane >> 1 : lane;
    float u1 = 0.f, v1 = 0.f, u2 = 0.f, v2 = 0.f;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const Keypoint a = k1[first[idx[j]]], b = k2[second[idx[j]]];
        const float pu1 = __fmul_rn(__fsub_rn(a.x, pr.norm[0]), pr.norm[1]), pv1 = __fmul_rn(__fsub_rn(a.y, pr.norm[2]), pr.norm[3]);
        const float pu2 = __fmul_rn(__fsub_rn(b.x, pr.norm[4]), pr.norm[5]), pv2 = __fmul_rn(__fsub_rn(b.y, pr.norm[6]), pr.norm[7]);
        if (mine == j) { u1 = pu1; v1 = pv1; u2 = pu2; v2 = pv2; }
    }
    float row[9];
    if (model == 0) {
        const float row0[9] = {0.f, 0.f, 0.f, -u1, -v1, -1.f, __fmul_rn(v2, u1), __fmul_rn(v2, v1), v2};
        const float row1[9] = {u1, v1, 1.f, 0.f, 0.f, 0.f, __fmul_rn(-u2, u1), __fmul_rn(-u2, v1), -u2};
#pragma unroll
        for (int c = 0; c < 9; c++) row[c] = lane & 1 ? row1[c] : row0[c];
    } else {
        const float rowF[9] = {__fmul_rn(u2, u1), __fmul_rn(u2, v1), u2, __fmul_rn(v2, u1), __fmul_rn(v2, v1), v2, u1, v1, 1.f};
#pragma unroll
        for (int c = 0; c < 9; c++) row[c] = rowF[c];
    }
#pragma unroll
    for (int c = 0; c < 9; c++) row[c] = lane < M ? row[c] : 0.0f;
    float n9[9];
    nullVector9Wave<M>(row, n9);
    tvDenormalise(model, n9, pr, m);
}
#endif

// the two score terms of one match and whether it is an inlier (:340-388 / :416-468); m = M21 | M12
__device__ __forceinline__ bool tvTerms(int model, const float (&m)[18], float invSigmaSquare, float u1, float v1, float u2, float v2, float& t1,
                                        float& t2) {
    auto lin = [](float a, float x, float b, float y, float c) { return __fadd_rn(__fadd_rn(__fmul_rn(a, x), __fmul_rn(b, y)), c); };
    float chi1, chi2, th, thScore;
    if (model == 0) {
        th = thScore = 5.991f;
        const float w2 = tvInvDouble(lin(m[15], u2, m[16], v2, m[17]));
        const float du1 = __fsub_rn(u1, __fmul_rn(lin(m[9], u2, m[10], v2, m[11]), w2)), dv1 = __fsub_rn(v1, __fmul_rn(lin(m[12], u2, m[13], v2, m[14]), w2));
        chi1 = __fmul_rn(__fadd_rn(__fmul_rn(du1, du1), __fmul_rn(dv1, dv1)), invSigmaSquare);
        const float w1 = tvInvDouble(lin(m[6], u1, m[7], v1, m[8]));
        const float du2 = __fsub_rn(u2, __fmul_rn(lin(m[0], u1, m[1], v1, m[2]), w1)), dv2 = __fsub_rn(v2, __fmul_rn(lin(m[3], u1, m[4], v1, m[5]), w1));
        chi2 = __fmul_rn(__fadd_rn(__fmul_rn(du2, du2), __fmul_rn(dv2, dv2)), invSigmaSquare);
    } else {
        th = 3.841f; thScore = 5.991f;
        const float a2 = lin(m[0], u1, m[1], v1, m[2]), b2 = lin(m[3], u1, m[4], v1, m[5]), c2 = lin(m[6], u1, m[7], v1, m[8]);
        const float num2 = lin(a2, u2, b2, v2, c2);
        chi1 = __fmul_rn(__fdiv_rn(__fmul_rn(num2, num2), __fadd_rn(__fmul_rn(a2, a2), __fmul_rn(b2, b2))), invSigmaSquare);
        const float a1 = lin(m[0], u2, m[3], v2, m[6]), b1 = lin(m[1], u2, m[4], v2, m[7]), c1 = lin(m[2], u2, m[5], v2, m[8]);
        const float num1 = lin(a1, u1, b1, v1, c1);
        chi2 = __fmul_rn(__fdiv_rn(__fmul_rn(num1, num1), __fadd_rn(__fmul_rn(a1, a1), __fmul_rn(b1, b1))), invSigmaSquare);
    }
    const bool out1 = chi1 > th, out2 = chi2 > th;
    t1 = out1 ? 0.0f : __fsub_rn(thScore, chi1);
    t2 = out2 ? 0.0f : __fsub_rn(thScore, chi2);
    return !out1 && !out2;
}

// the score of matrix m over the N matches of a pair, by one wave; inl (or NULL) receives vbMatchesInliers.  Returns the score on every lane.
__device__ __forceinline__ float tvScore(int lane, int model, const float (&m)[18], float sigma, int N, const int* __restrict__ first,
                                         const int* __restrict__ second, const Keypoint* __restrict__ k1, const Keypoint* __restrict__ k2,
                                         uint8_t* inl, int* nInliers) {
    const float invSigmaSquare = tvInvDouble(__fmul_rn(sigma, sigma));
    float score = 0.0f;
    int count = 0;
    for (int base = 0; base < N; base += kTvLanes) {
        const int k = base + lane;
        float t1 = 0.0f, t2 = 0.0f;
        bool in = false;
        if (k < N) {
            const Keypoint a = k1[first[k]], b = k2[second[k]];
            in = tvTerms(model, m, invSigmaSquare, a.x, a.y, b.x, b.y, t1, t2);
            if (inl) inl[k] = in ? 1 : 0;
        }
        count += __popcll(__ballot(in));
        score = tvChainAdd(score, t1, t2);
    }
    if (nInliers) *nInliers = count;
    return score;
}

__device__ __forceinline__ void tvStoreMotion(ORBX_LDS float* mo, const float (&R)[9], const float (&t)[3], const TwoViewParams& q) {
    // P2 = K * [R | t] (:824-827), O2 = -R.t() * t (:829)
    const float K[9] = {q.fx, 0.f, q.cx, 0.f, q.fy, q.cy, 0.f, 0.f, 1.f};
#pragma unroll
    for (int c = 0; c < 9; c++) mo[c] = R[c];
#pragma unroll
    for (int c = 0; c < 3; c++) mo[9 + c] = t[c];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const float col[3] = {c < 3 ? R[c] : t[0], c < 3 ? R[3 + c] : t[1], c < 3 ? R[6 + c] : t[2]};
            mo[12 + 4 * r + c] = gemmRow(K[3 * r], K[3 * r + 1], K[3 * r + 2], col, 1.0, 0.f, false);
        }
        mo[24 + r] = gemmRow(R[r], R[3 + r], R[6 + r], t, -1.0, 0.f, false);
    }
}

// t / cv::norm(t)
__device__ __forceinline__ void tvUnit(float (&t)[3]) {
    const float inv = (float)__ddiv_rn(1.0, __dsqrt_rn(dot3Double(t[0], t[1], t[2], t[0], t[1], t[2])));
#pragma unroll
    for (int c = 0; c < 3; c++) t[c] = __fmul_rn(t[c], inv);
}

// ReconstructF's four motions (:482-500): (R1, t) (R2, t) (R1, -t) (R2, -t)
__device__ __forceinline__ void tvMotionsF(const float (&F21)[9], const TwoViewParams& q, ORBX_LDS float* sMot) {
    const float K[9] = {q.fx, 0.f, q.cx, 0.f, q.fy, q.cy, 0.f, 0.f, 1.f}, Kt[9] = {q.fx, 0.f, 0.f, 0.f, q.fy, 0.f, q.cx, q.cy, 1.f};
    float tmp[9], E[9], U[9], w[3], Vt[9], R1[9], R2[9];
    gemm3(Kt, F21, 1.0, tmp);
    gemm3(tmp, K, 1.0, E);
    svd3(E, U, w, Vt);
    float t[3] = {U[2], U[5], U[8]};
    tvUnit(t);
    const float W[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f}, Wt[9] = {0.f, 1.f, 0.f, -1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    gemm3(U, W, 1.0, tmp);
    gemm3(tmp, Vt, 1.0, R1);
    if (det3(R1) < 0.0)
#pragma unroll
        for (int c = 0; c < 9; c++) R1[c] = -R1[c];
    gemm3(U, Wt, 1.0, tmp);
    gemm3(tmp, Vt, 1.0, R2);
    if (det3(R2) < 0.0)
#pragma unroll
        for (int c = 0; c < 9; c++) R2[c] = -R2[c];
    const float tn[3] = {-t[0], -t[1], -t[2]};
    tvStoreMotion(sMot, R1, t, q);
    tvStoreMotion(sMot + kTvMotionFloats, R2, t, q);
    tvStoreMotion(sMot + 2 * kTvMotionFloats, R1, tn, q);
    tvStoreMotion(sMot + 3 * kTvMotionFloats, R2, tn, q);
}

// ReconstructH's eight motions (:587-689); false: d1 / d2 < 1.00001 || d2 / d3 < 1.00001 (:600)
__device__ __forceinline__ bool tvMotionsH(const float (&H21)[9], const TwoViewParams& q, ORBX_LDS float* sMot) {
    const float K[9] = {q.fx, 0.f, q.cx, 0.f, q.fy, q.cy, 0.f, 0.f, 1.f};
    float invK[9], tmp[9], A[9], U[9], w[3], Vt[9];
    inv3(K, invK);
    gemm3(invK, H21, 1.0, tmp);
    gemm3(tmp, K, 1.0, A);
    svd3(A, U, w, Vt);
    const float s = (float)__dmul_rn(det3(U), det3(Vt));
    const float d1 = w[0], d2 = w[1], d3 = w[2];
    if ((double)__fdiv_rn(d1, d2) < 1.00001 || (double)__fdiv_rn(d2, d3) < 1.00001) return false;
    const float d11 = __fmul_rn(d1, d1), d22 = __fmul_rn(d2, d2), d33 = __fmul_rn(d3, d3);
    const float a12 = __fsub_rn(d11, d22), a23 = __fsub_rn(d22, d33), a13 = __fsub_rn(d11, d33);
    const float aux1 = sqrtFloat32(__fdiv_rn(a12, a13)), aux3 = sqrtFloat32(__fdiv_rn(a23, a13));
    const float root = sqrtFloat32(__fmul_rn(a12, a23));
    const float denT = __fmul_rn(__fadd_rn(d1, d3), d2), denP = __fmul_rn(__fsub_rn(d1, d3), d2);
    const float auxS = __fdiv_rn(root, denT), ctheta = __fdiv_rn(__fadd_rn(d22, __fmul_rn(d1, d3)), denT);
    const float auxP = __fdiv_rn(root, denP), cphi = __fdiv_rn(__fsub_rn(__fmul_rn(d1, d3), d22), denP);
    const float x1[4] = {aux1, aux1, -aux1, -aux1}, x3[4] = {aux3, -aux3, aux3, -aux3};
    const float st[4] = {auxS, -auxS, -auxS, auxS}, sp[4] = {auxP, -auxP, -auxP, auxP};
    const float dm = __fsub_rn(d1, d3), dp = __fadd_rn(d1, d3);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int j = i & 3;
        const bool second = i >= 4;
        const float Rp[9] = {second ? cphi : ctheta, 0.f, second ? sp[j] : -st[j], 0.f, second ? -1.f : 1.f, 0.f, second ? sp[j] : st[j], 0.f,
                             second ? -cphi : ctheta};
        float R[9];
        gemm3(U, Rp, (double)s, tmp);
        gemm3(tmp, Vt, 1.0, R);
        const float tp[3] = {__fmul_rn(x1[j], second ? dp : dm), __fmul_rn(0.0f, second ? dp : dm), __fmul_rn(second ? x3[j] : -x3[j], second ? dp : dm)};
        float t[3];
#pragma unroll
        for (int r = 0; r < 3; r++) t[r] = gemmRow(U[3 * r], U[3 * r + 1], U[3 * r + 2], tp, 1.0, 0.f, false);
        tvUnit(t);
        tvStoreMotion(sMot + i * kTvMotionFloats, R, t, q);
    }
    return true;
}

// CheckRT's loop body for one match (:835-896) under motion mo = R | t | P2 | O2.  active: an inlier match of the list.
struct TvPoint { bool counted, good; float cosPar; float p[3]; };
__device__ __forceinline__ TvPoint tvCheckPoint(bool active, const ORBX_LDS float* mo, const TwoViewParams& q, float th2, float u1, float v1,
                                                float u2, float v2) {
    TvPoint out;
    out.counted = out.good = false; out.cosPar = 0.0f; out.p[0] = out.p[1] = out.p[2] = 0.0f;
    if (!waveAny(active)) return out;                                                           // (wave-uniform)
    const float P1[12] = {q.fx, 0.f, q.cx, 0.f, 0.f, q.fy, q.cy, 0.f, 0.f, 0.f, 1.f, 0.f};
    float A[16], vt[4], x[3];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        A[c] = __fsub_rn(__fmul_rn(u1, P1[8 + c]), P1[c]);
        A[4 + c] = __fsub_rn(__fmul_rn(v1, P1[8 + c]), P1[4 + c]);
        A[8 + c] = __fsub_rn(__fmul_rn(u2, mo[20 + c]), mo[12 + c]);
        A[12 + c] = __fsub_rn(__fmul_rn(v2, mo[20 + c]), mo[16 + c]);
    }
    nullVector4(A, vt);
#pragma unroll
    for (int r = 0; r < 3; r++) x[r] = __fdiv_rn(vt[r], vt[3]);
    const bool finite = tvFinite(x[0]) && tvFinite(x[1]) && tvFinite(x[2]);
    const float n1[3] = {__fsub_rn(x[0], 0.0f), __fsub_rn(x[1], 0.0f), __fsub_rn(x[2], 0.0f)};
    const float n2[3] = {__fsub_rn(x[0], mo[24]), __fsub_rn(x[1], mo[25]), __fsub_rn(x[2], mo[26])};
    const float dist1 = (float)__dsqrt_rn(dot3Double(n1[0], n1[1], n1[2], n1[0], n1[1], n1[2])),
                dist2 = (float)__dsqrt_rn(dot3Double(n2[0], n2[1], n2[2], n2[0], n2[1], n2[2]));
    const float cosPar = (float)__ddiv_rn(dot3Double(n1[0], n1[1], n1[2], n2[0], n2[1], n2[2]), (double)__fmul_rn(dist1, dist2));
    const bool lowCos = (double)cosPar < 0.99998;
    float x2[3];
#pragma unroll
    for (int r = 0; r < 3; r++) x2[r] = gemmRow(mo[3 * r], mo[3 * r + 1], mo[3 * r + 2], x, 1.0, mo[9 + r], true);
    const bool behind = (x[2] <= 0.0f && lowCos) || (x2[2] <= 0.0f && lowCos);
    const float invZ1 = tvInvDouble(x[2]), invZ2 = tvInvDouble(x2[2]);
    const float e1x = __fsub_rn(__fadd_rn(__fmul_rn(__fmul_rn(q.fx, x[0]), invZ1), q.cx), u1),
                e1y = __fsub_rn(__fadd_rn(__fmul_rn(__fmul_rn(q.fy, x[1]), invZ1), q.cy), v1);
    const float e2x = __fsub_rn(__fadd_rn(__fmul_rn(__fmul_rn(q.fx, x2[0]), invZ2), q.cx), u2),
                e2y = __fsub_rn(__fadd_rn(__fmul_rn(__fmul_rn(q.fy, x2[1]), invZ2), q.cy), v2);
    const bool err1 = __fadd_rn(__fmul_rn(e1x, e1x), __fmul_rn(e1y, e1y)) > th2, err2 = __fadd_rn(__fmul_rn(e2x, e2x), __fmul_rn(e2y, e2y)) > th2;
    out.counted = active && finite && !behind && !err1 && !err2;
    out.good = out.counted && lowCos;
    if (out.counted) { out.cosPar = cosPar; out.p[0] = x[0]; out.p[1] = x[1]; out.p[2] = x[2]; }
    return out;
}

// whether v is element idx of the ascending order of the counted cosines (a NaN larger than everything)
__device__ __forceinline__ bool tvRankHit(const float* cosv, const uint8_t* counted, int N, float v, int idx) {
    int less = 0, leq = 0;
    for (int k = 0; k < N; k++) {
        const float x = cosv[k];
        less += counted[k] && x < v;
        leq += counted[k] && x <= v;
    }
    return less <= idx && idx < leq;
}
// (a NaN leaves as THE quiet NaN, canonNaN: which NaN 0 / 0 gives differs between the host's and the device's arithmetic)
__device__ __forceinline__ float tvParallax(float cosPar) {
    const float p = (float)__ddiv_rn((double)__fmul_rn(acosFloat32(cosPar), 180.0f), 3.1415926535897932384626433832795);
    return canonNaN(p);
}

// the end of ReconstructF (:502-573) / ReconstructH (:692-734) on the counts and parallaxes of the motions; N = the inliers
__device__ __forceinline__ int tvDecide(int model, const ORBX_LDS int* nGood, const ORBX_LDS float* parallax, int N, const TwoViewParams& q, int& chosen) {
    chosen = -1;
    if (model == 1) {
        const int maxGood = max(nGood[0], max(nGood[1], max(nGood[2], nGood[3])));
        const int nMinGood = max((int)__dmul_rn(0.9, (double)N), q.minTriangulated);
        int nsimilar = 0;
        for (int i = 0; i < 4; i++) nsimilar += (double)nGood[i] > __dmul_rn(0.7, (double)maxGood);
        if (maxGood < nMinGood) return kTvFFewPoints;
        if (nsimilar > 1) return kTvFAmbiguous;
        int i = 0;
        while (nGood[i] != maxGood) i++;
        if (parallax[i] > q.minParallax) { chosen = i; return kTvAcceptedF; }
        return kTvFLowParallax;
    }
    int bestGood = 0, second = 0, bestIdx = -1;
    float bestParallax = -1.0f;
    for (int i = 0; i < 8; i++) {
        if (nGood[i] > bestGood) { second = bestGood; bestGood = nGood[i]; bestIdx = i; bestParallax = parallax[i]; }
        else if (nGood[i] > second) second = nGood[i];
    }
    if (!((double)second < __dmul_rn(0.75, (double)bestGood))) return kTvHAmbiguous;
    if (!(bestParallax >= q.minParallax)) return kTvHLowParallax;
    if (!(bestGood > q.minTriangulated)) return kTvHFewPoints;
    if (!((double)bestGood > __dmul_rn(0.9, (double)N))) return kTvHBelowInlierShare;
    chosen = bestIdx;
    return kTvAcceptedH;
}

__device__ __forceinline__ int tvClampCount(int n, int cap) { return max(0, min(n, cap)); }

// ---- the three kernels' bodies, one wave each ------------------------------------------------------------------------------------------
// 1. per pair: zero the outputs, compact the matches, N, the exits before any arithmetic, Normalize of both frames, the T matrices.
//    A bad index decides before the count does.
__device__ __forceinline__ void tvPreparePair(int lane, int pair, const Keypoint* __restrict__ kps, const int* __restrict__ nOut,
                                              const int* matches12, const TwoViewParams& q, const TvWork& w, TwoViewResult* result, float* p3d,
                                              uint8_t* tri) {
    const int cap = q.capacity;
    const long long f1 = q.f1First + (long long)pair * q.f1Step, f2 = q.f2First + (long long)pair * q.f2Step, at = (long long)pair * cap;
    const int n1 = tvClampCount(nOut[f1], cap), n2 = tvClampCount(nOut[f2], cap);
    TvPrep& pr = w.prep[pair];
    TwoViewResult& res = result[pair];
    if (lane == 0) {
        int* words = (int*)&res;
        for (int k = 0; k < (int)(sizeof(TwoViewResult) / 4); k++) words[k] = 0;
    }
    for (int i = lane; i < n1; i += kTvLanes) { p3d[(at + i) * 3] = p3d[(at + i) * 3 + 1] = p3d[(at + i) * 3 + 2] = 0.0f; tri[at + i] = 0; }
    int n = 0;
    bool bad = false;
    for (int base = 0; base < n1; base += kTvLanes) {
        const int i = base + lane, m = i < n1 ? matches12[at + i] : -1;
        const unsigned long long has = __ballot(m >= 0);
        bad = bad || __ballot(m >= n2) != 0ull;
        if (m >= 0) {
            const int pos = n + __popcll(has & ((1ull << lane) - 1ull));
            w.first[at + pos] = i; w.second[at + pos] = m;
        }
        n += __popcll(has);
    }
    const int status = bad ? kTvBadIndex : n < 8 ? kTvTooFewMatches : kTvRunning;
    if (status == kTvRunning)
        for (int c = lane; c < 4; c += kTvLanes) {
            const bool secondFrame = c >= 2;
            tvNormalizeChain(kps + (secondFrame ? f2 : f1) * cap, secondFrame ? n2 : n1, c & 1, pr.norm[2 * c], pr.norm[2 * c + 1]);
        }
    __syncthreads();
    if (lane != 0) return;
    pr.status = status; pr.n = n; pr.n1 = n1; pr.n2 = n2;
    res.status = status; res.nMatches = n; res.chosen = -1; res.bestItH = res.bestItF = -1; res.model = -1;
    if (status != kTvRunning) return;
    float T1[9], T2[9], T2inv[9];
    tvNormalizeT(pr.norm, T1);
    tvNormalizeT(pr.norm + 4, T2);
    inv3(T2, T2inv);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) { pr.T1[3 * r + c] = T1[3 * r + c]; pr.T2[3 * r + c] = T2[3 * r + c]; pr.T2inv[3 * r + c] = T2inv[3 * r + c]; pr.T2t[3 * r + c] = T2[3 * c + r]; }
}

// 2. per (pair, model, iteration): the hypothesis on lane 0, its score by the wave.  sMem: kTvHypLdsFloats floats.
template <bool Spread>
__device__ __forceinline__ void tvHypothesisWave(int lane, int pair, int model, int it, const Keypoint* __restrict__ kps,
                                                 const int* __restrict__ rnd, const TwoViewParams& q, const TvWork& w, ORBX_LDS float* sMem) {
    const TvPrep& pr = w.prep[pair];
    if (pr.status != kTvRunning) return;
    const int cap = q.capacity, N = pr.n;
    const long long f1 = q.f1First + (long long)pair * q.f1Step, f2 = q.f2First + (long long)pair * q.f2Step, at = (long long)pair * cap;
    const Keypoint *k1 = kps + f1 * cap, *k2 = kps + f2 * cap;
    ORBX_LDS float* out18 = sMem + 2 * 144 + 81;
    float m[18];
#ifndef ORBX_HOST_ROW
    if constexpr (Spread) {
        int idx[8];
        drawSet<8>(rnd + ((long long)pair * q.iterations + it) * 8, N, idx);
        if (model == 0) tvHypothesisSpread<16>(idx, pr, w.first + at, w.second + at, k1, k2, m);
        else tvHypothesisSpread<8>(idx, pr, w.first + at, w.second + at, k1, k2, m);
    } else
#endif
    {
        if (lane == 0) {
            int idx[8];
            drawSet<8>(rnd + ((long long)pair * q.iterations + it) * 8, N, idx);
            tvHypothesis(model, idx, pr, w.first + at, w.second + at, k1, k2, sMem, sMem + 144, sMem + 288, out18);
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 18; c++) m[c] = out18[c];
    }
    const float score = tvScore(lane, model, m, q.sigma, N, w.first + at, w.second + at, k1, k2, nullptr, nullptr);
    if (lane == 0) {
        const long long slot = ((long long)pair * 2 + model) * q.iterations + it;
        w.score[slot] = score;
        for (int c = 0; c < 9; c++) w.mats[slot * 9 + c] = m[c];
    }
}

// 3. per pair: the best of each model, RH, the branch, its motions, CheckRT of each, the decision, the outputs, the pruning.
//    sMem: kTvDecideLdsFloats floats.
__device__ __forceinline__ void tvDecidePair(int lane, int pair, const Keypoint* __restrict__ kps, int* matches12, int* nMatches,
                                             const TwoViewParams& q, const TvWork& w, TwoViewResult* result, float* p3d, uint8_t* tri,
                                             ORBX_LDS float* sMem) {
    const TvPrep& pr = w.prep[pair];
    if (pr.status != kTvRunning) return;
    TwoViewResult& res = result[pair];
    const int cap = q.capacity, N = pr.n;
    const long long f1 = q.f1First + (long long)pair * q.f1Step, f2 = q.f2First + (long long)pair * q.f2Step, at = (long long)pair * cap;
    const Keypoint *k1 = kps + f1 * cap, *k2 = kps + f2 * cap;
    const int *first = w.first + at, *second = w.second + at;
    ORBX_LDS float* sPar = sMem + 8 * kTvMotionFloats;
    ORBX_LDS int* sInt = (ORBX_LDS int*)(sPar + 8);
    // :151-174, :202-225: uniform on every lane
    float S[2] = {0.0f, 0.0f};
    int bestIt[2] = {-1, -1};
#pragma unroll
    for (int model = 0; model < 2; model++)
        for (int it = 0; it < q.iterations; it++) {
            const float s = w.score[((long long)pair * 2 + model) * q.iterations + it];
            if (s > S[model]) { S[model] = s; bestIt[model] = it; }
        }
    const float sum = __fadd_rn(S[0], S[1]);
    if (sum == 0.0f) {                                                                        // :111
        if (lane == 0) res.status = kTvZeroScores;
        return;
    }
    const float RH = __fdiv_rn(S[0], sum);
    const int model = RH > q.rhThreshold ? 0 : 1;
    float m[18];
#pragma unroll
    for (int c = 0; c < 18; c++) m[c] = 0.0f;
    float M[9];
    {
        const long long slot = ((long long)pair * 2 + model) * q.iterations + bestIt[model];
#pragma unroll
        for (int c = 0; c < 9; c++) M[c] = m[c] = w.mats[slot * 9 + c];
        if (model == 0) {
            float M12[9];
            inv3(M, M12);
#pragma unroll
            for (int c = 0; c < 9; c++) m[9 + c] = M12[c];
        }
    }
    int nInliers = 0;
    (void)tvScore(lane, model, m, q.sigma, N, first, second, k1, k2, w.inl + at, &nInliers);
    if (lane == 0) {
        res.model = model; res.SH = S[0]; res.SF = S[1]; res.RH = RH; res.bestItH = bestIt[0]; res.bestItF = bestIt[1]; res.nInliers = nInliers;
        for (int hm = 0; hm < 2; hm++) {
            if (bestIt[hm] < 0) continue;
            const long long slot = ((long long)pair * 2 + hm) * q.iterations + bestIt[hm];
            for (int c = 0; c < 9; c++) (hm ? res.F21 : res.H21)[c] = w.mats[slot * 9 + c];
        }
        bool ok = true;
        if (model == 0) ok = tvMotionsH(M, q, sMem);
        else tvMotionsF(M, q, sMem);
        sInt[0] = ok ? kTvRunning : kTvHDegenerate;
    }
    __syncthreads();
    if (sInt[0] != kTvRunning) {
        if (lane == 0) res.status = kTvHDegenerate;
        return;
    }
    const int nMot = model == 0 ? 8 : 4;
    const float th2 = (float)__dmul_rn(4.0, (double)__fmul_rn(q.sigma, q.sigma));
    ORBX_LDS int* sGood = sInt + 4;
    if (lane == 0)
        for (int h = 0; h < 8; h++) { sGood[h] = 0; sPar[h] = 0.0f; }
    for (int h = 0; h < nMot; h++) {
        int good = 0;
        for (int base = 0; base < N; base += kTvLanes) {
            const int k = base + lane;
            const bool active = k < N && w.inl[at + k];
            float u1 = 0.f, v1 = 0.f, u2 = 0.f, v2 = 0.f;
            if (active) { const Keypoint a = k1[first[k]], b = k2[second[k]]; u1 = a.x; v1 = a.y; u2 = b.x; v2 = b.y; }
            const TvPoint pt = tvCheckPoint(active, sMem + h * kTvMotionFloats, q, th2, u1, v1, u2, v2);
            if (k < N) { w.counted[at + k] = pt.counted ? 1 : 0; w.cosv[at + k] = pt.cosPar; }
            good += __popcll(__ballot(pt.counted));
        }
        if (lane == 0) { sGood[h] = good; sPar[h] = good > 0 ? quietNaN() : 0.0f; }
        __syncthreads();
        if (good > 0) {
            const int idx = min(50, good - 1);
            for (int k = lane; k < N; k += kTvLanes)
                if (w.counted[at + k] && tvRankHit(w.cosv + at, w.counted + at, N, w.cosv[at + k], idx)) sPar[h] = tvParallax(w.cosv[at + k]);
        }
        __syncthreads();
    }
    int chosen;
    const int status = tvDecide(model, sGood, sPar, nInliers, q, chosen);
    if (lane == 0) {
        res.status = status; res.chosen = chosen;
        for (int h = 0; h < 8; h++) { res.nGood[h] = sGood[h]; res.parallax[h] = sPar[h]; }
    }
    if (status > kTvAcceptedF) return;
    const ORBX_LDS float* mo = sMem + chosen * kTvMotionFloats;
    if (lane == 0) {
        for (int c = 0; c < 9; c++) res.R21[c] = mo[c];
        for (int c = 0; c < 3; c++) res.t21[c] = mo[9 + c];
    }
    int pruned = 0;
    for (int base = 0; base < N; base += kTvLanes) {
        const int k = base + lane;
        const bool active = k < N && w.inl[at + k];
        float u1 = 0.f, v1 = 0.f, u2 = 0.f, v2 = 0.f;
        if (active) { const Keypoint a = k1[first[k]], b = k2[second[k]]; u1 = a.x; v1 = a.y; u2 = b.x; v2 = b.y; }
        const TvPoint pt = tvCheckPoint(active, mo, q, th2, u1, v1, u2, v2);
        if (k < N) {
            const long long i = at + first[k];
            if (pt.counted) { p3d[i * 3] = pt.p[0]; p3d[i * 3 + 1] = pt.p[1]; p3d[i * 3 + 2] = pt.p[2]; }
            if (pt.good) tri[i] = 1;
            if (q.prune && !pt.good) matches12[i] = -1;                                      // Tracking.cc:2083-2090
        }
        pruned += __popcll(__ballot(k < N && !pt.good));
    }
    if (lane == 0 && q.prune) nMatches[pair] -= pruned;
}

// drawSet<8>'s earlier name, ONLY for tests/cpp/two_view_host_check.cpp, which the existing tests build as it is; the library does not call it
__device__ __forceinline__ void tvDrawSet(const int* __restrict__ r8, int N, int (&idx)[8]) { drawSet<8>(r8, N, idx); }

}  // namespace orbx
