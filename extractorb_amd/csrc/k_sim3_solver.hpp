// k_sim3_solver.hpp - Sim3Solver (reference src/Sim3Solver.cc) as LoopClosing calls it (src/LoopClosing.cc:673-684): the constructor,
// SetRansacParameters(probability, minInliers, maxIterations) and the iterate(20, bNoMore, vbInliers, nInliers, bConverge) loop until it
// converges or has no more iterations.  k_sim3_solver.hip holds the three kernels around the three functions at the end of this file;
// everything they compute is stated here.  The reference's own loops and orders are kept; what is OpenCV's (cv::Mat expressions, cv::eigen,
// cv::Rodrigues) is the project's definition, "parity unpinned" (DESIGN.md section 2), each stated ONCE here:
//   slots        the caller's table is vpMatched12 indexed by i1; a slot with an octave of -1 stands for every `continue` of :73-91
//                (no match, no MapPoint, isBad, a point not observed in pKF1 / pKF2 - GetIndexInKeyFrame stays with the caller).  The present
//                slots in ascending i1 are the correspondences; N = their count; mvnIndices1[k] = i1 (idx1);
//   mvnMaxError  std::vector<size_t> (inc/Sim3Solver.h:78-79): 9.210 * sigma2 is a DOUBLE product TRUNCATED to an unsigned integer (9 at
//                level 0, 13 at level 1 of scale 1.2), and `err < mvnMaxError[i]` compares a float with that integer converted to float
//                (ssMaxError);
//   X3Dc         Rcw * Xw + tcw: one gemmRow per row with the addend (k_match_helpers.hpp); mvP1im1 / mvP2im2 their own projections;
//   projectMat   virtual: Pinhole::project fx * x / z + cx in binary32 as written, or KannalaBrandt8::project (kb8Project); the unused invz of
//                Project / FromCameraToImage is not built;
//   iterations   SetRansacParameters (:126-150): epsilon a float, pow / log / ceil in double, 1 when minInliers == N, then max(1, min(., max)).
//                N is known only on the device: the C entry fills its[N], N = 0 .. capacity, with the host's libm (sim3RansacIterations,
//                orbx_entry.hpp) and the first kernel looks it up.  A double outside the int range converts as the reference's x86-64
//                build does (cvttsd2si: INT_MIN), which max(1, .) turns into 1;
//   sets         the three indices of an iteration from the CALLER'S raw rand() values r: randi = int(((double)r / 2147483648.0) * size)
//                (DUtils/Random.cpp:47-50) clamped into [0, size - 1], idx = avail[randi], avail[randi] = avail.back(), pop_back (:251-262):
//                drawSet<3> (k_small_math.hpp; TwoViewReconstruction's sets are its K = 8);
//   ComputeSim3  :316-427.  cv::reduce's row sums are left-to-right float sums, `C / P.cols` a float product with (float)(1.0 / 3);
//                M = Pr2 * Pr1.t() one gemmRow per element; N's ten entries are FLOAT sums as written (assigned to doubles and narrowed again:
//                no effect); the quaternion is topEigenvector4; norm(vec) the double root of a double sum of double products; ang = atan2 in
//                double (atan2Double); `2 * ang * vec / norm(vec)` scales vec by (float)((2 * ang) * (1 / norm)) (as t / cv::norm(t) in
//                k_two_view.hpp); cv::Rodrigues is ssRodrigues; P3 = R * Pr2 (gemm3); nom = Pr1.dot(P3) a double sum of double products in
//                row-major order, den a double sum of the FLOAT squares (cv::pow), ms12i = (float)(nom / den), 1.0f when the scale is fixed;
//                mt12i = O1 - ms12i * R * O2 one gemmRow per row with alpha = -s and the addend O1; sR = fmul(s, R); sRinv =
//                fmul(R.t(), (float)(1.0 / s)); tinv = -sRinv * mt12i a gemmRow with alpha = -1;
//   quaternion   topEigenvector4 (k_small_svd.hpp): cv::eigen's row 0 on the symmetric 4x4 N.  N is traceless and, with three points, has the eigenvalues +-(s1 + s2), +-(s1 - s2):
//                the top eigenvalue has a partner of equal size and opposite sign, which a one-sided iteration cannot tell apart.  So the
//                iteration runs on N + mu * I, mu = the Frobenius norm of N (a float sum of float squares, left to right, sqrtFloat32) - positive
//                semi-definite with the same eigenvectors, the top eigenvalue now the unique largest singular value: nullVector4's Hestenes
//                iteration (jacobiAngle, kJacobiSweeps, pair order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)) on its columns with V from the
//                identity; the column of LARGEST squared norm selects V's column, of equal norms (three collinear points: two equal top
//                eigenvalues, any unit vector of their plane is an eigenvector - the iteration's own is taken) the lowest index.  SIGN: q and
//                -q are the same rotation but round differently, so the first component that is not zero is made positive (the real part
//                is >= 0 and ang lies in [0, pi / 2]);
//   ssRodrigues  cv::Rodrigues of a float 1x3: in double theta = sqrt(rx^2 + ry^2 + rz^2); theta < DBL_EPSILON gives the identity; else
//                c = cos, s = sin, c1 = 1 - c, r *= 1 / theta, R[i][j] = float((c * I[i][j] + c1 * r[i] * r[j]) + s * [r]x[i][j]);
//   atan2, sin, cos   atan2Double and sinCosDouble of k_small_math.hpp, not libm's;
//   CheckInliers :430-454 per correspondence: P2 in image 1 under mT12i, P1 in image 2 under mT21i, dist.dot(dist) a double sum of double
//                products narrowed to float, err1 < max1 && err2 < max2.  A point with z <= 0 projects as the arithmetic says;
//   iterate      sequential semantics, stated once.  mnBestInliers starts at 0 and the update test is >=: the first iteration always becomes
//                best, and of equal counts the LATER iteration wins.  The call returns at the first iteration whose count is above minInliers
//                (every earlier count was <= minInliers, or the call would have returned there).  The chunks of 20 change nothing.  So the
//                iterations are evaluated independently and a decision step takes the first count above minInliers (CONVERGED) or else the
//                LAST arg-max (NO_MORE, the best Sim3 so far as the second overload returns it).  tests/sim3_solver_walk.py is written as the
//                reference's loop and holds this form against it;
//   NaN          three points that align exactly (P1 == P2) give a quaternion whose imaginary part is exactly 0: ang = 0, norm = 0,
//                2 * ang / norm = 0 * inf = NaN, a NaN rotation, 0 inliers - and, by >=, a "best" when no count is above 0.  The statement
//                keeps that.  Which NaN 0 * inf gives differs between host and device arithmetic: every NaN leaves in the result row as THE
//                quiet NaN (canonNaN, k_small_math.hpp).
// One workgroup is ONE WAVE everywhere (kSsLanes lanes); the host build (ORBX_HOST_ROW, tests/cpp/host_shim) runs the same functions with a
// wave of one lane.
// Takes kb8Project from k_camera_kb8.hpp, topEigenvector4 / gemm3 from k_small_svd.hpp, drawSet / atan2Double / sinCosDouble /
// pinholeProject / transformPoint / canonNaN from k_small_math.hpp, gemmRow / dot3Double from k_match_helpers.hpp, the parameter blocks from
// orbx_params.hpp.
#pragma once
#include "k_camera_kb8.hpp"
#include "k_match_helpers.hpp"
#include "k_small_math.hpp"
#include "k_small_svd.hpp"
#include "orbx_device.hpp"
#include "orbx_params.hpp"

namespace orbx {

// == orbx_sim3_solve_status
enum { kSsConverged = 0, kSsNoMore, kSsTooFew, kSsBadArgument, kSsStatuses };
constexpr int kSsRunning = -1;                            // SsPrep::status while no exit has been taken

// == orbx_sim3_problem
struct Sim3Problem {
    int n1, fixScale, model1, model2;                     // model: 0 Pinhole (cam[0..3] = fx, fy, cx, cy), 1 KannalaBrandt8 (mvParameters)
    float cam1[8], cam2[8], Tcw1[12], Tcw2[12], sigma2[kMaxLevels];
};
// == orbx_sim3_result
struct Sim3Result {
    int status, n, maxIts, iterations, bestIt, nInliers, bestInliers;
    float scale, R[9], t[3], T12[16];
};

#ifdef ORBX_HOST_ROW
constexpr int kSsLanes = 1;
#else
constexpr int kSsLanes = 64;
#endif

// mvnMaxError: (size_t)(9.210 * sigmaSquare), then the float the comparison converts it to
__device__ __forceinline__ float ssMaxError(float sigma2) {
    const double v = __dmul_rn(9.210, (double)sigma2);
    if (!(v >= 0.0)) return 0.0f;                                                             // (a negative or NaN sigma2 is the caller's error)
    return (float)(unsigned long long)(v < 1.0e19 ? v : 1.0e19);
}

// ---- cv::Rodrigues -----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ssRodrigues(const float (&rv)[3], float (&R)[9]) {
    double r[3] = {(double)rv[0], (double)rv[1], (double)rv[2]};
    const double theta = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(r[0], r[0]), __dmul_rn(r[1], r[1])), __dmul_rn(r[2], r[2])));
    if (theta < 2.2204460492503131e-16) {                                                      // DBL_EPSILON
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = (k % 4 == 0) ? 1.0f : 0.0f;
        return;
    }
    double s, c;
    sinCosDouble(theta, s, c);
    const double c1 = __dsub_rn(1.0, c), itheta = __ddiv_rn(1.0, theta);
#pragma unroll
    for (int k = 0; k < 3; k++) r[k] = __dmul_rn(r[k], itheta);
    const double rx[9] = {0.0, -r[2], r[1], r[2], 0.0, -r[0], -r[1], r[0], 0.0};
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double sym = __dadd_rn(__dmul_rn(c, i == j ? 1.0 : 0.0), __dmul_rn(c1, __dmul_rn(r[i], r[j])));
            R[3 * i + j] = (float)__dadd_rn(sym, __dmul_rn(s, rx[3 * i + j]));
        }
}

// ---- ComputeSim3 ---------------------------------------------------------------------------------------------------------------------------
struct Sim3Hyp { float R[9], t[3], s, T12[12], T21[12]; };      // T12 / T21: the first three rows of mT12i / mT21i, row-major 3x4

// ComputeCentroid: P is 3x3 with point i in column i (P[3 * r + i])
__device__ __forceinline__ void ssCentroid(const float (&P)[9], float (&Pr)[9], float (&O)[3]) {
    const float third = (float)__ddiv_rn(1.0, 3.0);
#pragma unroll
    for (int r = 0; r < 3; r++) {
        O[r] = __fmul_rn(__fadd_rn(__fadd_rn(P[3 * r], P[3 * r + 1]), P[3 * r + 2]), third);
#pragma unroll
        for (int i = 0; i < 3; i++) Pr[3 * r + i] = __fsub_rn(P[3 * r + i], O[r]);
    }
}

__device__ __forceinline__ void ssComputeSim3(const float (&P1)[9], const float (&P2)[9], bool fixScale, Sim3Hyp& h) {
    float Pr1[9], Pr2[9], O1[3], O2[3], M[9];
    ssCentroid(P1, Pr1, O1);
    ssCentroid(P2, Pr2, O2);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const float col[3] = {Pr1[3 * c], Pr1[3 * c + 1], Pr1[3 * c + 2]};
            M[3 * r + c] = gemmRow(Pr2[3 * r], Pr2[3 * r + 1], Pr2[3 * r + 2], col, 1.0, 0.f, false);
        }
    const float N11 = __fadd_rn(__fadd_rn(M[0], M[4]), M[8]), N12 = __fsub_rn(M[5], M[7]), N13 = __fsub_rn(M[6], M[2]), N14 = __fsub_rn(M[1], M[3]);
    const float N22 = __fsub_rn(__fsub_rn(M[0], M[4]), M[8]), N23 = __fadd_rn(M[1], M[3]), N24 = __fadd_rn(M[6], M[2]);
    const float N33 = __fsub_rn(__fadd_rn(-M[0], M[4]), M[8]), N34 = __fadd_rn(M[5], M[7]), N44 = __fadd_rn(__fsub_rn(-M[0], M[4]), M[8]);
    const float Nm[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44};
    float q[4];
    topEigenvector4(Nm, q);
    const double nrm = __dsqrt_rn(dot3Double(q[1], q[2], q[3], q[1], q[2], q[3]));
    const double ang = atan2Double(nrm, (double)q[0]);
    const float alpha = (float)__dmul_rn(__dmul_rn(2.0, ang), __ddiv_rn(1.0, nrm));
    const float rv[3] = {__fmul_rn(q[1], alpha), __fmul_rn(q[2], alpha), __fmul_rn(q[3], alpha)};
    ssRodrigues(rv, h.R);
    if (!fixScale) {
        float P3[9];
        gemm3(h.R, Pr2, 1.0, P3);
        double nom = __dmul_rn((double)Pr1[0], (double)P3[0]), den = 0.0;
#pragma unroll
        for (int k = 1; k < 9; k++) nom = __dadd_rn(nom, __dmul_rn((double)Pr1[k], (double)P3[k]));
#pragma unroll
        for (int k = 0; k < 9; k++) den = __dadd_rn(den, (double)__fmul_rn(P3[k], P3[k]));
        h.s = (float)__ddiv_rn(nom, den);
    } else
        h.s = 1.0f;
    const float sInv = (float)__ddiv_rn(1.0, (double)h.s);
#pragma unroll
    for (int r = 0; r < 3; r++) h.t[r] = gemmRow(h.R[3 * r], h.R[3 * r + 1], h.R[3 * r + 2], O2, -(double)h.s, O1[r], true);
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) { h.T12[4 * r + c] = __fmul_rn(h.s, h.R[3 * r + c]); h.T21[4 * r + c] = __fmul_rn(h.R[3 * c + r], sInv); }
        h.T12[4 * r + 3] = h.t[r];
    }
#pragma unroll
    for (int r = 0; r < 3; r++) h.T21[4 * r + 3] = gemmRow(h.T21[4 * r], h.T21[4 * r + 1], h.T21[4 * r + 2], h.t, -1.0, 0.f, false);
}

// ---- projections and the inlier test ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ssProjectCam(int model, const float (&k)[8], float x, float y, float z, float& u, float& v) {
    if (model) kb8Project(k, x, y, z, u, v);
    else pinholeProject(k, x, y, z, u, v);
}
__device__ __forceinline__ float ssErr(float au, float av, float bu, float bv) {
    const float du = __fsub_rn(au, bu), dv = __fsub_rn(av, bv);
    return (float)__dadd_rn(__dmul_rn((double)du, (double)du), __dmul_rn((double)dv, (double)dv));
}
// the workspace of problem p: component c of correspondence k is pts[c * cap + k]
__device__ __forceinline__ bool ssInlier(const Sim3Hyp& h, const Sim3Problem& pb, const float* __restrict__ pts, int cap, int k) {
    const float X1[3] = {pts[k], pts[cap + k], pts[2 * cap + k]}, X2[3] = {pts[3 * cap + k], pts[4 * cap + k], pts[5 * cap + k]};
    float a[3], b[3], u21, v21, u12, v12;
    transformPoint(h.T12, X2, a);
    ssProjectCam(pb.model1, pb.cam1, a[0], a[1], a[2], u21, v21);                            // vP2im1
    transformPoint(h.T21, X1, b);
    ssProjectCam(pb.model2, pb.cam2, b[0], b[1], b[2], u12, v12);                            // vP1im2
    const float err1 = ssErr(pts[6 * cap + k], pts[7 * cap + k], u21, v21), err2 = ssErr(u12, v12, pts[8 * cap + k], pts[9 * cap + k]);
    return err1 < pts[10 * cap + k] && err2 < pts[11 * cap + k];
}
// iteration `it` of problem p: the draw and ComputeSim3 (uniform over the wave)
__device__ __forceinline__ void ssHypothesis(const int* __restrict__ rnd, long long slot, int N, const float* __restrict__ pts, int cap, bool fixScale,
                                             Sim3Hyp& h) {
    int idx[3];
    drawSet<3>(rnd + slot * 3, N, idx);
    float P1[9], P2[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int r = 0; r < 3; r++) { P1[3 * r + i] = pts[r * cap + idx[i]]; P2[3 * r + i] = pts[(3 + r) * cap + idx[i]]; }
    ssComputeSim3(P1, P2, fixScale, h);
}

// ---- the three kernels' bodies, one wave each ------------------------------------------------------------------------------------------------
// 1. per problem: zero the result row and the flags, compact the present slots in ascending i1, X3Dc1 / X3Dc2, their projections, the integer
//    thresholds, N, mRansacMaxIts, the exits that need no iteration.  BAD_ARGUMENT is what the reference would index out of bounds on: n1
//    outside [0, capacity], a model that is neither, an octave outside [-1, nlevels), fewer than three correspondences with N >= minInliers.
__device__ __forceinline__ void ssPrepareProblem(int lane, int p, const Sim3Problem* __restrict__ problems, const float* __restrict__ x1w,
                                                 const float* __restrict__ x2w, const int* __restrict__ oct1, const int* __restrict__ oct2,
                                                 const Sim3SolveParams& q, const SsWork& w, Sim3Result* result, uint8_t* flags) {
    const int cap = q.capacity;
    const Sim3Problem& pb = problems[p];
    const long long at = (long long)p * cap;
    const int n1 = pb.n1 < 0 || pb.n1 > cap ? 0 : pb.n1;
    const bool noModel = (pb.model1 & ~1) || (pb.model2 & ~1);
    bool bad = n1 != pb.n1 || noModel;
    if (lane == 0) {
        int* words = (int*)&result[p];
        for (int k = 0; k < (int)(sizeof(Sim3Result) / 4); k++) words[k] = 0;
    }
    float* pts = w.pts + at * kSsPointFloats;
    int n = 0;
    for (int base = 0; base < n1; base += kSsLanes) {
        const int i = base + lane, o1 = i < n1 ? oct1[at + i] : -1, o2 = i < n1 ? oct2[at + i] : -1;
        if (i < n1) flags[at + i] = 0;
        const bool wrong = o1 < -1 || o2 < -1 || o1 >= q.nlevels || o2 >= q.nlevels, has = !wrong && !noModel && o1 >= 0 && o2 >= 0;
        const unsigned long long mask = __ballot(has);
        bad = bad || __ballot(wrong) != 0ull;
        if (has) {
            const int pos = n + __popcll(mask & ((1ull << lane) - 1ull));
            const float Xa[3] = {x1w[(at + i) * 3], x1w[(at + i) * 3 + 1], x1w[(at + i) * 3 + 2]},
                        Xb[3] = {x2w[(at + i) * 3], x2w[(at + i) * 3 + 1], x2w[(at + i) * 3 + 2]};
            float c1[3], c2[3], u1, v1, u2, v2;
            transformPoint(pb.Tcw1, Xa, c1);
            transformPoint(pb.Tcw2, Xb, c2);
            ssProjectCam(pb.model1, pb.cam1, c1[0], c1[1], c1[2], u1, v1);
            ssProjectCam(pb.model2, pb.cam2, c2[0], c2[1], c2[2], u2, v2);
            w.idx1[at + pos] = i;
#pragma unroll
            for (int r = 0; r < 3; r++) { pts[r * cap + pos] = c1[r]; pts[(3 + r) * cap + pos] = c2[r]; }
            pts[6 * cap + pos] = u1; pts[7 * cap + pos] = v1; pts[8 * cap + pos] = u2; pts[9 * cap + pos] = v2;
            pts[10 * cap + pos] = ssMaxError(pb.sigma2[o1]); pts[11 * cap + pos] = ssMaxError(pb.sigma2[o2]);
        }
        n += __popcll(mask);
    }
    if (lane != 0) return;
    const int status = bad ? kSsBadArgument : n < q.minInliers ? kSsTooFew : n < 3 ? kSsBadArgument : kSsRunning;
    if (bad) n = 0;                                                                           // nothing was counted
    const int maxIts = bad ? 0 : max(1, min(w.its[n], q.maxIterations));
    SsPrep& pr = w.prep[p];
    pr.status = status; pr.n = n; pr.maxIts = maxIts; pr.n1 = n1;
    Sim3Result& res = result[p];
    res.status = status; res.n = n; res.maxIts = maxIts; res.bestIt = -1;
}

// 2. per (problem, iteration): the hypothesis (uniform), then CheckInliers one lane per correspondence; one count per iteration
__device__ __forceinline__ void ssHypothesisWave(int lane, int p, int it, const Sim3Problem* __restrict__ problems, const int* __restrict__ rnd,
                                                 const Sim3SolveParams& q, const SsWork& w) {
    const SsPrep& pr = w.prep[p];
    if (pr.status != kSsRunning || it >= pr.maxIts) return;
    const Sim3Problem& pb = problems[p];
    const int cap = q.capacity, N = pr.n;
    const long long slot = (long long)p * q.maxIterations + it;
    const float* pts = w.pts + (long long)p * cap * kSsPointFloats;
    Sim3Hyp h;
    ssHypothesis(rnd, slot, N, pts, cap, pb.fixScale != 0, h);
    int count = 0;
    for (int base = 0; base < N; base += kSsLanes) {
        const int k = base + lane;
        count += __popcll(__ballot(k < N && ssInlier(h, pb, pts, cap, k)));
    }
    if (lane == 0) w.counts[slot] = count;
}

// 3. per problem: the first count above minInliers, or else the last arg-max; its Sim3 again, the flags of a converged one, the result row
__device__ __forceinline__ void ssDecideProblem(int lane, int p, const Sim3Problem* __restrict__ problems, const int* __restrict__ rnd,
                                                const Sim3SolveParams& q, const SsWork& w, Sim3Result* result, uint8_t* flags) {
    const SsPrep& pr = w.prep[p];
    if (pr.status != kSsRunning) return;
    const Sim3Problem& pb = problems[p];
    const int cap = q.capacity, N = pr.n;
    const long long at = (long long)p * cap, first = (long long)p * q.maxIterations;
    const float* pts = w.pts + at * kSsPointFloats;
    int bestIt = 0, best = 0;
    bool converged = false;
    for (int it = 0; it < pr.maxIts && !converged; it++) {
        const int c = w.counts[first + it];
        if (c >= best) { best = c; bestIt = it; }
        converged = c > q.minInliers;
    }
    Sim3Hyp h;
    ssHypothesis(rnd, first + bestIt, N, pts, cap, pb.fixScale != 0, h);
    if (converged)
        for (int base = 0; base < N; base += kSsLanes) {
            const int k = base + lane;
            if (k < N && ssInlier(h, pb, pts, cap, k)) flags[at + w.idx1[at + k]] = 1;
        }
    if (lane != 0) return;
    Sim3Result& res = result[p];
    res.status = converged ? kSsConverged : kSsNoMore;
    res.iterations = converged ? bestIt + 1 : pr.maxIts;
    res.bestIt = bestIt; res.nInliers = converged ? best : 0; res.bestInliers = best;
    res.scale = canonNaN(h.s);
    for (int c = 0; c < 9; c++) res.R[c] = canonNaN(h.R[c]);
    for (int c = 0; c < 3; c++) res.t[c] = canonNaN(h.t[c]);
    for (int c = 0; c < 12; c++) res.T12[c] = canonNaN(h.T12[c]);
    res.T12[12] = res.T12[13] = res.T12[14] = 0.0f; res.T12[15] = 1.0f;
}

// Earlier names, ONLY for tests/cpp/sim3_solver_host_check.cpp, which the existing tests build as it is; the library does not call them
__device__ __forceinline__ void ssDraw3(const int* __restrict__ r3, int N, int (&idx)[3]) { drawSet<3>(r3, N, idx); }
__device__ __forceinline__ void ssEigenTop4(const float (&Nm)[16], float (&q)[4]) { topEigenvector4(Nm, q); }
__device__ __forceinline__ double ssAtan2(double y, double x) { return atan2Double(y, x); }
__device__ __forceinline__ void ssSinCos(double theta, double& s, double& c) { sinCosDouble(theta, s, c); }

}  // namespace orbx
