// k_pose_optimization.hpp - Optimizer::PoseOptimization (reference src/Optimizer.cc:854-1168), the motion-only bundle adjustment the tracker
// runs between its searches, for a batch of independent problems, one per frame.  k_pose_optimization.hip holds the kernel around
// poSolveProblem at the end of this file; everything it computes is stated here, and tests/pose_optimization_walk.py states it a second time.
// What is g2o's and Eigen's is the project's definition, "parity unpinned" (DESIGN.md section 2), each stated ONCE here:
//   edges        edge k of a problem is keypoint i = k % capacity of eye k / capacity (one camera: one eye; a rig: eye 0 = mpCamera with the
//                RAW mvKeys, eye 1 = mpCamera2 with mvKeysRight).  It exists when i < N of its frame and its match row holds a MapPoint
//                (>= 0).  Kinds: mono (EdgeSE3ProjectXYZOnlyPose: one camera with mvuRight < 0, or a rig's left eye), stereo
//                (g2o::EdgeStereoSE3ProjectXYZOnlyPose: one camera and NOT mvuRight < 0 - a NaN is stereo, as the reference's else), right
//                (EdgeSE3ProjectXYZOnlyPoseToBody: a rig's right eye).  invSigma2 is a float widened to double;
//   sums         the 28 double sums of a linearisation (robust chi2, the 21 upper entries of H, the 6 of b) and the one of a trial's chi2
//                have ONE order, a function of the edge index only: kPoSlots = 256 slots, slot s adds the terms of the ACTIVE edges
//                k = s, s + 256, s + 512, .. in ascending k onto 0.0; then the balanced tree over the slots in index order
//                (level by level v[s] = v[s] + v[s ^ stride], stride = 1, 2, .. 128).  On the device a slot is a lane, strides below 64 are
//                cross-lane exchanges and the last two go through LDS; the host build runs the slots one after the other (poSum);
//   edge terms   info * e with the zero off-diagonals as products (0 * inf is NaN: a point with z == 0 has a NaN chi2, which is NOT > 5.991f);
//                chi2 = e . (info * e) left to right; b[j] = -(sum of rho1 * (sum_r A[r][j] * (info e)[r])), H[j][k] += sum_r (A[r][j] *
//                (rho1 * w)) * A[r][k], r ascending; robustInformation is rho[1] * information, its second-order term is dead code;
//   Huber        e <= dsqr: (e, 1); else (2 sqrt(e) delta - dsqr, delta / sqrt(e)), delta = (double)(float)sqrt(5.991 | 7.815), dsqr = delta * delta;
//                rounds 0 - 2 only (setRobustKernel(0) follows round 2's classification);
//   LM           OptimizationAlgorithmLevenberg::solve as written: lambda = 1e-5 * max |H[j][j]| (std::max's NaN behaviour kept) at iteration
//                0 of EVERY round; rho = (currentChi - tempChi) / (sum_j x[j] * (lambda * x[j] + b[j]) + 1e-3); accepted when rho > 0 and
//                tempChi is finite: lambda *= max(1/3, min(1 - (2 rho - 1)^3, 2/3)), the cube two products; else lambda *= ni, ni *= 2 and the
//                pose is restored; at most 10 trials while rho < 0 (a NaN rho ends the trials and is NOT a termination); Terminate on
//                qmax == 10 || rho == 0; (iniChi - currentChi) * 1e3 < iniChi three times in a row terminates; at most 10 iterations;
//   stale error  nothing recomputes the errors after the last trial: an ACTIVE edge is classified at the pose of the LAST TRIAL, accepted or
//                rejected (errPose), an edge flagged before the round at the estimate (its computeError is fresh);
//   rounds       every round restarts from the INITIAL pose; only the flags carry over.  A round with no active edge has no index
//                mapping: optimize returns -1 at once (its = -1, the bit in emptyRounds), every edge is classified at the initial pose.
//                edges().size() < 10 is nInitialCorrespondences < 10, tested after round 0;
//   solve        the 6x6 system by Cholesky L L^T in place of LinearSolverDense's LDLT: a pivot that is not > 0 (a NaN included) fails the
//                solve, x keeps its value (zero at the start of a round), tempChi becomes DBL_MAX;
//   SE3Quat      exp (theta < 1e-5: R = I + Omega + Omega^2, V = R, the quaternion of that non-orthonormal matrix), the product with its
//                normalisation (w < 0 negated, then divided by the norm), map, Quaterniond(Matrix3d) (the trace branch and the three
//                diagonal branches), toRotationMatrix, Converter::toSE3Quat (float to double, then the quaternion) and toCvMat (narrowed);
//   cameras      Pinhole / KannalaBrandt8 project and projectJac, Eigen overloads, as written: KB8 project narrows to float for atan2f and
//                sqrtf (atan2f32, sqrtFloat32) and takes a DOUBLE cos / sin of psi (sinCosDouble of |psi|, the sine's sign restored); projectJac a
//                double atan2 (atan2Double) and float products 3 * k1 ..; the stereo edge's invz is a float of a double quotient;
//   NaN          every NaN leaves in the pose and the result row as one quiet NaN (canonNaN).
// One workgroup of kPoSlots lanes is one problem through all four rounds.  The pose, lambda and the LM state are uniform: every lane computes
// them from the same reduced sums.  The host build (ORBX_HOST_ROW, tests/cpp/host_shim) runs the same function with the slots in a loop.
// Takes atan2f32 from k_camera_kb8.hpp, sqrtFloat32 / atan2Double / sinCosDouble / canonNaN from k_small_math.hpp; nothing from another solver.
#pragma once
#include "k_camera_kb8.hpp"
#include "k_small_math.hpp"
#include "orbx_device.hpp"
#include "orbx_params.hpp"

namespace orbx {

// == orbx_pose_optimization_status
enum { kPoAllRounds = 0, kPoFewEdges, kPoTooFew, kPoBadArgument, kPoStatuses };
constexpr int kPoSlots = 256;
constexpr int kPoSums = 28;                               // chi2, H's upper triangle row by row, b
constexpr int kPoLdsBytes = (kPoSlots / 64) * kPoSums * 8;

// == orbx_pose_problem
struct PoseProblem {
    int model, model2;                                    // 0 Pinhole (cam[0..3] = fx, fy, cx, cy), 1 KannalaBrandt8 (mvParameters); model2: mpCamera2 of a rig
    float cam[8], cam2[8], mbf, Trl[12], invSigma2[kMaxLevels];
};
// == orbx_pose_result
struct PoseResult {
    int status, nInitial, nBad, nInliers, rounds, emptyRounds, its[4], trials[4];
    double lambda[4], chi2[4];
};

struct PoSE3 { double q[4], t[3]; };                      // q = x, y, z, w
struct PoEdge { int kind; double obs[3], X[3], w; };      // kind: 0 none, 1 mono, 2 stereo, 3 right
struct PoArgs {                                           // what a problem reads, resolved to its rows
    const Keypoint* kps[2]; const int* matches[2]; const float* uRight; const float* world; uint8_t* flags[2];
    int n[2], cap, eyes, nMapPoints, nlevels;
};

__device__ __forceinline__ double poSqrtOfFloat(double v) { return (double)(float)__dsqrt_rn(v); }      // deltaMono, deltaStereo

// ---- Eigen's quaternion and g2o's SE3Quat ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ void poNormalize(double (&q)[4]) {
    if (q[3] < 0.0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
    const double n = __dsqrt_rn(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = __ddiv_rn(q[k], n);
}
// one diagonal branch of Quaterniond(Matrix3d): R(i,i), R(j,j), R(k,k), R(k,j), R(j,k), R(j,i), R(i,j), R(k,i), R(i,k) -> q[i], q[j], q[k], w
__device__ __forceinline__ void poQuatDiag(double Rii, double Rjj, double Rkk, double Rkj, double Rjk, double Rji, double Rij, double Rki, double Rik,
                                           double& qi, double& qj, double& qk, double& w) {
    double t = __dsqrt_rn(((Rii - Rjj) - Rkk) + 1.0);
    qi = 0.5 * t;
    t = __ddiv_rn(0.5, t);
    w = (Rkj - Rjk) * t;
    qj = (Rji + Rij) * t;
    qk = (Rki + Rik) * t;
}
__device__ __forceinline__ void poQuatFromMatrix(const double (&R)[9], double (&q)[4]) {
    double t = (R[0] + R[4]) + R[8];
    if (t > 0.0) {
        t = __dsqrt_rn(t + 1.0);
        q[3] = 0.5 * t;
        t = __ddiv_rn(0.5, t);
        q[0] = (R[7] - R[5]) * t; q[1] = (R[2] - R[6]) * t; q[2] = (R[3] - R[1]) * t;
        return;
    }
    // the largest diagonal element i, then j = i + 1, k = j + 1 (mod 3).  The three branches are computed on named values and one is selected
    // (a branch not taken may hold a NaN): no register is indexed
    const bool i1 = R[4] > R[0], i2 = R[8] > (i1 ? +R[4] : +R[0]);
    double a0, a1, a2, aw, b0, b1, b2, bw, c0, c1, c2, cw;
    poQuatDiag(R[0], R[4], R[8], R[7], R[5], R[3], R[1], R[6], R[2], a0, a1, a2, aw);      // i = 0: x, y, z
    poQuatDiag(R[4], R[8], R[0], R[2], R[6], R[7], R[5], R[1], R[3], b1, b2, b0, bw);      // i = 1: y, z, x
    poQuatDiag(R[8], R[0], R[4], R[3], R[1], R[2], R[6], R[5], R[7], c2, c0, c1, cw);      // i = 2: z, x, y
    q[0] = i2 ? c0 : i1 ? b0 : a0; q[1] = i2 ? c1 : i1 ? b1 : a1; q[2] = i2 ? c2 : i1 ? b2 : a2; q[3] = i2 ? cw : i1 ? bw : aw;
}
__device__ __forceinline__ void poRotMatrix(const double (&q)[4], double (&R)[9]) {
    const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3], txx = tx * q[0], txy = ty * q[0], txz = tz * q[0], tyy = ty * q[1], tyz = tz * q[1],
                 tzz = tz * q[2];
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}
// q * v as Eigen's _transformVector: uv = 2 (q.vec x v); v + w uv + q.vec x uv
__device__ __forceinline__ void poRotate(const double (&q)[4], const double (&v)[3], double (&out)[3]) {
    double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
#pragma unroll
    for (int k = 0; k < 3; k++) uv[k] = uv[k] + uv[k];
    const double c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
#pragma unroll
    for (int k = 0; k < 3; k++) out[k] = (v[k] + q[3] * uv[k]) + c[k];
}
__device__ __forceinline__ void poMap(const PoSE3& T, const double (&X)[3], double (&out)[3]) {
    poRotate(T.q, X, out);
#pragma unroll
    for (int k = 0; k < 3; k++) out[k] = out[k] + T.t[k];
}
// SE3Quat::operator*
__device__ __forceinline__ void poMul(const PoSE3& A, const PoSE3& B, PoSE3& out) {
    double r[3];
    poRotate(A.q, B.t, r);
    const double (&a)[4] = A.q;
    const double (&b)[4] = B.q;
    double q[4];
    q[3] = ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2];
    q[0] = ((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1];
    q[1] = ((a[3] * b[1] + a[1] * b[3]) + a[2] * b[0]) - a[0] * b[2];
    q[2] = ((a[3] * b[2] + a[2] * b[3]) + a[0] * b[1]) - a[1] * b[0];
    poNormalize(q);
#pragma unroll
    for (int k = 0; k < 3; k++) out.t[k] = A.t[k] + r[k];
#pragma unroll
    for (int k = 0; k < 4; k++) out.q[k] = q[k];
}
// Converter::toSE3Quat of a float 3x4 and Converter::toCvMat back
__device__ __forceinline__ void poFromFloat(const float* T, PoSE3& out) {
    double R[9];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) R[3 * r + c] = (double)T[4 * r + c];
        out.t[r] = (double)T[4 * r + 3];
    }
    poQuatFromMatrix(R, out.q);
    poNormalize(out.q);
}
__device__ __forceinline__ void poToFloat(const PoSE3& T, float* out) {
    double R[9];
    poRotMatrix(T.q, R);
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) out[4 * r + c] = canonNaN((float)R[3 * r + c]);
        out[4 * r + 3] = canonNaN((float)T.t[r]);
    }
}
__device__ __forceinline__ void poMat3(const double (&A)[9], const double (&B)[9], double (&C)[9]) {
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) C[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
}
// SE3Quat::exp: x = omega[3], upsilon[3]
__device__ __forceinline__ void poExp(const double (&x)[6], PoSE3& out) {
    const double theta = __dsqrt_rn((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
    const double Om[9] = {0.0, -x[2], x[1], x[2], 0.0, -x[0], -x[1], x[0], 0.0};
    double Om2[9], R[9], V[9];
    poMat3(Om, Om, Om2);
    if (theta < 0.00001) {
#pragma unroll
        for (int k = 0; k < 9; k++) { R[k] = ((k % 4 == 0 ? 1.0 : 0.0) + Om[k]) + Om2[k]; V[k] = R[k]; }
    } else {
        double s, c;
        sinCosDouble(theta, s, c);
        const double th2 = theta * theta, a = __ddiv_rn(s, theta), b = __ddiv_rn(1.0 - c, th2), d = __ddiv_rn(theta - s, th2 * theta);
#pragma unroll
        for (int k = 0; k < 9; k++) {
            const double id = k % 4 == 0 ? 1.0 : 0.0;
            R[k] = (id + a * Om[k]) + b * Om2[k];
            V[k] = (id + b * Om[k]) + d * Om2[k];
        }
    }
    poQuatFromMatrix(R, out.q);
    poNormalize(out.q);
#pragma unroll
    for (int r = 0; r < 3; r++) out.t[r] = (V[3 * r] * x[3] + V[3 * r + 1] * x[4]) + V[3 * r + 2] * x[5];
}

// ---- the cameras, Eigen overloads ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void poProject(int model, const float (&k)[8], const double (&X)[3], double (&uv)[2]) {
    if (!model) {
        uv[0] = __ddiv_rn((double)k[0] * X[0], X[2]) + (double)k[2];
        uv[1] = __ddiv_rn((double)k[1] * X[1], X[2]) + (double)k[3];
        return;
    }
    const double x2y2 = X[0] * X[0] + X[1] * X[1];
    const double theta = (double)atan2f32(sqrtFloat32((float)x2y2), (float)X[2]), psi = (double)atan2f32((float)X[1], (float)X[0]);
    const double t2 = theta * theta, t3 = theta * t2, t5 = t3 * t2, t7 = t5 * t2, t9 = t7 * t2;
    const double r = (((theta + (double)k[4] * t3) + (double)k[5] * t5) + (double)k[6] * t7) + (double)k[7] * t9;
    double s, c;
    sinCosDouble(fabs(psi), s, c);
    if (psi < 0.0) s = -s;
    uv[0] = ((double)k[0] * r) * c + (double)k[2];
    uv[1] = ((double)k[1] * r) * s + (double)k[3];
}
__device__ __forceinline__ void poProjectJac(int model, const float (&k)[8], const double (&X)[3], double (&J)[6]) {
    if (!model) {
        J[0] = __ddiv_rn((double)k[0], X[2]); J[1] = 0.0; J[2] = __ddiv_rn((double)(-k[0]) * X[0], X[2] * X[2]);
        J[3] = 0.0; J[4] = __ddiv_rn((double)k[1], X[2]); J[5] = __ddiv_rn((double)(-k[1]) * X[1], X[2] * X[2]);
        return;
    }
    const double x2 = X[0] * X[0], y2 = X[1] * X[1], z2 = X[2] * X[2], r2 = x2 + y2, r = __dsqrt_rn(r2), r3 = r2 * r;
    const double theta = atan2Double(r, X[2]);
    const double t2 = theta * theta, t3 = t2 * theta, t4 = t2 * t2, t5 = t4 * theta, t6 = t2 * t4, t7 = t6 * theta, t8 = t4 * t4, t9 = t8 * theta;
    const double f = (((theta + t3 * (double)k[4]) + t5 * (double)k[5]) + t7 * (double)k[6]) + t9 * (double)k[7];
    const double fd = (((1.0 + (double)__fmul_rn(3.0f, k[4]) * t2) + (double)__fmul_rn(5.0f, k[5]) * t4) + (double)__fmul_rn(7.0f, k[6]) * t6) +
                      (double)__fmul_rn(9.0f, k[7]) * t8;
    const double den = r2 * (r2 + z2), fz = fd * X[2];
    const double cross = __ddiv_rn((fz * X[1]) * X[0], den) - __ddiv_rn((f * X[1]) * X[0], r3);
    J[0] = (double)k[0] * (__ddiv_rn(fz * x2, den) + __ddiv_rn(f * y2, r3));
    J[3] = (double)k[1] * cross;
    J[1] = (double)k[0] * cross;
    J[4] = (double)k[1] * (__ddiv_rn(fz * y2, den) + __ddiv_rn(f * x2, r3));
    J[2] = __ddiv_rn(((double)(-k[0]) * fd) * X[0], r2 + z2);
    J[5] = __ddiv_rn(((double)(-k[1]) * fd) * X[1], r2 + z2);
}

// ---- an edge ---------------------------------------------------------------------------------------------------------------------------------
// the uniform part of a pose: the estimate, mTrl * estimate and mTrl's rotation matrix
struct PoFrame { PoSE3 T, Tr, Trl; double Rrl[9]; };
__device__ __forceinline__ void poSetPose(PoFrame& F, const PoSE3& T, bool rig) {
    F.T = T;
    if (rig) poMul(F.Trl, T, F.Tr);
}
// computeError: e[0 .. dim)
__device__ __forceinline__ int poError(const PoseProblem& pb, const PoFrame& F, const PoEdge& E, double (&e)[3]) {
    double Xc[3], uv[2];
    e[2] = 0.0;
    if (E.kind == 2) {
        poMap(F.T, E.X, Xc);
        const double invz = (double)(float)__ddiv_rn(1.0, Xc[2]);
        const double u = ((Xc[0] * invz) * (double)pb.cam[0]) + (double)pb.cam[2], v = ((Xc[1] * invz) * (double)pb.cam[1]) + (double)pb.cam[3];
        e[0] = E.obs[0] - u; e[1] = E.obs[1] - v; e[2] = E.obs[2] - (u - (double)pb.mbf * invz);
        return 3;
    }
    if (E.kind == 3) { poMap(F.Tr, E.X, Xc); poProject(pb.model2, pb.cam2, Xc, uv); }
    else { poMap(F.T, E.X, Xc); poProject(pb.model, pb.cam, Xc, uv); }
    e[0] = E.obs[0] - uv[0]; e[1] = E.obs[1] - uv[1];
    return 2;
}
// information * e with every product, then e . (information * e)
__device__ __forceinline__ double poChi2(const PoEdge& E, int dim, const double (&e)[3], double (&we)[3]) {
    if (dim == 2) {
        we[0] = E.w * e[0] + 0.0 * e[1]; we[1] = 0.0 * e[0] + E.w * e[1]; we[2] = 0.0;
        return e[0] * we[0] + e[1] * we[1];
    }
    we[0] = (E.w * e[0] + 0.0 * e[1]) + 0.0 * e[2]; we[1] = (0.0 * e[0] + E.w * e[1]) + 0.0 * e[2]; we[2] = (0.0 * e[0] + 0.0 * e[1]) + E.w * e[2];
    return (e[0] * we[0] + e[1] * we[1]) + e[2] * we[2];
}
// RobustKernelHuber::robustify's rho[0], rho[1]; without a kernel (chi2, 1)
__device__ __forceinline__ void poRobust(const PoEdge& E, bool huber, double chi2, double& rho0, double& rho1) {
    rho0 = chi2; rho1 = 1.0;
    if (!huber) return;
    const double delta = poSqrtOfFloat(E.kind == 2 ? 7.815 : 5.991), dsqr = delta * delta;
    if (chi2 <= dsqr) return;
    const double sq = __dsqrt_rn(chi2);
    rho0 = (2.0 * sq) * delta - dsqr;
    rho1 = __ddiv_rn(delta, sq);
}
// (-J[2x3]) * D[3x6], D = SE3deriv of X: every product, k ascending
__device__ __forceinline__ void poChain(const double (&J)[6], const double (&X)[3], double (&A)[18]) {
    const double D[18] = {0.0, X[2], -X[1], 1.0, 0.0, 0.0, -X[2], 0.0, X[0], 0.0, 1.0, 0.0, X[1], -X[0], 0.0, 0.0, 0.0, 1.0};
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
        for (int c = 0; c < 6; c++) A[6 * r + c] = ((-J[3 * r]) * D[c] + (-J[3 * r + 1]) * D[6 + c]) + (-J[3 * r + 2]) * D[12 + c];
}
// linearizeOplus: A[dim x 6]
__device__ __forceinline__ void poJacobian(const PoseProblem& pb, const PoFrame& F, const PoEdge& E, double (&A)[18]) {
    double Xl[3], J[6];
    poMap(F.T, E.X, Xl);
#pragma unroll
    for (int k = 12; k < 18; k++) A[k] = 0.0;
    if (E.kind == 2) {
        const double x = Xl[0], y = Xl[1], invz = __ddiv_rn(1.0, Xl[2]), invz2 = invz * invz, fx = (double)pb.cam[0], fy = (double)pb.cam[1], bf = (double)pb.mbf;
        A[0] = ((x * y) * invz2) * fx; A[1] = (-(1.0 + (x * x) * invz2)) * fx; A[2] = (y * invz) * fx; A[3] = (-invz) * fx; A[4] = 0.0; A[5] = (x * invz2) * fx;
        A[6] = (1.0 + (y * y) * invz2) * fy; A[7] = ((-x * y) * invz2) * fy; A[8] = ((-x) * invz) * fy; A[9] = 0.0; A[10] = (-invz) * fy; A[11] = (y * invz2) * fy;
        A[12] = A[0] - (bf * y) * invz2; A[13] = A[1] + (bf * x) * invz2; A[14] = A[2]; A[15] = A[3]; A[16] = 0.0; A[17] = A[5] - bf * invz2;
        return;
    }
    if (E.kind == 3) {
        double Xr[3], M[6];
        poMap(F.Trl, Xl, Xr);
        poProjectJac(pb.model2, pb.cam2, Xr, J);
#pragma unroll
        for (int r = 0; r < 2; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) M[3 * r + c] = ((-J[3 * r]) * F.Rrl[c] + (-J[3 * r + 1]) * F.Rrl[3 + c]) + (-J[3 * r + 2]) * F.Rrl[6 + c];
#pragma unroll
        for (int k = 0; k < 6; k++) M[k] = -M[k];             // poChain negates: (-J * Rrl) * D
        poChain(M, Xl, A);
        return;
    }
    poProjectJac(pb.model, pb.cam, Xl, J);
    poChain(J, Xl, A);
}

// edge k of the problem, or kind 0
__device__ __forceinline__ void poLoadEdge(const PoseProblem& pb, const PoArgs& a, int k, PoEdge& E) {
    const int eye = k / a.cap, i = k - eye * a.cap;
    E.kind = 0;
    if (i >= (eye ? a.n[1] : a.n[0])) return;
    const int m = (eye ? a.matches[1] : a.matches[0])[i];
    if (m < 0) return;
    const Keypoint kp = (eye ? a.kps[1] : a.kps[0])[i];
    E.obs[0] = (double)kp.x; E.obs[1] = (double)kp.y; E.obs[2] = 0.0;
    E.w = (double)pb.invSigma2[kp.octave];
#pragma unroll
    for (int c = 0; c < 3; c++) E.X[c] = (double)a.world[(long long)m * 3 + c];
    E.kind = eye ? 3 : 1;
    if (a.eyes == 1 && a.uRight) {
        const float ur = a.uRight[i];
        if (!(ur < 0.0f)) { E.kind = 2; E.obs[2] = (double)ur; }
    }
}

// ---- the sums ------------------------------------------------------------------------------------------------------------------------------------
// term(k, acc) adds edge k's terms onto its slot's accumulators; out = the tree over the slots.  `lds`: kPoLdsBytes of the workgroup.
#ifdef ORBX_HOST_ROW
template <int N, class F> inline void poSum(int, int nEdges, double*, F term, double (&out)[N]) {
    static thread_local double acc[kPoSlots][N], nxt[kPoSlots][N];
    for (int s = 0; s < kPoSlots; s++) {
        for (int c = 0; c < N; c++) acc[s][c] = 0.0;
        for (int k = s; k < nEdges; k += kPoSlots) term(k, acc[s]);
    }
    for (int stride = 1; stride < kPoSlots; stride *= 2) {
        for (int s = 0; s < kPoSlots; s++)
            for (int c = 0; c < N; c++) nxt[s][c] = acc[s][c] + acc[s ^ stride][c];
        for (int s = 0; s < kPoSlots; s++)
            for (int c = 0; c < N; c++) acc[s][c] = nxt[s][c];
    }
    for (int c = 0; c < N; c++) out[c] = acc[0][c];
}
#else
template <int N, class F> __device__ __forceinline__ void poSum(int tid, int nEdges, double* lds, F term, double (&out)[N]) {
    double acc[N];
#pragma unroll
    for (int c = 0; c < N; c++) acc[c] = 0.0;
    for (int k = tid; k < nEdges; k += kPoSlots) term(k, acc);
#pragma unroll
    for (int stride = 1; stride < 64; stride *= 2)
#pragma unroll
        for (int c = 0; c < N; c++) acc[c] = acc[c] + __shfl_xor(acc[c], stride, 64);
    const int wave = tid >> 6;
    if ((tid & 63) == 0)
#pragma unroll
        for (int c = 0; c < N; c++) lds[wave * N + c] = acc[c];
    __syncthreads();
#pragma unroll
    for (int c = 0; c < N; c++) out[c] = (lds[c] + lds[N + c]) + (lds[2 * N + c] + lds[3 * N + c]);
    __syncthreads();
}
#endif

// ---- the 6x6 solve -------------------------------------------------------------------------------------------------------------------------------
// (H + lambda I) x = b, H's upper triangle row by row in Hu[21].  false: a pivot was not > 0 and x is untouched
__device__ __forceinline__ bool poSolve6(const double (&Hu)[21], double lambda, const double (&b)[6], double (&x)[6]) {
    double L[36];
    int at = 0;
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
        for (int c = r; c < 6; c++) { L[6 * c + r] = Hu[at] + (r == c ? lambda : 0.0); at++; }      // the lower triangle
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double d = L[6 * j + j];
#pragma unroll
        for (int k = 0; k < j; k++) d = d - L[6 * j + k] * L[6 * j + k];
        if (!(d > 0.0)) ok = false;
        d = __dsqrt_rn(d);
        L[6 * j + j] = d;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double s = L[6 * i + j];
#pragma unroll
            for (int k = 0; k < j; k++) s = s - L[6 * i + k] * L[6 * j + k];
            L[6 * i + j] = __ddiv_rn(s, d);
        }
    }
    if (!ok) return false;
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; k++) s = s - L[6 * i + k] * y[k];
        y[i] = __ddiv_rn(s, L[6 * i + i]);
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) s = s - L[6 * k + i] * x[k];
        x[i] = __ddiv_rn(s, L[6 * i + i]);
    }
    return true;
}

// ---- one problem ---------------------------------------------------------------------------------------------------------------------------------
// the robust chi2 of the active edges at F (a trial's computeActiveErrors + activeRobustChi2)
__device__ __forceinline__ double poChiPass(int tid, const PoseProblem& pb, const PoArgs& a, const PoFrame& F, bool huber, double* lds) {
    double out[1];
    poSum<1>(tid, a.eyes * a.cap, lds, [&](int k, double (&acc)[1]) {
        PoEdge E;
        poLoadEdge(pb, a, k, E);
        const int eye = k / a.cap;
        if (!E.kind || (eye ? a.flags[1] : a.flags[0])[k - eye * a.cap]) return;
        double e[3], we[3], rho0, rho1;
        const int dim = poError(pb, F, E, e);
        poRobust(E, huber, poChi2(E, dim, e, we), rho0, rho1);
        acc[0] = acc[0] + rho0;
    }, out);
    return out[0];
}
// computeActiveErrors, activeRobustChi2 and buildSystem at F: S = chi2, Hu[21], g[6] with b = -g
__device__ __forceinline__ void poSystemPass(int tid, const PoseProblem& pb, const PoArgs& a, const PoFrame& F, bool huber, double* lds,
                                             double (&S)[kPoSums]) {
    poSum<kPoSums>(tid, a.eyes * a.cap, lds, [&](int k, double (&acc)[kPoSums]) {
        PoEdge E;
        poLoadEdge(pb, a, k, E);
        const int eye = k / a.cap;
        if (!E.kind || (eye ? a.flags[1] : a.flags[0])[k - eye * a.cap]) return;
        double e[3], we[3], A[18], rho0, rho1;
        const int dim = poError(pb, F, E, e);
        poRobust(E, huber, poChi2(E, dim, e, we), rho0, rho1);
        poJacobian(pb, F, E, A);
        acc[0] = acc[0] + rho0;
        const double w = rho1 * E.w;
        int at = 1;
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
            for (int c = r; c < 6; c++) {
                double h = (A[r] * w) * A[c] + (A[6 + r] * w) * A[6 + c];
                if (dim == 3) h = h + (A[12 + r] * w) * A[12 + c];
                acc[at] = acc[at] + h;
                at++;
            }
#pragma unroll
        for (int j = 0; j < 6; j++) {
            double g = A[j] * we[0] + A[6 + j] * we[1];
            if (dim == 3) g = g + A[12 + j] * we[2];
            acc[22 + j] = acc[22 + j] + rho1 * g;
        }
    }, S);
}

// Everything from :856 to :1167 for problem p.  `pose`: the frame's 12 floats, read and (on the two optimising exits) written.
__device__ __forceinline__ void poSolveProblem(int tid, const PoseProblem& pb, const PoArgs& a, float* pose, PoseResult* result, double* lds) {
    const int nEdges = a.eyes * a.cap;
    // the row's head in registers, the per-round fields written where they stand (lane 0)
    struct { int status, nInitial, nBad, nInliers, rounds, emptyRounds; } res = {kPoBadArgument, 0, 0, 0, 0, 0};
    if (tid == 0)
        for (int r = 0; r < 4; r++) { result->its[r] = result->trials[r] = 0; result->lambda[r] = result->chi2[r] = 0.0; }
    auto head = [&] {
        if (tid != 0) return;
        result->status = res.status; result->nInitial = res.nInitial; result->nBad = res.nBad; result->nInliers = res.nInliers;
        result->rounds = res.rounds; result->emptyRounds = res.emptyRounds;
    };
    bool bad = (pb.model & ~1) || (a.eyes == 2 && (pb.model2 & ~1));
    bad = bad || a.n[0] < 0 || a.n[0] > a.cap || (a.eyes == 2 && (a.n[1] < 0 || a.n[1] > a.cap));
    double cnt[2] = {0.0, 0.0}, one[1] = {0.0};
    // the correspondences and what the reference would index out of bounds on
    if (!bad)
        poSum<2>(tid, nEdges, lds, [&](int k, double (&acc)[2]) {
            const int eye = k / a.cap, i = k - eye * a.cap;
            if (i >= (eye ? a.n[1] : a.n[0])) return;
            const int m = (eye ? a.matches[1] : a.matches[0])[i];
            if (m < -1 || m >= a.nMapPoints) { acc[1] = acc[1] + 1.0; return; }
            if (m < 0) return;
            const int o = (eye ? a.kps[1] : a.kps[0])[i].octave;
            if (o < 0 || o >= a.nlevels) { acc[1] = acc[1] + 1.0; return; }
            acc[0] = acc[0] + 1.0;
        }, cnt);
    bad = bad || cnt[1] != 0.0;
    if (bad) {
        head();
        return;
    }
    res.nInitial = (int)cnt[0];
    // mvbOutlier[i] = false of every edge
    poSum<1>(tid, nEdges, lds, [&](int k, double (&)[1]) {
        const int eye = k / a.cap, i = k - eye * a.cap;
        if (i < (eye ? a.n[1] : a.n[0]) && (eye ? a.matches[1] : a.matches[0])[i] >= 0) (eye ? a.flags[1] : a.flags[0])[i] = 0;
    }, one);
    if (res.nInitial < 3) {
        res.status = kPoTooFew;
        head();
        return;
    }
    PoFrame F;
    PoSE3 T0, T;
    poFromFloat(pose, T0);
    const bool rig = a.eyes == 2;
    if (rig) { poFromFloat(pb.Trl, F.Trl); poRotMatrix(F.Trl.q, F.Rrl); }
    T = T0;
    for (int round = 0; round < 4; round++) {
        const bool huber = round < 3;
        T = T0;
        PoSE3 errT = T0;
        poSetPose(F, T, rig);
        double S[kPoSums];
        poSum<1>(tid, nEdges, lds, [&](int k, double (&acc)[1]) {
            const int eye = k / a.cap, i = k - eye * a.cap;
            if (i < (eye ? a.n[1] : a.n[0]) && (eye ? a.matches[1] : a.matches[0])[i] >= 0 && !(eye ? a.flags[1] : a.flags[0])[i]) acc[0] = acc[0] + 1.0;
        }, one);
        res.rounds = round + 1;
        if (one[0] == 0.0) {
            if (tid == 0) result->its[round] = -1;
            res.emptyRounds |= 1 << round;
        } else {
            double lambda = 0.0, ni = 2.0, currentChi = 0.0, x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            int nBadLm = 0, cj = 0, trials = 0;
            for (int it = 0; it < 10; it++) {
                poSetPose(F, T, rig);
                poSystemPass(tid, pb, a, F, huber, lds, S);
                currentChi = S[0];
                const double iniChi = currentChi;
                double Hu[21], b[6];
#pragma unroll
                for (int k = 0; k < 21; k++) Hu[k] = S[1 + k];
#pragma unroll
                for (int k = 0; k < 6; k++) b[k] = -S[22 + k];
                if (it == 0) {
                    double maxD = 0.0;
                    int at = 0;
#pragma unroll
                    for (int j = 0; j < 6; j++) { const double h = fabs(Hu[at]); maxD = h < maxD ? maxD : h; at += 6 - j; }
                    lambda = 1e-5 * maxD; ni = 2.0; nBadLm = 0;
                }
                double rho = 0.0;
                int qmax = 0;
                do {
                    const PoSE3 backup = T;
                    const bool ok2 = poSolve6(Hu, lambda, b, x);
                    PoSE3 dT, Tn;
                    poExp(x, dT);
                    poMul(dT, T, Tn);
                    T = Tn; errT = Tn;
                    poSetPose(F, T, rig);
                    double tempChi = poChiPass(tid, pb, a, F, huber, lds);
                    if (!ok2) tempChi = 1.7976931348623157e308;
                    rho = currentChi - tempChi;
                    double scale = 0.0;
#pragma unroll
                    for (int j = 0; j < 6; j++) scale = scale + x[j] * (lambda * x[j] + b[j]);
                    scale = scale + 1e-3;
                    rho = __ddiv_rn(rho, scale);
                    if (rho > 0.0 && fabs(tempChi) <= 1.7976931348623157e308) {
                        const double t = 2.0 * rho - 1.0;
                        double alpha = 1.0 - (t * t) * t;
                        const double hi = __ddiv_rn(2.0, 3.0), lo = __ddiv_rn(1.0, 3.0);
                        alpha = hi < alpha ? hi : alpha;
                        lambda = lambda * (lo < alpha ? alpha : lo);
                        ni = 2.0;
                        currentChi = tempChi;
                    } else {
                        lambda = lambda * ni;
                        ni = ni * 2.0;
                        T = backup;
                    }
                    qmax++;
                } while (rho < 0.0 && qmax < 10);
                trials += qmax; cj++;
                if (qmax == 10 || rho == 0.0) break;
                if ((iniChi - currentChi) * 1e3 < iniChi) nBadLm++;
                else nBadLm = 0;
                if (nBadLm >= 3) break;
            }
            if (tid == 0) { result->its[round] = cj; result->trials[round] = trials; result->lambda[round] = canonNaN(lambda); result->chi2[round] = canonNaN(currentChi); }
        }
        // the classification: an active edge keeps the last trial's error, a flagged one is recomputed at the estimate
        PoFrame Fe = F;
        poSetPose(F, T, rig);
        poSetPose(Fe, errT, rig);
        poSum<1>(tid, nEdges, lds, [&](int k, double (&acc)[1]) {
            PoEdge E;
            poLoadEdge(pb, a, k, E);
            if (!E.kind) return;
            const int eye = k / a.cap, i = k - eye * a.cap;
            double e[3], we[3];
            uint8_t* flag = (eye ? a.flags[1] : a.flags[0]) + i;
            int dim;
            if (*flag) dim = poError(pb, F, E, e);
            else dim = poError(pb, Fe, E, e);
            const float chi2 = (float)poChi2(E, dim, e, we);
            const bool out = chi2 > (E.kind == 2 ? 7.815f : 5.991f);
            *flag = out ? 1 : 0;
            if (out) acc[0] = acc[0] + 1.0;
        }, one);
        res.nBad = (int)one[0];
        if (res.nInitial < 10) break;
    }
    res.status = res.rounds == 4 ? kPoAllRounds : kPoFewEdges;
    res.nInliers = res.nInitial - res.nBad;
    if (tid == 0) poToFloat(T, pose);
    head();
}

}  // namespace orbx
