// k_new_map_points.hpp - the per-match arithmetic of LocalMapping::CreateNewMapPoints' triangulation loop (reference src/LocalMapping.cc:481-707):
// from vMatchedIndices[ikp] to the last `continue` of the scale-consistency test, for one-camera keyframes (Pinhole; monocular, rectified
// stereo, RGB-D) and for two-camera keyframes (a KannalaBrandt8 pair, mpCamera2 on both sides).  The map-changing tail (:709-723) and the
// per-neighbour prelude (:436-456) stay with the caller.  k_new_map_points.hip holds the kernel around these functions.
// The roundings ("parity unpinned" where a cv::Mat / cv::MatExpr hides them), each stated ONCE, here:
//   poses        Rcw | tcw, Rwc = Rcw.t(), Ow, and the right eye's GetRightRotation / GetRightTranslation / GetRightPose / GetRightCameraCenter
//                are the records of k_rig_two_eyes.hpp (KeyFrame.cc:118, :1232-1262); Twc's rotation is Rcw.t() and its translation Ow (:123-125);
//   which pose   only when both keyframes have mpCamera2 (the two-eye form) are pose and camera picked PER MATCH from bRight1, bRight2
//                (:503-568); all four branches assign everything, so nothing carries over from the match before;
//   rays         xn = unproject(kp.pt) (Pinhole.cpp:59-62: a float subtraction and division; kb8Unproject); ray = Rwc*xn one gemmRow per row;
//   parallax     ray1.dot(ray2) and cv::norm in double, the quotient rounded to float once (:576);
//   stereo       cosParallaxStereo = cosParallaxRays + 1 in float; cosParallaxStereo1 is replaced if bStereo1, ELSE IF bStereo2
//                cosParallaxStereo2 (with both stereo only the first, :582-585); cos(2*atan2(mb/2, depth)) is binary32 throughout (`using
//                namespace std` reaches LocalMapping.cc through TemplatedVocabulary.h:36, the float overloads are taken): nmpStereoCos;
//   branch       cosParallaxRays < cosParallaxStereo compares floats, > 0 compares with an int, < 0.9998 compares in double; mbInertial
//                changes nothing (:590-591: both alternatives are the same test);
//   A            a row is float(xn * Tcw.row(2)[c]) - Tcw.row(r)[c], each rounded in float; vt.row(3) = nullVector4; x3D[3] == 0 is an
//                explicit exit HERE (:605), unlike KannalaBrandt8::Triangulate; x3D = v[0..2] / v[3] a float division per element;
//   UnprojectStereo  (KeyFrame.cc:821-834, mvKeys not mvKeysUn) (u - cx)*z*invfx rounded per operation in float, invfx = 1.0f / fx;
//                Twc.R*x3Dc + Twc.t one gemmRow per element with the addend; mvDepth <= 0 gives the empty Mat of :627;
//   depths       z = Rcw.row(2).dot(x3Dt) + tcw[2] (and x, y): products and sums in double, rounded to float once;
//   gates        invz = 1.0 / z in double, rounded to float; monocular: project (Pinhole.cpp:30-33: fx*x/z + cx in float; kb8Project), the
//                squared error summed in float, > 5.991*sigma2 in double; stereo: u = fx*x*invz + cx, u_r = u - mbf*invz in float, three
//                squared errors summed in float, > 7.8*sigma2 in double;
//   distances    normal = x3D - Ow in float, dist = (float)cv::norm (sum in double); dist == 0 rejects; mbFarPoints && dist >= mThFarPoints;
//   scale        ratioDist = dist2/dist1, ratioOctave = mvScaleFactors[o1]/mvScaleFactors[o2], ratioDist*ratioFactor < ratioOctave ||
//                ratioDist > ratioOctave*ratioFactor, all in float.  An octave outside [0, nlevels) is CLAMPED into the tables.
// On a NaN pose every test is false: the match leaves as LOW_PARALLAX.
// Nothing returns early between the branch and the end: every stage is computed for every lane and the FIRST failing test decides (as
// kb8TriangulateMatches; the lanes of a wave run in lockstep).  The one region a wave skips is the SVD, when NO lane of it takes that branch
// (waveAny: a ballot on the device, the lane's own bit in the host build).
// Takes the KannalaBrandt8 camera from k_camera_kb8.hpp / k_camera_kb8_unproject.hpp, nullVector4 from k_small_svd.hpp, the Pinhole pair,
// quietNaN and waveAny from k_small_math.hpp, gemmRow and dot3Double from k_match_helpers.hpp, the eye records from k_rig_two_eyes.hpp.
// Plain arithmetic plus that one ballot: compiles for the host behind tests/cpp/host_shim (tests/cpp/new_map_points_host_check.cpp).
#pragma once
#include "k_camera_kb8_unproject.hpp"
#include "k_lds_vec.hpp"
#include "k_match_helpers.hpp"
#include "k_rig_two_eyes.hpp"
#include "k_small_math.hpp"
#include "k_small_svd.hpp"
#include "orbx_device.hpp"
#include "orbx_params.hpp"

namespace orbx {

// == orbx_new_point_exit
enum {
    kNmpTriangulated = 0, kNmpStereo1, kNmpStereo2,                                       // accepted: which branch made the point
    kNmpZeroW, kNmpLowParallax, kNmpEmptyStereo, kNmpBehind1, kNmpBehind2, kNmpReproj1, kNmpReproj2, kNmpZeroDist, kNmpFar, kNmpScale,
    kNmpBadIndex, kNmpExits
};

constexpr int kNmpThreads = 64;                           // matches of a workgroup, one per lane: one wave
constexpr int kNmpRigFloats = 4 * kRigEyeFloats;          // the staged records of a pair: [keyframe 1 | 2][eye][kRigEyeFloats]
constexpr int kNmpLdsFloats = kNmpRigFloats + 2 * kMaxLevels;      // ... then mvScaleFactors and mvLevelSigma2 (a lane indexes them by its octaves)

// one eye of a keyframe, as k_rig_two_eyes.hpp lays it out
struct NmpPose { float R[9], t[3], Ow[3]; };
// one observation: kp.pt and octave (mvKeysUn, or the eye's raw keypoint), kp_ur = mvuRight, and for bStereo mvDepth and mvKeys' pt
struct NmpObs { float u, v, ur, depth, rawU, rawV; int octave; bool stereo; };

// What thread tid of a workgroup stages before the barrier: element j < kNmpRigFloats of the records of the pair's keyframes (keyframe
// j / (2 * kRigEyeFloats), the rest as fuseTwoEyesRigElement numbers it; the one-camera form stages eye 0 only, the right eye's slots are
// never read), and in a second turn one entry of the level tables.  T1 / T2: the poses of the two keyframes (3x4 row-major).
template <bool TwoEyes>
__device__ __forceinline__ void nmpStage(int tid, const float* T1, const float* T2, const NewMapPointsParams& p, ORBX_LDS float* sRig) {
    const int kf = tid >= 2 * kRigEyeFloats, j = tid - kf * 2 * kRigEyeFloats;
    if (tid < kNmpRigFloats && (TwoEyes || j < kRigEyeFloats)) sRig[tid] = fuseTwoEyesRigElement(kf ? T2 : T1, p.tlr, j);
    if (tid < kMaxLevels) sRig[kNmpRigFloats + tid] = p.scale[tid];
    else if (tid < 2 * kMaxLevels) sRig[kNmpRigFloats + tid] = p.sigma2[tid - kMaxLevels];
}

// cos(2*atan2(mb/2, depth)) of :583 / :585 in binary32.  2*atan2f lies in [-2 pi, 2 pi]: past kb8SinCos's [-pi, pi] of the projection but
// inside the |y| < 120 its reduction holds for (tests/cpp/new_map_points_host_check.cpp compares every float of [pi, 2 pi] and its negative
// with the host libm; tests/test_kb8_math.py holds [-pi, pi]).
__device__ __forceinline__ float nmpStereoCos(float mb, float depth) {
    float s, c;
    kb8SinCos(__fmul_rn(2.0f, atan2f32(__fdiv_rn(mb, 2.0f), depth)), &s, &c);
    return c;
}

// unproject / project of the match's camera: Pinhole on k[0..3], or KannalaBrandt8
template <bool TwoEyes>
__device__ __forceinline__ void nmpUnproject(const float (&k)[8], float u, float v, float& x, float& y) {
    if constexpr (TwoEyes) kb8Unproject(k, u, v, x, y);
    else pinholeUnproject(k, u, v, x, y);
}
template <bool TwoEyes>
__device__ __forceinline__ void nmpProject(const float (&k)[8], float x, float y, float z, float& u, float& v) {
    if constexpr (TwoEyes) kb8Project(k, x, y, z, u, v);
    else pinholeProject(k, x, y, z, u, v);
}

// x, y, z of x3D in the eye (:629-640), then the reprojection gate of that keyframe (:643-663 / :670-688); behind = z <= 0
__device__ __forceinline__ float nmpRowDot(const NmpPose& P, int r, const float (&x3D)[3]) {
    return (float)__dadd_rn(dot3Double(P.R[3 * r], P.R[3 * r + 1], P.R[3 * r + 2], x3D[0], x3D[1], x3D[2]), (double)P.t[r]);
}
template <bool TwoEyes>
__device__ __forceinline__ void nmpGate(const NmpPose& P, const float (&k)[8], const NmpObs& o, const float (&x3D)[3], float sigma2, float mbf,
                                        bool& behind, bool& reproj) {
    const float z = nmpRowDot(P, 2, x3D), x = nmpRowDot(P, 0, x3D), y = nmpRowDot(P, 1, x3D);
    behind = z <= 0.0f;
    const float invz = (float)__ddiv_rn(1.0, (double)z);
    float pu, pv;
    nmpProject<TwoEyes>(k, x, y, z, pu, pv);
    const float ex = __fsub_rn(pu, o.u), ey = __fsub_rn(pv, o.v);
    const bool monoOut = (double)__fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey)) > __dmul_rn(5.991, (double)sigma2);
    bool stereoOut = false;
    if constexpr (!TwoEyes) {                                                                  // (bStereo is false on two-camera keyframes, :490, :499)
        const float su = __fadd_rn(__fmul_rn(__fmul_rn(k[0], x), invz), k[2]), sur = __fsub_rn(su, __fmul_rn(mbf, invz)),
                    sv = __fadd_rn(__fmul_rn(__fmul_rn(k[1], y), invz), k[3]);
        const float sx = __fsub_rn(su, o.u), sy = __fsub_rn(sv, o.v), sr = __fsub_rn(sur, o.ur);
        stereoOut = (double)__fadd_rn(__fadd_rn(__fmul_rn(sx, sx), __fmul_rn(sy, sy)), __fmul_rn(sr, sr)) > __dmul_rn(7.8, (double)sigma2);
    }
    reproj = o.stereo ? stereoOut : monoOut;
}

// One match.  P1 / P2, k1 / k2: pose record and camera of the eye each observation lies in; lev = mvLevelSigma2 of kp1's and kp2's octave,
// then mvScaleFactors of the two.  Returns the exit; x3D is the world point, zeros on every rejecting exit.  svd / stereoBranch: whether this match asked for the SVD / took an UnprojectStereo branch (the debug counters).
template <bool TwoEyes>
__device__ __forceinline__ int nmpMatch(const NmpPose& P1, const NmpPose& P2, const float (&k1)[8], const float (&k2)[8], const NmpObs& o1,
                                        const NmpObs& o2, const float (&lev)[4], const NewMapPointsParams& p, float (&x3D)[3], bool& svd,
                                        bool& stereoBranch) {
    // :571-576
    float xn1[3], xn2[3], ray1[3], ray2[3];
    nmpUnproject<TwoEyes>(k1, o1.u, o1.v, xn1[0], xn1[1]);
    nmpUnproject<TwoEyes>(k2, o2.u, o2.v, xn2[0], xn2[1]);
    xn1[2] = xn2[2] = 1.0f;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        ray1[r] = gemmRow(P1.R[r], P1.R[3 + r], P1.R[6 + r], xn1, 1.0, 0.f, false);
        ray2[r] = gemmRow(P2.R[r], P2.R[3 + r], P2.R[6 + r], xn2, 1.0, 0.f, false);
    }
    const double n1 = __dsqrt_rn(dot3Double(ray1[0], ray1[1], ray1[2], ray1[0], ray1[1], ray1[2])),
                 n2 = __dsqrt_rn(dot3Double(ray2[0], ray2[1], ray2[2], ray2[0], ray2[1], ray2[2]));
    const float cosRays = (float)__ddiv_rn(dot3Double(ray1[0], ray1[1], ray1[2], ray2[0], ray2[1], ray2[2]), __dmul_rn(n1, n2));
    // :578-587
    float cos1 = __fadd_rn(cosRays, 1.0f), cos2 = cos1;
    if (o1.stereo) cos1 = nmpStereoCos(p.mb, o1.depth);
    else if (o2.stereo) cos2 = nmpStereoCos(p.mb, o2.depth);
    const float cosStereo = cos2 < cos1 ? cos2 : cos1;                                        // std::min(cos1, cos2)
    // :590-623
    svd = cosRays < cosStereo && cosRays > 0.0f && (o1.stereo || o2.stereo || (double)cosRays < 0.9998);
    const bool st1 = !svd && o1.stereo && cos1 < cos2, st2 = !svd && !st1 && o2.stereo && cos2 < cos1;
    stereoBranch = st1 || st2;
    int first = svd || stereoBranch ? -1 : kNmpLowParallax;
    x3D[0] = x3D[1] = x3D[2] = 0.0f;
    if (waveAny(svd)) {                                                                         // (wave-uniform)
        float A[16], vt[4];
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const float r2a = c < 3 ? P1.R[6 + c] : P1.t[2], r0a = c < 3 ? P1.R[c] : P1.t[0], r1a = c < 3 ? P1.R[3 + c] : P1.t[1];
            const float r2b = c < 3 ? P2.R[6 + c] : P2.t[2], r0b = c < 3 ? P2.R[c] : P2.t[0], r1b = c < 3 ? P2.R[3 + c] : P2.t[1];
            A[c] = __fsub_rn(__fmul_rn(xn1[0], r2a), r0a);
            A[4 + c] = __fsub_rn(__fmul_rn(xn1[1], r2a), r1a);
            A[8 + c] = __fsub_rn(__fmul_rn(xn2[0], r2b), r0b);
            A[12 + c] = __fsub_rn(__fmul_rn(xn2[1], r2b), r1b);
        }
        nullVector4(A, vt);
        if (svd) {
            if (vt[3] == 0.0f) first = kNmpZeroW;                                              // :605
#pragma unroll
            for (int r = 0; r < 3; r++) x3D[r] = __fdiv_rn(vt[r], vt[3]);
        }
    }
    if constexpr (!TwoEyes) {
        if (stereoBranch) {                                                                    // KeyFrame::UnprojectStereo of the stereo keyframe
            const NmpObs& o = st1 ? o1 : o2;
            const NmpPose& P = st1 ? P1 : P2;
            const float (&k)[8] = st1 ? k1 : k2;
            const float z = o.depth;
            if (!(z > 0.0f)) first = kNmpEmptyStereo;                                          // :627
            const float c3[3] = {__fmul_rn(__fmul_rn(__fsub_rn(o.rawU, k[2]), z), __fdiv_rn(1.0f, k[0])),
                                 __fmul_rn(__fmul_rn(__fsub_rn(o.rawV, k[3]), z), __fdiv_rn(1.0f, k[1])), z};
#pragma unroll
            for (int r = 0; r < 3; r++) x3D[r] = gemmRow(P.R[r], P.R[3 + r], P.R[6 + r], c3, 1.0, P.Ow[r], true);
        }
    }
    // :629-688
    bool behind1, behind2, reproj1, reproj2;
    nmpGate<TwoEyes>(P1, k1, o1, x3D, lev[0], p.mbf, behind1, reproj1);
    nmpGate<TwoEyes>(P2, k2, o2, x3D, lev[1], p.mbf, behind2, reproj2);
    // :691-707
    const float a0 = __fsub_rn(x3D[0], P1.Ow[0]), a1 = __fsub_rn(x3D[1], P1.Ow[1]), a2 = __fsub_rn(x3D[2], P1.Ow[2]);
    const float b0 = __fsub_rn(x3D[0], P2.Ow[0]), b1 = __fsub_rn(x3D[1], P2.Ow[1]), b2 = __fsub_rn(x3D[2], P2.Ow[2]);
    const float dist1 = (float)__dsqrt_rn(dot3Double(a0, a1, a2, a0, a1, a2)), dist2 = (float)__dsqrt_rn(dot3Double(b0, b1, b2, b0, b1, b2));
    const bool zeroDist = dist1 == 0.0f || dist2 == 0.0f;
    const bool far = p.farPoints && (dist1 >= p.thFarPoints || dist2 >= p.thFarPoints);
    const float ratioDist = __fdiv_rn(dist2, dist1), ratioOctave = __fdiv_rn(lev[2], lev[3]);
    const bool scaleOut = __fmul_rn(ratioDist, p.ratioFactor) < ratioOctave || ratioDist > __fmul_rn(ratioOctave, p.ratioFactor);
    // the reference's order of `continue`s
    const int exit = first >= 0 ? first : behind1 ? kNmpBehind1 : behind2 ? kNmpBehind2 : reproj1 ? kNmpReproj1 : reproj2 ? kNmpReproj2 :
                     zeroDist ? kNmpZeroDist : far ? kNmpFar : scaleOut ? kNmpScale : svd ? kNmpTriangulated : st1 ? kNmpStereo1 : kNmpStereo2;
    if (exit > kNmpStereo2) x3D[0] = x3D[1] = x3D[2] = 0.0f;
    return exit;
}

// Where match k of a pair finds its two observations.  n1L / n1R / n2L / n2R: the keypoint counts of the keyframes' batch frames, clamped
// into [0, capacity] (one camera: nXR = 0).  false: an index outside its keyframe's [0, N) - nothing is read (the reference would index
// out of bounds).  eye / local: bRight and the index inside that eye.
__device__ __forceinline__ bool nmpLocate(int idx, int nL, int nR, int& eye, int& local) {
    eye = idx >= nL;
    local = idx - (eye ? nL : 0);
    return idx >= 0 && idx < nL + nR;
}

// the observation of keypoint `local` of batch frame f.  One camera: kps = mvKeysUn, raw = mvKeys, uRight / depth may be NULL (p.mono).
template <bool TwoEyes>
__device__ __forceinline__ NmpObs nmpLoadObs(long long f, int local, const Keypoint* __restrict__ kps, const Keypoint* __restrict__ raw,
                                             const float* __restrict__ uRight, const float* __restrict__ depth, const NewMapPointsParams& p) {
    const long long at = f * p.capacity + local;
    NmpObs o;
    o.u = kps[at].x; o.v = kps[at].y; o.octave = kps[at].octave;
    o.ur = -1.0f; o.depth = 0.0f; o.rawU = o.rawV = 0.0f; o.stereo = false;
    if constexpr (!TwoEyes) {
        if (!p.mono) {
            o.ur = uRight[at];
            o.stereo = o.ur >= 0.0f;                                                           // :490, :499
            if (o.stereo) { o.depth = depth[at]; o.rawU = raw[at].x; o.rawV = raw[at].y; }
        }
    }
    return o;
}

// bit 0 of byte `at` of a flag row, set and never cleared.  Several matches may share a keypoint and neighbouring bytes belong to other
// lanes: an atomic OR on the containing 32-bit word (the rows start 4-byte aligned and end on a word: include/orbx.h)
__device__ __forceinline__ void nmpMark(uint8_t* row, long long at) {
#ifdef ORBX_HOST_ROW
    row[at] |= 1;
#else
    const long long mis = (long long)(((uintptr_t)row + (uintptr_t)at) & 3);
    atomicOr((unsigned*)(row + (at - mis)), 1u << (8 * (int)mis));
#endif
}

// Match k < n of pair `pair` (the lane's whole work between the barrier and the count): the two indices, their observations, the poses
// of their eyes from the staged records sRig, nmpMatch, d_exit and d_x3d, the marks.  active = false (a lane past the list's end) computes
// on a NaN observation, takes no branch and writes nothing.  Returns whether the match was accepted.
template <bool TwoEyes>
__device__ __forceinline__ bool nmpLane(int pair, int k, bool active, const ORBX_LDS float* sRig, const int* __restrict__ pairs,
                                        const Keypoint* __restrict__ kps, const Keypoint* __restrict__ raw, const float* __restrict__ uRight,
                                        const float* __restrict__ depth, const int* __restrict__ nOut, const NewMapPointsParams& p,
                                        uint8_t* __restrict__ exitOut, float* __restrict__ x3dOut, uint8_t* mark1, uint8_t* mark2, bool& svd,
                                        bool& stereoBranch) {
    const int cap = p.capacity;
    const long long X1 = p.kf1First + (long long)pair * p.kf1Step, X2 = p.kf2First + (long long)pair * p.kf2Step;
    const long long f1 = TwoEyes ? 2 * X1 : X1, f2 = TwoEyes ? 2 * X2 : X2;                     // the (left eye's) batch frame
    const long long slot = (long long)pair * p.listCapacity + k;
    int eye1 = 0, eye2 = 0, local1 = 0, local2 = 0;
    bool inside = false;
    if (active) {
        const int n1L = max(0, min(nOut[f1], cap)), n1R = TwoEyes ? max(0, min(nOut[f1 + 1], cap)) : 0;
        const int n2L = max(0, min(nOut[f2], cap)), n2R = TwoEyes ? max(0, min(nOut[f2 + 1], cap)) : 0;
        const bool in1 = nmpLocate(pairs[2 * slot], n1L, n1R, eye1, local1), in2 = nmpLocate(pairs[2 * slot + 1], n2L, n2R, eye2, local2);
        inside = in1 && in2;
    }
    NmpObs o1, o2;
    if (inside) {
        o1 = nmpLoadObs<TwoEyes>(f1 + eye1, local1, kps, raw, uRight, depth, p);
        o2 = nmpLoadObs<TwoEyes>(f2 + eye2, local2, kps, raw, uRight, depth, p);
    } else {
        eye1 = eye2 = 0;
        o1.u = o1.v = quietNaN(); o1.ur = -1.0f; o1.depth = o1.rawU = o1.rawV = 0.0f; o1.octave = 0; o1.stereo = false;
        o2 = o1;
    }
    NmpPose P1, P2;
#pragma unroll
    for (int j = 0; j < kRigEyeFloats; j++) {
        const float a = sRig[eye1 * kRigEyeFloats + j], b = sRig[(2 + eye2) * kRigEyeFloats + j];
        if (j < 9) { P1.R[j] = a; P2.R[j] = b; }
        else if (j < 12) { P1.t[j - 9] = a; P2.t[j - 9] = b; }
        else { P1.Ow[j - 12] = a; P2.Ow[j - 12] = b; }
    }
    float k1[8], k2[8];
#pragma unroll
    for (int a = 0; a < 8; a++) { k1[a] = eye1 ? p.cam[1][a] : p.cam[0][a]; k2[a] = eye2 ? p.cam[1][a] : p.cam[0][a]; }      // pCamera1, pCamera2 (:517-566)
    const int l1 = min(max(o1.octave, 0), p.nlevels - 1), l2 = min(max(o2.octave, 0), p.nlevels - 1);      // (clamped: the reference would index past the tables)
    const float lev[4] = {sRig[kNmpRigFloats + kMaxLevels + l1], sRig[kNmpRigFloats + kMaxLevels + l2], sRig[kNmpRigFloats + l1], sRig[kNmpRigFloats + l2]};
    float x3D[3];
    int exit = nmpMatch<TwoEyes>(P1, P2, k1, k2, o1, o2, lev, p, x3D, svd, stereoBranch);
    if (!inside) { exit = kNmpBadIndex; x3D[0] = x3D[1] = x3D[2] = 0.0f; svd = stereoBranch = false; }
    if (!active) return false;
    exitOut[slot] = (uint8_t)exit;
    x3dOut[3 * slot] = x3D[0]; x3dOut[3 * slot + 1] = x3D[1]; x3dOut[3 * slot + 2] = x3D[2];
    const bool accepted = exit <= kNmpStereo2;
    if (accepted) {                                                                            // flag rows laid out as the searches' d_kf1_mp_flags / d_kf2_mp_flags
        if (mark1) nmpMark(mark1, TwoEyes ? (2LL * pair + eye1) * cap + local1 : (long long)pair * cap + local1);
        if (mark2) nmpMark(mark2, TwoEyes ? (2LL * pair + eye2) * cap + local2 : (long long)pair * cap + local2);
    }
    return accepted;
}

}  // namespace orbx
