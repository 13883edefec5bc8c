// pose_optimization_host_check.cpp - extractorb_amd/csrc/k_pose_optimization.hpp, the statement of k_pose_optimization.hip, compiled for
// the HOST (tests/cpp/host_shim stands in for the device vocabulary): the kernel's body runs problem by problem, its 256 sum slots one after
// the other, on arrays of exactly the entry's sizes.  Two uses, both without a GPU:
//   * as a shared library (tests/test_pose_optimization.py): po_host() over the scenes of the GPU tests, compared with the walk byte for
//     byte; po_exp(), po_quat(), po_solve6(), po_huber(), po_project(), po_project_jac(), po_sum() for the pieces;
//   * as a stand-alone program (-DPOSE_OPTIMIZATION_HOST_MAIN) under -fsanitize=address,undefined on exact-size heap blocks: n past the
//     capacity and negative, match indices outside the MapPoint table, octaves outside the level table, NaN points and poses, a camera
//     model that is neither.
#include "host_shim/pose_optimization_shim.h"

#include <cstdio>
#include <random>
#include <vector>

#include "../../extractorb_amd/csrc/k_pose_optimization.hpp"

using namespace orbx;

extern "C" {

int po_result_bytes() { return (int)sizeof(PoseResult); }
int po_problem_bytes() { return (int)sizeof(PoseProblem); }
int po_slots() { return kPoSlots; }
int po_lds_bytes() { return kPoLdsBytes; }
// SE3Quat::exp: out7 = q (x, y, z, w), t
void po_exp(const double* x6, double* out7) {
    double x[6];
    for (int k = 0; k < 6; k++) x[k] = x6[k];
    PoSE3 T;
    poExp(x, T);
    for (int k = 0; k < 4; k++) out7[k] = T.q[k];
    for (int k = 0; k < 3; k++) out7[4 + k] = T.t[k];
}
// Quaterniond(Matrix3d) normalised, and toRotationMatrix of it
void po_quat(const double* R9, double* q4, double* back9) {
    double R[9], q[4], B[9];
    for (int k = 0; k < 9; k++) R[k] = R9[k];
    poQuatFromMatrix(R, q);
    poNormalize(q);
    poRotMatrix(q, B);
    for (int k = 0; k < 4; k++) q4[k] = q[k];
    for (int k = 0; k < 9; k++) back9[k] = B[k];
}
int po_solve6(const double* Hu21, double lambda, const double* b6, double* x6) {
    double Hu[21], b[6], x[6];
    for (int k = 0; k < 21; k++) Hu[k] = Hu21[k];
    for (int k = 0; k < 6; k++) { b[k] = b6[k]; x[k] = x6[k]; }
    const bool ok = poSolve6(Hu, lambda, b, x);
    for (int k = 0; k < 6; k++) x6[k] = x[k];
    return ok ? 1 : 0;
}
void po_huber(int stereo, int huber, double chi2, double* rho2) {
    PoEdge E{};
    E.kind = stereo ? 2 : 1;
    poRobust(E, huber != 0, chi2, rho2[0], rho2[1]);
}
void po_project(int model, const float* cam8, const double* X3, double* uv2) {
    float k[8];
    for (int c = 0; c < 8; c++) k[c] = cam8[c];
    const double X[3] = {X3[0], X3[1], X3[2]};
    double uv[2];
    poProject(model, k, X, uv);
    uv2[0] = uv[0]; uv2[1] = uv[1];
}
void po_project_jac(int model, const float* cam8, const double* X3, double* J6) {
    float k[8];
    for (int c = 0; c < 8; c++) k[c] = cam8[c];
    const double X[3] = {X3[0], X3[1], X3[2]};
    double J[6];
    poProjectJac(model, k, X, J);
    for (int c = 0; c < 6; c++) J6[c] = J[c];
}
// the declared order on n terms, all active
double po_sum(const double* terms, int n) {
    double out[1];
    poSum<1>(0, n, nullptr, [&](int k, double (&acc)[1]) { acc[0] = acc[0] + terms[k]; }, out);
    return out[0];
}

// the arguments of orbx_optimize_pose_device on host arrays, and the handle's nlevels
void po_host(int nProblems, int frameFirst, int frameStep, int eyes, const void* problems, const void* kps, const int* nOut, const float* uRight,
             int capacity, const int* matches, const float* world, int nMapPoints, int nlevels, float* poses, uint8_t* outlier, void* result) {
    for (int p = 0; p < nProblems; p++) {
        const long long frame = frameFirst + (long long)p * frameStep;
        PoArgs a;
        a.cap = capacity; a.eyes = eyes; a.nMapPoints = nMapPoints; a.nlevels = nlevels; a.world = world;
        for (int e = 0; e < 2; e++) {
            const long long f = frame * eyes + (e < eyes ? e : 0), row = (long long)p * eyes + (e < eyes ? e : 0);
            a.kps[e] = (const Keypoint*)kps + f * capacity;
            a.matches[e] = matches + row * capacity;
            a.flags[e] = outlier + row * capacity;
            a.n[e] = nOut[f];
        }
        a.uRight = uRight ? uRight + frame * capacity : nullptr;
        poSolveProblem(0, ((const PoseProblem*)problems)[p], a, poses + frame * 12, (PoseResult*)result + p, nullptr);
    }
}

}  // extern "C"

#ifdef POSE_OPTIMIZATION_HOST_MAIN
int main() {
    std::mt19937 rng(26);
    auto U = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
    long rows = 0, optimised = 0;
    for (int trial = 0; trial < 8; trial++) {
        // trial: 0 plain stereo, 1 n past the capacity and negative, 2 match indices outside the MapPoint table, 3 octaves outside the level
        // table, 4 NaN points, 5 NaN poses, 6 a camera model that is neither, 7 a KannalaBrandt8 rig
        const int eyes = trial == 7 ? 2 : 1, cap = trial == 3 ? 7 : 90, nProblems = 3, nMp = nProblems * eyes * cap;
        // exact-size heap blocks: an access one element past any of them is reported
        std::vector<PoseProblem> pb(nProblems);
        std::vector<Keypoint> kps((size_t)nProblems * eyes * cap);
        std::vector<int> nOut((size_t)nProblems * eyes), matches((size_t)nProblems * eyes * cap);
        std::vector<float> uRight((size_t)nProblems * cap), world((size_t)nMp * 3), poses((size_t)nProblems * 12);
        std::vector<uint8_t> flags((size_t)nProblems * eyes * cap, 0xEE);
        std::vector<PoseResult> res(nProblems);
        const float pin[8] = {458.f, 457.f, 367.f, 248.f, 0.f, 0.f, 0.f, 0.f}, kb[8] = {190.9f, 190.9f, 254.9f, 256.9f, 0.0035f, 0.0007f, -0.002f, 0.0002f};
        for (int p = 0; p < nProblems; p++) {
            PoseProblem& q = pb[p];
            q = PoseProblem{};
            q.model = trial == 6 ? (p == 0 ? 2 : p == 1 ? -1 : 0) : trial == 7; q.model2 = trial == 7;
            for (int k = 0; k < 8; k++) { q.cam[k] = trial == 7 ? kb[k] : pin[k]; q.cam2[k] = kb[k]; }
            q.mbf = 47.9f;
            const float T[12] = {1.f, 0.f, 0.f, -0.1f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f};
            for (int k = 0; k < 12; k++) { q.Trl[k] = T[k]; poses[(size_t)p * 12 + k] = k % 5 == 0 ? 1.f : k == 3 ? 0.02f : 0.f; }
            if (trial == 5) poses[(size_t)p * 12 + p] = NAN;
            for (int l = 0; l < 8; l++) q.invSigma2[l] = 1.f / std::pow(1.2f, 2.f * l);
            for (int e = 0; e < eyes; e++) {
                const size_t row = (size_t)p * eyes + e;
                nOut[row] = trial == 1 ? (p == 0 ? cap + 50 : p == 1 ? -3 : cap) : cap - p;
                for (int i = 0; i < cap; i++) {
                    const size_t at = row * cap + i;
                    const float x = U(-2.f, 2.f), y = U(-1.5f, 1.5f), z = U(4.f, 8.f);
                    world[at * 3] = x; world[at * 3 + 1] = y; world[at * 3 + 2] = z;
                    if (trial == 4 && i % 9 == 0) world[at * 3 + 1] = NAN;
                    const float xe = e ? x - 0.1f : x;
                    const bool gross = i % 4 == 0;
                    Keypoint& k = kps[at];
                    k = Keypoint{};
                    if (trial == 7) {
                        const float r = std::sqrt(xe * xe + y * y), th = std::atan2(r, z);
                        k.x = kb[0] * th * xe / r + kb[2]; k.y = kb[1] * th * y / r + kb[3];
                    } else { k.x = pin[0] * x / z + pin[2]; k.y = pin[1] * y / z + pin[3]; }
                    k.x += gross ? U(20.f, 60.f) : U(-0.7f, 0.7f); k.y += gross ? U(-60.f, -20.f) : U(-0.7f, 0.7f);
                    k.octave = i % 8;
                    if (trial == 3 && i == 5) k.octave = p == 0 ? 8 : p == 1 ? -1 : 2000000000;
                    matches[at] = i % 5 == 4 ? -1 : (int)at;
                    if (trial == 2 && i == 11) matches[at] = p == 0 ? nMp : p == 1 ? -2 : 2000000000;
                    if (e == 0 && eyes == 1) uRight[(size_t)p * cap + i] = i % 2 ? -1.f : k.x - 47.9f / z;
                }
            }
        }
        po_host(nProblems, 0, 1, eyes, pb.data(), kps.data(), nOut.data(), eyes == 1 ? uRight.data() : nullptr, cap, matches.data(), world.data(), nMp, 8,
                poses.data(), flags.data(), res.data());
        for (int p = 0; p < nProblems; p++) {
            const PoseResult& r = res[p];
            if (r.status < 0 || r.status >= kPoStatuses) { std::printf("FAILED: status %d\n", r.status); return 1; }
            for (int e = 0; e < eyes; e++) {
                const size_t row = (size_t)p * eyes + e;
                const bool nok = nOut[row] >= 0 && nOut[row] <= cap;
                for (int i = 0; i < cap; i++) {
                    const uint8_t f = flags[row * cap + i];
                    const bool touched = r.status != kPoBadArgument && nok && i < nOut[row] && matches[row * cap + i] >= 0;
                    if (!touched && f != 0xEE) { std::printf("FAILED: a flag outside the edges was written\n"); return 1; }
                    if (touched && f > 1) { std::printf("FAILED: flag %d\n", f); return 1; }
                }
            }
            if (r.status == kPoAllRounds) optimised++;
            if (r.status != kPoBadArgument && r.nInliers != r.nInitial - r.nBad) { std::printf("FAILED: the return value\n"); return 1; }
            rows++;
        }
        std::printf("trial %d: status %d %d %d, n %d %d %d, bad %d %d %d, its %d %d %d\n", trial, res[0].status, res[1].status, res[2].status, res[0].nInitial,
                    res[1].nInitial, res[2].nInitial, res[0].nBad, res[1].nBad, res[2].nBad, res[0].its[0], res[1].its[0], res[2].its[0]);
    }
    if (optimised == 0) { std::printf("FAILED: nothing was optimised at all\n"); return 1; }
    std::printf("pose_optimization_host_check: every access inside its arrays, %ld rows, %ld through all rounds\n", rows, optimised);
    return 0;
}
#endif
