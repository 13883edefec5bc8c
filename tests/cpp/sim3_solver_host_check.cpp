// sim3_solver_host_check.cpp - extractorb_amd/csrc/k_sim3_solver.hpp, the statement of k_sim3_solver.hip, compiled for the HOST
// (tests/cpp/host_shim stands in for the device vocabulary) with a wave of one lane: the three kernels' bodies run as the launch wrapper
// orders them, on a workspace of exactly the entry's sizes, with the entry's own table of SetRansacParameters' iteration counts
// (orbx_entry.hpp: sim3RansacIterations).
// Three uses, all without a GPU:
//   * as a shared library (tests/test_sim3_solver.py): ss_host() over the scenes of the GPU tests, compared with the walk byte for byte;
//     ss_draw3(), ss_eigen_top4(), ss_rodrigues(), ss_compute_sim3(), ss_max_error(), ss_ransac_iterations() for the pieces;
//   * ss_check_math(): ssAtan2 and ssSinCos, rounded to float, against the host libm over a sweep - the counts of differing values;
//   * as a stand-alone program (-DSIM3_SOLVER_HOST_MAIN) under -fsanitize=address,undefined on exact-size heap blocks: n1 past the capacity
//     and negative, octaves outside the table, fewer than three correspondences, wild rand() values, NaN points, max_iterations = 1.
#include "host_shim/sim3_solver_shim.h"

#include <cstdio>
#include <random>
#include <vector>

#include "../../extractorb_amd/csrc/orbx_entry.hpp"
#include "../../extractorb_amd/csrc/k_sim3_solver.hpp"

using namespace orbx;

extern "C" {

int ss_result_bytes() { return (int)sizeof(Sim3Result); }
int ss_problem_bytes() { return (int)sizeof(Sim3Problem); }
int ss_ransac_iterations(double probability, int minInliers, int N) { return sim3RansacIterations(probability, minInliers, N); }
double ss_atan2(double y, double x) { return ssAtan2(y, x); }
void ss_sincos(double theta, double* s, double* c) { ssSinCos(theta, *s, *c); }
float ss_max_error(float sigma2) { return ssMaxError(sigma2); }
void ss_draw3(const int* r3, int N, int* idx3) {
    int idx[3];
    ssDraw3(r3, N, idx);
    for (int j = 0; j < 3; j++) idx3[j] = idx[j];
}
void ss_eigen_top4(const float* N16, float* q4) {
    float Nm[16], q[4];
    for (int k = 0; k < 16; k++) Nm[k] = N16[k];
    ssEigenTop4(Nm, q);
    for (int k = 0; k < 4; k++) q4[k] = q[k];
}
void ss_rodrigues(const float* rv3, float* R9) {
    float rv[3] = {rv3[0], rv3[1], rv3[2]}, R[9];
    ssRodrigues(rv, R);
    for (int k = 0; k < 9; k++) R9[k] = R[k];
}
// ComputeSim3 on two 3x3 point matrices (points in columns): out37 = R[9] t[3] s T12[12] T21[12]
void ss_compute_sim3(const float* P1, const float* P2, int fixScale, float* out37) {
    float A[9], B[9];
    for (int k = 0; k < 9; k++) { A[k] = P1[k]; B[k] = P2[k]; }
    Sim3Hyp h;
    ssComputeSim3(A, B, fixScale != 0, h);
    for (int k = 0; k < 9; k++) out37[k] = h.R[k];
    for (int k = 0; k < 3; k++) out37[9 + k] = h.t[k];
    out37[12] = h.s;
    for (int k = 0; k < 12; k++) { out37[13 + k] = h.T12[k]; out37[25 + k] = h.T21[k]; }
}

// the arguments of orbx_sim3_solve_device on host arrays, and the handle's nlevels
void ss_host(int nProblems, const void* problems, int capacity, const float* x1w, const float* x2w, const int* oct1, const int* oct2,
             double probability, int minInliers, int maxIterations, int nlevels, const int* rnd, void* result, uint8_t* flags) {
    const Sim3SolveParams q{capacity, maxIterations, minInliers, nlevels};
    const size_t entries = (size_t)nProblems * capacity;
    std::vector<SsPrep> prep(nProblems);
    std::vector<int> idx1(entries, -1), counts((size_t)nProblems * maxIterations, -1), its((size_t)capacity + 1);
    std::vector<float> pts(entries * kSsPointFloats, NAN);
    for (int n = 0; n <= capacity; n++) its[n] = sim3RansacIterations(probability, minInliers, n);
    const SsWork w{prep.data(), idx1.data(), pts.data(), counts.data(), its.data()};
    const Sim3Problem* pb = (const Sim3Problem*)problems;
    for (int p = 0; p < nProblems; p++) ssPrepareProblem(0, p, pb, x1w, x2w, oct1, oct2, q, w, (Sim3Result*)result, flags);
    for (int p = 0; p < nProblems; p++)
        for (int it = 0; it < maxIterations; it++) ssHypothesisWave(0, p, it, pb, rnd, q, w);
    for (int p = 0; p < nProblems; p++) ssDecideProblem(0, p, pb, rnd, q, w, (Sim3Result*)result, flags);
}

// ssAtan2 / ssSinCos rounded to float against atan2 / sin / cos of the host libm rounded to float.  The sweep: atan2(y, x) on `steps` x
// `steps` points of the quarter circle's grid y = i / steps, x = j / steps (what norm(vec) and the real part of a unit quaternion can be) and
// on negative x; sin / cos on `steps` * 8 angles of [0, 2 pi].  out6 = tested and differing for atan2, sin, cos; the worst difference in
// units of the double's last place goes to worst3.
void ss_check_math(int steps, long* out6, double* worst3) {
    for (int k = 0; k < 6; k++) out6[k] = 0;
    for (int k = 0; k < 3; k++) worst3[k] = 0.0;
    auto ulps = [](double got, double want) { return want == 0.0 ? std::fabs(got) : std::fabs(got - want) / (std::fabs(want) * 0x1p-52); };
    for (int i = 0; i <= steps; i++)
        for (int j = -steps; j <= steps; j++) {
            const double y = (double)i / steps * 1.0000001, x = (double)j / steps;
            const double got = ssAtan2(y, x), want = std::atan2(y, x);
            out6[0]++;
            out6[1] += (float)got != (float)want;
            worst3[0] = std::max(worst3[0], ulps(got, want));
        }
    for (long i = 0; i <= (long)steps * 8; i++) {
        const double theta = 6.283185307179586 * (double)i / ((double)steps * 8);
        double s, c;
        ssSinCos(theta, s, c);
        out6[2]++; out6[4]++;
        out6[3] += (float)s != (float)std::sin(theta);
        out6[5] += (float)c != (float)std::cos(theta);
        if (std::fabs(std::sin(theta)) > 1e-3) worst3[1] = std::max(worst3[1], ulps(s, std::sin(theta)));
        if (std::fabs(std::cos(theta)) > 1e-3) worst3[2] = std::max(worst3[2], ulps(c, std::cos(theta)));
    }
}

}  // extern "C"

#ifdef SIM3_SOLVER_HOST_MAIN
int main() {
    std::mt19937 rng(24);
    auto U = [&](float a, float b) { return std::uniform_real_distribution<float>(a, b)(rng); };
    long rows = 0, converged = 0;
    for (int trial = 0; trial < 8; trial++) {
        // trial: 0 plain, 1 n1 past the capacity and negative, 2 octaves outside the table, 3 fewer than three correspondences with
        // min_inliers 2, 4 wild rand() values, 5 NaN points, 6 max_iterations = 1 and capacity 7, 7 KannalaBrandt8 and a fixed scale
        const int cap = trial == 6 ? 7 : 90, nProblems = 3, iters = trial == 6 ? 1 : 40, minInliers = trial == 3 ? 2 : trial == 6 ? 4 : 15;
        // exact-size heap blocks: an access one element past any of them is reported
        std::vector<Sim3Problem> pb(nProblems);
        std::vector<float> x1w((size_t)nProblems * cap * 3), x2w((size_t)nProblems * cap * 3);
        std::vector<int> o1((size_t)nProblems * cap), o2((size_t)nProblems * cap), rnd((size_t)nProblems * iters * 3);
        std::vector<uint8_t> flags((size_t)nProblems * cap, 0xEE);
        std::vector<Sim3Result> res(nProblems);
        for (int p = 0; p < nProblems; p++) {
            Sim3Problem& q = pb[p];
            q = Sim3Problem{};
            q.n1 = trial == 1 ? (p == 0 ? cap + 50 : p == 1 ? -3 : cap) : cap - p;
            q.fixScale = trial == 7; q.model1 = q.model2 = trial == 7;
            const float pin[8] = {458.f, 457.f, 367.f, 248.f, 0.f, 0.f, 0.f, 0.f}, kb[8] = {190.9f, 190.9f, 254.9f, 256.9f, 0.0035f, 0.0007f, -0.002f, 0.0002f};
            for (int k = 0; k < 8; k++) q.cam1[k] = q.cam2[k] = trial == 7 ? kb[k] : pin[k];
            const float T[12] = {1.f, 0.f, 0.f, 0.1f, 0.f, 1.f, 0.f, -0.2f, 0.f, 0.f, 1.f, 0.3f};
            for (int k = 0; k < 12; k++) { q.Tcw1[k] = T[k]; q.Tcw2[k] = T[k]; }
            for (int l = 0; l < 8; l++) q.sigma2[l] = std::pow(1.2f, 2.f * l);
            const float yaw = 0.1f, c = std::cos(yaw), sn = std::sin(yaw), sc = trial == 7 ? 1.f : 1.7f;
            for (int i = 0; i < cap; i++) {
                const size_t at = ((size_t)p * cap + i) * 3;
                const float x = U(-2.f, 2.f), y = U(-1.5f, 1.5f), z = U(4.f, 8.f);
                x2w[at] = x; x2w[at + 1] = y; x2w[at + 2] = z;
                const bool gross = i % 3 == 0;
                x1w[at] = gross ? U(-4.f, 4.f) : sc * (c * x + sn * z) + 0.3f + U(-0.004f, 0.004f);
                x1w[at + 1] = gross ? U(-3.f, 3.f) : sc * y - 0.2f + U(-0.004f, 0.004f);
                x1w[at + 2] = gross ? U(6.f, 14.f) : sc * (-sn * x + c * z) + 0.4f + U(-0.004f, 0.004f);
                if (trial == 5 && i % 9 == 0) x1w[at] = NAN;
                o1[(size_t)p * cap + i] = i % 5 == 4 ? -1 : i % 4;
                o2[(size_t)p * cap + i] = i % 7 == 6 ? -1 : (i + 1) % 4;
                if (trial == 2 && i == 11) o1[(size_t)p * cap + i] = p == 0 ? 8 : p == 1 ? -2 : 2000000000;
                if (trial == 3 && i >= 1 + p) o1[(size_t)p * cap + i] = -1;
            }
        }
        for (auto& r : rnd) r = trial == 4 ? (int)(rng() & 0xffffffffu) : (int)(rng() & 0x7fffffffu);
        ss_host(nProblems, pb.data(), cap, x1w.data(), x2w.data(), o1.data(), o2.data(), 0.99, minInliers, iters, 8, rnd.data(), res.data(), flags.data());
        for (int p = 0; p < nProblems; p++) {
            const Sim3Result& r = res[p];
            if (r.status < 0 || r.status >= kSsStatuses) { std::printf("FAILED: status %d\n", r.status); return 1; }
            const bool n1ok = pb[p].n1 >= 0 && pb[p].n1 <= cap;
            int flagged = 0;
            for (int i = 0; i < cap; i++) {
                const uint8_t f = flags[(size_t)p * cap + i];
                if (!n1ok || i >= pb[p].n1) { if (f != 0xEE) { std::printf("FAILED: a flag past n1 was written\n"); return 1; } continue; }
                if (f > 1) { std::printf("FAILED: flag %d\n", f); return 1; }
                flagged += f;
            }
            if (r.status == kSsConverged) {
                converged++;
                if (flagged != r.nInliers || r.nInliers <= minInliers) { std::printf("FAILED: %d flags, %d inliers\n", flagged, r.nInliers); return 1; }
            } else if (flagged) { std::printf("FAILED: flags without convergence\n"); return 1; }
            rows++;
        }
        std::printf("trial %d: status %d %d %d, N %d %d %d, its %d %d %d, best %d %d %d, scale %.3f\n", trial, res[0].status, res[1].status, res[2].status,
                    res[0].n, res[1].n, res[2].n, res[0].iterations, res[1].iterations, res[2].iterations, res[0].bestInliers, res[1].bestInliers,
                    res[2].bestInliers, res[0].scale);
    }
    if (converged == 0) { std::printf("FAILED: nothing converged at all\n"); return 1; }
    std::printf("sim3_solver_host_check: every access inside its arrays, %ld rows, %ld converged\n", rows, converged);
    return 0;
}
#endif
