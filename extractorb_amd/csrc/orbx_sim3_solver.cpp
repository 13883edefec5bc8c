// orbx_sim3_solver.cpp - the C ABI of the loop-closing RANSAC alignment (include/orbx.h): Sim3Solver's constructor, SetRansacParameters and
// the iterate loop (reference src/Sim3Solver.cc, call site src/LoopClosing.cc:673-684) on a batch of problems (k_sim3_solver.hip).  Thin, as
// orbx_two_view.cpp is: argument checks, the workspace through growDevice, the table its[N] of SetRansacParameters filled with the host's
// libm (orbx_entry.hpp: sim3RansacIterations) and uploaded when (probability, min_inliers) or the workspace change, one launch wrapper.
// A file of its own for the reason orbx_two_view.cpp gives; the rejections of the entry here are held by tests/test_sim3_solver_gpu.py.
// No CPU path.
#include "orbx_internal.hpp"

static int g_sim3SolveSteps = 7;

extern "C" {

// which of the three kernels the next calls launch (process-wide; tools/sim3_solver_rate.py times the steps by difference): bit 0 prepare,
// bit 1 hypotheses, bit 2 decide.  Anything but 7 leaves the result rows unfinished.
int orbx_debug_sim3_solve_steps(int mask) {
    if (mask != 1 && mask != 3 && mask != 7) return ORBX_ERR_BAD_ARGUMENT;
    g_sim3SolveSteps = mask;
    return ORBX_OK;
}

int orbx_sim3_solve_device(orbx_handle* h, int n_problems, const orbx_sim3_problem* d_problems, int capacity, const float* d_x1w,
                           const float* d_x2w, const int* d_octave1, const int* d_octave2, double probability, int min_inliers,
                           int max_iterations, const int* d_rand, orbx_sim3_result* d_result, uint8_t* d_inliers) {
    static_assert(sizeof(orbx_sim3_result) == 144 && sizeof(orbx_sim3_problem) == 240, "orbx_sim3_result / orbx_sim3_problem layout");
    if (!h) return ORBX_ERR_BAD_ARGUMENT;
    // written so that a NaN probability is refused
    if (!d_problems || !d_x1w || !d_x2w || !d_octave1 || !d_octave2 || !d_rand || !d_result || !d_inliers || capacity < 1 || n_problems < 1 ||
        max_iterations < 1 || max_iterations > kSsMaxIterations || !(probability >= 0.0 && probability <= 1.0) ||
        (long long)n_problems * max_iterations > 0x7fffffffLL)
        return fail(h, ORBX_ERR_BAD_ARGUMENT, "null pointer, capacity/n_problems < 1, max_iterations outside 1 .. 4096, probability outside [0, 1] or "
                                              "more than 2^31 - 1 workgroups");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t probs = (size_t)n_problems, cap = (size_t)capacity, iters = (size_t)max_iterations;
    SsWork& w = h->sim3SolveWork;
    if (probs > h->sim3Solve.problems || cap > h->sim3Solve.cap || iters > h->sim3Solve.iters) {
        const orbx_handle::Sim3SolveShape want{std::max(probs, h->sim3Solve.problems), std::max(cap, h->sim3Solve.cap), std::max(iters, h->sim3Solve.iters)};
        const size_t entries = want.problems * want.cap;
        h->sim3Its.clear();
        if (int rc = growDevice(h, h->sim3Solve, want,
                                {{(void**)&w.prep, want.problems * sizeof(SsPrep)}, {(void**)&w.idx1, entries * sizeof(int)},
                                 {(void**)&w.pts, entries * kSsPointFloats * sizeof(float)}, {(void**)&w.counts, want.problems * want.iters * sizeof(int)},
                                 {(void**)&w.its, (want.cap + 1) * sizeof(int)}}))
            return rc;
    }
    // its[N] for N = 0 .. the workspace's capacity: this call reads N <= capacity of it
    if (h->sim3Its.size() != h->sim3Solve.cap + 1 || h->sim3ItsProb != probability || h->sim3ItsMin != min_inliers) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));      // an earlier call may still read the table, and the copy below reads sim3Its
        h->sim3Its.resize(h->sim3Solve.cap + 1);
        for (size_t n = 0; n < h->sim3Its.size(); n++) h->sim3Its[n] = sim3RansacIterations(probability, min_inliers, (int)n);
        h->sim3ItsProb = probability; h->sim3ItsMin = min_inliers;
        HIP_TRY(h, hipMemcpyAsync(w.its, h->sim3Its.data(), h->sim3Its.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    const Sim3SolveParams p{capacity, max_iterations, min_inliers, h->nlevels};
    {
        Prof pr(h, S_FRAME);
        launchSim3Solve(h->stream, d_problems, d_x1w, d_x2w, d_octave1, d_octave2, d_rand, p, w, d_result, d_inliers, n_problems, g_sim3SolveSteps, ldsPolluter(h));
    }
    return finishLaunch(h);
}

}  // extern "C"
