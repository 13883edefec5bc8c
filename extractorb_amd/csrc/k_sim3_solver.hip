// k_sim3_solver.hip - Sim3Solver (reference src/Sim3Solver.cc) as LoopClosing runs it between SearchByBoW and SearchByProjection(pKF, Scw, ..)
// (src/LoopClosing.cc:595-760): a batch of independent problems, one per loop candidate.  Three kernels, every workgroup ONE WAVE of 64
// lanes; what they compute is k_sim3_solver.hpp's, which the CPU suite compiles for the host:
//   k_sim3_prepare     grid n_problems: zeroes the result row and the flags below n1, compacts the present slots by ballots in ascending i1,
//                      one lane per slot computes X3Dc1 / X3Dc2, their projections and the integer thresholds into the workspace
//                      (component-major: the next kernel's loads of 64 correspondences are coalesced), looks mRansacMaxIts up in its[N]
//                      and takes the exits TOO_FEW / BAD_ARGUMENT;
//   k_sim3_hypotheses  grid n_problems * max_iterations (blockIdx.x = problem * max_iterations + it); a wave beyond the problem's
//                      mRansacMaxIts leaves at once.  The three draws, Horn's closed form, the 4x4 Jacobi iteration, atan2 / sin / cos and
//                      Rodrigues are uniform over the wave: every lane computes them in registers - no LDS, no barrier, nothing to broadcast.
//                      Then one lane per correspondence runs CheckInliers 64 at a time, the count is a ballot, and ONE int per iteration goes
//                      to the workspace.  No per-iteration inlier mask is stored: the decision recomputes the winner's (do not
//                      write what you can re-derive);
//   k_sim3_decide      grid n_problems: the first count above min_inliers or else the last arg-max, that iteration's Sim3 again (the same
//                      function on the same draws: bit-identical), the flags of a converged problem scattered by mvnIndices1, the result row.
// No LDS in any of the three.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orbx_lds_pollute.hpp"
#include "k_sim3_solver.hpp"

namespace orbx {

__global__ __launch_bounds__(kSsLanes) void k_sim3_prepare(const Sim3Problem* __restrict__ problems, const float* __restrict__ x1w,
                                                           const float* __restrict__ x2w, const int* __restrict__ oct1,
                                                           const int* __restrict__ oct2, Sim3SolveParams q, SsWork w, Sim3Result* result,
                                                           uint8_t* flags) {
    ssPrepareProblem(threadIdx.x, blockIdx.x, problems, x1w, x2w, oct1, oct2, q, w, result, flags);
}

__global__ __launch_bounds__(kSsLanes) void k_sim3_hypotheses(const Sim3Problem* __restrict__ problems, const int* __restrict__ rnd,
                                                              Sim3SolveParams q, SsWork w) {
    ssHypothesisWave(threadIdx.x, blockIdx.x / q.maxIterations, blockIdx.x % q.maxIterations, problems, rnd, q, w);
}

__global__ __launch_bounds__(kSsLanes) void k_sim3_decide(const Sim3Problem* __restrict__ problems, const int* __restrict__ rnd, Sim3SolveParams q,
                                                          SsWork w, Sim3Result* result, uint8_t* flags) {
    ssDecideProblem(threadIdx.x, blockIdx.x, problems, rnd, q, w, result, flags);
}

void launchSim3Solve(hipStream_t st, const void* problems, const float* x1w, const float* x2w, const int* oct1, const int* oct2, const int* rnd,
                     const Sim3SolveParams& q, const SsWork& w, void* result, uint8_t* flags, int nProblems, int steps, LdsPolluter pollute) {
    const Sim3Problem* pb = (const Sim3Problem*)problems;
    // steps: bit 0 prepare, bit 1 hypotheses, bit 2 decide (orbx_debug_sim3_solve_steps; a call takes all three)
    if (steps & 1) { pollute(st); hipLaunchKernelGGL(k_sim3_prepare, dim3((unsigned)nProblems), dim3(kSsLanes), 0, st, pb, x1w, x2w, oct1, oct2, q, w, (Sim3Result*)result, flags); }
    if (steps & 2) { pollute(st); hipLaunchKernelGGL(k_sim3_hypotheses, dim3((unsigned)((long long)nProblems * q.maxIterations)), dim3(kSsLanes), 0, st, pb, rnd, q, w); }
    if (steps & 4) { pollute(st); hipLaunchKernelGGL(k_sim3_decide, dim3((unsigned)nProblems), dim3(kSsLanes), 0, st, pb, rnd, q, w, (Sim3Result*)result, flags); }
}

}  // namespace orbx
