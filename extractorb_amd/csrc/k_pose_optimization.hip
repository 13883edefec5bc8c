// k_pose_optimization.hip - Optimizer::PoseOptimization (reference src/Optimizer.cc:854-1168) for a batch of frames: ONE kernel, one
// workgroup of kPoSlots = 256 lanes (four waves) per problem, resident through all four rounds - no launch per round, per LM iteration or per
// trial (an LM step is about a microsecond of arithmetic, a launch more).  What it computes is k_pose_optimization.hpp's, which the CPU suite
// compiles for the host.
//   lanes     an edge per lane and pass (edge k on lane k % 256); a pass reads the edge again from the arrays the searches wrote (28 + 4 + 12
//             + 4 bytes: L2 hits after the first pass) - nothing is staged, so the capacity has no bound;
//   sums      a lane's slot in registers, five cross-lane exchanges per value inside the wave, then one double per value and wave through
//             LDS: kPoLdsBytes = 4 * 28 * 8 = 896 bytes, two barriers per pass;
//   uniform   the pose, lambda, the 6x6 Cholesky, exp and the quaternion product are computed by every lane from the same reduced sums:
//             nothing is broadcast and no lane waits for another between two passes;
//   flags     d_outlier is the level flag of an edge between the rounds: written and read by the edge's own lane.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orbx_lds_pollute.hpp"
#include "k_pose_optimization.hpp"

namespace orbx {

static_assert(sizeof(PoseResult) == 120 && sizeof(PoseProblem) == 188, "orbx_pose_result / orbx_pose_problem layout");

__global__ __launch_bounds__(kPoSlots) void k_pose_optimization(const PoseProblem* __restrict__ problems, const Keypoint* __restrict__ kps,
                                                                 const int* __restrict__ nOut, const float* __restrict__ uRight,
                                                                 const int* __restrict__ matches, const float* __restrict__ world, PoseOptParams q,
                                                                 float* poses, uint8_t* outlier, PoseResult* result) {
    __shared__ double lds[kPoLdsBytes / 8];
    const int p = blockIdx.x;
    const long long frame = q.frameFirst + (long long)p * q.frameStep;
    PoArgs a;
    a.cap = q.capacity; a.eyes = q.eyes; a.nMapPoints = q.nMapPoints; a.nlevels = q.nlevels; a.world = world;
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const long long f = frame * q.eyes + (e < q.eyes ? e : 0), row = (long long)p * q.eyes + (e < q.eyes ? e : 0);
        a.kps[e] = kps + f * q.capacity;
        a.matches[e] = matches + row * q.capacity;
        a.flags[e] = outlier + row * q.capacity;
        a.n[e] = nOut[f];
    }
    a.uRight = uRight ? uRight + frame * q.capacity : nullptr;
    poSolveProblem(threadIdx.x, problems[p], a, poses + frame * 12, result + p, lds);
}

void launchPoseOptimization(hipStream_t st, const void* problems, const Keypoint* kps, const int* nOut, const float* uRight, const int* matches,
                            const float* world, const PoseOptParams& q, float* poses, uint8_t* outlier, void* result, int nProblems, LdsPolluter pollute) {
    pollute(st);
    hipLaunchKernelGGL(k_pose_optimization, dim3((unsigned)nProblems), dim3(kPoSlots), 0, st, (const PoseProblem*)problems, kps, nOut, uRight, matches,
                       world, q, poses, outlier, (PoseResult*)result);
}

}  // namespace orbx
