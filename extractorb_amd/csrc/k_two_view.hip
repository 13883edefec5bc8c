// k_two_view.hip - TwoViewReconstruction::Reconstruct (reference src/TwoViewReconstruction.cc:39-125) on the match tables
// orbx_search_for_initialization_device leaves in HBM.  Three kernels, every workgroup ONE WAVE of 64 lanes; what they compute is
// k_two_view.hpp's, which the CPU suite compiles for the host:
//   k_two_view_prepare     grid n_pairs: zeroes the pair's outputs, compacts vnMatches12 by ballots, takes the exits that need no arithmetic,
//                          runs Normalize's four sum chains over ALL keypoints of both frames on lanes 0 .. 3 (one chain each) and leaves
//                          T1, T2, T2inv, T2t in the workspace;
//   k_two_view_hypotheses<Spread>  grid n_pairs * 2 * iterations (blockIdx.x = (pair * 2 + model) * iterations + it).  Two forms of the
//                          SAME definition, bit for bit (tests/test_two_view_gpu.py runs both against the walk):
//                          <true>, the default: every lane draws the set (uniform), lane k holds row k of the 16x9 / 8x9 system, of its
//                          copy and of V in registers; a dot product over the rows is one chain of v_readlane + v_add over the lanes in row
//                          order (laneChain: the left-to-right sum), the angle is uniform, each lane rotates its own row
//                          (nullVector9Wave); every lane denormalises - no LDS, no barrier, 120 VGPRs;
//                          <false>, the first form built: lane 0 alone builds A in LDS and takes its null vector there (nullVector9),
//                          63 lanes wait at the barrier; 223 VGPRs.
//                          Then, in both, the 64 lanes compute the two score terms of 64 matches at a time and ONE chain of v_readlane +
//                          v_add adds them in match order (tvChainAdd): the reference's left-to-right binary32 sum.  Score and matrix go
//                          to the workspace;
//   k_two_view_decide      grid n_pairs: the first strictly greatest score of each model, RH, the branch; lane 0 decomposes (svd3) into 8 or
//                          4 motions in LDS; CheckRT of each motion one lane per match (nullVector4, skipped by a wave without an inlier),
//                          the count by ballots, the k-th smallest cosine by rank counting; the decision; then the chosen motion's points,
//                          flags and the pruning of the match table.
// Shapes compared (profiles/r23_two_view.md; 1000 keypoints, 300 matches, 200 iterations): the hypothesis kernel with the rows over the
// lanes against one lane out of LDS - 0.67 against 0.93 ms for one pair, 9.9 against 17.8 ms for 256; the faster is the default
// (orbx_debug_two_view_shape selects).  prepare and decide exist in one form: one wave per pair.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orbx_lds_pollute.hpp"
#include "k_two_view.hpp"

namespace orbx {

__global__ __launch_bounds__(kTvLanes) void k_two_view_prepare(const Keypoint* __restrict__ kps, const int* __restrict__ nOut,
                                                               const int* matches12, TwoViewParams q, TvWork w, TwoViewResult* result,
                                                               float* p3d, uint8_t* tri) {
    tvPreparePair(threadIdx.x, blockIdx.x, kps, nOut, matches12, q, w, result, p3d, tri);
}

// Spread = false: lane 0 takes the null vector out of LDS (the first shape built); true: the rows of A over the lanes, no LDS
template <bool Spread>
__global__ __launch_bounds__(kTvLanes) void k_two_view_hypotheses(const Keypoint* __restrict__ kps, const int* __restrict__ rnd, TwoViewParams q,
                                                                  TvWork w) {
    __shared__ float sMemRaw[Spread ? 1 : kTvHypLdsFloats];
    const int it = blockIdx.x % q.iterations, pm = blockIdx.x / q.iterations;
    tvHypothesisWave<Spread>(threadIdx.x, pm >> 1, pm & 1, it, kps, rnd, q, w, (ORBX_LDS float*)sMemRaw);
}

// Which hypothesis kernel a launch takes (process-wide): 1 = the rows over the lanes (the default: profiles/r23_two_view.md), 0 = one lane
// out of LDS.  Both are the same definition bit for bit (tests/test_two_view_gpu.py runs both against the walk).
static int g_twoViewShape = 1;
extern "C" int orbx_debug_two_view_shape(int shape) {
    if (shape != 0 && shape != 1) return -2;               // ORBX_ERR_BAD_ARGUMENT
    g_twoViewShape = shape;
    return 0;
}

__global__ __launch_bounds__(kTvLanes) void k_two_view_decide(const Keypoint* __restrict__ kps, int* matches12, int* nMatches, TwoViewParams q,
                                                              TvWork w, TwoViewResult* result, float* p3d, uint8_t* tri) {
    __shared__ float sMemRaw[kTvDecideLdsFloats];
    tvDecidePair(threadIdx.x, blockIdx.x, kps, matches12, nMatches, q, w, result, p3d, tri, (ORBX_LDS float*)sMemRaw);
}

void launchTwoView(hipStream_t st, const Keypoint* kps, const int* nOut, int* matches12, int* nMatches, const int* rnd, const TwoViewParams& q,
                   const TvWork& w, void* result, float* p3d, uint8_t* tri, int nPairs, LdsPolluter pollute) {
    pollute(st);
    hipLaunchKernelGGL(k_two_view_prepare, dim3((unsigned)nPairs), dim3(kTvLanes), 0, st, kps, nOut, matches12, q, w, (TwoViewResult*)result, p3d, tri);
    const dim3 hyps((unsigned)((long long)nPairs * 2 * q.iterations));
    pollute(st);
    if (g_twoViewShape) hipLaunchKernelGGL(k_two_view_hypotheses<true>, hyps, dim3(kTvLanes), 0, st, kps, rnd, q, w);
    else hipLaunchKernelGGL(k_two_view_hypotheses<false>, hyps, dim3(kTvLanes), 0, st, kps, rnd, q, w);
    pollute(st);
    hipLaunchKernelGGL(k_two_view_decide, dim3((unsigned)nPairs), dim3(kTvLanes), 0, st, kps, matches12, nMatches, q, w, (TwoViewResult*)result, p3d, tri);
}

}  // namespace orbx
