// k_covisibility.hip - KeyFrame::UpdateConnections (reference src/KeyFrame.cc:388-511), the vote of Tracking::UpdateLocalKeyFrames
// (src/Tracking.cc:3030-3102) and the redundancy test of LocalMapping::KeyFrameCulling (src/LocalMapping.cc:977-1043) for a batch of
// subjects: THREE kernels.  What they compute is k_covisibility.hpp's, which the CPU suite compiles for the host.
//   k_covis_rank            a wave per frame, four to a workgroup: the rank of the frame's key among all keys - 64 keys per step, the smaller
//                           ones counted by ballot -, the inverse table, and one word per workgroup "two keys are equal".  (A lane per frame
//                           walking all keys took 120 us of a 150 us call at 2048 frames: profiles/r34_covisibility.md);
//   k_covis_vote            one workgroup of 256 lanes per subject runs cvVote: a lane per slot walks the MapPoint's observations and adds
//                           to the observer's counter in LDS (integer adds: the schedule does not matter), the counters - indexed by key
//                           rank - are compacted in order into the counter block, nmax is an LDS maximum and a minimum over its holders, the
//                           counts >= th are sorted as weight << 32 | rank by a bitonic sort in LDS.  8 bytes per list slot (a power of
//                           two of slots) and 4 per frame of LDS;
//   k_keyframe_redundancy   one workgroup per subject runs rdKeyFrame: a lane per slot, the slot states held in a byte of LDS each until
//                           every index has been checked.
// No launch depends on the data.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orbx_lds_pollute.hpp"
#include "k_covisibility.hpp"

namespace orbx {

__global__ __launch_bounds__(64 * kCvRankBlock) void k_covis_rank(CovisArrays a, CovisParams p) {
    const int lane = threadIdx.x & 63, f = blockIdx.x * kCvRankBlock + (threadIdx.x >> 6);
    bool dup = false;
    if (f < p.nFrames) {                                          // (the same for every lane of a wave)
        const int rank = cvRank(lane, f, a.kfKey, p.nFrames, dup);
        if (lane == 0) { a.wsRank[f] = rank; a.wsByRank[rank] = f; }
    }
    const int any = __syncthreads_or(dup ? 1 : 0);
    if (threadIdx.x == 0) a.wsDup[blockIdx.x] = any;
}

__global__ __launch_bounds__(kCvThreads) void k_covis_vote(CovisArrays a, CovisParams p) {
    ORBX_DYNAMIC_LDS(lds);
    cvVote(threadIdx.x, blockIdx.x, a, p, lds);
}

__global__ __launch_bounds__(kCvThreads) void k_keyframe_redundancy(CovisArrays a, CovisParams p) {
    ORBX_DYNAMIC_LDS(lds);
    rdKeyFrame(threadIdx.x, blockIdx.x, a, p, lds);
}

void launchCovisibility(hipStream_t st, const CovisArrays& a, const CovisParams& p, LdsPolluter pollute) {
    pollute(st);
    hipLaunchKernelGGL(k_covis_rank, dim3((unsigned)cvRankBlocks(p.nFrames)), dim3(64 * kCvRankBlock), 0, st, a, p);
    pollute(st);
    hipLaunchKernelGGL(k_covis_vote, dim3((unsigned)p.nSubjects), dim3(kCvThreads), cvVoteLdsBytes(p.nFrames), st, a, p);
}

void launchKeyFrameRedundancy(hipStream_t st, const CovisArrays& a, const CovisParams& p, LdsPolluter pollute) {
    pollute(st);
    hipLaunchKernelGGL(k_keyframe_redundancy, dim3((unsigned)p.nSubjects), dim3(kCvThreads), rdLdsBytes(p.capacity), st, a, p);
}

}  // namespace orbx
