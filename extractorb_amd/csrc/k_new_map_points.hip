// k_new_map_points.hip - the triangulation loop of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:481-707) on the match lists
// the two triangulation searches leave in HBM (k_triangulate_match.hip, k_triangulate_match_two_eyes.hip): every matched pair becomes a
// world point or is rejected with the reference's `continue` named (orbx_new_point_exit).  One kernel template over the rig kind; the
// arithmetic of a match is k_new_map_points.hpp's, which the CPU suite compiles for the host.
//   k_new_map_points_init     d_n_new[p] = 0 (the atomics below need it);
//   k_new_map_points<TwoEyes> ONE LANE PER MATCH: matches do not contend, so the matches of a pair are tiled over workgroups of kNmpThreads = 64
//   lanes (one wave).  A match is ~6 k instructions for a two-camera pair (two unprojections, the 4x4 Jacobi, two KannalaBrandt8
//   projections) and a fraction of that for a Pinhole pair, a list holds some hundred matches: a small call is bound by one lane's latency,
//   and a wave per 64 matches puts the waves of a pair on different CUs.  Larger workgroups only add a barrier's wait.  n_matches lives on
//   the device: the grid covers the list capacity and a workgroup past the list's end leaves on its first compare.
//   STAGING: the pose records of the pair's two keyframes (2 keyframes x up to 2 eyes x kRigEyeFloats, k_rig_two_eyes.hpp) and the two
//   level tables go to LDS once per workgroup, one element per lane, behind one barrier; a lane then reads the records of its own eyes.
//   COUNT: d_n_new[p] += popcount(ballot(accepted)), one atomic per workgroup; the marks are atomic ORs (nmpMark).
//   The SVD is skipped wave-uniformly when no lane of the wave takes that branch (waveAny).
// Registers (gfx950, kernel_table.json): k_new_map_points<0> 178 VGPRs, k_new_map_points<1> 160, no scratch, no spill, with the library's
// common flags (no TRI2_FLAGS: the first build showed no scalar spill).  Two waves per SIMD would fit; a pair's grid offers a handful
// of waves to the whole device, so occupancy does not bound the call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orbx_lds_pollute.hpp"
#include "k_new_map_points.hpp"

namespace orbx {

// Diagnostics, OFF unless orbx_debug_new_map_points_enable(1) was called: a launch then zeroes the two counters and its workgroups add
// the matches that asked for the SVD and those that took an UnprojectStereo branch.  A production launch pays nothing for them.
__device__ int g_newMapPointsStats[2];
static bool g_newMapPointsStatsOn = false;
extern "C" int orbx_debug_new_map_points_enable(int on) { g_newMapPointsStatsOn = on != 0; return 0; }
extern "C" int orbx_debug_new_map_points_stats(int* out2) {
    if (!out2) return -2;                                  // ORBX_ERR_BAD_ARGUMENT
    if (hipDeviceSynchronize() != hipSuccess) return -6;   // (the handle's stream may be a non-blocking one: the copy below would not wait for it)
    return hipMemcpyFromSymbol(out2, HIP_SYMBOL(g_newMapPointsStats), sizeof(int) * 2) == hipSuccess ? 0 : -6;      // ORBX_ERR_HIP
}

// grid: ceil(n_pairs / 256)
__global__ __launch_bounds__(256) void k_new_map_points_init(int* __restrict__ nNew, int nPairs) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < nPairs) nNew[i] = 0;
}

// grid: n_pairs * p.tiles (blockIdx.x = pair * p.tiles + tile); kNmpThreads threads
template <bool TwoEyes>
__global__ __launch_bounds__(kNmpThreads) void k_new_map_points(const int* __restrict__ pairs, const int* __restrict__ nMatches,
                                                                const float* __restrict__ poses, const Keypoint* __restrict__ kps,
                                                                const Keypoint* __restrict__ raw, const float* __restrict__ uRight,
                                                                const float* __restrict__ depth, const int* __restrict__ nOut,
                                                                NewMapPointsParams p, uint8_t* __restrict__ exitOut, float* __restrict__ x3dOut,
                                                                int* __restrict__ nNew, uint8_t* mark1, uint8_t* mark2) {
    __shared__ float sRigMem[kNmpLdsFloats];
    ORBX_LDS float* sRig = (ORBX_LDS float*)sRigMem;
    const int tid = threadIdx.x, pair = blockIdx.x / p.tiles, tile = blockIdx.x - pair * p.tiles;
    const int n = max(0, min(nMatches[pair], p.listCapacity));                                  // (clamped into the list)
    if (tile * kNmpThreads >= n) return;                                                        // past the list's end: the whole workgroup leaves
    const long long X1 = p.kf1First + (long long)pair * p.kf1Step, X2 = p.kf2First + (long long)pair * p.kf2Step;
    nmpStage<TwoEyes>(tid, poses + X1 * 12, poses + X2 * 12, p, sRig);
    __syncthreads();
    const int k = tile * kNmpThreads + tid;
    bool svd = false, stereoBranch = false;
    const bool accepted = nmpLane<TwoEyes>(pair, k, k < n, sRig, pairs, kps, raw, uRight, depth, nOut, p, exitOut, x3dOut, mark1, mark2, svd, stereoBranch);
    const int count = __popcll(__ballot(accepted));
    if (tid == 0 && count) atomicAdd(&nNew[pair], count);
    if (p.countStats) {
        const int nSvd = __popcll(__ballot(svd)), nStereo = __popcll(__ballot(stereoBranch));
        if (tid == 0 && nSvd) atomicAdd(&g_newMapPointsStats[0], nSvd);
        if (tid == 0 && nStereo) atomicAdd(&g_newMapPointsStats[1], nStereo);
    }
}

int newMapPointsTiles(int listCapacity) { return (listCapacity + kNmpThreads - 1) / kNmpThreads; }

void launchNewMapPoints(hipStream_t st, bool twoEyes, const int* pairs, const int* nMatches, const float* poses, const Keypoint* kps,
                        const Keypoint* raw, const float* uRight, const float* depth, const int* nOut, const NewMapPointsParams& params,
                        uint8_t* exitOut, float* x3dOut, int* nNew, uint8_t* mark1, uint8_t* mark2, int nPairs, LdsPolluter pollute) {
    NewMapPointsParams p = params;
    p.tiles = newMapPointsTiles(p.listCapacity);
    p.countStats = g_newMapPointsStatsOn ? 1 : 0;
    void* stats = nullptr;
    if (p.countStats && hipGetSymbolAddress(&stats, HIP_SYMBOL(g_newMapPointsStats)) == hipSuccess) (void)hipMemsetAsync(stats, 0, sizeof(int) * 2, st);
    pollute(st);
    hipLaunchKernelGGL(k_new_map_points_init, dim3((unsigned)((nPairs + 255) / 256)), dim3(256), 0, st, nNew, nPairs);
    const dim3 grid((unsigned)(nPairs * p.tiles));
    pollute(st);
    if (twoEyes)
        hipLaunchKernelGGL(k_new_map_points<true>, grid, dim3(kNmpThreads), 0, st, pairs, nMatches, poses, kps, raw, uRight, depth, nOut, p, exitOut,
                           x3dOut, nNew, mark1, mark2);
    else
        hipLaunchKernelGGL(k_new_map_points<false>, grid, dim3(kNmpThreads), 0, st, pairs, nMatches, poses, kps, raw, uRight, depth, nOut, p, exitOut,
                           x3dOut, nNew, mark1, mark2);
}

}  // namespace orbx
