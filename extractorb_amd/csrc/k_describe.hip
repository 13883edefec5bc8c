// k_describe.hip — IC_Angle orientation, rotated BRIEF and final placement
// (reference ORBextractor.cc:75-145, 1137-1158).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "orbx_device.hpp"
#define ORBX_DESCRIBE_TU 1
#include "k_describe_body.hpp"

namespace orbx {

template <bool PB>
__global__ __launch_bounds__(256) void k_describe(const DescLevels dl,
                                                   const uint8_t* __restrict__ pyr, const uint8_t* __restrict__ blur,
                                                   const uint2* __restrict__ sel, int selPerFrame,
                                                   const int* __restrict__ levelCount, const int* __restrict__ levelLap,
                                                   Keypoint* __restrict__ outK, uint8_t* __restrict__ outD, int capacity,
                                                   int* __restrict__ nOut, int* __restrict__ monoOut,
                                                   Keypoint* __restrict__ outLevelK, int* __restrict__ outLevelCounts, int f0, int nFrames, int fewWaves,
                                                   int chunk0, int levelLo, int levelHi) {
    __shared__ __align__(16) uint8_t smem[DescLds<PB>::kSmem];
    __shared__ __align__(16) unsigned wtab[2][16][PB ? 12 : 8];   // [m10 weights | disc mask][|v|][dword of the aligned row]
    // Every argument the kernel reads is requested by its first instructions and waited for once: left to the compiler, the loads of the argument
    // block sink to their uses, each a trip to memory of its own in the middle of the wave's life (the pointers of the gathers and of the results, five
    // trips).  An empty statement that takes a value in a scalar register is where the value has to be there.
    int nlevels = dl.nlevels, so[kMaxLevels], gridX = (int)gridDim.x;
#pragma unroll
    for (int l = 0; l < kMaxLevels; l++) so[l] = dl.firstSlot[l];
    (void)gridX;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : : "s"(pyr), "s"(blur), "s"(sel), "s"(selPerFrame), "s"(levelCount), "s"(levelLap), "s"(outK), "s"(outD), "s"(capacity),
                 "s"(nOut), "s"(monoOut), "s"(outLevelK), "s"(outLevelCounts), "s"(f0), "s"(nFrames), "s"(chunk0), "s"(levelLo), "s"(levelHi), "s"(gridX));
    asm volatile("" : : "s"(nlevels), "s"(so[1]), "s"(so[2]), "s"(so[3]), "s"(so[4]), "s"(so[5]), "s"(so[6]), "s"(so[7]), "s"(so[8]), "s"(so[9]),
                 "s"(so[10]), "s"(so[11]), "s"(so[12]), "s"(so[13]), "s"(so[14]), "s"(so[15]));
#endif
    int chunk, fr;
    if (!xcdChunkFrame(nFrames, chunk, fr)) return;   // all keypoints of a frame on one XCD: overlapping patches share its L2
    describeBlock<PB>(dl, nlevels, so, pyr, blur, sel, selPerFrame, levelCount, levelLap, outK, outD, capacity, nOut, monoOut, outLevelK, outLevelCounts,
                      smem, wtab, fewWaves, chunk0 + chunk, f0 + fr, levelLo, levelHi);
}

// The keypoints of levels [levelLo, levelHi) of B frames: their selection slots are [slotLo, slotHi) (DescLevels::firstSlot).  One launch covers every
// level; two launches (levels below the split with the blur per keypoint, the rest from the blurred levels) cover a blur that is split by level
// (orbx_api.cpp) - a workgroup that straddles the boundary appears in both, and each of its waves runs in the launch its level belongs to.
void launchDescribe(hipStream_t st, const DescLevels& dl, const uint8_t* pyr, const uint8_t* blur,
                    const uint2* sel, int selPerFrame, const int* levelCount, const int* levelLap, Keypoint* outK,
                    uint8_t* outD, int capacity, int* nOut, int* monoOut, Keypoint* outLevelK, int* outLevelCounts,
                    bool patchBlur, int levelLo, int levelHi, int slotLo, int slotHi, int f0, int B, int sumsForm) {
    const int perBlock = 2 * kDescWaves, chunk0 = slotLo / perBlock, groups = (slotHi + perBlock - 1) / perBlock - chunk0;
    if (groups <= 0) return;
    // at most eight workgroups per CU in the whole launch: the latency form of the level sums (sumsForm >= 0: a test pins the form)
    const int fewWaves = sumsForm >= 0 ? sumsForm : (long long)groups * B <= 8 * 256;
    if (patchBlur)
        hipLaunchKernelGGL(k_describe<true>, xcdGrid(groups, B), dim3(256), 0, st, dl,
                           pyr, blur, sel, selPerFrame, levelCount, levelLap, outK, outD, capacity, nOut, monoOut, outLevelK,
                           outLevelCounts, f0, B, fewWaves, chunk0, levelLo, levelHi);
    else
        hipLaunchKernelGGL(k_describe<false>, xcdGrid(groups, B), dim3(256), 0, st, dl,
                           pyr, blur, sel, selPerFrame, levelCount, levelLap, outK, outD, capacity, nOut, monoOut, outLevelK,
                           outLevelCounts, f0, B, fewWaves, chunk0, levelLo, levelHi);
}
bool checkUmax(const int* umax16) {      // the static device table is the one the reference's constructor computes
    for (int i = 0; i < 16; i++) if (umax16[i] != kUmaxStatic[i]) return false;
    return true;
}
void describeTables(unsigned* pb384, unsigned* plain256) {      // the arrays the __constant__ weight words are initialised from
    memcpy(pb384, &kWeightsPb, sizeof(kWeightsPb));
    memcpy(plain256, &kWeightsPlain, sizeof(kWeightsPlain));
}


}  // namespace orbx
