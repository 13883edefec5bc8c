// k_wave_min.hpp - minima (and one sum) across lanes by DPP (no LDS round trip), for the kernels that share candidates among the lanes of a
// wave or of a 16-lane row.  Device only: kept apart from k_match_helpers.hpp, which the CPU suite compiles for the host.
#pragma once
#include <hip/hip_runtime.h>

namespace orbx {

template <int CTRL, int ROWMASK, class T>
__device__ __forceinline__ T dppMin(T v) { return min(v, (T)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROWMASK, 0xF, false)); }

// minimum over each row of 16 lanes, returned in every lane of the row
template <class T>
__device__ __forceinline__ T rowMin16(T v) {
    v = dppMin<0xB1, 0xF>(v);     // quad_perm [1,0,3,2]
    v = dppMin<0x4E, 0xF>(v);     // quad_perm [2,3,0,1]
    v = dppMin<0x141, 0xF>(v);    // row_half_mirror
    v = dppMin<0x140, 0xF>(v);    // row_mirror: every lane of a row holds the row's minimum
    return v;
}
// minimum over the 64 lanes, returned wave-uniform (int or unsigned)
template <class T>
__device__ __forceinline__ T waveMin(T v) {
    v = rowMin16(v);
    v = dppMin<0x142, 0xA>(v);    // row_bcast:15 into rows 1 and 3
    v = dppMin<0x143, 0xC>(v);    // row_bcast:31 into rows 2 and 3
    return (T)__builtin_amdgcn_readlane((int)v, 63);
}

// sum of an int over the 64 lanes, wave-uniform: the butterfly of rowMin16 leaves every lane of a row with the row's sum, four lane reads
// add the rows.  Every lane of the wave must be active
__device__ __forceinline__ int waveSum(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, false);
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48);
}

}  // namespace orbx
