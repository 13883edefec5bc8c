// k_wave_min.hpp - minima across lanes by DPP (no LDS round trip), for the kernels that share candidates among the lanes of a wave or of a
// 16-lane row.  Device only: kept apart from k_match_helpers.hpp, which the CPU suite compiles for the host.
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

}  // namespace orbx
