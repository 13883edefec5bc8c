// k_lds_vec.hpp - the 128-bit word the two-camera kernels read descriptors with, and the address space of their LDS tables: on the device a
// compiler vector that can live behind address_space(3) (a table typed so is read with DS instructions, never FLAT), in the host builds of
// the CPU suite (ORBX_HOST_ROW, tests/cpp/host_shim) HIP's uint4 in plain memory.  Shared by k_triangulate_match_two_eyes.hip and
// k_stereo_fisheye.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#if defined(ORBX_HOST_ROW) || !defined(__HIPCC__)
#define ORBX_LDS
namespace orbx { typedef uint4 LdsU4; }
#else
#define ORBX_LDS __attribute__((address_space(3)))
namespace orbx { typedef uint32_t LdsU4 __attribute__((ext_vector_type(4))); }
#endif
