// tests/cpp/host_shim/kb8_shim.h - what extractorb_amd/csrc/k_camera_kb8.hpp and k_project_last_two_eyes_point.hpp need for a host build
// beyond hip/hip_runtime.h and frustum_shim.h of this directory: the bit casts and the double subtraction.  With -ffp-contract=off
// the plain operators round as the intrinsics do.  Include it in front of the headers.
#pragma once
#include "frustum_shim.h"
static inline uint32_t __float_as_uint(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }
static inline float __uint_as_float(uint32_t u) { float f; std::memcpy(&f, &u, 4); return f; }
static inline double __dsub_rn(double a, double b) { return a - b; }
