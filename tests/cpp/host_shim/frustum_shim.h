// tests/cpp/host_shim/frustum_shim.h - what extractorb_amd/csrc/k_frustum_point.hpp needs for a host build beyond hip/hip_runtime.h of this
// directory (which stays as k_fuse.hip's): the double division of isInFrustum's viewCos.  With -ffp-contract=off the plain operator rounds
// as the intrinsic does.  Include it in front of the header (tests/cpp/frustum_host_check.cpp).
#pragma once
#include <hip/hip_runtime.h>
static inline double __ddiv_rn(double a, double b) { return a / b; }
