// tests/cpp/host_shim/fuse_two_eyes_shim.h - what extractorb_amd/csrc/k_fuse_two_eyes.hip needs for a host build beyond hip/hip_runtime.h,
// frustum_shim.h and kb8_shim.h of this directory: the words of its kernel wrapper.  The wrapper itself (stage, barrier, lane) is compiled but
// not run on the host: tests/cpp/fuse_two_eyes_host_check.cpp runs a workgroup as every thread's fuseTwoEyesStage, then every thread's
// fuseTwoEyesLane, one thread at a time, over arrays of its own.  Include it in front of the kernel file.
#pragma once
#include "kb8_shim.h"
#define __shared__ static
static inline void __syncthreads() {}
