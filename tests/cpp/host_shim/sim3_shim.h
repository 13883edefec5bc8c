// tests/cpp/host_shim/sim3_shim.h - what extractorb_amd/csrc/k_project_sim3.hip and k_sim3_decide.hpp need for a host build beyond
// hip/hip_runtime.h of this directory (which stays as k_fuse.hip's): the __host__ word of the shared decision function.  Include it in
// front of the kernel source (tests/cpp/sim3_host_check.cpp).
#pragma once
#include <hip/hip_runtime.h>
#define __host__
