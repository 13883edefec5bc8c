// tests/cpp/host_shim/pose_optimization_shim.h - what extractorb_amd/csrc/k_pose_optimization.hpp needs for a host build: the vocabulary of
// sim3_solver_shim.h of this directory.  Its ORBX_HOST_ROW tells that header that the 256 sum slots of a workgroup run one after the other and
// that the tree over them is a loop (poSum): "lane 0" is every lane.  tests/cpp/pose_optimization_host_check.cpp runs the kernel's body
// problem by problem.  Include it in front of the header.
#pragma once
#include "sim3_solver_shim.h"
