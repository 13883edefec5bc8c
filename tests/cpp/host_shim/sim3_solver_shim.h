// tests/cpp/host_shim/sim3_solver_shim.h - what extractorb_amd/csrc/k_sim3_solver.hpp needs for a host build: the vocabulary of
// two_view_shim.h of this directory (ORBX_HOST_ROW: a wave is ONE lane, kSsLanes = 1, ballots are the lane's own bit).
// tests/cpp/sim3_solver_host_check.cpp runs the three kernels' bodies problem by problem, iteration by iteration.  Include it in front of
// the header.
#pragma once
#include "two_view_shim.h"
