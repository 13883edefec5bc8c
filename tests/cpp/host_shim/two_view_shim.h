// tests/cpp/host_shim/two_view_shim.h - what extractorb_amd/csrc/k_two_view.hpp needs for a host build: the vocabulary of
// new_map_points_shim.h of this directory.  Its ORBX_HOST_ROW tells that header that LDS is plain memory and that a wave is ONE lane
// (kTvLanes = 1): ballots are the lane's own bit, the score chain adds one match at a time, lane 0 is every lane.
// tests/cpp/two_view_host_check.cpp runs the three kernels' bodies pair by pair, hypothesis by hypothesis.  Include it in front of the header.
#pragma once
#include "new_map_points_shim.h"
