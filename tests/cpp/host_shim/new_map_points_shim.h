// tests/cpp/host_shim/new_map_points_shim.h - what extractorb_amd/csrc/k_new_map_points.hpp needs for a host build: the vocabulary of
// triangulation_two_eyes_shim.h of this directory, whose ORBX_HOST_ROW also tells that header that LDS is plain memory, that a wave is ONE
// lane (waveAny is the lane's own bit: the SVD runs exactly for the matches that ask for it) and that a mark is a plain OR on its byte.
// tests/cpp/new_map_points_host_check.cpp runs a workgroup as every thread's nmpStage and then every lane's nmpLane, and states the count's
// ballot and atomic as a sum.  Include it in front of the header.
#pragma once
#include "triangulation_two_eyes_shim.h"
