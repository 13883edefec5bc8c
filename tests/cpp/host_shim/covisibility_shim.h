// tests/cpp/host_shim/covisibility_shim.h - what extractorb_amd/csrc/k_covisibility.hpp needs for a host build: the vocabulary of
// place_recognition_shim.h of this directory, whose ORBX_HOST_ROW makes a workgroup ONE lane: an ordered count is the lane's own flag, barriers
// are nothing, atomics are plain, LDS is plain memory.  tests/cpp/covisibility_host_check.cpp runs cvRank frame by frame and cvVote /
// rdKeyFrame subject by subject.  Include it in front of the header.
#pragma once
#include "place_recognition_shim.h"
