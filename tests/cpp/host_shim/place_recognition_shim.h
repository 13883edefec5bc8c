// tests/cpp/host_shim/place_recognition_shim.h - what extractorb_amd/csrc/k_place_recognition.hpp needs for a host build: the vocabulary of
// pose_optimization_shim.h of this directory.  Its ORBX_HOST_ROW tells that header that a wave and a workgroup are ONE lane: a ballot is the
// lane's own bit, a cross-lane read is the lane's own value, barriers are nothing, atomics are plain, LDS is plain memory.
// tests/cpp/place_recognition_host_check.cpp runs prPair pair by pair and prQuery query by query.  Include it in front of the header.
#pragma once
#include "pose_optimization_shim.h"
