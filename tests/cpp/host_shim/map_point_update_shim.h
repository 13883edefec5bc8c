// tests/cpp/host_shim/map_point_update_shim.h - what extractorb_amd/csrc/k_map_point_update.hpp needs for a host build: the vocabulary of
// triangulation_two_eyes_shim.h of this directory (whose ORBX_HOST_ROW tells the header that LDS is plain memory and brings in
// mpuPointSerial, the statement of one point in one thread).  tests/cpp/map_point_update_host_check.cpp runs the listed points one after
// the other.  Include it in front of the header.
#pragma once
#include "triangulation_two_eyes_shim.h"
