// tests/cpp/host_shim/triangulation_two_eyes_shim.h - what extractorb_amd/csrc/k_triangulate_match_two_eyes.hip needs for a host build beyond
// fuse_two_eyes_shim.h of this directory.  ORBX_HOST_ROW tells the kernel file that a row is ONE lane here (rowMin16 is the identity, the lane
// walks every candidate of its row: the geometry is then evaluated strictly in increasing key order until one passes), that LDS is plain
// memory, and to leave out the kernel wrappers (dynamic LDS, ballots, barriers inside loops): tests/cpp/
// triangulation_two_eyes_host_check.cpp runs a workgroup as every thread's stage and slots, every entry's segments, every entry's row, and
// closes the search with a scan of its own.  Include it in front of the kernel file.
#pragma once
#include "fuse_two_eyes_shim.h"
#define ORBX_HOST_ROW 1
namespace orbx {
template <class T> static inline T rowMin16(T v) { return v; }
}  // namespace orbx
