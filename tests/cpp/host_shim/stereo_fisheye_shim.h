// tests/cpp/host_shim/stereo_fisheye_shim.h - what extractorb_amd/csrc/k_stereo_fisheye.hip needs for a host build: the vocabulary of
// triangulation_two_eyes_shim.h of this directory, whose ORBX_HOST_ROW also tells this kernel file that LDS is plain memory and to leave
// out the kernel wrappers (barriers inside the chunk loop, ballots, the atomics).  tests/cpp/stereo_fisheye_host_check.cpp runs a workgroup
// as every row's sfScanChunk over chunks of the kernel's size, sfRatioPass and sfGeometry, and states the two atomics as a maximum and two
// sums.  Include it in front of the kernel file.
#pragma once
#include "triangulation_two_eyes_shim.h"
