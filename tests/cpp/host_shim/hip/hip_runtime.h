// tests/cpp/host_shim/hip/hip_runtime.h - NOT the HIP runtime: host stand-ins for the device vocabulary of extractorb_amd/csrc/k_fuse.hip, so
// that the kernel's own source compiles with g++ and runs one "thread" at a time (tests/cpp/fuse_host_check.cpp; tests/test_fuse.py puts this
// directory in front of the include path).  With -ffp-contract=off the plain operators round as the __f*_rn / __d*_rn intrinsics do.  A wave
// is one lane here: __ballot sees only its own thread, so d_n_fused is NOT emulated (lane 0 of every wave adds its own bit).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#define __global__
#define __device__
#define __forceinline__ inline
#define __launch_bounds__(...)
#define __restrict__
struct uint4 { uint32_t x, y, z, w; };
struct dim3 { unsigned x, y, z; dim3(unsigned a = 1, unsigned b = 1, unsigned c = 1) : x(a), y(b), z(c) {} };
typedef void* hipStream_t;
static thread_local dim3 blockIdx, threadIdx;
using std::max;
using std::min;
static inline float __fmul_rn(float a, float b) { return a * b; }
static inline float __fadd_rn(float a, float b) { return a + b; }
static inline float __fsub_rn(float a, float b) { return a - b; }
static inline float __fdiv_rn(float a, float b) { return a / b; }
static inline double __dmul_rn(double a, double b) { return a * b; }
static inline double __dadd_rn(double a, double b) { return a + b; }
static inline double __dsqrt_rn(double a) { return std::sqrt(a); }
static inline int __popc(uint32_t v) { return __builtin_popcount(v); }
static inline int __popcll(unsigned long long v) { return __builtin_popcountll(v); }
static inline unsigned long long __ballot(bool c) { return c ? 1ull : 0ull; }
static inline int atomicAdd(int* p, int v) { const int o = *p; *p += v; return o; }
#define hipLaunchKernelGGL(...) ((void)0)
