// k_fast_body.hpp - the FAST cell's arithmetic and the one-cell-per-wave body as device functions: k_fast.hip launches it as a kernel of its
// own (and has the workgroup-per-cell form of single frames).  See k_fast.hip for the
// algorithm.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orbx_device.hpp"
#include "k_blur_body.hpp"

namespace orbx {


// Two pixels per register: u16 halves holding 0..255.  As IEEE binary16 bit patterns those are non-negative
// denormals, whose order is the integer order, and minimum/maximum return one operand unchanged (the kernel runs
// with FP16 denormals preserved, the HIP default), so the packed 3-input f16 ops ARE integer min3/max3 on both halves.
__device__ __forceinline__ unsigned pkmin3(unsigned a, unsigned b, unsigned c) {
    unsigned r;
    asm("v_pk_minimum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ unsigned pkmax3(unsigned a, unsigned b, unsigned c) {
    unsigned r;
    asm("v_pk_maximum3_f16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ unsigned pksub(unsigned a, unsigned b) {
    unsigned r;
    asm("v_pk_sub_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ unsigned pkmax(unsigned a, unsigned b) {
    unsigned r;
    asm("v_pk_max_u16 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
// bytes O, O+1 of the 12-byte string L|C|R (three consecutive dwords of a tile row), zero-extended to two u16
template <int O>
__device__ __forceinline__ unsigned pairAt(unsigned L, unsigned C, unsigned R) {
    static_assert(O >= 0 && O <= 10, "pair outside the three dwords");
    if constexpr (O <= 6) return __builtin_amdgcn_perm(C, L, 0x0C000C00u | O | ((O + 1) << 16));
    else return __builtin_amdgcn_perm(R, C, 0x0C000C00u | (O - 4) | ((O - 3) << 16));
}

// The two pair masks of a byte mask (0xFF per kept pixel of a tile dword): bytes 0, 1 and bytes 2, 3 of m, each widened to its u16 half
__device__ __forceinline__ unsigned pairMaskLo(unsigned m) { return __builtin_amdgcn_perm(0u, m, 0x01010000u); }
__device__ __forceinline__ unsigned pairMaskHi(unsigned m) { return __builtin_amdgcn_perm(0u, m, 0x03030202u); }

// ---- the score tile.  Two forms, chosen per tile shape at compile time (kFastPairTile):
//   byte form: one byte per pixel on the pixel tile's dword grid (row stride TS, an item = one dword);
//   pair form: one u16 per pixel, i.e. the score pass's two result registers sA | sB stored as they are (row stride 2 * TS, an item = 8 bytes).
// Row 0 and rows ch + 1, ch + 2 and the dword left / right of every row's items stand for "outside the cell interior" and hold 0.
template <bool PAIR, int TS> struct ScoreTile {
    static constexpr int kStride = PAIR ? 2 * TS : TS;      // bytes per score row
    static constexpr int kItem = PAIR ? 8 : 4;              // bytes of one item (four pixels) in a score row
};
// 48-byte rows take the pair form: k_fast<48,45> with the score rows laid over the pixel tile (orbx_device.hpp: FastAlias; 17 232 B per
// workgroup as before), k_fast_wide<48,45> with a tile of its own (6.3 KB per workgroup instead of 4.3).  The 72-byte tile (cells up to 63 px)
// keeps the byte form: its workgroup holds 39 KB already (four per CU); a pair tile of its own would make it 58 KB (two per CU).
#ifndef ORBX_FAST_PAIR_TILE
#define ORBX_FAST_PAIR_TILE 1   // 0 (A/B builds): the byte form for every tile
#endif
template <int TS> constexpr bool kFastPairTile = ORBX_FAST_PAIR_TILE && TS <= 48;

// The neighbour maximum of the NMS pass, the one statement of it for every kernel and both tile forms.  base: the item in the score row ABOVE
// the centre row.  Out: sA, sB = the item's four scores as two u16 pairs, mA, mB = per pixel the maximum of its eight neighbours and minThFAST
// (thPair), so "strict local maximum above minThFAST" is S > m.
// Pair form: per row the four dwords P | A | B | N (previous pair, the item's two, next pair: one 4-, one 8- and one 4-byte read);
// V[k] = max(up, down, th) per dword, the three pairs shifted by one pixel (x-1,x) (x+1,x+2) (x+3,x+4) of V and of the centre row by
// v_alignbyte - the middle one serves both centres - and two 3-input maxima per centre pair: 4 + 6 + 4 instructions.
// Byte form: nine dwords, the 3 x 5 pairs cut out with v_perm (15), nine maxima.
template <bool PAIR, int TS>
__device__ __forceinline__ void nmsNeighbourMax(const uint8_t* base, const unsigned thPair, unsigned& sA, unsigned& sB, unsigned& mA, unsigned& mB) {
    constexpr int RS = ScoreTile<PAIR, TS>::kStride;
    if constexpr (PAIR) {
        unsigned R[3][4];
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const uint2 ab = *(const uint2*)(base + r * RS);
            R[r][0] = *(const unsigned*)(base + r * RS - 4);
            R[r][1] = ab.x; R[r][2] = ab.y;
            R[r][3] = *(const unsigned*)(base + r * RS + 8);
        }
        unsigned V[4];
#pragma unroll
        for (int k = 0; k < 4; k++) V[k] = pkmax3(R[0][k], R[2][k], thPair);
        const unsigned Vl = __builtin_amdgcn_alignbyte(V[1], V[0], 2), Vm = __builtin_amdgcn_alignbyte(V[2], V[1], 2), Vr = __builtin_amdgcn_alignbyte(V[3], V[2], 2);
        const unsigned Ml = __builtin_amdgcn_alignbyte(R[1][1], R[1][0], 2), Mm = __builtin_amdgcn_alignbyte(R[1][2], R[1][1], 2), Mr = __builtin_amdgcn_alignbyte(R[1][3], R[1][2], 2);
        sA = R[1][1]; sB = R[1][2];
        mA = pkmax3(pkmax3(V[1], Vl, Vm), Ml, Mm);
        mB = pkmax3(pkmax3(V[2], Vm, Vr), Mm, Mr);
    } else {
        unsigned U[3], M[3], D[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            U[k] = *(const unsigned*)(base + 4 * k - 4);
            M[k] = *(const unsigned*)(base + RS + 4 * k - 4);
            D[k] = *(const unsigned*)(base + 2 * RS + 4 * k - 4);
        }
        // pairs a..e = bytes (3,4) (4,5) (5,6) (6,7) (7,8) of L|C|R; up/down maxima per pair column, threshold folded in
        const unsigned Wa = pkmax3(pairAt<3>(U[0], U[1], U[2]), pairAt<3>(D[0], D[1], D[2]), thPair);
        const unsigned Wb = pkmax3(pairAt<4>(U[0], U[1], U[2]), pairAt<4>(D[0], D[1], D[2]), thPair);
        const unsigned Wc = pkmax3(pairAt<5>(U[0], U[1], U[2]), pairAt<5>(D[0], D[1], D[2]), thPair);
        const unsigned Wd = pkmax3(pairAt<6>(U[0], U[1], U[2]), pairAt<6>(D[0], D[1], D[2]), thPair);
        const unsigned We = pkmax3(pairAt<7>(U[0], U[1], U[2]), pairAt<7>(D[0], D[1], D[2]), thPair);
        const unsigned Ma = pairAt<3>(M[0], M[1], M[2]), Mc = pairAt<5>(M[0], M[1], M[2]), Me = pairAt<7>(M[0], M[1], M[2]);
        sA = pairAt<4>(M[0], M[1], M[2]); sB = pairAt<6>(M[0], M[1], M[2]);
        mA = pkmax3(pkmax3(Wa, Wb, Wc), Ma, Mc); mB = pkmax3(pkmax3(Wc, Wd, We), Mc, Me);
    }
}
// The score pass's store of one item: sA, sB = the four scores as two u16 pairs, m = the item's byte mask (0xFF per pixel inside the interior)
// in the byte form, (mLo, mHi) = its pair masks in the pair form.
template <bool PAIR>
__device__ __forceinline__ void storeScores(uint8_t* dst, unsigned sA, unsigned sB, unsigned mLo, unsigned mHi) {
    if constexpr (PAIR) *(uint2*)dst = uint2{sA & mLo, sB & mHi};
    else *(unsigned*)dst = __builtin_amdgcn_perm(sB, sA, 0x06040200u) & mLo;
}
// Zero what the NMS pass reads as "outside the interior" and the score pass does not write (it writes every item of rows 1 .. ch, masked):
// row 0, the BELOW rows under the interior (whole rows, 8-byte stores), and the dword left of item q0 and right of item q1 of rows 1 .. ch
// (thread t: row t + 1).  t: the thread's index among the >= 64 that call it (3 * kStride / 8 <= 64, ch <= 63).
// TRIM (pair form, called BEHIND a score pass that stored every item whole): also the pixels past the interior in the last item of every row,
// validLast .. 3 of item q1 - then the score pass carries no masks at all (two registers and two v_and per trip).  The registers matter: with
// the two pair masks k_fast<48,45> needed 58 VGPRs, allocated as 64, and the step was 0.4 % SLOWER than with the byte tile although the kernel
// alone was 2 % faster; at 53 (allocated 56, as the byte form's 56) the step is 1.4 % faster (profiles/r32_fast_pair_scores.md).  Beside the
// waves of the kernels that overlap it, 56 registers a wave let one more cell-wave onto a SIMD than 64.  Keep k_fast<48,45> at or under 56.
template <bool PAIR, int TS, int BELOW, bool TRIM = false>
__device__ __forceinline__ void clearScoreApron(uint8_t* score, int t, int ch, int q0, int q1, int validLast = 4) {
    constexpr int RS = ScoreTile<PAIR, TS>::kStride, IB = ScoreTile<PAIR, TS>::kItem, RD = RS / 8;
    static_assert(RS % 8 == 0 && (1 + BELOW) * RD <= 64, "the zero rows are one trip of 8-byte stores");
    static_assert(!TRIM || PAIR, "whole u16 pixels");
    if (t < (1 + BELOW) * RD) {
        const int r = t / RD, c = t - r * RD;
        *(uint2*)(score + (r == 0 ? 0 : ch + r) * RS + 8 * c) = uint2{0u, 0u};
    }
    if (t < ch) {
        *(unsigned*)(score + (t + 1) * RS + IB * q0 - 4) = 0u;
        *(unsigned*)(score + (t + 1) * RS + IB * (q1 + 1)) = 0u;
        if constexpr (TRIM) {      // (validLast is uniform) 1: pixel 1 and pixels 2, 3; 2: pixels 2, 3; 3: pixel 3
            uint8_t* last = score + (t + 1) * RS + IB * q1;
            if (validLast & 1) *(unsigned short*)(last + 2 * validLast) = 0;
            if (validLast <= 2) *(unsigned*)(last + 4) = 0u;
        }
    }
}

// Ring of the two pixels at bytes P, P+1 of the centre dword (P = 0 or 2) in cv::FAST order, r[16] = the centre pair:
// L/C/R[d] = the three dwords of tile row (centre row + d - 3).
template <int P>
__device__ __forceinline__ void pairRing(const unsigned (&L)[7], const unsigned (&C)[7], const unsigned (&R)[7], unsigned (&r)[17]) {
    constexpr int B = 4 + P;      // byte of the first pixel inside L|C|R
    r[0] = pairAt<B>(L[6], C[6], R[6]);       r[1] = pairAt<B + 1>(L[6], C[6], R[6]);   r[2] = pairAt<B + 2>(L[5], C[5], R[5]);
    r[3] = pairAt<B + 3>(L[4], C[4], R[4]);   r[4] = pairAt<B + 3>(L[3], C[3], R[3]);   r[5] = pairAt<B + 3>(L[2], C[2], R[2]);
    r[6] = pairAt<B + 2>(L[1], C[1], R[1]);   r[7] = pairAt<B + 1>(L[0], C[0], R[0]);   r[8] = pairAt<B>(L[0], C[0], R[0]);
    r[9] = pairAt<B - 1>(L[0], C[0], R[0]);   r[10] = pairAt<B - 2>(L[1], C[1], R[1]);  r[11] = pairAt<B - 3>(L[2], C[2], R[2]);
    r[12] = pairAt<B - 3>(L[3], C[3], R[3]);  r[13] = pairAt<B - 3>(L[4], C[4], R[4]);  r[14] = pairAt<B - 2>(L[5], C[5], R[5]);
    r[15] = pairAt<B - 1>(L[6], C[6], R[6]);
    r[16] = pairAt<B>(L[3], C[3], R[3]);
}
// BRIGHT: max over the 16 arcs of the arc minimum (and the centre); else min over the arcs of the arc maximum (and the
// centre).  Arcs k and k+1 (k even) share the 8 ring pixels k+1..k+8, and
//     max(min(core, r_k), min(core, r_k+9)) = min(core, max(r_k, r_k+9)),
// so 8 "arc pairs" replace 16 arcs.  The cores are two 4-runs starting at odd positions, each 4-run two 2-runs:
// 8 + 8 + 8 (end points) + 8 (3-input) + 4 (reduction) = 36 instructions per polarity.
template <bool BRIGHT>
__device__ __forceinline__ unsigned arcExtreme(const unsigned (&r)[17]) {
    unsigned x2[8], x4[8], g[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {            // x2[i] = extreme of ring pixels 2i+1, 2i+2
        const int p = 2 * i + 1;
        x2[i] = BRIGHT ? pkmin3(r[p], r[(p + 1) & 15], r[(p + 1) & 15]) : pkmax3(r[p], r[(p + 1) & 15], r[(p + 1) & 15]);
    }
#pragma unroll
    for (int i = 0; i < 8; i++)              // x4[i] = extreme of ring pixels 2i+1 .. 2i+4
        x4[i] = BRIGHT ? pkmin3(x2[i], x2[(i + 1) & 7], x2[(i + 1) & 7]) : pkmax3(x2[i], x2[(i + 1) & 7], x2[(i + 1) & 7]);
#pragma unroll
    for (int i = 0; i < 8; i++) {            // arcs 2i and 2i+1: core = pixels 2i+1 .. 2i+8, end points 2i and 2i+9
        const int k = 2 * i;
        const unsigned e = BRIGHT ? pkmax3(r[k], r[(k + 9) & 15], r[(k + 9) & 15]) : pkmin3(r[k], r[(k + 9) & 15], r[(k + 9) & 15]);
        g[i] = BRIGHT ? pkmin3(x4[i], x4[(i + 2) & 7], e) : pkmax3(x4[i], x4[(i + 2) & 7], e);
    }
    return BRIGHT ? pkmax3(pkmax3(g[0], g[1], g[2]), pkmax3(g[3], g[4], g[5]), pkmax3(g[6], g[7], r[16]))
                  : pkmin3(pkmin3(g[0], g[1], g[2]), pkmin3(g[3], g[4], g[5]), pkmin3(g[6], g[7], r[16]));
}
// One polarity per pixel (round 4).  A pixel is a corner in at most one polarity, and which one is decided exactly by the opposite ring pairs: a
// 9-arc holds one pixel of EVERY pair (k, k+8), so a dark corner has min(r_k, r_k+8) < v for all eight pairs; a bright corner's arc k..k+8
// holds BOTH pixels of pair k, so for it that test fails.  "max over the pairs of the pair minimum < v" therefore selects dark for every
// dark corner and bright for every bright one; where it picks the wrong side of a non-corner the score comes out as that side's S, which is
// <= the true S <= minThFAST - and the NMS pass counts everything <= minThFAST alike (thPair).  For a corner the other side's S is 0 (any
// other arc shares >= 2 pixels with the corner's arc), so the stored score IS S.  A dark pixel's ring and centre are complemented (x ^ 255
// reverses the order and keeps the halves inside 0..255), after which dark is bright: 12 + 2 + 17 (full-rate v_xor) + 36 + 1 instructions
// per pixel pair instead of 75.
__device__ __forceinline__ unsigned pairScore(const unsigned (&r)[17]) {
    unsigned m[8];
#pragma unroll
    for (int k = 0; k < 8; k++) m[k] = pkmin3(r[k], r[k + 8], r[k + 8]);
    const unsigned M = pkmax3(pkmax3(m[0], m[1], m[2]), pkmax3(m[3], m[4], m[5]), pkmax3(m[6], m[7], m[7]));
    unsigned flip;                                   // per half: M < v  <=>  M - v is negative  <=>  its high byte is 0xFF (|M - v| <= 255)
    asm("v_pk_lshrrev_b16 %0, %2, %1" : "=v"(flip) : "v"(pksub(M, r[16])), "s"(0x00080008u));
    unsigned x[17];
#pragma unroll
    for (int i = 0; i < 17; i++) x[i] = r[i] ^ flip;
    __builtin_amdgcn_sched_barrier(0);
    return pksub(arcExtreme<true>(x), x[16]);        // the centre took part in the reduction: never negative
}

#if defined(ORBX_FAST_CLOCK) && defined(ORBX_FAST_TU)      // (diagnostic builds stamp the kernel of k_fast.hip only)
// diagnostic build only (tools/fast_clock.py): the clock k_fast's waves actually run at = sum of delta s_memtime / sum of delta s_memrealtime
// x 100 MHz over every cell-wave (MI355X_MICROARCH.md, DVFS give-back (6)); the stamps go to a buffer nothing else reads
constexpr int kFastClockSlots = 4096;      // one sampled wave per slot: plain stores (an atomic per wave would BE the load)
__device__ unsigned long long g_fastClock[2 * kFastClockSlots];
extern "C" int orbx_debug_fast_clock(unsigned long long* out, int reset) {
    if (reset) return (int)hipMemset((void*)nullptr, 0, 0) + (int)hipMemcpyToSymbol(HIP_SYMBOL(g_fastClock), out, sizeof(unsigned long long) * 2 * kFastClockSlots);
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fastClock), sizeof(unsigned long long) * 2 * kFastClockSlots);
}
// ... and the span of every wave of frame 0 (tools/fast_spans.py): [2 * (chunk * 4 + wave)] = start, end in s_memrealtime ticks
__device__ unsigned long long g_fastSpans[2 * 4096], g_fastMid[4 * 4096];      // (mid: staged, scored, counted, ... of a FAST wave)
extern "C" int orbx_debug_fast_spans(unsigned long long* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fastSpans), sizeof(g_fastSpans)); }
extern "C" int orbx_debug_fast_mid(unsigned long long* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fastMid), sizeof(g_fastMid)); }
#define FAST_MID(which) do { const int fsI = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6); \
        if ((threadIdx.x & 63) == 0 && blockIdx.x == 0 && blockIdx.z == 0 && fsI < 4096) g_fastMid[4 * fsI + (which)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define FAST_SPAN(which) do { const int fsI = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6); \
        if ((threadIdx.x & 63) == 0 && blockIdx.x == 0 && blockIdx.z == 0 && fsI < 4096) g_fastSpans[2 * fsI + (which)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#define FAST_CLOCK_BEGIN const unsigned long long fcR0 = __builtin_amdgcn_s_memrealtime(), fcT0 = __builtin_amdgcn_s_memtime();
#define FAST_CLOCK_END do { const unsigned long long fcT1 = __builtin_amdgcn_s_memtime(), fcR1 = __builtin_amdgcn_s_memrealtime(); \
        const unsigned fcW = (unsigned)(f * nCells + ci); \
        if (lane == 0 && (fcW & 63u) == 0u) { g_fastClock[2 * ((fcW >> 6) & (kFastClockSlots - 1))] = fcT1 - fcT0; \
                                              g_fastClock[2 * ((fcW >> 6) & (kFastClockSlots - 1)) + 1] = fcR1 - fcR0; } } while (0)
#else
#define FAST_CLOCK_BEGIN
#define FAST_CLOCK_END do {} while (0)
#define FAST_SPAN(which) do {} while (0)
#define FAST_MID(which) do {} while (0)
#endif
constexpr int kFastWaves = 4;
#ifndef ORBX_FAST_WAVES
#define ORBX_FAST_WAVES 4   // waves per SIMD the kernel is compiled for
#endif
#ifndef ORBX_FAST_SKIP
#define ORBX_FAST_SKIP 0   // diagnostic builds (tools/fast_breakdown.py): 1 = no score pass, 2 = stop after the score pass, 4 = no staging loads
#endif
#ifndef ORBX_FAST_LDS_PAD
#define ORBX_FAST_LDS_PAD 0   // A/B builds: bytes of unused static LDS added to a k_fast workgroup (what a larger tile would cost in resident workgroups)
#endif

// Atomics on an LDS word whose address the compiler may see as a generic pointer (a body inlined behind pointer arguments): the cast names the
// address space, so the instruction is a ds_* whatever the optimiser merged around it.
typedef __attribute__((address_space(3))) unsigned LdsU32;
__device__ __forceinline__ void ldsAtomicAdd(unsigned* p, unsigned v) { (void)__hip_atomic_fetch_add((LdsU32*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void ldsAtomicMax(unsigned* p, unsigned v) { (void)__hip_atomic_fetch_max((LdsU32*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// LDS operations of one wave execute in issue order, so lanes of a wave only need the COMPILER to keep the
// order of the stores before and the loads after this point.
__device__ __forceinline__ void waveLdsSync() {
    asm volatile("" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");
}

// What the fused form needs to run the blur's lanes behind the FAST cells (small batches: the two kernels are independent, both only
// read the pyramid, and a launch costs ~6 us of latency whatever its size)
struct BlurTail { const BlurItem* items; const unsigned short* laneItem; int nLanes; uint8_t* blur; int fastChunks; };

// LDS of one FAST workgroup (four cell-waves): the pixel tiles behind 16 bytes of padding (the packed score pass reads the dword left of every
// row's first interior dword), the score tiles as an array of their own (their base is then one scalar, and the NMS pass's nine reads are
// immediate offsets of ONE address register; inside one array they sat 2 KB behind the pixel tile's base, past the reach of ds_read2's
// offsets: four v_add per trip), and the cells' x / y path codes (small batches: leaf tables).
// Pair form: the score tile lives in the pixel tiles' array, one region of FastAlias::kWaveBytes per wave (orbx_device.hpp has the layout and
// why the two may share bytes); there is no second array.
template <int TS, int ROWS>
struct FastLds {
    static constexpr bool kPair = kFastPairTile<TS>;
    static constexpr int kTileBytes = TS * ROWS, kScoreBytes = kPair ? 0 : TS * (ROWS - 3);
    static constexpr int kWaveBytes = kPair ? FastAlias<TS, ROWS>::kWaveBytes : kTileBytes;      // a wave's share of the first array
    static constexpr int kTiles = 16 + kFastWaves * kWaveBytes, kScores = kFastWaves * kScoreBytes, kCodes = kFastWaves * 2 * 64;
    static constexpr int kScoreOff = (kTiles + 15) & ~15, kCodeOff = (kScoreOff + kScores + 15) & ~15, kBytes = kCodeOff + kCodes;
};

// One cell on one wave (the whole of k_fast's work).  smem / scoreS / codeL: the workgroup's
// three LDS arrays (FastLds; scoreS is not used in the pair form), chunk: the workgroup's group of four cells, f: the frame.  No workgroup barrier.
// BIG: the candidates are written in the two-dword format of frames beyond 4096 px (orbx_device.hpp: CandFmt).
template <int TS, int ROWS, bool BIG = false>
__device__ __forceinline__ void fastCell(const CellDesc* __restrict__ cells, int nCells, const LevelGeom* __restrict__ lv,
                                         const uint8_t* __restrict__ pyr, int iniTh, int minTh,
                                         typename CandFmt<BIG>::T* __restrict__ candSeg, unsigned* __restrict__ cellCount, LeafTables lt,
                                         uint8_t* smem, uint8_t* scoreS, uint8_t (*codeL)[2][64], int chunk, int f) {
    constexpr bool PAIR = kFastPairTile<TS>;          // the score tile's form (ScoreTile)
    constexpr int RS = ScoreTile<PAIR, TS>::kStride, IB = ScoreTile<PAIR, TS>::kItem;
    constexpr int kScoreBytes = RS * (ROWS - 3);      // score tile: (ch + 2) rows <= ROWS - 4, and one more zero row for the NMS lanes past the last item
    using L = FastLds<TS, ROWS>;
    using A = FastAlias<TS, ROWS>;                    // (pair form only)
    static_assert(!PAIR || (A::kScoreStride == RS && A::kScoreItem == IB && kScoreBytes <= A::kWaveBytes), "FastAlias states this tile");
    constexpr int DW = TS / 4;                       // dwords per tile row
    constexpr int LPR = DW <= 16 ? 8 : 16;            // lanes per row while staging: a lane moves TWO dwords (one 8-byte load, one 8-byte LDS store)
    constexpr int RPI = 64 / LPR;                     // rows per staging step
    constexpr int STEPS = (ROWS + RPI - 1) / RPI;
    static_assert(DW % 2 == 0 && TS % 8 == 0, "dword pairs per tile row");
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;   // scalar: the cell and its geometry load through the scalar unit
    const int ci = chunk * kFastWaves + wave;
    if (ci >= nCells) return;   // wave-uniform; the kernel has no workgroup barrier
    FAST_CLOCK_BEGIN
    const CellDesc c = cells[ci];
    const LevelGeom g = lv[c.level];
    uint8_t* const region = smem + 16 + wave * L::kWaveBytes;
    uint8_t* tile = PAIR ? region + A::kPixelOff : region;
    uint8_t* score = PAIR ? region : scoreS + wave * kScoreBytes;
    const int roiW = c.roiW, roiH = c.roiH, cw = roiW - 6, ch = roiH - 6;
    // small batches (leaf tables): the x / y path codes of the cell's interior columns and rows are fetched WITH the ROI (lane i: column i and
    // row i) and kept in LDS: read from memory where the emit needs them they were two dependent L2 round trips at the end of every cell
    const bool leaf = lt.hist != nullptr && g.leafOK && f < lt.frames;      // wave-uniform
    uint8_t myXc = 0, myYc = 0;
    if (leaf) {
        myXc = lt.xcode[c.level * lt.XT + min(c.shiftX + 3 + lane, g.rectW - 1)];
        myYc = lt.ycode[c.level * lt.XT + min(c.shiftY + 3 + lane, g.rectH - 1)];
    }

    // ---- stage the ROI, re-aligned: tile byte k of row r is ROI pixel (k - 1, r), whatever the ROI's alignment in
    //      HBM, so the interior (ROI pixels 3 ..) always starts on a dword of the tile.  The packed passes walk the
    //      interior dword by dword: a 31- or 32-pixel cell is then 8 dwords wide, not 9, and its 8 x 32 four-pixel
    //      items are exactly 4 wave iterations.  Cost: the lane's right neighbour's dword (DPP) and one v_alignbyte. ----
    const int gx1 = kPadL + c.x0 - 1;                   // byte column of tile byte 0 in the bordered row
    const int gsh = gx1 & 3;                            // its offset inside the aligned dword the lanes load
    constexpr int mis = kFastTileShift;                              // tile byte of ROI pixel 0 (the passes below are written for any value)
    {
        // wave-uniform base + 32-bit lane offsets; rows / dword columns past the ROI are clamped, not predicated (their
        // tile bytes are never read by an interior pixel)
        const uint8_t* sp = pyr + c.pyrOff + (long long)f * c.pyrFrameBytes + (long long)(kEdge + c.y0) * c.pyrStride + (gx1 - gsh);
        const int dcol = lane & (LPR - 1), rsub = lane / LPR;                    // dcol: the lane's dword PAIR of the row
        const unsigned colOff = 8u * (unsigned)min(dcol, (gsh + roiW) >> 3);    // last pair holding a needed byte (its second dword still lies inside the bordered row)
        const unsigned off0 = (unsigned)__mul24(rsub, c.pyrStride) + colOff, offMax = (unsigned)__mul24(roiH - 1, c.pyrStride) + colOff;
        const unsigned stepOff = (unsigned)(RPI * c.pyrStride);
        uint2 w[STEPS];
#pragma unroll
        for (int s = 0; s < STEPS; s++) {
            if (ORBX_FAST_SKIP & 4) w[s] = uint2{0u, 0u};
            else __builtin_memcpy(&w[s], sp + min(off0 + s * stepOff, offMax), 8);      // (4-byte aligned: one global_load_dwordx2)
        }
#pragma unroll
        for (int s = 0; s < STEPS; s++) {
            const int r = s * RPI + rsub;
            const unsigned next = (unsigned)__builtin_amdgcn_update_dpp(0, (int)w[s].x, 0x130 /* wave_shl:1: lane i <- lane i+1 */, 0xF, 0xF, true);
            if (dcol < DW / 2 && r < ROWS)
                *(uint2*)(tile + r * TS + 8 * dcol) = uint2{__builtin_amdgcn_alignbyte(w[s].y, w[s].x, (unsigned)gsh), __builtin_amdgcn_alignbyte(next, w[s].y, (unsigned)gsh)};
        }
    }
    if (leaf) { codeL[wave][0][lane] = myXc; codeL[wave][1][lane] = myYc; }
    // "items" of the packed passes: one tile dword (4 pixels) of an interior row; q0..q1 are the dwords that touch it
    const int q0 = (mis + 3) >> 2, q1 = (mis + 2 + cw) >> 2, nq = q1 - q0 + 1;
    const int nItems = nq * ch;
    constexpr int lo = mis + 3 - 4 * ((mis + 3) >> 2);      // first valid byte of dword q0
    const int hi = mis + 3 + cw - 4 * q1;                   // valid bytes of dword q1 (1 .. 4)
    // zero the score tile's apron (it stands for "outside the ROI interior"); the score pass writes the rest.  (Pair form: behind the score
    // pass, the apron's bytes hold pixel rows until then.)
    if constexpr (!PAIR) clearScoreApron<PAIR, TS, 2>(score, lane, ch, q0, q1);
    waveLdsSync();
    FAST_MID(0);

    // ---- pass 1: scores ----
    if (!(ORBX_FAST_SKIP & 1)) {
        // one lane = the four pixels of one tile dword (two packed pairs); 21 dword reads feed 4 scores.  Score row y+1
        // keeps the tile's item grid, so the four scores are one store (pair form: the two result registers as they are,
        // 8 bytes; byte form: packed to a dword); pixels outside the interior (first / last item of a row) are written
        // as 0 = "outside the ROI interior" (byte form) or zeroed behind the pass (pair form: clearScoreApron, TRIM).
        static_assert(!PAIR || lo == 0, "the pair form trims the last item of a row only");
        const unsigned maskFirst = 0xFFFFFFFFu << (8 * lo), maskLast = hi >= 4 ? 0xFFFFFFFFu : ~(0xFFFFFFFFu << (8 * hi));
        const int sy = (64 * c.itemRecip) >> 16, sx = 64 - sy * nq;           // 64 / nq, 64 % nq (exact: CellDesc::itemRecip)
        int y = (lane * c.itemRecip) >> 16, qi = lane - y * nq;                  // lane / nq, lane % nq
        // An LDS read is served in two groups of 32 lanes (banks = dword index mod 32).  With 8 items per row a group is four rows of 8 dwords, and
        // four CONSECUTIVE rows at 12 dwords per row start at banks 0, 12, 24, 4: the fourth collides with the first (every read of the pass
        // 2-way).  Rows 0, 2, 4, 6 start at 0, 24, 16, 8 (and 1, 3, 5, 7 at 12, 4, 28, 20): disjoint.  The order of the items does not matter here.
        if (DW == 12 && nq == 8) y = ((y & 3) << 1) | (y >> 2);
        // base: the item's dword in tile row y (= centre row - 3); dst: the item in score row y + 1; mLo, mHi: its mask(s) as storeScores takes them
        auto scoreItem = [&](const uint8_t* base, uint8_t* dst, const unsigned mLo, const unsigned mHi) {
            unsigned L[7], C[7], R[7];
#pragma unroll
            for (int d = 0; d < 7; d++) {
                L[d] = *(const unsigned*)(base + d * TS - 4);
                C[d] = *(const unsigned*)(base + d * TS);
                R[d] = *(const unsigned*)(base + d * TS + 4);
            }
            unsigned rA[17], rB[17];
            pairRing<0>(L, C, R, rA);
            pairRing<2>(L, C, R, rB);
            __builtin_amdgcn_sched_barrier(0);
            const unsigned sA = pairScore(rA);
            __builtin_amdgcn_sched_barrier(0);
            const unsigned sB = pairScore(rB);
            storeScores<PAIR>(dst, sA, sB, mLo, mHi);
        };
        if (sx == 0) {
            // the items of a row divide the wave (8 items: the usual 29..32-px cells; 1, 2, 4, 16): a lane keeps its item column, so its edge masks are
            // fixed and a trip is "sy rows further": two pointer steps and a compare instead of re-deriving (item, row), the masks and the address
            const unsigned m = (qi == 0 ? maskFirst : 0xFFFFFFFFu) & (qi == nq - 1 ? maskLast : 0xFFFFFFFFu);
            const unsigned mLo = PAIR ? 0xFFFFFFFFu : m, mHi = 0xFFFFFFFFu;
            const uint8_t* base = tile + y * TS + 4 * (q0 + qi);
            // (the item's place in score row y + 1 follows from its place in tile row y - one add on a scalar - and is not carried as a register)
            for (; y < ch; y += sy, base += sy * TS) scoreItem(base, score + RS + (IB / 4) * (base - tile), mLo, mHi);
        } else {
            for (; y < ch;) {
                unsigned m = qi == 0 ? maskFirst : 0xFFFFFFFFu;
                m = qi == nq - 1 ? (m & maskLast) : m;
                scoreItem(tile + y * TS + 4 * (q0 + qi), score + (y + 1) * RS + IB * (q0 + qi), PAIR ? 0xFFFFFFFFu : m, 0xFFFFFFFFu);
                qi += sx; y += sy;
                if (qi >= nq) { qi -= nq; y++; }
            }
        }
    }
    if constexpr (PAIR) clearScoreApron<PAIR, TS, 2, true>(score, lane, ch, q0, q1, hi);
    waveLdsSync();
    if (ORBX_FAST_SKIP & 2) { if (lane == 0) cellCount[(long long)f * nCells + ci] = 0u; return; }

    FAST_MID(1);
    // ---- pass 2: strict local maxima, four pixels per lane (the score rows keep the tile's item grid): the neighbour
    //      maximum with minThFAST folded in (nmsNeighbourMax), so "keep" is simply S > max.  Survivors are appended in
    //      raster order (lane order, then pixel order inside the lane) to a list that reuses the pixel tile (no longer
    //      needed).
    //      Banks of the pair form's reads (rows of 24 dwords; a read is served in two groups of 32 lanes = four score rows of 8 items): the 8-byte
    //      read of A | B has 64 banks and a row's 8 items are 16 consecutive dwords; rows y .. y + 3 start at banks 0, 24, 48, 8 (+ 2 q0), so the
    //      fourth row shares 8 of its 16 banks with the first: that group takes 2 LDS cycles instead of 1.  The 4-byte reads of P and N have 32
    //      banks and touch every second dword: rows start at banks 0, 24, 16, 8 and reach over 16 banks each, so every row shares 4 of its 8
    //      dwords' banks with the next: 2-way as well.  (The byte form: 12 dwords per row, rows at 0, 12, 24, 4: the fourth row's 8 dwords share 4
    //      banks with the first.)  Raster order fixes which rows a group holds, so unlike pass 1 the rows cannot be re-dealt here. ----
    //      The list (pair form: over the score rows the pass has left behind, FastAlias).  An entry is one dword per kept PIXEL PAIR: the pair's
    //      score register as the pass holds it (two u16 halves of 0 .. 255) with the coordinates in the bytes the scores leave free:
    //          bits 0-7 S of the pair's first pixel | 8-13 x of the pair's first pixel (4 * item + 0 or 2) | 16-23 S of its second pixel | 24-29 y
    //      A trip then spends one v_or per kept pair on the entry; which pixel of the pair was kept, its x and its S are taken from the word
    //      by the one dense pass over the list below (pass 3).  0 = no entry. ----
    static_assert(lo == 0, "an item's first pixel is x = 4 * item: bits 0, 1 of an entry's x field are the pair and the pixel of the pair");
    unsigned* list = (unsigned*)region;
    int nMin = 0;
    {
        const unsigned thPair = (unsigned)minTh | ((unsigned)minTh << 16);
        const int sy = (64 * c.itemRecip) >> 16, sx = 64 - sy * nq;
        int y = (lane * c.itemRecip) >> 16, qi = lane - y * nq;
        // one trip of 64 items: base = the item's dword in score row y (the row above the centre row), xy = x << 8 | y << 24 of its pixel 0 (x <= 60,
        // y <= 62 where a pixel can be kept; beyond, y may run past its field: only kept pairs are stored).  Lanes past the last item (y >= ch) take
        // centre row ch + 1, the zero row below the interior: S = 0 keeps nothing, so the pass needs no "active" predicate
        auto nmsTrip = [&](const uint8_t* base, const unsigned xy) {
            unsigned sA, sB, mA, mB;
            nmsNeighbourMax<PAIR, TS>(base, thPair, sA, sB, mA, mB);
            unsigned dA, dB;                             // per half: S - max, saturated at 0: nonzero <=> strict maximum above minThFAST
            asm("v_pk_sub_u16 %0, %1, %2 clamp" : "=v"(dA) : "v"(sA), "v"(mA));
            asm("v_pk_sub_u16 %0, %1, %2 clamp" : "=v"(dB) : "v"(sB), "v"(mB));
            // two horizontal neighbours are never both strict maxima, so a pixel PAIR keeps at most one pixel: one ballot per pair, not per pixel
            const bool fA = dA != 0u, fB = dB != 0u;
            const unsigned long long bA = __ballot(fA), bB = __ballot(fB);
            if (bA | bB) {
                int at = nMin;                           // + kept pixels of the lower lanes: one v_mbcnt pair per ballot
                at = __builtin_amdgcn_mbcnt_hi((unsigned)(bA >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bA, at));
                at = __builtin_amdgcn_mbcnt_hi((unsigned)(bB >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bB, at));
                // a lane's first entry (A's, else B's) under one mask; a second one only where both pairs keep a pixel, which most trips skip
                // (two predicated stores, one per pair, were 2 vector instructions and one mask save / restore more per trip)
                const unsigned wB = sB | xy | 0x200u;
                if (fA || fB) list[at] = fA ? (sA | xy) : wB;
                if (fA && fB) list[at + 1] = wB;
                nMin += __popcll(bA) + __popcll(bB);
            }
        };
        const int trips = (nItems + 63) >> 6;
        if (sx == 0) {      // a lane keeps its item column (scoreItem has the reason): a trip is sy rows further
            const uint8_t* base = score + y * RS + IB * (q0 + qi);
            const uint8_t* const baseEnd = score + ch * RS + IB * (q0 + qi);
            unsigned xy = ((unsigned)qi << 10) | ((unsigned)y << 24);
            for (int t = 0; t < trips; t++, base += sy * RS, xy += (unsigned)sy << 24) nmsTrip(base < baseEnd ? base : baseEnd, xy);
        } else {
            for (int t = 0; t < trips; t++) {
                nmsTrip(score + min(y, ch) * RS + IB * (q0 + qi), ((unsigned)qi << 10) | ((unsigned)y << 24));
                qi += sx; y += sy;
                if (qi >= nq) { qi -= nq; y++; }
            }
        }
    }
    waveLdsSync();
    // every cell owns a fixed, exactly sized segment of the level's candidate arena (no two 8-adjacent NMS survivors
    // => at most ceil(cw/2)*ceil(ch/2) of them), so the emit needs no atomic; the quad-tree kernel compacts the
    // segments in cell order, which is the reference's vToDistributeKeys order (cell row, cell column, y, x)
    typename CandFmt<BIG>::T* outPos = candSeg + g.candOff + (long long)f * g.candCap + c.segOff;
    const unsigned segCap = (unsigned)(((cw + 1) >> 1) * ((ch + 1) >> 1));
    // Small batches: the quad-tree's first sweep is done here, by 800 waves instead of one workgroup per level (k_octree_body.inc,
    // preCounted): every kept key adds 1 to its leaf cell of its root's 32 x 32 grid and offers (response, then smallest segment slot = first
    // in the reference's vector) as the leaf's best key.  Both operations commute, so the order of the cells' waves does not matter.  A cell
    // touches only a small rectangle of leaf cells (x / y path codes are monotone), so the wave first collects them in LDS (the score tile
    // is dead by now) and sends ONE pair of L2 atomics per touched leaf instead of one per key (100 k keys per frame otherwise: the L2
    // atomics on a few hundred hot lines cost more than the sweep they replace).
    constexpr int kLeafCap = TS * (ROWS - 3) / 8;      // (the same in both tile forms)
    static_assert(!PAIR || kLeafCap == A::kLeafCap, "FastAlias states the leaf tables");
    unsigned *tHist = (unsigned*)(PAIR ? region + A::kLeafOff : score), *tBest = tHist + kLeafCap;
    int xc0 = 0, yc0 = 0, nxl = 1, nLeafLocal = 0;
    const uint8_t *xcL = codeL[wave][0], *ycL = codeL[wave][1];      // code of interior column x / row y of the cell (pixel shift + 3 + x, clamped to the rectangle)
    if (leaf && nMin > 0) {      // (ahead of the first trip over the list; a cell without entries has no leaf cell to report)
        xc0 = xcL[0]; yc0 = ycL[0];
        nxl = (int)xcL[cw - 1] - xc0 + 1;
        const int nyl = (int)ycL[ch - 1] - yc0 + 1;
        nLeafLocal = nxl * nyl <= kLeafCap ? nxl * nyl : 0;      // 0: a cell over too many leaf cells (tiny leaves) goes to L2 key by key
        for (int e = lane; e < nLeafLocal; e += 64) { tHist[e] = 0u; tBest[e] = 0u; }
        waveLdsSync();
    }
    // ---- pass 3: one dense pass over the list decodes, counts and emits.  It runs at iniThFAST; the reference retries the cell at minThFAST
    //      only when the first call returned nothing (:835-838), and a trip that kept nothing has stored nothing and touched no leaf table,
    //      so the retry is a second trip of the same loop.  base = the keys kept by the last trip made = the cell's count.
    //      Decode: a kept pixel is a strict maximum over its eight neighbours and the other pixel of its pair is one of them, so the kept
    //      pixel is the strictly larger half of the entry: S = max(halves), x = the pair's x + (second half > first half). ----
    unsigned base = 0;
#pragma nounroll
    for (int th = iniTh; nMin > 0; th = minTh) {
        for (int i0 = 0; i0 < nMin; i0 += 64) {
            const unsigned e = i0 + lane < nMin ? list[i0 + lane] : 0u;      // 0 marks "past the end": S = 0
            const int s0 = (int)(e & 0xFFu), s1 = (int)((e >> 16) & 0xFFu);
            const int s = max(s0, s1), x = (int)((e >> 8) & 63u) + (s1 > s0 ? 1 : 0), y = (int)((e >> 24) & 63u);
            const bool keep = s > th;                       // entries hold S > minTh
            const unsigned long long m = __ballot(keep);
            if (keep) {
                const unsigned at = base + __popcll(m & ((1ull << lane) - 1));
                if (at < segCap) {
                    const unsigned kx = (unsigned)(c.shiftX + x + 3), ky = (unsigned)(c.shiftY + y + 3);
                    const typename CandFmt<BIG>::T w = CandFmt<BIG>::make(kx, ky, (unsigned)(s - 1));   // response = S - 1
                    outPos[at] = w;
                    if (leaf) {
                        const int xc = xcL[x], yc = ycL[y];
                        const unsigned val = CandFmt<BIG>::respKey(w) | (0xffffffu - ((unsigned)c.segOff + at));
                        if (nLeafLocal) {
                            const int li = (yc - yc0) * nxl + (xc - xc0);
                            // (LDS by type: with the tables reached through the body's pointer arguments the compiler merged this pair with the
                            // global pair of the other branch into ONE atomic on a generic pointer - a flat_atomic, docs/history/DESIGN_rounds_1-5.md §4i's construct)
                            ldsAtomicAdd(&tHist[li], 1u);
                            ldsAtomicMax(&tBest[li], val);
                        } else {
                            const unsigned cellOfRoot = leafTableEntry(lt, f, c.level, xc, yc);
                            atomicAdd(lt.hist + cellOfRoot, 1);
                            atomicMax(lt.best + cellOfRoot, val);
                        }
                    }
                }
            }
            base += __popcll(m);
        }
        if (base != 0u || th == minTh) break;
    }
    if (lane == 0) cellCount[(long long)f * nCells + ci] = base;
    FAST_CLOCK_END;
    FAST_SPAN(1);
    FAST_MID(2);
    if (base == 0u) return;
    if (nLeafLocal) {
        waveLdsSync();
        for (int e = lane; e < nLeafLocal; e += 64) {
            const unsigned n = tHist[e];
            if (n) {
                const int er = (int)(((float)e + 0.5f) * __frcp_rn((float)nxl));      // e / nxl (exact: e < 1024, the quotient is >= 0.5 / nxl away from an integer)
                const int xc = xc0 + (e - er * nxl), yc = yc0 + er;
                const unsigned cellOfRoot = leafTableEntry(lt, f, c.level, xc, yc);
                atomicAdd(lt.hist + cellOfRoot, (int)n);
                atomicMax(lt.best + cellOfRoot, tBest[e]);
            }
        }
    }
    FAST_SPAN(1);      // (diagnostic builds: the wave's end including the emit; the stamp above stays as the end of a cell without keys)
}


}  // namespace orbx
