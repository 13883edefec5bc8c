// k_describe_body.hpp - IC_Angle, rotated BRIEF and the final placement of one workgroup's eight keypoints as a device function; k_describe.hip
// launches it.  See k_describe.hip for the algorithm.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orbx_device.hpp"
#include "k_blur_body.hpp"      // hsums4, satPack4: the patch-blur form blurs a keypoint's 37 x 37 patch out of its raw 43 x 43 tile

namespace orbx {
// ================================================================================================
// IC_Angle + rotated BRIEF + final placement.  One wave64 per kept keypoint.
// ================================================================================================
// The tables below are the same for every extractor (HALF_PATCH_SIZE = 15 and the learned pattern are compile-time constants of the reference,
// ORBextractor.cc:71, 148-406), so they are initialised statically: no upload, nothing for a second handle's creation to overwrite while a
// first handle's kernels read them.  checkUmax compares kUmaxStatic with the table the host derives by the reference's formula (:459-474).
constexpr int kUmaxStatic[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
constexpr int kBriefReach = 18;                       // |rounded rotated pattern coordinate| <= 18 (max radius 18.385)
// IC_Angle's weight words: row |v| = a of the disc as the dwords of a staged tile row, byte b of dword j <-> u = 4 j + b - U0; plane 0 holds u + 16
// inside the disc (|u| <= umax[a]; sum(u I) = dot(I, u + 16) - 16 dot(I, 1)), plane 1 holds 1 there, both 0 outside.  A function of kUmaxStatic and
// the tile layout alone, so it is evaluated by the compiler: ONE constexpr array initialises the __constant__ copy a workgroup fills its LDS table
// from and is what the host exports (describeTables; tests/test_describe_tables.py restates it from the reference's formula).
template <int W> struct WeightWords { unsigned w[2][16][W]; };
template <int W, int U0>
constexpr WeightWords<W> makeWeightWords() {
    WeightWords<W> t{};
    for (int which = 0; which < 2; which++)
        for (int a = 0; a < 16; a++)
            for (int j = 0; j < W; j++)
                for (int b = 0; b < 4; b++) {
                    const int u = 4 * j + b - U0, au = u < 0 ? -u : u;
                    if (au <= kHalfPatch && au <= kUmaxStatic[a]) t.w[which][a][j] |= (unsigned)(which ? 1 : u + 16) << (8 * b);
                }
    return t;
}
constexpr WeightWords<12> kWeightsPb = makeWeightWords<12, kBriefReach + 4>();      // the re-aligned 44-byte tile row of the patch-blur form: u = t - 22
constexpr WeightWords<8> kWeightsPlain = makeWeightWords<8, kHalfPatch>();          // the 32 bytes from the patch's first column on: u = k - 15
static __constant__ WeightWords<12> c_weightsPb = kWeightsPb;
static __constant__ WeightWords<8> c_weightsPlain = kWeightsPlain;
static __constant__ __attribute__((aligned(16))) float c_patternF[1024] = {   // the rBRIEF pattern as floats
#include "orbx_brief_pattern.inc"
};

// cv::fastAtan2: every operation rounded separately in binary32.
__device__ __forceinline__ float fastAtan2Deg(float y, float x) {
    const float sc = (float)(180.0 / 3.1415926535897932384626433832795);
    const float p1 = 0.9997878412794807f * sc, p3 = -0.3258083974640975f * sc, p5 = 0.1555786518463281f * sc,
                p7 = -0.04432655554792128f * sc;
    const float eps = (float)2.2204460492503131e-16;
    const float ax = fabsf(x), ay = fabsf(y);
    float a, c, c2;
    if (ax >= ay) {
        c = __fdiv_rn(ay, __fadd_rn(ax, eps));
        c2 = __fmul_rn(c, c);
        a = __fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(p7, c2), p5), c2), p3), c2), p1), c);
    } else {
        c = __fdiv_rn(ax, __fadd_rn(ay, eps));
        c2 = __fmul_rn(c, c);
        a = __fsub_rn(90.f, __fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fadd_rn(__fmul_rn(p7, c2), p5), c2), p3), c2), p1), c));
    }
    if (x < 0) a = __fsub_rn(180.f, a);
    if (y < 0) a = __fsub_rn(360.f, a);
    return a;
}

// sinf/cosf as glibc >= 2.28 evaluates them for 0 <= y < 120: double-precision minimax polynomials after
// a quadrant reduction (constants of the published algorithm; tests compare the CPU twin of this routine
// with the host libm over every float in [0, 2*pi]).  Doubles, no contraction.
__device__ __forceinline__ void sincosGlibc(float y, float* s_out, float* c_out) {
    const double hpi_inv = 0x1.45F306DC9C883p+23, hpi = 0x1.921FB54442D18p0;
    const double C0 = 0x1p0, C1 = -0x1.ffffffd0c621cp-2, C2 = 0x1.55553e1068f19p-5, C3 = -0x1.6c087e89a359dp-10,
                 C4 = 0x1.99343027bf8c3p-16;
    const double S1 = -0x1.555545995a603p-3, S2 = 0x1.1107605230bc4p-7, S3 = -0x1.994eb3774cf24p-13;
    double x = (double)y;
    const unsigned top12 = (__float_as_uint(y) >> 20) & 0x7ff;
    int n = 0;
    if (top12 < 0x3f4) {
        if (top12 < 0x398) { *s_out = y; *c_out = 1.0f; return; }
    } else {
        const double r = __dmul_rn(x, hpi_inv);
        n = ((int)r + 0x800000) >> 24;
        x = __dsub_rn(x, __dmul_rn((double)n, hpi));
    }
    const double x2 = __dmul_rn(x, x);
    auto polySin = [&](double xx) {
        const double x3 = __dmul_rn(xx, x2), s1 = __dadd_rn(S2, __dmul_rn(x2, S3)), x7 = __dmul_rn(x3, x2),
                     s = __dadd_rn(xx, __dmul_rn(x3, S1));
        return __dadd_rn(s, __dmul_rn(x7, s1));
    };
    auto polyCos = [&](double sg) {
        const double x4 = __dmul_rn(x2, x2), c2 = __dadd_rn(sg * C3, __dmul_rn(x2, sg * C4)),
                     c1 = __dadd_rn(sg * C0, __dmul_rn(x2, sg * C1)), x6 = __dmul_rn(x4, x2),
                     c = __dadd_rn(c1, __dmul_rn(x4, sg * C2));
        return __dadd_rn(c, __dmul_rn(x6, c2));
    };
    // sin(y) and cos(y) = "sin" of quadrants n and n + 1; a quadrant takes the sine polynomial when even and the cosine
    // polynomial when odd, so exactly one of each is evaluated and the parity of n says which result is which.
    const bool odd = (n & 1) != 0;
    const int ns = odd ? n + 1 : n, nc = odd ? n : n + 1;
    const double sgnS = ((ns & 3) == 1 || (ns & 3) == 2) ? -1.0 : 1.0;   // sign[ns & 3]
    const float ps = (float)polySin(x * sgnS), pc = (float)polyCos((nc & 2) ? -1.0 : 1.0);
    *s_out = odd ? pc : ps;
    *c_out = odd ? ps : pc;
}

constexpr int kDescWaves = 4;                         // waves per workgroup; each half-wave (32 lanes) owns one keypoint
constexpr int kRawRows = 2 * kHalfPatch + 1;          // 31
constexpr int kRawStride = 40;                        // 3 + 31 bytes -> 9 dwords, staged as five 8-byte pairs
constexpr int kBlurRows = 2 * kBriefReach + 1;        // 37
constexpr int kBlurStride = 40;                       // 3 + 37 bytes -> 10 dwords
constexpr int kPatchLds = kRawRows * kRawStride + kBlurRows * kBlurStride;   // 2596 bytes per keypoint (dword multiple)
// Patch-blur form (PB): ONE raw tile of 43 rows (v = -21 .. 21) x 44 bytes (byte t <-> u = t - 22: one spare column in front, so that the blur's
// aligned dword triples x0 - 4 .. x0 + 7 of output group g start at dword g), re-aligned to the patch when it is staged; the 37 x 37 blurred
// patch the descriptor reads is computed from it into the blurred tile (same layout as above, no misalignment).
constexpr int kPbRows = 2 * (kBriefReach + 3) + 1;    // 43
constexpr int kPbStride = 44;                         // 11 dwords
constexpr int kPbRawBytes = (kPbRows * kPbStride + 15) & ~15;               // 1904
constexpr int kPbLds = kPbRawBytes + kBlurRows * kBlurStride;               // 3384 bytes per keypoint
// The patch blur's lanes (round 5).  The rotated pattern only reaches a DISC of the 37 x 37 blurred patch: a sample (row r, column q) is the
// rounding of a point at most sqrt(338) = 18.385 from the keypoint (the largest |(x, y)| of the pattern, ORBextractor.cc:148-406), so column
// group g (columns q = 4 g - 18 .. 4 g - 15) is read at |r| <= rmax(g) = floor(1/2 + sqrt(338.5 - max(min|q| - 1/2, 0)^2)) only: 11, 15, 17, 18,
// 18, 18, 18, 16, 13, 6 -> 310 of the box's 370 (group, row) items; tests/test_tables.py derives the bounds from the pattern and sweeps every
// 0.0005 degrees for samples outside them.  The 32 lanes of a keypoint take (group, first row, rows) runs of at most 12 rows (six trips of the
// two-row blur loop; the box dealt as 10 groups x 3 runs of 13 was seven): entry = group | first row << 8 | rows << 16.  WHERE the runs of a group are cut
// matters: the 32 lanes read tile rows (first row + i) x 11 dwords + group, and a first cut (runs of 10 / 12 rows from the top) had them collide in the LDS
// banks 4.4-fold on average (SQ_LDS_BANK_CONFLICT: 514 cycles per wave, the old 10 x 3 layout: 2-fold) - which ate the instructions the disc saves.  The cuts
// below came from a search (simulated annealing over the partitions; cost = sum over the loop's LDS instructions of the largest number of lanes on one
// bank, loads of the raw tile and stores of the blurred one): 143 against 259 for the first cut and 66 for a conflict-free walk.
// Round 7: a run of n rows read n + 6 tile rows and made the horizontal sums of all of them, so the six halo rows of a run were summed twice - by the
// lane and by its neighbour in the group: 32 lanes x 18 = 576 row passes for the 370 (group, tile row) items the disc needs.  Now every item is summed by
// ONE lane (32 x 12 = 384 passes) and the halo travels between lanes by DPP, no memory: the groups are laid end to end on two VIRTUAL columns of 192
// rows, one per DPP row of 16 lanes (tools/pb_lane_search.py: groups 2 4 9 7 3 | 0 6 1 5 8).  Lane l of a DPP row sums virtual rows 12 l .. 12 l + 11 - six
// row PAIRS, two u16 sums to a register -, takes the first three pairs of lane l + 1 (row_shl:1) and blurs output rows 12 l .. 12 l + 11 out of the
// nine.  A group of n output rows takes n + 6 virtual rows (tile rows 18 - rmax .. 24 + rmax) from an even one on; the six outputs over its last rows
// mix two groups and are not stored - they are the halo, so nothing is lost: 370 + 10 of the 384 rows are used.  The groups are ordered and padded so
// that the rows a lane STORES lie in one group (c_pbRun keeps its format: one run per lane, what the lane stores) and a group lies in one DPP row, its
// stored rows ending before the last lane's row 6.  c_pbSrc says what a lane READS: its rows i < split are tile bytes offA + 44 i (group A's tail),
// the others (offB - 1024) + 44 i (the head of the group it stores to); split is even, so a row pair has one address.  Rows between two groups (padding:
// at most tile row 43, which is not staged - the bytes behind the tile, inside the keypoint's own LDS) only reach outputs that are not stored.
// entry = offA | offB << 11 | split << 23 | k0 << 27, k0 = the lane's output (0 .. 11) that is row 0 of its run.  tests/test_patch_blur_lanes.py replays
// both tables.  The search takes the layout with the fewest bank collisions of those that fit (its cost: 144; worst: 192).
static __constant__ unsigned c_pbRun[32] = {
    0x0c0102, 0x0c0d02, 0x0b1902, 0x060004, 0x0c0604, 0x0c1204, 0x071e04, 0x0a0c09, 0x031609, 0x0c0207, 0x0c0e07, 0x091a07, 0x080003, 0x0c0803, 0x0c1403,
    0x052003, 0x0c0700, 0x0b1300, 0x060006, 0x0c0606, 0x0c1206, 0x071e06, 0x0a0301, 0x0c0d01, 0x091901, 0x080005, 0x0c0805, 0x0c1405, 0x052005, 0x0c0508,
    0x0c1108, 0x031d08};
static __constant__ unsigned c_pbSrc[32] = {
    0x0621a034, 0x06322244, 0x0642a454, 0x33184664, 0x0628c118, 0x06394328, 0x0649c538, 0x112ee748, 0x063f63ec, 0x0623a074, 0x06342284, 0x0644a494,
    0x221ae6a4, 0x062b616c, 0x063be37c, 0x064c658c, 0x0629a134, 0x063a2344, 0x33188554, 0x06290120, 0x06398330, 0x064a0540, 0x11218750, 0x06320240,
    0x06428450, 0x221b2660, 0x062ba174, 0x063c2384, 0x064ca594, 0x0627e0fc, 0x0638630c, 0x0648e51c};

// The patch blur of one lane (see c_pbSrc): horizontal sums of its own six row pairs (hsums4: the arithmetic of blurRun), the next lane's first three
// by DPP, then the vertical pass of blurRun on the nine pairs W[0 .. 8] - output 2 t reads pairs t .. t + 2 and the low half of pair t + 3, output
// 2 t + 1 the high half of pair t and pairs t + 1 .. t + 3: the same dot2 taps in the same order, the same integers.  Outputs kLo <= k < kHi are stored,
// output k at dst + k * kBlurStride.  All indices are static (a run-time index into W would be scratch).  Every lane of the wave must be active.
__device__ __forceinline__ void blurPatchLanes(const uint8_t* srcA, const uint8_t* srcB, int split, uint8_t* dst, int kLo, int kHi) {
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    auto dot2 = [](unsigned pair, unsigned short w0, unsigned short w1, unsigned acc) {
        return __builtin_amdgcn_udot2(__builtin_bit_cast(u16x2, pair), u16x2{w0, w1}, acc, false);
    };
    unsigned W[9][4];
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const unsigned* r0 = (const unsigned*)((2 * k < split ? srcA : srcB) + 2 * k * kPbStride);
        const unsigned* r1 = r0 + kPbStride / 4;
        unsigned he[4], ho[4];
        hsums4(r0[0], r0[1], r0[2], he);
        hsums4(r1[0], r1[1], r1[2], ho);
#pragma unroll
        for (int j = 0; j < 4; j++) W[k][j] = (ho[j] << 16) | he[j];
    }
#pragma unroll
    for (int k = 0; k < 3; k++)
#pragma unroll
        for (int j = 0; j < 4; j++) W[6 + k][j] = (unsigned)__builtin_amdgcn_update_dpp(0, (int)W[k][j], 0x101, 0xF, 0xF, true);      // row_shl:1: lane l + 1's
#pragma unroll
    for (int t = 0; t < 6; t++) {
        unsigned e[4], o[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            e[j] = dot2(W[t + 3][j], 18, 0, dot2(W[t + 2][j], 49, 34, dot2(W[t + 1][j], 49, 55, dot2(W[t][j], 18, 34, 32768u))));
            o[j] = dot2(W[t + 3][j], 34, 18, dot2(W[t + 2][j], 55, 49, dot2(W[t + 1][j], 34, 49, dot2(W[t][j], 0, 18, 32768u))));
        }
        if (2 * t >= kLo && 2 * t < kHi) *(unsigned*)(dst + 2 * t * kBlurStride) = satPack4(e);
        if (2 * t + 1 >= kLo && 2 * t + 1 < kHi) *(unsigned*)(dst + (2 * t + 1) * kBlurStride) = satPack4(o);
    }
}

// One half-wave (32 lanes) per kept keypoint; the two keypoints of a wave share a level (selOff is even):
//   * both patches are staged in LDS with aligned dword loads that are all in flight at once: a half-wave covers
//     three patch rows per step (lane = (row % 3, dword column)), so the address of step s is one add away from
//     step 0's and the LDS destination is an immediate offset;
//   * IC_Angle: lane = patch row; the row's 31 pixels are byte-aligned with v_alignbyte and reduced with
//     v_dot4_u32_u8 against per-row weight words (u+16 inside the disc, 0 outside) — sum(u*I) = dot(I, u+16) - 16*dot(I, 1);
//   * rBRIEF: lane = 8 of the 256 test pairs; a ballot per group of 32 pairs packs 4 descriptor bytes of each keypoint.
#if defined(ORBX_DESC_STAMPS) && defined(ORBX_DESCRIBE_TU)      // (diagnostic builds stamp the kernel of k_describe.hip only)
// diagnostic build (tools/desc_spans.py): stage stamps of every wave of frame 0, s_memrealtime ticks
__device__ unsigned long long g_descStamps[6 * 1024];      // per wave: [0 .. 4] the stages in order, [5] (PB only) the end of the patch blur, between [3] and [4]
extern "C" int orbx_debug_desc_stamps(unsigned long long* out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_descStamps), sizeof(g_descStamps)); }
#define DSTAMP(i) do { const int dsW = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6); \
        if ((threadIdx.x & 63) == 0 && blockIdx.x == 0 && blockIdx.z == 0 && dsW < 1024) g_descStamps[6 * dsW + (i)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define DSTAMP(i) do {} while (0)
#endif
// PB (patch blur, large frames with few features per pixel: orbx_api.cpp): the blurred LEVELS are never made - a half-wave stages the raw
// 43 x 43 patch around its keypoint (the bordered pyramid's REFLECT_101 frame is the reflection of the level itself, which is what the
// reference's border-less clone blurs against: ORBextractor.cc:1126-1127), blurs the 37 x 37 patch the rotated pattern can reach with the same
// integer arithmetic (blurRun) and describes from that.  1920x1080 x 2000 features: 2000 x 43 x 37 = 3.2 M pixels of horizontal pass against
// 6.4 M for the whole pyramid, no 6.4-MB write + 5.5-MB sparse re-read of blurred levels per frame.
// LDS of one description workgroup (eight keypoints): the patches, then the weight words of IC_Angle's rows.
template <bool PB>
struct DescLds {
    static constexpr int kPatches = 2 * kDescWaves * (PB ? kPbLds : kPatchLds), kWtabWords = 2 * 16 * (PB ? 12 : 8);
    // The rBRIEF pattern (4 KB).  The plain form stages it behind the patches, one 16-byte load per thread, and its loop reads LDS: the eight 16-byte
    // global loads per wave of the loop were a quarter of the L1 look-ups of a kernel that is bound by them (139 -> 123 us per 512 frames; six
    // workgroups per CU instead of seven).  The patch-blur form reads the __constant__ table in its loop: with the copy its LDS passes 32 000 bytes,
    // four workgroups per CU instead of five (248 -> 260 us).  docs/history/r28_describe_chain.md.
    static constexpr int kPatternBytes = PB ? 0 : 4096;
    static constexpr int kSmem = kPatches + kPatternBytes;
    static constexpr int kWtabOff = (kSmem + 15) & ~15, kBytes = kWtabOff + 4 * kWtabWords;
    static_assert(kPatches % 16 == 0, "the pattern's float4 entries are 16-byte aligned");
};

// One workgroup = eight keypoint slots [8 chunk, 8 chunk + 8) of frame f.  smem: the patches (DescLds::kPatches bytes) and, in the plain form, the pattern; wtab: the weight words.
// One workgroup barrier (behind the weight table, a copy of the static one).  A wave whose level lies outside [levelLo, levelHi) belongs to another launch and leaves.
// A wave goes to memory three times, one trip behind the other: the kernel's arguments (the level table dl among them, by value); then everything
// whose address the arguments and the wave's first slot give - the frame's rows of the per-level counts, the level's geometry, the selection entry,
// the weight words, the plain form's copy of the pattern and the patch blur's lane tables -; then the patch gather.  (The patch-blur form's loop
// still reads the pattern behind IC_Angle: DescLds.)
template <bool PB>
__device__ __forceinline__ void describeBlock(const DescLevels& dl, int nlevels, const int (&firstSlot)[kMaxLevels],
                                              const uint8_t* __restrict__ pyr, const uint8_t* __restrict__ blur,
                                              const uint2* __restrict__ sel, int selPerFrame,
                                              const int* __restrict__ levelCount, const int* __restrict__ levelLap,
                                              Keypoint* __restrict__ outK, uint8_t* __restrict__ outD, int capacity,
                                              int* __restrict__ nOut, int* __restrict__ monoOut,
                                              Keypoint* __restrict__ outLevelK, int* __restrict__ outLevelCounts,
                                              uint8_t* smem, unsigned (*wtab)[16][PB ? 12 : 8], int fewWaves, int chunk, int f, int levelLo, int levelHi) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, half = lane >> 5, hl = lane & 31;
    DSTAMP(0);
    const int slot0 = __builtin_amdgcn_readfirstlane((chunk * kDescWaves + wave) * 2);   // wave-uniform
    const int slot = slot0 + half;
    // the selection entry: its address needs the frame and the slot only (clamped: a slot past the frame's slab reads its last entry and is idle)
    const uint2 eRaw = sel[(long long)f * selPerFrame + min(slot, selPerFrame - 1)];
    // the weight words: requested here, stored to LDS in front of the barrier (nothing before it needs them)
    constexpr int kWords = DescLds<PB>::kWtabWords;      // 384 (PB) / 256
    const unsigned* wsrc;
    if constexpr (PB) wsrc = &c_weightsPb.w[0][0][0]; else wsrc = &c_weightsPlain.w[0][0][0];
    const unsigned wA = wsrc[tid];
    unsigned wB = 0;
    if (kWords > 256 && tid < kWords - 256) wB = wsrc[256 + tid];
    // the plain form's copy of the rBRIEF pattern: one 16-byte load per thread, stored to LDS in front of the barrier
    float4* const patL = (float4*)(smem + DescLds<PB>::kPatches);
    float4 patS = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (!PB) patS = ((const float4*)c_patternF)[tid];
    unsigned pbRun = 0, pbSrc = 0;
    if constexpr (PB) { pbRun = c_pbRun[hl]; pbSrc = c_pbSrc[hl]; }
    // the level this wave belongs to: the levels' first slots ascend from 0, and those of levels >= nlevels are INT_MAX (makeDescLevels)
    int level = 0;
#pragma unroll
    for (int l = 1; l < kMaxLevels; l++) level += slot0 >= firstSlot[l] ? 1 : 0;
    // its geometry - scalar loads of the argument block - and the frame's rows of the two count arrays in batches of eight scalar dwords (a batch may
    // reach past the row, for the last frame past the arrays - kLevelCountPad -: what lies at or beyond nlevels is never used): all in flight with the
    // loads above, one wait (the empty statement: see k_describe.hip)
    const DescLevel& L = dl.lv[level];
    int selOff = L.selOff, gw = L.w, gh = L.h, pyrStride = L.pyrStride, blurStride = L.blurStride, patchSizeI = L.patchSize;
    float scale = L.scale;
    long long pyrOff = L.pyrOff, pyrFrameBytes = L.pyrFrameBytes, blurOff = L.blurOff, blurFrameBytes = L.blurFrameBytes;
    // (read through the constant address space - the quad-tree's launch wrote the counts, nothing of this launch does -, which is what makes these
    //  scalar loads whatever stands in front of them)
    typedef __attribute__((address_space(4))) const int* ConstInts;
    const ConstInts cRow = (ConstInts)(levelCount + f * nlevels), lRow = (ConstInts)(levelLap + f * nlevels);
    int c[8], lp[8];
#pragma unroll
    for (int k = 0; k < 8; k++) { c[k] = cRow[k]; lp[k] = lRow[k]; }
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : : "s"(c[0]), "s"(c[1]), "s"(c[2]), "s"(c[3]), "s"(c[4]), "s"(c[5]), "s"(c[6]), "s"(c[7]), "s"(lp[0]), "s"(lp[1]), "s"(lp[2]),
                 "s"(lp[3]), "s"(lp[4]), "s"(lp[5]), "s"(lp[6]), "s"(lp[7]), "s"(selOff), "s"(gw), "s"(gh), "s"(pyrStride), "s"(blurStride),
                 "s"(patchSizeI), "s"(scale), "s"(pyrOff), "s"(pyrFrameBytes), "s"(blurOff), "s"(blurFrameBytes));
#endif
    const uint8_t* pyrL = pyr + pyrOff + (long long)f * pyrFrameBytes;      // wave-uniform bases:
    const uint8_t* blurL = blur + blurOff + (long long)f * blurFrameBytes;   // lanes add 32-bit offsets
    // totals of this frame and the sums in front of the wave's level: scalar arithmetic with static indices
    int total = 0, totalLap = 0, seqBase = 0, lapBase = 0, levelN = 0;
    auto sumBatch = [&](int l0) {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int l = l0 + k, cl = l < nlevels ? c[k] : 0, ll = l < nlevels ? lp[k] : 0;
            if (l == level) { seqBase = total; lapBase = totalLap; levelN = cl; }
            total += cl;
            totalLap += ll;
        }
    };
    // Two forms of the sums, by the launch (wave-uniform):
    //  * few waves on the chip (small batches: the wave's own latency is the launch's): lane l < nlevels loads level l's count and lapping count, running
    //    sums by four DPP steps inside the first row of 16 lanes (nlevels <= kMaxLevels = 16), the wave's sums by v_readlane - some twenty vector
    //    instructions where the scalar form below takes a hundred scalar ones, one behind the other (one frame per call: 35.5 against 36.2 us);
    //  * a full chip: the scalar form - its instructions hide behind the other waves, while two more vector loads per wave cost L1 look-ups, which
    //    is what this kernel is short of.
    if (fewWaves) {
        int myCnt = 0, myLap = 0;
        if (lane < nlevels) { myCnt = levelCount[f * nlevels + lane]; myLap = levelLap[f * nlevels + lane]; }
        int incC = myCnt, incL = myLap;
        static_assert(kMaxLevels == 16, "the scan below covers one DPP row of 16 lanes");
        incC += __builtin_amdgcn_update_dpp(0, incC, 0x111, 0xF, 0xF, true); incL += __builtin_amdgcn_update_dpp(0, incL, 0x111, 0xF, 0xF, true);      // row_shr:1
        incC += __builtin_amdgcn_update_dpp(0, incC, 0x112, 0xF, 0xF, true); incL += __builtin_amdgcn_update_dpp(0, incL, 0x112, 0xF, 0xF, true);      // row_shr:2
        incC += __builtin_amdgcn_update_dpp(0, incC, 0x114, 0xF, 0xF, true); incL += __builtin_amdgcn_update_dpp(0, incL, 0x114, 0xF, 0xF, true);      // row_shr:4
        incC += __builtin_amdgcn_update_dpp(0, incC, 0x118, 0xF, 0xF, true); incL += __builtin_amdgcn_update_dpp(0, incL, 0x118, 0xF, 0xF, true);      // row_shr:8
        total = __builtin_amdgcn_readlane(incC, kMaxLevels - 1); totalLap = __builtin_amdgcn_readlane(incL, kMaxLevels - 1);      // (lanes >= nlevels add 0)
        seqBase = __builtin_amdgcn_readlane(incC - myCnt, level); lapBase = __builtin_amdgcn_readlane(incL - myLap, level);
        levelN = __builtin_amdgcn_readlane(myCnt, level);
    } else {
    sumBatch(0);
    static_assert(kMaxLevels == 16 && kLevelCountPad >= 16, "two batches of eight cover every level");
    if (nlevels > 8) {
#pragma unroll
        for (int k = 0; k < 8; k++) { c[k] = cRow[8 + k]; lp[k] = lRow[8 + k]; }
        sumBatch(8);
    }
    }
    if (slot0 == 0 && outLevelCounts && lane < nlevels) outLevelCounts[f * nlevels + lane] = levelCount[f * nlevels + lane];
    if (slot0 == 0 && lane == 0) { nOut[f] = total; monoOut[f] = total - totalLap; }      // monoIndex after the loop (:1161)
    const bool mine = level >= levelLo && level < levelHi;      // (wave-uniform: the other launch of a blur split by level describes the other levels)
    const int i = slot - selOff;
    const bool active = mine && slot < selPerFrame && i < levelN;
    (&wtab[0][0][0])[tid] = wA;
    if (kWords > 256 && tid < kWords - 256) (&wtab[0][0][0])[256 + tid] = wB;
    if constexpr (!PB) patL[tid] = patS;
    const uint2 e = active ? eRaw : make_uint2(0u, 0u);
    __syncthreads();
    if (!mine) return;
    if (__ballot(active) == 0) return;
    DSTAMP(1);
    if constexpr (PB) asm volatile("" : "+v"(pbRun), "+v"(pbSrc));      // (keeps the two loads at the top, where they are written)
    int kx = e.x & 0xffff, ky = e.x >> 16;      // (orbx_device.hpp: the selection entry)
    const float response = (float)(e.y >> 24);
    // the quad-tree only emits points of the FAST rectangle; clamp anyway so a corrupted entry (or an idle half)
    // can never turn into an out-of-bounds gather
    kx = min(max(kx, kEdge), gw - kEdge - 1);
    ky = min(max(ky, kEdge), gh - kEdge - 1);

    DSTAMP(2);
    int m10 = 0, m01 = 0;
    uint8_t* blurT;
    int blurMis;
    if constexpr (PB) {
        // ---- stage the raw 43 x 44 tile, re-aligned: 8 lanes per tile row (6 load an 8-byte pair of source dwords - 4-byte aligned: one
        //      global_load_dwordx2 -, 11 re-aligned dwords stored), four rows per step: 11 load instructions per wave (dword loads: 22; the gather is bound
        //      by the L1's look-up rate: profiles/r04_l1_l2_counters.md) ----
        uint8_t* rawT = smem + (wave * 2 + half) * kPbLds;
        blurT = rawT + kPbRawBytes;
        blurMis = 0;
        constexpr int kSteps = (kPbRows + 3) / 4;            // 11
        const int l8 = hl & 7, rsub = hl >> 3;
        const int col0 = kPadL + kx - (kBriefReach + 4), mis = col0 & 3;
        const int rOff = __mul24(kEdge + ky - (kBriefReach + 3) + rsub, pyrStride) + (col0 - mis) + 8 * l8;
        uint2 wr[kSteps];
#pragma unroll
        for (int s = 0; s < kSteps; s++) {
            wr[s] = uint2{0u, 0u};
            if (l8 < 6 && rsub + 4 * s < kPbRows) __builtin_memcpy(&wr[s], pyrL + ((unsigned)rOff + (unsigned)(4 * s * pyrStride)), 8);
        }
        uint8_t* rdst = rawT + rsub * kPbStride + 8 * l8;
#pragma unroll
        for (int s = 0; s < kSteps; s++) {
            const unsigned nxt = (unsigned)__builtin_amdgcn_update_dpp(0, (int)wr[s].x, 0x101, 0xF, 0xF, false);      // row_shl:1: the next pair's first dword (same tile row for l8 < 5)
            const unsigned v0 = __builtin_amdgcn_alignbyte(wr[s].y, wr[s].x, (unsigned)mis), v1 = __builtin_amdgcn_alignbyte(nxt, wr[s].y, (unsigned)mis);
            if (l8 < 6 && rsub + 4 * s < kPbRows) {
                *(unsigned*)(rdst + 4 * s * kPbStride) = v0;
                if (l8 < 5) *(unsigned*)(rdst + 4 * s * kPbStride + 4) = v1;      // (a tile row is 11 dwords: the sixth pair stores its first only)
            }
        }
        asm volatile("" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        asm volatile("" ::: "memory");
        DSTAMP(3);
        // ---- IC_Angle (:75-102): lane = patch row v = hl - 15 = tile row hl + 6; the weight words know the layout (u = t - 22) ----
        if (hl < kRawRows) {
            const int v = hl - kHalfPatch, a = v < 0 ? -v : v;
            const unsigned* row = (const unsigned*)(rawT + (hl + 6) * kPbStride);
            unsigned s1 = 0, s0 = 0;
#pragma unroll
            for (int j = 1; j <= 9; j++) {          // bytes 7 .. 37 lie in dwords 1 .. 9
                const unsigned px = row[j];
                s1 = __builtin_amdgcn_udot4(px, wtab[0][a][j], s1, false);
                s0 = __builtin_amdgcn_udot4(px, wtab[1][a][j], s0, false);
            }
            m10 = (int)s1 - 16 * (int)s0;     // sum u*I
            m01 = v * (int)s0;                // v * sum I
        }
        // ---- the 7x7 blur of the part of the 37 x 37 patch the rotated pattern can reach (:1126-1127): the lane stores the (column group, run of
        //      rows) of c_pbRun and sums the tile rows of c_pbSrc; output row o reads tile rows o .. o + 6 ----
        {
            const int g4 = (int)(pbRun & 0xff), o0 = (int)((pbRun >> 8) & 0xff), nOut = (int)(pbRun >> 16);
            const int k0 = (int)(pbSrc >> 27), split = (int)((pbSrc >> 23) & 15);
            blurPatchLanes(rawT + (pbSrc & 0x7ff), rawT + ((int)((pbSrc >> 11) & 0xfff) - 1024), split,
                           blurT + (o0 - k0) * kBlurStride + 4 * g4, k0, k0 + nOut);
        }
        DSTAMP(5);
        asm volatile("" ::: "memory");
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        asm volatile("" ::: "memory");
    } else {
    // ---- stage both patches: raw level rows/cols +-15 (IC_Angle), blurred level rows/cols +-18 (rBRIEF) ----
    uint8_t* rawT = smem + (wave * 2 + half) * kPatchLds;
    blurT = rawT + kRawRows * kRawStride;
    const int rawCol0 = kPadL + kx - kHalfPatch, rawMis = rawCol0 & 3;
    const int blurCol0 = kx - kBriefReach;
    blurMis = blurCol0 & 3;
    {
        // 8-byte loads (4-byte aligned: one global_load_dwordx2 each): a half-wave covers SIX tile rows per step (lane = (row % 6, dword pair)), 6 + 7
        // load instructions per wave instead of 11 + 13 with dword loads - the patch gather is bound by the L1's rate of line look-ups (0.9 per cycle
        // and CU in this kernel: profiles/r04_l1_l2_counters.md), and a wave instruction's look-ups go with its 16-lane groups x the lines each touches
        constexpr int kPairs = 5, kRowsPerStep = 6;
        static_assert(kRawStride == 8 * kPairs && kBlurStride == 8 * kPairs, "tile rows are five 8-byte pairs");
        constexpr int kRawSteps = (kRawRows + kRowsPerStep - 1) / kRowsPerStep, kBlurSteps = (kBlurRows + kRowsPerStep - 1) / kRowsPerStep;   // 6, 7
        const int rr = (hl * 52) >> 8, rc = hl - rr * kPairs;     // hl / 5 for hl < 32: lanes 0..29: row (mod 6) and dword pair of both tiles
        const bool stLane = hl < kRowsPerStep * kPairs;
        // (every aligned dword that starts inside a level's padded row lies inside it: strides are multiples of 64; the pairs reach at most 9 bytes
        //  past the raw patch - inside the 19-px border - and 3 + 3 bytes past the blurred one - inside the row, kx <= w - 20)
        const int rOff = __mul24(kEdge + ky - kHalfPatch + rr, pyrStride) + (rawCol0 - rawMis) + 8 * rc;   // 24-bit: full-rate multiplies
        const int bOff = __mul24(ky - kBriefReach + rr, blurStride) + (blurCol0 - blurMis) + 8 * rc;
        uint2 wr[kRawSteps], wb[kBlurSteps];
#pragma unroll
        for (int s = 0; s < kRawSteps; s++) {
            wr[s] = uint2{0u, 0u};
            if (stLane && rr + kRowsPerStep * s < kRawRows) __builtin_memcpy(&wr[s], pyrL + ((unsigned)rOff + (unsigned)(kRowsPerStep * s * pyrStride)), 8);   // uniform base + u32 offset
        }
#pragma unroll
        for (int s = 0; s < kBlurSteps; s++) {
            wb[s] = uint2{0u, 0u};
            if (stLane && rr + kRowsPerStep * s < kBlurRows) __builtin_memcpy(&wb[s], blurL + ((unsigned)bOff + (unsigned)(kRowsPerStep * s * blurStride)), 8);
        }
        uint8_t* rdst = rawT + rr * kRawStride + 8 * rc;
        uint8_t* bdst = blurT + rr * kBlurStride + 8 * rc;
#pragma unroll
        for (int s = 0; s < kRawSteps; s++)
            if (stLane && rr + kRowsPerStep * s < kRawRows) *(uint2*)(rdst + kRowsPerStep * s * kRawStride) = wr[s];
#pragma unroll
        for (int s = 0; s < kBlurSteps; s++)
            if (stLane && rr + kRowsPerStep * s < kBlurRows) *(uint2*)(bdst + kRowsPerStep * s * kBlurStride) = wb[s];
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    asm volatile("" ::: "memory");

    DSTAMP(3);
    // ---- IC_Angle (:75-102): integer moments over the radius-15 disc of the unblurred level ----
    if (hl < kRawRows) {
        const int v = hl - kHalfPatch, a = v < 0 ? -v : v;
        const unsigned* row = (const unsigned*)(rawT + hl * kRawStride);
        unsigned d[9];
#pragma unroll
        for (int j = 0; j < 9; j++) d[j] = row[j];
        unsigned s1 = 0, s0 = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            // bytes u = 4j-15 .. 4j-12 of the row: shift the dword pair by the patch's misalignment
            const unsigned px = __builtin_amdgcn_alignbyte(d[j + 1], d[j], (unsigned)rawMis);   // the shift comes from a register
            s1 = __builtin_amdgcn_udot4(px, wtab[0][a][j], s1, false);
            s0 = __builtin_amdgcn_udot4(px, wtab[1][a][j], s0, false);
        }
        m10 = (int)s1 - 16 * (int)s0;     // sum u*I
        m01 = v * (int)s0;                // v * sum I
    }
    }
    // reduce inside the half-wave: four DPP steps cover a row of 16 lanes, one cross-lane exchange joins the two rows
    auto rowSum = [](int v) {
        v += __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);     // quad_perm [1,0,3,2]
        v += __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);     // quad_perm [2,3,0,1]
        v += __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, false);    // row_half_mirror
        v += __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, false);    // row_mirror
        return v;
    };
    m10 = rowSum(m10); m01 = rowSum(m01);
    m10 += __shfl_xor(m10, 16);
    m01 += __shfl_xor(m01, 16);
    const float angle = fastAtan2Deg((float)m01, (float)m10);

    // ---- computeOrbDescriptor (:106-145) on the blurred level ----
    const float factorPI = (float)(3.1415926535897932384626433832795 / 180.0);   // (float)(CV_PI/180.f)
    float a, b;
    sincosGlibc(__fmul_rn(angle, factorPI), &b, &a);
    // (int)rintf(v) is v_rndne_f32 + v_cvt_i32_f32.  One addition does both: v + 1.5 * 2^23 lies in [2^23, 2^24), where the spacing of binary32 is 1, so
    // the addition itself rounds v to an integer, to nearest and ties to even as rintf does (|v| <= 18.4 here, any |v| <= 2^22 would do), and the bits
    // of the sum are 0x4B400000 + rint(v).  v_mad_u32_u24 multiplies the low 24 bits of the row's sum, 0x400000 + r, by the tile's stride and adds the
    // column's: 40 r + q + kRintOff, and the lane's base address carries - kRintOff (LDS addresses are 32 bits and wrap): four instructions per sample
    // instead of six.  tests/test_rint_by_addition.py compares the two roundings over every float of the range.
    constexpr float kRintMagic = 12582912.f;                                          // 1.5 * 2^23 = 0x4B400000
    constexpr unsigned kRintOff = kBlurStride * 0x400000u + 0x4B400000u;
    typedef __attribute__((address_space(3))) const uint8_t* LdsBytes;
    const unsigned bc = (unsigned)(uintptr_t)(LdsBytes)(blurT + kBriefReach * kBlurStride + blurMis + kBriefReach) - kRintOff;
    unsigned myWord = 0;                   // lane hl < 8 ends up holding descriptor bytes 4*hl .. 4*hl+3 of its keypoint
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int p = hl + 32 * j;        // test pair index; bit (p & 7) of descriptor byte (p >> 3)
        float4 pt;
        if constexpr (PB) pt = ((const float4*)c_patternF)[p]; else pt = patL[p];
        const float x0 = pt.x, y0 = pt.y, x1 = pt.z, y1 = pt.w;
        const unsigned r0 = __float_as_uint(__fadd_rn(__fadd_rn(__fmul_rn(x0, b), __fmul_rn(y0, a)), kRintMagic));
        const unsigned q0 = __float_as_uint(__fadd_rn(__fsub_rn(__fmul_rn(x0, a), __fmul_rn(y0, b)), kRintMagic));
        const unsigned r1 = __float_as_uint(__fadd_rn(__fadd_rn(__fmul_rn(x1, b), __fmul_rn(y1, a)), kRintMagic));
        const unsigned q1 = __float_as_uint(__fadd_rn(__fsub_rn(__fmul_rn(x1, a), __fmul_rn(y1, b)), kRintMagic));
        const int t0 = *(LdsBytes)(uintptr_t)(bc + __umul24(r0, kBlurStride) + q0), t1 = *(LdsBytes)(uintptr_t)(bc + __umul24(r1, kBlurStride) + q1);
        const unsigned long long m = __ballot(t0 < t1);
        const unsigned mine = half ? (unsigned)(m >> 32) : (unsigned)m;
        myWord = hl == j ? mine : myWord;
    }
    DSTAMP(4);
    if (!active) return;

    // ---- placement (:1137-1158): non-lapping keys fill from the front, lapping keys from the back ----
    const int lapRank = (int)(e.y & 0x7fffff), isLap = (int)((e.y >> 23) & 1);
    const int lapBefore = lapBase + lapRank;
    const int monoBefore = (seqBase - lapBase) + (i - lapRank);
    const int at = isLap ? total - 1 - lapBefore : monoBefore;
    float ox = (float)kx, oy = (float)ky;
    if (level != 0) { ox = __fmul_rn(ox, scale); oy = __fmul_rn(oy, scale); }
    const float patchSize = (float)patchSizeI;
    if (at < capacity) {
        if (hl == 0) {
            Keypoint k;
            k.x = ox; k.y = oy; k.size = patchSize; k.angle = angle; k.response = response;
            k.octave = level; k.class_id = -1;
            outK[(long long)f * capacity + at] = k;
        }
        if (hl < 8) ((unsigned*)(outD + ((long long)f * capacity + at) * 32))[hl] = myWord;
    }
    if (outLevelK && hl == 0 && seqBase + i < capacity) {
        Keypoint k;
        k.x = (float)kx; k.y = (float)ky; k.size = patchSize; k.angle = angle; k.response = response;
        k.octave = level; k.class_id = -1;
        outLevelK[(long long)f * capacity + seqBase + i] = k;
    }
}


}  // namespace orbx
