// k_stereo_fisheye.hip - Frame::ComputeStereoFishEyeMatches (reference src/Frame.cc:1139-1179; called by the two-camera Frame constructor,
// :1108): cv::BFMatcher(NORM_HAMMING).knnMatch(left lapping rows, right lapping rows, 2), Lowe's ratio 0.7, and for every row that passes it
// KannalaBrandt8::TriangulateMatches(mpCamera2, mvKeys[i], mvKeysRight[j], mRlr, mtlr, sigma1, sigma2) > 0.0001f (k_camera_kb8_unproject.hpp).
// The fisheye counterpart of k_stereo.hip (Frame::ComputeStereoMatches).  The definitions (include/orbx.h):
//   * the 2-NN of a left row over the right lapping rows in increasing index: [0] is the FIRST index of the smallest distance, [1] the smallest
//     of the remaining distances, which may equal [0]'s (OpenCV's batchDistance insertion: strict compares);
//   * the ratio test (float)d0 < (float)d1 * 0.7 in double is 10 * d0 < 7 * d1 on every pair of 0 .. 256; fewer than two right rows: no match;
//   * mvLeftToRightMatch, mvDepth and mvStereo3Dpoints are per left row; mvRightToLeftMatch[j] is overwritten by every accepted left row
//     that chose j in increasing left index, so it ends as the LARGEST of them: one atomicMax on a row of -1.
// Rig r is batch frames 2r (left) and 2r + 1 (right).  Two launches on the stream:
//   k_stereo_fisheye_init   the right eye's row of d_right_to_left to -1 and the rig's two counters to 0 (the atomics below need them);
//   k_stereo_fisheye        a workgroup of kSfThreads threads per (rig, tile of kSfThreads left LAPPING rows), in two stages.
//   STAGE A, brute force: a lane holds one left descriptor in 8 registers.  The right lapping descriptors stream through LDS in chunks of
//   kSfChunk (4 KB; one size for every capacity: there is no capacity bound); thread t carries descriptor t of the next chunk in registers
//   while the current one is scanned, so a chunk costs two barriers and no exposed load.  Every lane reads the same LDS address (a
//   broadcast); a candidate costs 8 xor, 8 popcount-adds, a compare, three selects and a minimum (sfInsert).
//   STAGE B, geometry: the rows that passed the ratio test are COMPACTED - ballot, wave counts through LDS, prefix - into dense lanes:
//   kb8TriangulateMatches is ~5400 instructions without early returns and a wave a quarter full costs what a full one does, so a tile
//   whose survivors fit 64 lanes runs it in one wave and the other skips it.  A dense lane unprojects both keypoints, triangulates, writes
//   its left row and takes the atomicMax on the right row.
// Every entry of the left eye's rows is written: a lapping row by the lane that holds it (stage A: rejected by the ratio; stage B: the
// geometry's result), a row outside [monoLeft, Nleft) by the workgroup whose tile covers its INDEX.
// The statement is sfRig, sfInsert, sfScanChunk, sfRatioPass and sfGeometry; the kernel is those around its barriers.  The CPU suite compiles
// them for the HOST (tests/cpp/stereo_fisheye_host_check.cpp behind tests/cpp/host_shim/stereo_fisheye_shim.h, which defines ORBX_HOST_ROW:
// LDS is memory there and the kernel wrappers are left out).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orbx_lds_pollute.hpp"
#include "k_camera_kb8_unproject.hpp"
#include "k_lds_vec.hpp"
#include "k_match_helpers.hpp"
#include "orbx_device.hpp"
#include "orbx_params.hpp"

namespace orbx {

constexpr int kSfThreads = 128;                           // left lapping rows of a tile, one per thread: 1302 rows are 11 workgroups of two waves
constexpr int kSfWaves = kSfThreads / 64;
constexpr int kSfChunk = kSfThreads;                      // right descriptors per LDS chunk: thread t stages descriptor t
constexpr int kSfNoDistance = 512;                        // above every Hamming distance of 256 bits

// Nleft, Nright, monoLeft, monoRight of the rig whose left eye is batch frame fL, each clamped: N into [0, capacity], mono into [0, N] (the
// reference would index out of bounds)
struct SfRig { int nL, nR, monoL, monoR; };
__device__ __forceinline__ SfRig sfRig(const int* __restrict__ nOut, const int* __restrict__ monoOut, long long fL, int cap) {
    SfRig g;
    g.nL = max(0, min(nOut[fL], cap)); g.nR = max(0, min(nOut[fL + 1], cap));
    g.monoL = max(0, min(monoOut[fL], g.nL)); g.monoR = max(0, min(monoOut[fL + 1], g.nR));
    return g;
}

// knnMatch(..., 2) of one left row: matches[0].distance, matches[0].trainIdx + monoRight, matches[1].distance
struct SfBest { int d0, i0, d1; };
// the insertion of the candidate at RAW right index j: it enters only if strictly smaller than the second, in front only if strictly smaller
// than the first
__device__ __forceinline__ void sfInsert(SfBest& b, int d, int j) {
    const bool front = d < b.d0;
    b.d1 = front ? b.d0 : min(b.d1, d);
    b.i0 = front ? j : b.i0;
    b.d0 = front ? d : b.d0;
}
// n staged right descriptors, the first of them RAW right index `first`, against the left descriptor (a, b)
__device__ __forceinline__ void sfScanChunk(const LdsU4& a, const LdsU4& b, const ORBX_LDS LdsU4* chunk, int n, int first, SfBest& best) {
    for (int t = 0; t < n; t++) {
        const LdsU4 x = chunk[2 * t], y = chunk[2 * t + 1];
        sfInsert(best, hamming256(a, b, x, y), first + t);
    }
}
// (*it).size() >= 2 && (*it)[0].distance < (*it)[1].distance * 0.7 (:1164), over nLap right lapping rows
__device__ __forceinline__ bool sfRatioPass(const SfBest& b, int nLap) { return nLap >= 2 && 10 * b.d0 < 7 * b.d1; }

// :1168-1170 of a row that passed the ratio test: depth = TriangulateMatches on the two RAW keypoints; true: depth > 0.0001f (NaN and -1
// reject, +inf accepts).  sGate[l] = 5.991 * (double)mvLevelSigma2[l], an octave outside the table clamped into it.
__device__ __forceinline__ bool sfGeometry(const StereoFisheyeParams& p, const double* sGate, const Keypoint& K1, const Keypoint& K2,
                                           float& depth, float (&x3D)[3]) {
    float k1[8], k2[8];
#pragma unroll
    for (int a = 0; a < 8; a++) { k1[a] = p.cam[0][a]; k2[a] = p.cam[1][a]; }
    Kb8Relative q;
    kb8RelativeFrom(p.R12, p.t12, q);
    const float u1 = K1.x, v1 = K1.y, u2 = K2.x, v2 = K2.y;
    float r1x, r1y, r2x, r2y;
    kb8Unproject(k1, u1, v1, r1x, r1y);
    kb8Unproject(k2, u2, v2, r2x, r2y);
    int why;
    depth = kb8TriangulateMatches(k1, k2, r1x, r1y, r2x, r2y, u1, v1, u2, v2, q, sGate[min(max(K1.octave, 0), p.nlevels - 1)],
                                  sGate[min(max(K2.octave, 0), p.nlevels - 1)], x3D, why);
    return depth > 0.0001f;
}

#ifndef ORBX_HOST_ROW

// Diagnostics, OFF unless orbx_debug_stereo_fisheye_enable(1) was called: a launch then zeroes the counter and its workgroups add their
// kb8TriangulateMatches calls.  A production launch pays nothing for it.
__device__ int g_stereoFisheyeStats[1];
static bool g_stereoFisheyeStatsOn = false;
extern "C" int orbx_debug_stereo_fisheye_enable(int on) { g_stereoFisheyeStatsOn = on != 0; return 0; }
extern "C" int orbx_debug_stereo_fisheye_stats(int* out1) {
    if (!out1) return -2;                                  // ORBX_ERR_BAD_ARGUMENT
    if (hipDeviceSynchronize() != hipSuccess) return -6;   // (the handle's stream may be a non-blocking one: the copy below would not wait for it)
    return hipMemcpyFromSymbol(out1, HIP_SYMBOL(g_stereoFisheyeStats), sizeof(int)) == hipSuccess ? 0 : -6;      // ORBX_ERR_HIP
}

// grid: (ceil(capacity / 256), n_rigs folded into x: blockIdx.x = q * groups + group)
__global__ __launch_bounds__(256) void k_stereo_fisheye_init(StereoFisheyeParams p, int groups, int* __restrict__ r2l, int* __restrict__ nMatches,
                                                             int* __restrict__ nDescMatches) {
    const int q = blockIdx.x / groups, i = (blockIdx.x - q * groups) * 256 + threadIdx.x;
    const long long fR = 2 * (p.rigFirst + (long long)q * p.rigStep) + 1;
    if (i < p.capacity) r2l[fR * p.capacity + i] = -1;
    if (i == 0) { nMatches[q] = 0; if (nDescMatches) nDescMatches[q] = 0; }
}

// grid: n_rigs * p.tiles (blockIdx.x = q * p.tiles + tile); kSfThreads threads
__global__ __launch_bounds__(kSfThreads) void k_stereo_fisheye(const Keypoint* __restrict__ kps, const uint8_t* __restrict__ desc,
                                                               const int* __restrict__ nOut, const int* __restrict__ monoOut,
                                                               StereoFisheyeParams p, int* __restrict__ l2r, int* __restrict__ r2l,
                                                               float* __restrict__ depth, float* __restrict__ x3d, int* __restrict__ nMatches,
                                                               int* __restrict__ nDescMatches) {
    __shared__ LdsU4 sChunkMem[2 * kSfChunk];
    __shared__ double sGate[kMaxLevels];
    __shared__ int sWave[kSfWaves], sRow[kSfThreads], sCand[kSfThreads];
    ORBX_LDS LdsU4* sChunk = (ORBX_LDS LdsU4*)sChunkMem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, cap = p.capacity;
    const int q = blockIdx.x / p.tiles, tile = blockIdx.x - q * p.tiles;
    const long long fL = 2 * (p.rigFirst + (long long)q * p.rigStep), fR = fL + 1;
    const SfRig g = sfRig(nOut, monoOut, fL, cap);
    int* l2rRow = l2r + fL * cap;
    float *depthRow = depth + fL * cap, *x3dRow = x3d + fL * cap * 3;
    auto writeLeft = [&](int i, int j, float z, float x, float y, float w) {
        l2rRow[i] = j; depthRow[i] = z;
        x3dRow[3LL * i] = x; x3dRow[3LL * i + 1] = y; x3dRow[3LL * i + 2] = w;
    };
    // the left rows outside the lapping area whose index falls in this tile (:1147-1151)
    const int outside = tile * kSfThreads + tid;
    if (outside < cap && (outside < g.monoL || outside >= g.nL)) writeLeft(outside, -1, -1.0f, 0.0f, 0.0f, 0.0f);
    const int tileFirst = g.monoL + tile * kSfThreads;                  // (monoL <= capacity and tile * kSfThreads < capacity + kSfThreads)
    if (tileFirst >= g.nL) return;                                      // no lapping row in this tile (the whole workgroup leaves)
    const int i = tileFirst + tid, nLap = g.nR - g.monoR;
    const bool active = i < g.nL;
    if (tid < kMaxLevels) sGate[tid] = 5.991 * (double)p.sigma2[min(tid, p.nlevels - 1)];      // the float promoted, the product in double
    const LdsU4 *descL = (const LdsU4*)(desc + fL * cap * 32), *descR = (const LdsU4*)(desc + fR * cap * 32);
    const LdsU4 zero = {0u, 0u, 0u, 0u};
    const LdsU4 a = active ? descL[2LL * i] : zero, b = active ? descL[2LL * i + 1] : zero;

    // ---- stage A ----
    SfBest best{kSfNoDistance, -1, kSfNoDistance};
    LdsU4 n0 = zero, n1 = zero;
    if (g.monoR + tid < g.nR) { n0 = descR[2LL * (g.monoR + tid)]; n1 = descR[2LL * (g.monoR + tid) + 1]; }
    for (int c = 0; c < nLap; c += kSfChunk) {
        __syncthreads();                                                // the chunk before this one has been scanned
        sChunk[2 * tid] = n0; sChunk[2 * tid + 1] = n1;
        __syncthreads();
        const int j = g.monoR + c + kSfChunk + tid;                     // this thread's descriptor of the next chunk, in flight during the scan
        if (j < g.nR) { n0 = descR[2LL * j]; n1 = descR[2LL * j + 1]; }
        if (active) sfScanChunk(a, b, sChunk, min(kSfChunk, nLap - c), g.monoR + c, best);
    }
    const bool pass = active && sfRatioPass(best, nLap);
    if (active && !pass) writeLeft(i, -1, -1.0f, 0.0f, 0.0f, 0.0f);

    // ---- stage B: the rows that passed, compacted into dense lanes ----
    const unsigned long long vote = __ballot(pass);
    if (lane == 0) sWave[wave] = __popcll(vote);
    __syncthreads();                                                    // (also: sGate is written)
    int before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kSfWaves; w++) { const int n = sWave[w]; all += n; before += w < wave ? n : 0; }
    if (pass) {
        const int slot = before + __popcll(vote & ((1ull << lane) - 1ull));
        sRow[slot] = tid; sCand[slot] = best.i0;
    }
    __syncthreads();
    bool ok = false;
    if (tid < all) {                                                    // (a wave past the survivors skips the geometry whole)
        const int row = tileFirst + sRow[tid], j = sCand[tid];
        float z, x[3];
        ok = sfGeometry(p, sGate, kps[fL * cap + row], kps[fR * cap + j], z, x);
        if (ok) {                                                       // :1171-1175
            writeLeft(row, j, z, x[0], x[1], x[2]);
            atomicMax(&r2l[fR * cap + j], row);
        } else {
            writeLeft(row, -1, -1.0f, 0.0f, 0.0f, 0.0f);
        }
    }
    const int accepted = __popcll(__ballot(ok));
    if (lane == 0 && accepted) atomicAdd(&nMatches[q], accepted);       // nMatches
    if (tid == 0 && all) {
        if (nDescMatches) atomicAdd(&nDescMatches[q], all);             // descMatches
        if (p.countStats) atomicAdd(&g_stereoFisheyeStats[0], all);
    }
}

int stereoFisheyeTiles(int capacity) { return (capacity + kSfThreads - 1) / kSfThreads; }

void launchStereoFisheye(hipStream_t st, const Keypoint* kps, const uint8_t* desc, const int* nOut, const int* monoOut,
                         const StereoFisheyeParams& params, int* l2r, int* r2l, float* depth, float* x3d, int* nMatches, int* nDescMatches,
                         int nRigs, LdsPolluter pollute) {
    StereoFisheyeParams p = params;
    p.tiles = stereoFisheyeTiles(p.capacity);
    p.countStats = g_stereoFisheyeStatsOn ? 1 : 0;
    void* stats = nullptr;
    if (p.countStats && hipGetSymbolAddress(&stats, HIP_SYMBOL(g_stereoFisheyeStats)) == hipSuccess) (void)hipMemsetAsync(stats, 0, sizeof(int), st);
    const int groups = (p.capacity + 255) / 256;
    pollute(st);
    hipLaunchKernelGGL(k_stereo_fisheye_init, dim3((unsigned)(nRigs * groups)), dim3(256), 0, st, p, groups, r2l, nMatches, nDescMatches);
    pollute(st);
    hipLaunchKernelGGL(k_stereo_fisheye, dim3((unsigned)(nRigs * p.tiles)), dim3(kSfThreads), 0, st, kps, desc, nOut, monoOut, p, l2r, r2l, depth,
                       x3d, nMatches, nDescMatches);
}

#endif  // ORBX_HOST_ROW

}  // namespace orbx
