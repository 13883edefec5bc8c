// k_project_sim3.hip — loop closing's matcher: the two Sim3 overloads of ORBmatcher::SearchByProjection
//   projection 0: SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming)                           reference src/ORBmatcher.cc:473-586
//   projection 1: SearchByProjection(pKF, Scw, vpPoints, vpPointsKFs, vpMatched, vpMatchedKF, th, ratioHamming) reference src/ORBmatcher.cc:588-704
// (callers: src/LoopClosing.cc:730, :755, :1008) for keyframes with NLeft == -1 and the Pinhole model.
// Up to the cell window the two are Fuse's Sim3 overload: the front end (projectIntoKeyFrame), the keyframe's tables with their clamps
// (keyFrameView; keyFrameSlotsInGrid alone in the settling kernel) and the visit of the window (keyFrameVisitArea) are
// k_keyframe_project.hpp's, shared with k_fuse.hip and k_fuse_two_eyes.hip; sim3Scan below is this search's body of the visit.  What Fuse does
// not have: a match CLOSES its keypoint for every later MapPoint of the list (vpMatched[bestIdx] = pMP at :579 / :696 is read back at
// :558 / :675), so the requests of one call are a sequential chain.  Two kernels:
//   k_sim3_window  one thread per (pair, MapPoint), grid over the whole GPU as k_fuse: the front end, then the window from L2.  Of the
//                  candidates that pass the STATIC tests (level filter, not occupied on entry, distance within the bound) it keeps the
//                  kSim3Top smallest keys (distance << 16 | CSR slot) and the count of all of them, and writes the exit codes 0 .. 5.
//                  (The reference takes the best open candidate and THEN tests the bound; the best is the minimum, so it passes iff some
//                  open candidate passes and is then the minimum of those: filtering by the bound first gives the same answer.)
//   k_sim3_settle  one workgroup per pair, requests strided over its threads: the parallel fixed point of k_search_proj (k_project.hip).
//                  closedBy[slot] = the smallest request index currently deciding for the slot; request i decides for the first key of
//                  its list not closed by a j < i (k_sim3_decide.hpp); rounds repeat until no decision changes.  By induction the decisions
//                  of requests 0 .. k are final after round k + 1 (whether some j < i closes a slot depends only on decisions of requests
//                  < i), so the fixed point IS the sequential result, after at most n + 1 rounds.  closedBy and the decisions live in LDS
//                  (4 bytes per keypoint slot + 4 per request), the key lists are read from global memory.  A request whose whole
//                  TRUNCATED list is closed scans its window again under the current closedBy (k_sim3_window left it the window: 16
//                  bytes): exact, and counted.  From the second round on a request that holds its smallest key and still sees it open
//                  keeps it without reading its list (sim3Stays): a round then costs LDS reads for all but the contended requests.
// Keys order candidates as the reference visits them: a window is one slot range of mGrid's CSR order per cell column (ix outer, iy inner,
// push order in a cell), and the strict "<" of :570 / :687 keeps the first of equal distances.
// This file is also compiled for the HOST by the CPU suite (tests/cpp/sim3_host_check.cpp behind tests/cpp/host_shim): everything outside
// the __HIPCC__ block - the window kernel, the re-scan and the round step - runs there one thread at a time.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orbx_lds_pollute.hpp"
#include "k_keyframe_project.hpp"
#include "k_sim3_decide.hpp"
#include "k_match_helpers.hpp"
#include "orbx_device.hpp"
#include "orbx_params.hpp"

namespace orbx {

namespace {
enum { kSim3Flag = 0, kSim3NoMatch = 6, kSim3Matched = 7 };      // == ORBX_SIM3_SEARCH_*; 1 .. 5 are the front end's
constexpr int kSettleThreads = 1024;
}  // namespace

__device__ int g_sim3Stats[4];      // diagnostics: pair 0's rounds, requests settled by a re-scan (last launch), pair 0's ticks, 0

// What a request whose window holds more than kSim3Top candidates leaves for a later re-scan: the projection, the radius, and the level and
// the four cell bounds packed (level | minCX << 5 | maxCX << 11 | minCY << 17 | maxCY << 23: a level is below 16, a cell below 64)
struct Sim3Window { float u, v, r; int cells; };
// What k_sim3_window leaves per (pair, MapPoint) for k_sim3_settle, one record (one pointer in the settling kernel, which is short of SGPRs):
// the kSim3Top smallest keys ascending, the count of all candidates, and - only where count > kSim3Top, nobody else scans again - the window
struct Sim3Record { int keys[kSim3Top]; Sim3Window win; int cnt, pad[3]; };
static_assert(sizeof(Sim3Record) % 16 == 0, "records are read with 128-bit loads");

// The candidate tests of :555-575 / :672-692 over KeyFrame::GetFeaturesInArea's visit of q's window (keyFrameVisitArea).  occ: the pair's
// vpMatched on entry (may be NULL).  closedBy == nullptr: the static tests only.  Returns the number of passing candidates, their kSim3Top
// smallest keys in `keys`; any = vIndices is not empty.
__device__ __forceinline__ int sim3Scan(const KfProjection& q, const KeyFrameView& kf, const uint8_t* occ, const uint4& dlo, const uint4& dhi,
                                        int maxDist, const int* closedBy, int i, int (&keys)[kSim3Top], bool& any) {
#pragma unroll
    for (int k = 0; k < kSim3Top; k++) keys[k] = kSim3NoKey;
    int count = 0;
    any = keyFrameVisitArea(kf, q, [&](int s, int idx, float, float) {
        if (occ && occ[idx]) return;                                                 // vpMatched[idx] on entry (:558, :675)
        if (closedBy && closedBy[s] < i) return;                                     // ... or set by an earlier request
        const int lv = kf.K[idx].octave;
        if (lv < q.level - 1 || lv > q.level) return;                                // :563, :680
        const uint4 e = kf.D[2 * idx], g = kf.D[2 * idx + 1];
        const int dist = hamming256(dlo, dhi, e, g);
        if (dist > maxDist) return;                                                  // :577, :694 (header: applied before the minimum, same result)
        count++;
        sortedInsert(keys, (dist << 16) | s);        // slots are distinct, so keys are: the sorted insert keeps the first of equal distances
    });
    return count;
}

// grid (ceil(mpCapacity / 256), pairs).  rec[o] (keys and cnt; win only where cnt > kSim3Top) and exitOut[o] (may be NULL) with
// o = pair*mpCapacity + i: all written.
__global__ __launch_bounds__(256) void k_sim3_window(const float* __restrict__ mpWorld, const float* __restrict__ mpNormal,
                                                     const float* __restrict__ mpDist, const uint8_t* __restrict__ mpDesc,
                                                     const int* __restrict__ nMp, const uint8_t* __restrict__ mpFlags,
                                                     const float* __restrict__ poses, const Keypoint* __restrict__ kpsUn,
                                                     const uint8_t* __restrict__ desc, const int* __restrict__ nOut,
                                                     const int* __restrict__ gridOff, const int* __restrict__ gridIdx,
                                                     const uint8_t* __restrict__ occupied, Sim3SearchParams p,
                                                     Sim3Record* __restrict__ rec, uint8_t* __restrict__ exitOut) {
    const int pair = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (pair == 0 && i == 0) g_sim3Stats[1] = 0;      // the settling workgroups of this launch count into it (they start after this kernel)
    if (i >= p.mpCapacity) return;
    const long long f = p.kfFirst + (long long)pair * p.kfStep, list = p.mpFirst + (long long)pair * p.mpStep;
    const long long m = list * p.mpCapacity + i, o = (long long)pair * p.mpCapacity + i;
    const int NM = nMp ? min(max(nMp[list], 0), p.mpCapacity) : p.mpCapacity;
    int code = kSim3Flag, count = 0;
    int keys[kSim3Top];
#pragma unroll
    for (int k = 0; k < kSim3Top; k++) keys[k] = kSim3NoKey;
    do {
        if (i >= NM || !(mpFlags[o] & 1)) break;                                     // :501, :617
        KfProjection q;
        code = projectIntoKeyFrame(poses + (long long)pair * 12, mpWorld + 3 * m, mpNormal + 3 * m, mpDist + 3 * m, p, p.projection, q);
        if (code != kFrontPassed) break;
        const uint8_t* occ = occupied ? occupied + (long long)pair * p.capacity : nullptr;
        const KeyFrameView kf = keyFrameView(f, kpsUn, desc, nOut, gridOff, gridIdx, p.capacity);
        const uint4 dlo = *(const uint4*)(mpDesc + m * 32), dhi = *(const uint4*)(mpDesc + m * 32 + 16);
        bool any;
        count = sim3Scan(q, kf, occ, dlo, dhi, p.maxDist, nullptr, i, keys, any);
        code = any ? (int)kSim3NoMatch : (int)kFrontEmptyWindow;                               // vIndices.empty() (:547, :664) comes before any keypoint state
        if (count > kSim3Top) {
            Sim3Window w;
            w.u = q.u; w.v = q.v; w.r = q.r;
            w.cells = q.level | q.minCX << 5 | q.maxCX << 11 | q.minCY << 17 | q.maxCY << 23;
            rec[o].win = w;
        }
    } while (false);
#pragma unroll
    for (int k = 0; k < kSim3Top; k++) rec[o].keys[k] = keys[k];
    rec[o].cnt = count;
    if (exitOut) exitOut[o] = (uint8_t)code;
}

// One request's step of a round: the decision (k_sim3_decide.hpp) of request i of the pair under closedBy (the previous round's), given its
// previous decision `prev`.  *rescanned: the decision came from scanning the window again (the truncated list was used up).
__device__ __forceinline__ int sim3RoundStep(int i, int pair, int prev, const uint8_t* __restrict__ mpDesc, const Keypoint* __restrict__ kpsUn,
                                             const uint8_t* __restrict__ desc, const int* __restrict__ nOut,
                                             const int* __restrict__ gridOff, const int* __restrict__ gridIdx,
                                             const uint8_t* __restrict__ occupied, const Sim3SearchParams& p,
                                             const Sim3Record* __restrict__ rec, const int* closedBy, bool* rescanned) {
    *rescanned = false;
    if (sim3Stays(prev, closedBy, i)) return prev;
    const Sim3Record* me = rec + ((long long)pair * p.mpCapacity + i);
    int keys[kSim3Top];
#pragma unroll
    for (int k = 0; k < kSim3Top; k++) keys[k] = me->keys[k];
    if (keys[0] == kSim3NoKey) return kSim3Dead;
    bool rescan;
    const int d = sim3Decide(keys, keys[kSim3Top - 1] != kSim3NoKey ? me->cnt : 0, closedBy, i, &rescan);      // (only a full list can be a truncated one)
    if (!rescan) return d == kSim3NoKey ? d : d | (d == keys[0] ? kSim3First : 0);
    *rescanned = true;
    const long long f = p.kfFirst + (long long)pair * p.kfStep, m = (p.mpFirst + (long long)pair * p.mpStep) * p.mpCapacity + i;
    const Sim3Window w = me->win;
    KfProjection q;
    q.u = w.u; q.v = w.v; q.r = w.r; q.invz = 0.f;
    q.level = w.cells & 31; q.minCX = (w.cells >> 5) & 63; q.maxCX = (w.cells >> 11) & 63; q.minCY = (w.cells >> 17) & 63; q.maxCY = (w.cells >> 23) & 63;
    const uint8_t* occ = occupied ? occupied + (long long)pair * p.capacity : nullptr;
    const KeyFrameView kf = keyFrameView(f, kpsUn, desc, nOut, gridOff, gridIdx, p.capacity);
    const uint4 dlo = *(const uint4*)(mpDesc + m * 32), dhi = *(const uint4*)(mpDesc + m * 32 + 16);
    bool any;
    sim3Scan(q, kf, occ, dlo, dhi, p.maxDist, closedBy, i, keys, any);
    return keys[0];
}

#if defined(__HIPCC__)
size_t sim3RecordBytes() { return sizeof(Sim3Record); }
size_t sim3SettleLdsBytes(int capacity, int mpCapacity) { return 4 * ((size_t)capacity + (size_t)mpCapacity) + 64; }

extern "C" int orbx_debug_sim3_search_stats(int* out4) {
    if (!out4) return -2;                                  // ORBX_ERR_BAD_ARGUMENT
    return hipMemcpyFromSymbol(out4, HIP_SYMBOL(g_sim3Stats), sizeof(int) * 4) == hipSuccess ? 0 : -6;      // ORBX_ERR_HIP
}

extern "C" int orbx_debug_sim3_search_list_length(void) { return kSim3Top; }

// grid: pairs; kSettleThreads threads; dynamic LDS sim3SettleLdsBytes(capacity, mpCapacity).
__global__ __launch_bounds__(kSettleThreads) void k_sim3_settle(const uint8_t* __restrict__ mpDesc, const Keypoint* __restrict__ kpsUn,
                                                                const uint8_t* __restrict__ desc, const int* __restrict__ nOut,
                                                                const int* __restrict__ gridOff, const int* __restrict__ gridIdx,
                                                                const uint8_t* __restrict__ occupied, Sim3SearchParams p,
                                                                const Sim3Record* __restrict__ rec, int* __restrict__ matches, int* __restrict__ matchIdx,
                                                                int* __restrict__ matchDist, uint8_t* __restrict__ exitOut,
                                                                int* __restrict__ nMatches) {
    extern __shared__ __align__(16) int smem[];
    int* closedBy = smem;                       // [capacity] by CSR slot: the smallest request deciding for it, INT_MAX = nobody
    int* dec = closedBy + p.capacity;           // [mpCapacity] the decision of every request (k_sim3_decide.hpp)
    int* flags = dec + p.mpCapacity;            // [0], [1]: "a decision changed" (alternating), [2]: matches, [3]: the start tick (low word)
    const int pair = blockIdx.x, tid = threadIdx.x;
    const long long f = p.kfFirst + (long long)pair * p.kfStep;
    const int* gi = gridIdx + f * p.capacity;
    const int nIn = keyFrameSlotsInGrid(f, nOut, gridOff, p.capacity);      // as the scans' view: every slot of a key is below it
    int* out = matches + (long long)pair * p.capacity;
    for (int s = tid; s < p.capacity; s += kSettleThreads) { closedBy[s] = 0x7fffffff; out[s] = -1; }
    for (int i = tid; i < p.mpCapacity; i += kSettleThreads) dec[i] = kSim3NoKey;
    if (tid < 3) flags[tid] = 0;
    if (tid == 3) flags[3] = (int)__builtin_amdgcn_s_memrealtime();      // (kept in LDS: the kernel has no SGPR pair to spare for it)
    __syncthreads();
    int rounds = 0, myRescans = 0;
    for (int round = 1; round <= p.mpCapacity + 1; round++) {
        bool mineChanged = false;
        myRescans = 0;
        for (int i = tid; i < p.mpCapacity; i += kSettleThreads) {
            bool rescanned;
            const int d = sim3RoundStep(i, pair, dec[i], mpDesc, kpsUn, desc, nOut, gridOff, gridIdx, occupied, p, rec, closedBy, &rescanned);
            myRescans += rescanned ? 1 : 0;
            if (d != dec[i]) {
                mineChanged |= !(sim3IsNone(d) && sim3IsNone(dec[i]));      // (none -> dead changes no closedBy: not a reason for another round)
                dec[i] = d;
            }
        }
        if (mineChanged) flags[round & 1] = 1;
        __syncthreads();
        rounds = round;
        const bool any = flags[round & 1] != 0;
        if (tid == 0) flags[(round & 1) ^ 1] = 0;          // the other slot is written again only after the next barriers
        if (!any) break;
        for (int s = tid; s < nIn; s += kSettleThreads) closedBy[s] = 0x7fffffff;
        __syncthreads();
        for (int i = tid; i < p.mpCapacity; i += kSettleThreads) {
            const int d = dec[i];
            if (!sim3IsNone(d)) atomicMin(&closedBy[min(sim3Slot(d), p.capacity - 1)], i);
        }
        __syncthreads();
    }
    // the tables the walk leaves: no two requests hold the same slot at the fixed point
    int nm = 0;
    for (int i = tid; i < p.mpCapacity; i += kSettleThreads) {
        const long long o = (long long)pair * p.mpCapacity + i;
        const int d = dec[i];
        if (sim3IsNone(d)) { matchIdx[o] = -1; matchDist[o] = 256; continue; }
        const int idx = min(max(gi[min(sim3Slot(d), p.capacity - 1)], 0), p.capacity - 1);
        out[idx] = i;                                                                // vpMatched[bestIdx] = pMP (:579, :696)
        matchIdx[o] = idx; matchDist[o] = sim3Dist(d);
        if (exitOut) exitOut[o] = (uint8_t)kSim3Matched;
        nm++;
    }
    if (nm) atomicAdd(&flags[2], nm);
    if (myRescans) atomicAdd(&g_sim3Stats[1], myRescans);      // (of the last round: the requests whose final decision is a re-scan's)
    __syncthreads();
    if (tid == 0) {
        nMatches[pair] = flags[2];
        if (pair == 0) { g_sim3Stats[0] = rounds; g_sim3Stats[2] = (int)__builtin_amdgcn_s_memrealtime() - flags[3]; g_sim3Stats[3] = 0; }
    }
}

void launchSim3Search(hipStream_t st, const float* mpWorld, const float* mpNormal, const float* mpDist, const uint8_t* mpDesc, const int* nMp,
                      const uint8_t* mpFlags, const float* poses, const Keypoint* kpsUn, const uint8_t* desc, const int* nOut, const int* gridOff,
                      const int* gridIdx, const uint8_t* occupied, const Sim3SearchParams& p, void* rec, int* matches,
                      int* matchIdx, int* matchDist, uint8_t* exitCode, int* nMatches, int nPairs, LdsPolluter pollute) {
    pollute(st);
    hipLaunchKernelGGL(k_sim3_window, dim3((p.mpCapacity + 255) / 256, nPairs), dim3(256), 0, st, mpWorld, mpNormal, mpDist, mpDesc, nMp, mpFlags,
                       poses, kpsUn, desc, nOut, gridOff, gridIdx, occupied, p, (Sim3Record*)rec, exitCode);
    pollute(st);
    hipLaunchKernelGGL(k_sim3_settle, dim3(nPairs), dim3(kSettleThreads), sim3SettleLdsBytes(p.capacity, p.mpCapacity), st, mpDesc, kpsUn, desc,
                       nOut, gridOff, gridIdx, occupied, p, (const Sim3Record*)rec, matches, matchIdx, matchDist, exitCode,
                       nMatches);
}
#endif

}  // namespace orbx
