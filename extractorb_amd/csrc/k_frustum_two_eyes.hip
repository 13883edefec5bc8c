// k_frustum_two_eyes.hip - the front half of the local-map projection search for TWO-CAMERA rigs (Nleft != -1, a KannalaBrandt8 pair), on the
// device: a list of MapPoints and a rig pose in, the compacted request lists of orbx_search_by_projection_two_eyes_device out.  The statement
// is k_frustum_two_eyes_point.hpp (Frame::isInFrustumChecks per eye, reference src/Frame.cc:571-581, :1181-1254; Tracking::SearchLocalPoints'
// loop, src/Tracking.cc:2941-2959; the matcher's prelude, src/ORBmatcher.cc:50-73, :145-151), also compiled for the host by the CPU suite;
// this file is the launch shape and the compaction.
// THE SPREAD FORM, two launches (k_frustum.hip is the one-workgroup form, which one CU bounds: DESIGN.md "Frustum requests"):
//   k_frustum_two_eyes_check  grid (ceil(mp_capacity / kPoints), n_pairs).  One thread per (MapPoint, eye), the eye is the lane's parity: the
//       KannalaBrandt8 code (two software atan2f, a sincos, the polynomial) is instantiated once and no lane waits for another eye's
//       projection.  The eye's pose, centre and camera come from LDS by the eye index; thirty lanes compute the thirty rig invariants once per
//       workgroup.  The far decision and the slot predicate take the neighbour lane's result (__shfl_xor by 1).  It writes the two track
//       records of every list entry and ONE (slot count, in-view count) pair per workgroup into the handle's workspace.
//   k_frustum_two_eyes_place  the same grid.  A workgroup's base is the sum of the slot counts of the lower workgroups of its pair (a few dozen
//       integers); inside it a ballot, a popcount of the lower lanes and the wave totals through LDS, as in k_frustum.  No atomic decides a
//       position: the order is the list's, the same in every run.  The two requests of a slot are rebuilt from the track records (they hold u,
//       v, view_cos and level; bit 1 comes from the flags), each lane copies its half of the descriptor, the left lane writes the source.  Slots
//       from the count up to query_capacity are zero-filled by all workgroups of the pair together; slots beyond query_capacity are dropped.
// (One thread per MapPoint looping over the eyes was not built: it halves the threads per point while the statement's cost per point stays,
// and both eyes' invariants and cameras would have to live in registers at once.)
// LDS: 30 + 16 + 32 floats of invariants, cameras and level tables, a few counters: no capacity bound.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orbx_lds_pollute.hpp"
#include "k_frustum_two_eyes_point.hpp"
#include "orbx_device.hpp"
#include "orbx_params.hpp"

namespace orbx {

namespace {
constexpr int kThreads = 512, kWaves = kThreads / 64, kPoints = kThreads / 2;      // MapPoints per workgroup: one lane pair each
struct TwoEyesView {
    float minX, maxX, minY, maxY, viewCosLimit, th, thFarPoints;
    int farPoints;
    const float* scale;
    const float* breaks;
    static constexpr int nlevels = kMaxLevels;      // the staged breakpoints from the handle's nlevels - 1 on are NaN, which no ratio reaches
};
}  // namespace

int frustumTwoEyesGroups(int mpCapacity) { return (mpCapacity + kPoints - 1) / kPoints; }

// grid (p.groups, n_pairs).  counts[(pair * groups + g) * 2 + {0: slots, 1: MapPoints in view}]
__global__ __launch_bounds__(kThreads) void k_frustum_two_eyes_check(const float* __restrict__ mpWorld, const float* __restrict__ mpNormal,
                                                                     const float* __restrict__ mpDist, const int* __restrict__ nMp,
                                                                     const uint8_t* __restrict__ mpFlags, const float* __restrict__ prevDepth,
                                                                     const float* __restrict__ poses, FrustumTwoEyesParams p,
                                                                     TrackRecord* __restrict__ track, int* __restrict__ counts) {
    __shared__ float sPose[12], sTrl[12], sTlr[12], sEye[2 * kFrustumEyeFloats], sCam[16], sScale[kMaxLevels], sBreaks[kMaxLevels];
    __shared__ int sSlots[kWaves], sViews[kWaves];
    const int g = blockIdx.x, pair = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long f = p.curFirst + (long long)pair * p.curStep, list = p.mpFirst + (long long)pair * p.mpStep;
    if (tid < 12) { sPose[tid] = poses[f * 12 + tid]; sTrl[tid] = p.trl[tid]; sTlr[tid] = p.tlr[tid]; }
    if (tid >= 64 && tid < 64 + kMaxLevels) {
        const int l = tid - 64;
        sScale[l] = p.scale[l]; sBreaks[l] = l + 1 < p.nlevels ? p.breaks[l] : __builtin_nanf(""); sCam[l] = p.cam[l >> 3][l & 7];
    }
    __syncthreads();
    if (tid < 2 * kFrustumEyeFloats) sEye[tid] = frustumTwoEyesRigElement(sPose, sTrl, sTlr, tid);
    __syncthreads();
    const TwoEyesView pv{p.minX, p.maxX, p.minY, p.maxY, p.viewCosLimit, p.th, p.thFarPoints, p.farPoints, sScale, sBreaks};
    const long long o0 = (long long)pair * p.mpCapacity, m0 = list * p.mpCapacity;
    const int NM = nMp ? min(max(nMp[list], 0), p.mpCapacity) : p.mpCapacity;
    const int eye = tid & 1, i = g * kPoints + (tid >> 1);
    const bool look = i < NM && (mpFlags[o0 + i] & 1);                               // Tracking.cc:2945-2948; entries beyond the list carry FLAG
    TrackRecord t = frustumUntouched();
    int code = kFrustumFlag;
    if (look) {
        float e[kFrustumEyeFloats], k[8];
#pragma unroll
        for (int a = 0; a < kFrustumEyeFloats; a++) e[a] = sEye[eye * kFrustumEyeFloats + a];
#pragma unroll
        for (int a = 0; a < 8; a++) k[a] = sCam[eye * 8 + a];
        const long long m = m0 + i;
        code = frustumEyeCheck(e, k, mpWorld + 3 * m, mpNormal + 3 * m, mpDist + 3 * m, pv, t);
    }
    // every lane takes part in the exchange, whatever its own path was
    const int in = code == kFrustumRequest, inOther = __shfl_xor(in, 1);
    const float depthOther = __shfl_xor(t.depth, 1);
    const bool any = in || inOther;                                                  // mbTrackInView || mbTrackInViewR (ORBmatcher.cc:53)
    const float prev = any && prevDepth ? prevDepth[o0 + i] : 0.0f;
    const bool far = any && frustumTwoEyesFar(eye ? inOther != 0 : in != 0, eye ? depthOther : t.depth, prev, pv);      // :56
    if (in && far) t.exit = kFrustumFar;
    if (i < p.mpCapacity) track[(o0 + i) * 2 + eye] = t;
    const unsigned long long slots = __ballot(any && !far && eye == 0), views = __ballot(any && eye == 0);
    if (lane == 0) { sSlots[wave] = __popcll(slots); sViews[wave] = __popcll(views); }
    __syncthreads();
    if (tid == 0) {
        int s = 0, v = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) { s += sSlots[w]; v += sViews[w]; }
        int* c = counts + ((long long)pair * p.groups + g) * 2;
        c[0] = s; c[1] = v;
    }
}

// grid (p.groups, n_pairs)
__global__ __launch_bounds__(kThreads) void k_frustum_two_eyes_place(const uint8_t* __restrict__ mpDesc, const uint8_t* __restrict__ mpFlags,
                                                                     const TrackRecord* __restrict__ track, const int* __restrict__ counts,
                                                                     FrustumTwoEyesParams p, ProjQuery* __restrict__ queries,
                                                                     uint8_t* __restrict__ queryDesc, int* __restrict__ querySrc,
                                                                     int* __restrict__ nQueries, int* __restrict__ nWanted, int* __restrict__ nInView) {
    __shared__ float sScale[kMaxLevels];
    __shared__ int sRed[kWaves][3], sSlots[kWaves];
    const int g = blockIdx.x, pair = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long list = p.mpFirst + (long long)pair * p.mpStep;
    const long long o0 = (long long)pair * p.mpCapacity, m0 = list * p.mpCapacity, q0 = (long long)pair * p.queryCapacity;
    if (tid < kMaxLevels) sScale[tid] = p.scale[tid];
    // the slots of the lower workgroups of the pair, of all of them, and the MapPoints in view
    int before = 0, total = 0, view = 0;
    for (int gg = tid; gg < p.groups; gg += kThreads) {
        const int* c = counts + ((long long)pair * p.groups + gg) * 2;
        const int s = c[0];
        before += gg < g ? s : 0; total += s; view += c[1];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { before += __shfl_xor(before, o); total += __shfl_xor(total, o); view += __shfl_xor(view, o); }
    const int eye = tid & 1, i = g * kPoints + (tid >> 1);
    TrackRecord t = frustumUntouched();
    if (i < p.mpCapacity) t = track[(o0 + i) * 2 + eye];
    const int mine = t.exit == kFrustumRequest, other = __shfl_xor(mine, 1);
    const bool slot = mine || other;
    const unsigned long long slots = __ballot(slot && eye == 0);
    if (lane == 0) { sRed[wave][0] = before; sRed[wave][1] = total; sRed[wave][2] = view; sSlots[wave] = __popcll(slots); }
    __syncthreads();
    before = total = view = 0;
    int inFront = 0;
#pragma unroll
    for (int w = 0; w < kWaves; w++) {
        before += sRed[w][0]; total += sRed[w][1]; view += sRed[w][2];
        inFront += w < wave ? sSlots[w] : 0;
    }
    const int k = before + inFront + __popcll(slots & ((1ull << (lane & ~1)) - 1ull));      // the slot of this lane pair, in list order
    if (slot && k < p.queryCapacity) {                                               // k <= i; slots beyond the capacity are dropped from the end
        const TwoEyesView pv{0.f, 0.f, 0.f, 0.f, 0.f, p.th, 0.f, 0, sScale, nullptr};
        queries[(q0 + k) * 2 + eye] = frustumTwoEyesRequest(t, eye, mpFlags[o0 + i], pv);
        *(uint4*)(queryDesc + (q0 + k) * 32 + eye * 16) = *(const uint4*)(mpDesc + (m0 + i) * 32 + eye * 16);
        if (eye == 0) querySrc[q0 + k] = i;
    }
    // the unused slots: all-zero requests (flags = 0: not searched) and no source, dealt over the workgroups of the pair; their descriptors stay
    const int written = min(total, p.queryCapacity);
    for (long long r = 2LL * written + (long long)g * kThreads + tid; r < 2LL * p.queryCapacity; r += (long long)p.groups * kThreads) {
        queries[q0 * 2 + r] = ProjQuery{0.f, 0.f, 0.f, 0.f, 0, 0, 0, 0.f};
        if (!(r & 1)) querySrc[q0 + (r >> 1)] = -1;
    }
    if (g == 0 && tid == 0) {
        nQueries[pair] = written; nInView[pair] = view;
        if (nWanted) nWanted[pair] = total;
    }
}

void launchFrustumTwoEyes(hipStream_t st, const float* mpWorld, const float* mpNormal, const float* mpDist, const uint8_t* mpDesc, const int* nMp,
                          const uint8_t* mpFlags, const float* prevDepth, const float* poses, const FrustumTwoEyesParams& p, int* counts,
                          ProjQuery* queries, uint8_t* queryDesc, int* querySrc, int* nQueries, int* nWanted, TrackRecord* track, int* nInView,
                          int nPairs, LdsPolluter pollute) {
    pollute(st);
    hipLaunchKernelGGL(k_frustum_two_eyes_check, dim3(p.groups, nPairs), dim3(kThreads), 0, st, mpWorld, mpNormal, mpDist, nMp, mpFlags, prevDepth,
                       poses, p, track, counts);
    pollute(st);
    hipLaunchKernelGGL(k_frustum_two_eyes_place, dim3(p.groups, nPairs), dim3(kThreads), 0, st, mpDesc, mpFlags, (const TrackRecord*)track,
                       (const int*)counts, p, queries, queryDesc, querySrc, nQueries, nWanted, nInView);
}

}  // namespace orbx
