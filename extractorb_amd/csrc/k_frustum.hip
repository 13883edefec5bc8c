// k_frustum.hip - the front half of the two map-to-frame projection searches, on the device: a list of MapPoints and a frame pose in,
// the compacted request lists of orbx_search_by_projection_device out.
//   mode 0: Tracking::SearchLocalPoints' loop over the local map (reference src/Tracking.cc:2941-2959: Frame::isInFrustum, src/Frame.cc:493-570,
//           Nleft == -1) plus the prelude of ORBmatcher::SearchByProjection(F, vpMapPoints, ...) (src/ORBmatcher.cc:50-73)
//   mode 1: the projection of pKF's MapPoints in ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (:2183-2230)
// The per-MapPoint statement is frustumPoint of k_frustum_point.hpp (also compiled for the host by the CPU suite); this file is the
// launch shape and the compaction.
// ONE WORKGROUP PER PAIR walks its list in chunks of kThreads MapPoints.  The requests of a chunk are placed in list order without an atomic:
// a ballot and a popcount of the lower lanes inside a wave, the wave totals through LDS (two buffers, so one barrier per chunk), and a
// running base that every thread keeps for itself.  The search that follows sizes its rounds and its LDS by the request capacity, and a
// local map is several times its in-view share, hence compaction and not holes.  A chunk is ~150 double / float operations per thread and
// three 12-byte loads, 3.7 us on an MI355X: a 16 384-point list is 16 chunks of one workgroup, 61 us, and that single workgroup bounds the
// one-frame call (tools/frustum_rate.py, profiles/r11_frustum_requests.md; DESIGN.md "Frustum requests" names the form that would not).
// Nothing lives in LDS but 2 x 2 x 16 counters and the two level tables: no capacity bound.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orbx_lds_pollute.hpp"
#include "k_frustum_point.hpp"
#include "orbx_device.hpp"
#include "orbx_params.hpp"

namespace orbx {

namespace {
constexpr int kThreads = 1024, kWaves = kThreads / 64;
// frustumPoint's parameter block as the kernel hands it over: the two level tables through LDS (as the pose).  (Read from the kernel arguments they are 32
// scalar registers held across the chunk loop, beside the pose, the camera and fifteen pointers: more than a wave has.)
struct FrustumView {
    float fx, fy, cx, cy, minX, maxX, minY, maxY;
    const float* scale;
    const float* breaks;
    float mbf, viewCosLimit, th, thFarPoints;
    int mode, farPoints;
    static constexpr int nlevels = kMaxLevels;      // the staged breakpoints from the handle's nlevels - 1 on are NaN, which no ratio reaches
};
}  // namespace

// grid: n_pairs.
__global__ __launch_bounds__(kThreads) void k_frustum(const float* __restrict__ mpWorld, const float* __restrict__ mpNormal,
                                                      const float* __restrict__ mpDist, const uint8_t* __restrict__ mpDesc,
                                                      const float* __restrict__ mpAngle, const int* __restrict__ nMp,
                                                      const uint8_t* __restrict__ mpFlags, const float* __restrict__ poses, FrustumParams p,
                                                      ProjQuery* __restrict__ queries, uint8_t* __restrict__ queryDesc,
                                                      int* __restrict__ querySrc, int* __restrict__ nQueries,
                                                      TrackRecord* __restrict__ track, int* __restrict__ nInView) {
    __shared__ int sReq[2][kWaves], sView[2][kWaves];
    __shared__ float sScale[kMaxLevels], sBreaks[kMaxLevels], sPose[12], sPar[12];
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const long long f = p.curFirst + (long long)pair * p.curStep, list = p.mpFirst + (long long)pair * p.mpStep;
    // the pose goes through LDS as well: its twelve floats, their double forms and the camera centre made of them are loop invariants, and as
    // scalars they do not fit beside the rest either; read from LDS they are vector registers, of which there are plenty
    if (tid < kMaxLevels) { sScale[tid] = p.scale[tid]; sBreaks[tid] = tid + 1 < p.nlevels ? p.breaks[tid] : __builtin_nanf(""); }
    if (tid < 12) sPose[tid] = poses[f * 12 + tid];
    if (tid == 64) {      // (and the float parameters: the nested early exits of the statement need the scalar registers for their lane masks)
        sPar[0] = p.fx; sPar[1] = p.fy; sPar[2] = p.cx; sPar[3] = p.cy; sPar[4] = p.minX; sPar[5] = p.maxX; sPar[6] = p.minY; sPar[7] = p.maxY;
        sPar[8] = p.mbf; sPar[9] = p.viewCosLimit; sPar[10] = p.th; sPar[11] = p.thFarPoints;
    }
    __syncthreads();
    const FrustumView pv{sPar[0], sPar[1], sPar[2], sPar[3], sPar[4], sPar[5], sPar[6], sPar[7], sScale, sBreaks, sPar[8], sPar[9], sPar[10], sPar[11],
                         p.mode, p.farPoints};
    const long long o0 = (long long)pair * p.mpCapacity, m0 = list * p.mpCapacity;
    const int NM = nMp ? min(max(nMp[list], 0), p.mpCapacity) : p.mpCapacity;
    const float* T = sPose;
    int base = 0, inView = 0;      // requests / MapPoints in view of the chunks walked so far: the same in every thread
    for (int c0 = 0, buf = 0; c0 < p.mpCapacity; c0 += kThreads, buf ^= 1) {
        const int i = c0 + tid;
        int code = kFrustumFlag;
        ProjQuery q{};
        if (i < p.mpCapacity) {
            TrackRecord t = frustumUntouched();      // entries beyond the list carry FLAG
            if (i < NM) {
                const long long m = m0 + i;
                code = frustumPoint(T, mpWorld + 3 * m, mpNormal ? mpNormal + 3 * m : nullptr, mpDist + 3 * m, mpAngle ? mpAngle[m] : 0.0f,
                                    mpFlags[o0 + i], pv, t, q);
            }
            track[o0 + i] = t;
        }
        const bool req = code == kFrustumRequest;
        const unsigned long long reqs = __ballot(req), views = __ballot(code >= kFrustumFar);
        if (lane == 0) { sReq[buf][wave] = __popcll(reqs); sView[buf][wave] = __popcll(views); }
        __syncthreads();      // the other buffer is written in the next chunk, this one again only after the next barrier
        int before = 0, total = 0, view = 0;
#pragma unroll
        for (int w = 0; w < kWaves; w++) {
            const int c = sReq[buf][w];
            before += w < wave ? c : 0;
            total += c;
            view += sView[buf][w];
        }
        if (req) {      // k <= i: inside the pair's block
            const long long k = o0 + base + before + __popcll(reqs & ((1ull << lane) - 1ull));
            queries[k] = q;
            querySrc[k] = i;
            const uint4* D = (const uint4*)(mpDesc + (m0 + i) * 32);
            uint4* Q = (uint4*)(queryDesc + k * 32);
            Q[0] = D[0]; Q[1] = D[1];
        }
        base += total;
        inView += view;
    }
    // the unused slots: an all-zero request (flags = 0: not searched) and no source; their descriptor slots stay as they were
    for (int k = base + tid; k < p.mpCapacity; k += kThreads) {
        queries[o0 + k] = ProjQuery{0.f, 0.f, 0.f, 0.f, 0, 0, 0, 0.f};
        querySrc[o0 + k] = -1;
    }
    if (tid == 0) { nQueries[pair] = base; nInView[pair] = inView; }
}

void launchFrustum(hipStream_t st, const float* mpWorld, const float* mpNormal, const float* mpDist, const uint8_t* mpDesc, const float* mpAngle,
                   const int* nMp, const uint8_t* mpFlags, const float* poses, const FrustumParams& p, ProjQuery* queries, uint8_t* queryDesc,
                   int* querySrc, int* nQueries, TrackRecord* track, int* nInView, int nPairs, LdsPolluter pollute) {
    pollute(st);
    hipLaunchKernelGGL(k_frustum, dim3(nPairs), dim3(kThreads), 0, st, mpWorld, mpNormal, mpDist, mpDesc, mpAngle, nMp, mpFlags, poses, p, queries,
                       queryDesc, querySrc, nQueries, track, nInView);
}

}  // namespace orbx
