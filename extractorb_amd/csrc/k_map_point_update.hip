// k_map_point_update.hip - MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth (reference src/MapPoint.cc:330-403,
// :427-494) for the MapPoints a caller lists, on observation lists in HBM: the rows of d_mp_desc / d_mp_normal / d_mp_dist that Fuse, the
// frustum and the projection searches read are produced where the keyframes' descriptors and poses already are.  One kernel template over the
// rig kind; the statements are k_map_point_update.hpp's, which the CPU suite compiles for the host.
// LAUNCH SHAPE.  Lists are short (2 for a fresh point, a mean of 5-10) with a tail into the hundreds: a wave per point would idle 60 lanes on
// the common case, a lane per point would serialise the tail.  A workgroup of kMpuThreads = 256 takes kMpuPoints = 16 consecutive points
// and walks three phases, each point in exactly one:
//   A  N <= 16   one DPP row of 16 lanes per point, all sixteen points at once.  Lane i owns entry i and ROW i of the distance matrix: its
//                sixteen distances stay in registers, the nine bisection steps count them without talking to any lane, and the winner is
//                rowMin16 (k_wave_min.hpp) over median << 16 | i;
//   B  N <= 64   one wave per point (wave w takes points w, w + 4, ...).  The wave walks the rows; lane j holds D[i][j] and a step's count
//                is a DPP sum over the wave (waveSum);
//   C  N <= 1024 the workgroup per point, one after the other: 32 KB of descriptors in LDS, read as 16-byte halves; wave w walks rows
//                w, w + 4, ..., a lane holds up to sixteen D[i][j] (j = lane + 64 c), counts its own and the wave sums the counts; the four waves' minima meet in LDS.
// In every phase a lane first checks and stages its own entries: the descriptor (two uint4), the entry's product normali * (1 / norm) with
// the camera centre computed HERE from the pose (no launch of its own for the centres: docs/history/r21_map_point_update.md), and whether the
// entry takes part.  The serial sum of UpdateNormalAndDepth then runs in ONE lane per point over the staged products, in list order.
// LDS is static (48 KB: three workgroups per CU) and typed address_space(3): no generic pointer, no FLAT instruction.  No scratch: every
// register array is indexed by unrolled constants.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orbx_lds_pollute.hpp"
#include "k_map_point_update.hpp"
#include "k_wave_min.hpp"

namespace orbx {

namespace {
constexpr int kMpuThreads = 256, kMpuPoints = 16;
static_assert(kMpuMaxObservations == 64 * 16, "phase C's largest body holds sixteen columns per lane");
constexpr int kMpuNoKey = 0x7fffffff;

// 1 where x <= v, as arithmetic: a compare would make a lane mask, a scalar register pair, per column
__device__ __forceinline__ int mpuLe(int x, int v) { return (int)((unsigned)(x - 1 - v) >> 31); }

struct MpuLds {
    ORBX_LDS LdsU4* desc;      // [2 * e], [2 * e + 1]: entry e's descriptor
    ORBX_LDS float* unit;      // [3 * e + c]: entry e's product
    ORBX_LDS int* part;        // [e]: 1 = the entry takes part in the descriptor selection
    __device__ MpuLds at(int e) const { return MpuLds{desc + 2 * e, unit + 3 * e, part + e}; }
};

struct MpuHead { long long off0, slot; int ref; bool ok; float pos[3]; };

__device__ __forceinline__ MpuHead mpuHead(const MapPointUpdateArrays& a, const MapPointUpdateParams& p, long long m, int n) {
    MpuHead h;
    const int off0 = a.obsOff[m];
    h.off0 = off0; h.ref = a.ref[m]; h.slot = a.slot ? a.slot[m] : m;
    h.ok = mpuHeadOk(off0, h.slot, h.ref, n);
    for (int c = 0; c < 3; c++) h.pos[c] = h.ok && (p.what & 2) ? a.mpWorld[3 * h.slot + c] : 0.f;
    return h;
}

// checks entry e of the point and stages it at L[e]; false: BAD_INDEX
template <bool TwoEyes>
__device__ __forceinline__ bool mpuStage(const MapPointUpdateArrays& a, const MapPointUpdateParams& p, const MpuHead& h, int e, const MpuLds& L) {
    int f, row;
    const long long o = h.off0 + e;
    if (!mpuEntryOk(a.obs, o, a.nOut, p, f, row)) return false;
    L.part[e] = !(a.obsFlags && (a.obsFlags[o] & 1));
    if (p.what & 1) {
        const LdsU4* D = (const LdsU4*)(a.desc + ((long long)f * p.capacity + row) * 32);
        L.desc[2 * e] = D[0]; L.desc[2 * e + 1] = D[1];
    }
    if (p.what & 2) {
        float Ow[3], t[3];
        mpuCentre<TwoEyes>(a.poses, p, f, false, Ow);
        mpuUnit(h.pos, Ow, t);
        for (int c = 0; c < 3; c++) L.unit[3 * e + c] = t[c];
    }
    return true;
}

// what the point's first lane writes after the selection: key = median << 16 | entry, or kMpuNoKey; before = the entries taking part in front of it
template <bool TwoEyes>
__device__ __forceinline__ void mpuClose(const MapPointUpdateArrays& a, const MapPointUpdateParams& p, long long m, int n, const MpuHead& h, int key,
                                         int before, const MpuLds& L) {
    const bool chosen = (p.what & 1) && key != kMpuNoKey;
    a.best[m] = chosen ? before : -1;
    a.bestMedian[m] = chosen ? key >> 16 : -1;
    if (p.what & 2) mpuNormalAndDepth<TwoEyes>(a, p, n, h.off0, h.ref, h.slot, h.pos, L.unit);
    a.status[m] = (p.what & 1) && !chosen ? kMpuNoDescriptor : kMpuOk;
}
__device__ __forceinline__ void mpuRefuse(const MapPointUpdateArrays& a, long long m, int status) {
    a.best[m] = -1; a.bestMedian[m] = -1; a.status[m] = (uint8_t)status;
}
// the winner's 32 bytes, a half per lane (half = 0, 1)
__device__ __forceinline__ void mpuCopyRow(const MapPointUpdateArrays& a, long long slot, int entry, int half, const MpuLds& L) {
    *(LdsU4*)(a.mpDesc + slot * 32 + 16 * half) = L.desc[2 * entry + half];
}

// phase A: lane gl of a 16-lane row, the point's n <= 16 entries at L; shift = the row's first lane within the wave
template <bool TwoEyes>
__device__ __forceinline__ void mpuRowPoint(const MapPointUpdateArrays& a, const MapPointUpdateParams& p, long long m, int n, int gl, int shift,
                                            const MpuLds& L) {
    if (n == 0) { if (gl == 0) mpuRefuse(a, m, kMpuEmpty); return; }
    const MpuHead h = mpuHead(a, p, m, n);
    const bool mine = gl < n;
    bool ok = h.ok;
    if (ok && mine) ok = mpuStage<TwoEyes>(a, p, h, gl, L);
    const bool bad = ((__ballot(!ok) >> shift) & 0xffffull) != 0ull;
    ORBX_WAVE_LDS_SYNC();
    if (bad) { if (gl == 0) mpuRefuse(a, m, kMpuBadIndex); return; }
    const int takes = mine ? L.part[gl] : 0;
    const unsigned pm = (unsigned)((__ballot(takes != 0) >> shift) & 0xffffull);
    int key = kMpuNoKey;
    if ((p.what & 1) && pm) {
        const LdsU4 lo = L.desc[2 * gl], hi = L.desc[2 * gl + 1];
        int d[16];
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const LdsU4 x = L.desc[2 * j], y = L.desc[2 * j + 1];
            d[j] = (pm >> j) & 1 ? hamming256(lo, hi, x, y) : 512;
        }
        const int median = mpuRankSelect(mpuNeed(__popc(pm)), [&](int v) {
            int c = 0;
#pragma unroll
            for (int j = 0; j < 16; j++) c += mpuLe(d[j], v);
            return c;
        });
        key = rowMin16(takes ? median << 16 | gl : kMpuNoKey);
        if (gl < 2) mpuCopyRow(a, h.slot, key & 0xffff, gl, L);
    }
    if (gl == 0) mpuClose<TwoEyes>(a, p, m, n, h, key, __popc(pm & ((1u << (key & 15)) - 1u)), L);
}

// The rows first, first + step, ... of a list of n <= 64 * Chunks staged entries, walked by one wave: the smallest median << 16 | row.
// participants = the entries taking part (wave-uniform).  Lane l holds D[i][l + 64 c]; a column past the list or out of the selection
// gets a distance of 512 or more and is never counted.  A bisection step's count is each lane's own count of its columns, summed over the wave by
// DPP (sixteen ballots a step held sixteen scalar register pairs at once and spilled them).
template <int Chunks>
__device__ __forceinline__ int mpuWaveRows(const MpuLds& L, int n, int lane, int first, int step, int participants) {
    const int need = mpuNeed(participants);
    unsigned cols = 0;      // bit c: column lane + 64 c takes part
#pragma unroll
    for (int c = 0; c < Chunks; c++) cols |= (unsigned)(mpuLe(lane + 64 * c, n - 1) & L.part[min(lane + 64 * c, n - 1)]) << c;
    int key = kMpuNoKey;
    for (int i = first; i < n; i += step) {
        if (!L.part[i]) continue;                                           // (wave-uniform: i is)
        const LdsU4 lo = L.desc[2 * i], hi = L.desc[2 * i + 1];
        int d[Chunks];
#pragma unroll
        for (int c = 0; c < Chunks; c++) {      // (no branch per column: a column out of the selection reads the list's last entry and gets bit 9)
            const int j = min(lane + 64 * c, n - 1);
            const LdsU4 x = L.desc[2 * j], y = L.desc[2 * j + 1];
            d[c] = hamming256(lo, hi, x, y) | (int)((~cols >> c) & 1u) << 9;
        }
        const int median = mpuRankSelect(need, [&](int v) {
            int cnt = 0;
#pragma unroll
            for (int c = 0; c < Chunks; c++) cnt += mpuLe(d[c], v);
            return waveSum(cnt);
        });
        key = min(key, median << 16 | i);
    }
    return key;
}
// the staged entries in front of entry `end` that take part, counted by one wave
template <int Chunks>
__device__ __forceinline__ int mpuWaveCount(const MpuLds& L, int n, int lane, int end) {
    int cnt = 0;
    const int last = min(n, end) - 1;
#pragma unroll
    for (int c = 0; c < Chunks; c++) cnt += mpuLe(lane + 64 * c, last) & L.part[min(lane + 64 * c, n - 1)];
    return waveSum(cnt);
}

// phase B: one wave, 16 < n <= 64
template <bool TwoEyes>
__device__ __forceinline__ void mpuWavePoint(const MapPointUpdateArrays& a, const MapPointUpdateParams& p, long long m, int n, int lane, const MpuLds& L) {
    const MpuHead h = mpuHead(a, p, m, n);
    bool ok = h.ok;
    if (ok && lane < n) ok = mpuStage<TwoEyes>(a, p, h, lane, L);
    const bool bad = __ballot(!ok) != 0ull;
    ORBX_WAVE_LDS_SYNC();
    if (bad) { if (lane == 0) mpuRefuse(a, m, kMpuBadIndex); return; }
    int key = kMpuNoKey, before = 0;
    const int participants = mpuWaveCount<1>(L, n, lane, n);
    if ((p.what & 1) && participants) {
        key = mpuWaveRows<1>(L, n, lane, 0, 1, participants);
        before = mpuWaveCount<1>(L, n, lane, key & 0xffff);
        if (lane < 2) mpuCopyRow(a, h.slot, key & 0xffff, lane, L);
    }
    if (lane == 0) mpuClose<TwoEyes>(a, p, m, n, h, key, before, L);
    ORBX_WAVE_LDS_SYNC();      // the wave's next point stages over these entries
}

// phase C: the workgroup, 64 < n <= 64 * Chunks.  Every thread of the workgroup calls it (barriers inside)
template <bool TwoEyes, int Chunks>
__device__ __forceinline__ void mpuGroupPoint(const MapPointUpdateArrays& a, const MapPointUpdateParams& p, long long m, int n, int tid,
                                              const MpuLds& L, ORBX_LDS int* sKey) {
    const MpuHead h = mpuHead(a, p, m, n);
    bool ok = h.ok;
    for (int e = tid; ok && e < n; e += kMpuThreads) ok = mpuStage<TwoEyes>(a, p, h, e, L);
    const bool bad = __syncthreads_or(!ok) != 0;                            // (the barrier behind the staging as well)
    if (bad) { if (tid == 0) mpuRefuse(a, m, kMpuBadIndex); return; }      // (workgroup-uniform)
    const int lane = tid & 63, wave = tid >> 6;
    const int participants = mpuWaveCount<Chunks>(L, n, lane, n);
    const bool select = (p.what & 1) && participants;
    if (select) {
        const int mine = mpuWaveRows<Chunks>(L, n, lane, wave, kMpuThreads / 64, participants);
        if (lane == 0) sKey[wave] = mine;
    }
    __syncthreads();
    if (wave == 0) {
        int key = kMpuNoKey, before = 0;
        if (select) {
            key = min(min(sKey[0], sKey[1]), min(sKey[2], sKey[3]));
            before = mpuWaveCount<Chunks>(L, n, lane, key & 0xffff);
            if (lane < 2) mpuCopyRow(a, h.slot, key & 0xffff, lane, L);
        }
        if (lane == 0) mpuClose<TwoEyes>(a, p, m, n, h, key, before, L);
    }
    __syncthreads();           // the next point stages over these entries
}
}  // namespace

// grid: ceil(n_points / kMpuPoints); kMpuThreads threads
template <bool TwoEyes>
__global__ __launch_bounds__(kMpuThreads) void k_map_point_update(MapPointUpdateArrays a, MapPointUpdateParams p) {
    __shared__ LdsU4 sDescMem[2 * kMpuMaxObservations];
    __shared__ float sUnitMem[3 * kMpuMaxObservations];
    __shared__ int sPartMem[kMpuMaxObservations], sNMem[kMpuPoints], sKeyMem[kMpuThreads / 64];
    const MpuLds L{(ORBX_LDS LdsU4*)sDescMem, (ORBX_LDS float*)sUnitMem, (ORBX_LDS int*)sPartMem};
    ORBX_LDS int* sN = (ORBX_LDS int*)sNMem;
    ORBX_LDS int* sKey = (ORBX_LDS int*)sKeyMem;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = tid >> 4;
    const long long m0 = (long long)blockIdx.x * kMpuPoints;
    if (tid < kMpuPoints) sN[tid] = m0 + tid < p.nPoints ? mpuListLength(a.obsOff, m0 + tid) : -1;      // -1: past the call's points
    __syncthreads();
    {   // A: a DPP row per point
        const int n = sN[row];
        if (n >= 0 && n <= 16) mpuRowPoint<TwoEyes>(a, p, m0 + row, n, tid & 15, lane & 48, L.at(16 * row));
    }
    __syncthreads();
    for (int k = wave; k < kMpuPoints; k += kMpuThreads / 64) {      // B: a wave per point
        const int n = sN[k];
        if (n > 16 && n <= 64) mpuWavePoint<TwoEyes>(a, p, m0 + k, n, lane, L.at(64 * wave));
    }
    __syncthreads();
    for (int k = 0; k < kMpuPoints; k++) {                           // C: the workgroup per point
        const int n = sN[k];
        if (n > kMpuMaxObservations) { if (tid == 0) mpuRefuse(a, m0 + k, kMpuTooLong); }
        else if (n > 512) mpuGroupPoint<TwoEyes, 16>(a, p, m0 + k, n, tid, L, sKey);      // (a lane's columns are register arrays: one body per size)
        else if (n > 256) mpuGroupPoint<TwoEyes, 8>(a, p, m0 + k, n, tid, L, sKey);
        else if (n > 128) mpuGroupPoint<TwoEyes, 4>(a, p, m0 + k, n, tid, L, sKey);
        else if (n > 64) mpuGroupPoint<TwoEyes, 2>(a, p, m0 + k, n, tid, L, sKey);
    }
}

void launchMapPointUpdate(hipStream_t st, bool twoEyes, const MapPointUpdateArrays& a, const MapPointUpdateParams& p, LdsPolluter pollute) {
    const dim3 grid((unsigned)((p.nPoints + kMpuPoints - 1) / kMpuPoints));
    pollute(st);
    if (twoEyes) hipLaunchKernelGGL(k_map_point_update<true>, grid, dim3(kMpuThreads), 0, st, a, p);
    else hipLaunchKernelGGL(k_map_point_update<false>, grid, dim3(kMpuThreads), 0, st, a, p);
}

}  // namespace orbx
