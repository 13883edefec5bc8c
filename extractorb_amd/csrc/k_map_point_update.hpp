// k_map_point_update.hpp - MapPoint::ComputeDistinctiveDescriptors (reference src/MapPoint.cc:330-403) and MapPoint::UpdateNormalAndDepth
// (:427-494) on observation lists, stated ONCE: what one observation contributes, what one row of the distance matrix decides, and how the
// point's table rows are finished.  k_map_point_update.hip deals these statements to the lanes of a group, a wave or a workgroup; the host
// build of the CPU suite (ORBX_HOST_ROW) runs them one point after the other (mpuPointSerial, tests/cpp/map_point_update_host_check.cpp).
// THE DESCRIPTOR HALF is integers throughout:
//   entries      one per descriptor, in the caller's order (the std::map order of mObservations; left then right of a rig keyframe,
//                :357-362).  An entry whose keyframe isBad() (bit 0 of its flag) takes no part (:353); positions count the others only;
//   Distances    [i][i] = 0, [i][j] = hamming256 of k_match_helpers.hpp (:375-381; the reference holds them as float, every value is an
//                integer of 0 .. 256);
//   median       vDists[0.5*(N-1)] of the sorted row (:391) is its element of rank (N-1)/2, the row's own 0 included: the smallest v with
//                #{j : D[i][j] <= v} >= (N-1)/2 + 1, found by nine bisection steps over counts (mpuRankSelect), no sort;
//   BestIdx      the FIRST row with the smallest median (strict <, :393): the minimum of median << 16 | row;  the row's 32 bytes are copied.
// THE NORMAL AND DEPTH HALF is cv::Mat arithmetic (parity unpinned):
//   centres      GetCameraCenter / GetRightCameraCenter are the records of k_rig_two_eyes.hpp (Ow = -Rcw.t()*tcw one gemmRow with alpha -1;
//                twr = Rwl*mTlr.t + Ow one gemmRow with the float addend);
//   normali      Pos - Owi, a float subtraction per element; cv::norm the sum of squares (dot3Double, k_match_helpers.hpp) and the root in double;
//   the sum      normal + normali/norm is cv::scaleAdd: normal[c] = fadd(fmul(normali[c], (float)(1.0/norm)), normal[c]), SEQUENTIALLY in
//                list order, one float rounding per step (mpuUnit makes the products, mpuAccumulate adds them: never a tree).  EVERY entry
//                counts, flagged or not: UpdateNormalAndDepth has no isBad() test;
//   normal/n     fmul(normal[c], (float)(1.0/(double)n));
//   distances    dist = (float)cv::norm(Pos - Ow_ref) with the LEFT centre of the reference entry's keyframe (:468), mfMaxDistance =
//                dist*mvScaleFactors[level], mfMinDistance = mfMaxDistance/mvScaleFactors[nlevels-1], the invariance bounds 0.8f* and
//                1.2f* of them, all float operations; level is the reference entry's keypoint octave, CLAMPED into the table.
// Plain arithmetic: compiles for the host behind tests/cpp/host_shim.
#pragma once
#include "k_lds_vec.hpp"
#include "k_match_helpers.hpp"
#include "k_rig_two_eyes.hpp"
#include "orbx_device.hpp"
#include "orbx_params.hpp"

namespace orbx {

// == orbx_map_point_update
enum { kMpuOk = 0, kMpuEmpty, kMpuNoDescriptor, kMpuBadIndex, kMpuTooLong };

constexpr int kMpuMaxObservations = 1024;      // == ORBX_MAX_OBSERVATIONS

// entries of MapPoint m's list, clamped at 0 from below and at kMpuMaxObservations + 1 (= too long) from above
__device__ __forceinline__ int mpuListLength(const int* obsOff, long long m) {
    const long long n = (long long)obsOff[m + 1] - (long long)obsOff[m];
    return n < 0 ? 0 : n > kMpuMaxObservations ? kMpuMaxObservations + 1 : (int)n;
}

// what is checked once per point: where its list starts, its table row and its reference entry
__device__ __forceinline__ bool mpuHeadOk(int off0, long long slot, int ref, int n) { return off0 >= 0 && slot >= 0 && ref >= 0 && ref < n; }

// entry o of d_obs: its frame inside the batch, its row inside the frame (the reference would index out of bounds otherwise)
__device__ __forceinline__ bool mpuEntryOk(const int* obs, long long o, const int* nOut, const MapPointUpdateParams& p, int& f, int& row) {
    f = obs[2 * o]; row = obs[2 * o + 1];
    if (f < 0 || f >= p.nFrames) return false;
    return row >= 0 && row < min(max(nOut[f], 0), p.capacity);
}

// the camera centre of device frame f: one camera GetCameraCenter of frame f; two eyes frame f is eye f & 1 of rig f >> 1 (left:
// GetCameraCenter, right: GetRightCameraCenter); leftOnly: GetCameraCenter of that rig whichever the eye (the reference keyframe, :468)
template <bool TwoEyes>
__device__ __forceinline__ void mpuCentre(const float* poses, const MapPointUpdateParams& p, int f, bool leftOnly, float (&Ow)[3]) {
    const long long kf = TwoEyes ? f >> 1 : f;
    const int eye = TwoEyes && !leftOnly ? f & 1 : 0;
    for (int r = 0; r < 3; r++) Ow[r] = fuseTwoEyesRigElement(poses + kf * 12, p.tlr, eye * kRigEyeFloats + 12 + r);
}

// cv::norm(Pos - Ow): the difference in float (d), squares summed and rooted in double
__device__ __forceinline__ double mpuNorm(const float (&pos)[3], const float (&Ow)[3], float (&d)[3]) {
    for (int c = 0; c < 3; c++) d[c] = __fsub_rn(pos[c], Ow[c]);
    return __dsqrt_rn(dot3Double(d[0], d[1], d[2], d[0], d[1], d[2]));
}

// normali * (float)(1.0 / norm): the products of one entry's scaleAdd (:456-457, :462-463)
__device__ __forceinline__ void mpuUnit(const float (&pos)[3], const float (&Ow)[3], float (&t)[3]) {
    float d[3];
    const float inv = (float)__ddiv_rn(1.0, mpuNorm(pos, Ow, d));
    for (int c = 0; c < 3; c++) t[c] = __fmul_rn(d[c], inv);
}

// ... and its sum onto normal, one entry after the other
__device__ __forceinline__ void mpuAccumulate(float (&normal)[3], float t0, float t1, float t2) {
    normal[0] = __fadd_rn(t0, normal[0]); normal[1] = __fadd_rn(t1, normal[1]); normal[2] = __fadd_rn(t2, normal[2]);
}

// :468-492: mNormalVector = normal/n into normalOut[3]; Fuse's triple 0.8f*mfMinDistance, 1.2f*mfMaxDistance, mfMaxDistance into distOut[3]
__device__ __forceinline__ void mpuFinish(const float (&normal)[3], int n, const float (&pos)[3], const float (&OwRef)[3], int octave,
                                          const MapPointUpdateParams& p, float* normalOut, float* distOut) {
    const float invN = (float)__ddiv_rn(1.0, (double)n);
    for (int c = 0; c < 3; c++) normalOut[c] = __fmul_rn(normal[c], invN);
    float d[3];
    const float dist = (float)mpuNorm(pos, OwRef, d);
    const int level = min(max(octave, 0), p.nlevels - 1);
    const float maxD = __fmul_rn(dist, p.scale[level]), minD = __fdiv_rn(maxD, p.scale[p.nlevels - 1]);
    distOut[0] = __fmul_rn(0.8f, minD); distOut[1] = __fmul_rn(1.2f, maxD); distOut[2] = maxD;
}

// the element of rank need - 1 of values in 0 .. 256: the smallest v with countLE(v) >= need.  Nine steps, countLE is called in every one
// (it may talk to other lanes)
template <class CountLE>
__device__ __forceinline__ int mpuRankSelect(int need, CountLE countLE) {
    int lo = 0, hi = 256;
    for (int s = 0; s < 9; s++) {
        const int mid = (lo + hi) >> 1;
        const bool enough = countLE(mid) >= need;
        if (lo < hi) { if (enough) hi = mid; else lo = mid + 1; }
    }
    return lo;
}
__device__ __forceinline__ int mpuNeed(int participants) { return (participants - 1) / 2 + 1; }

// the normal and depth half of one point once its entries' products lie in unit[3 * e + c]: the serial sum, the reference entry, the rows
template <bool TwoEyes, class UnitPtr>
__device__ __forceinline__ void mpuNormalAndDepth(const MapPointUpdateArrays& a, const MapPointUpdateParams& p, int n, long long off0, int ref,
                                                  long long slot, const float (&pos)[3], UnitPtr unit) {
    float normal[3] = {0.f, 0.f, 0.f};
    for (int e = 0; e < n; e++) mpuAccumulate(normal, unit[3 * e], unit[3 * e + 1], unit[3 * e + 2]);
    const int f = a.obs[2 * (off0 + ref)], row = a.obs[2 * (off0 + ref) + 1];
    float OwRef[3];
    mpuCentre<TwoEyes>(a.poses, p, f, true, OwRef);
    mpuFinish(normal, n, pos, OwRef, a.kps[(long long)f * p.capacity + row].octave, p, a.mpNormal + 3 * slot, a.mpDist + 3 * slot);
}

#ifdef ORBX_HOST_ROW
// One point, one thread: the whole statement in list order.  The host build only (the row of distances is a local array).
template <bool TwoEyes>
inline void mpuPointSerial(const MapPointUpdateArrays& a, const MapPointUpdateParams& p, long long m) {
    const int n = mpuListLength(a.obsOff, m);
    a.best[m] = -1; a.bestMedian[m] = -1;
    if (n == 0) { a.status[m] = kMpuEmpty; return; }
    if (n > kMpuMaxObservations) { a.status[m] = kMpuTooLong; return; }
    const int off0 = a.obsOff[m], ref = a.ref[m];
    const long long slot = a.slot ? a.slot[m] : m;
    bool ok = mpuHeadOk(off0, slot, ref, n);
    static thread_local int frames[kMpuMaxObservations], rows[kMpuMaxObservations], dist[kMpuMaxObservations];
    static thread_local float unit[3 * kMpuMaxObservations];
    for (int e = 0; ok && e < n; e++) ok = mpuEntryOk(a.obs, (long long)off0 + e, a.nOut, p, frames[e], rows[e]);
    if (!ok) { a.status[m] = kMpuBadIndex; return; }
    int status = kMpuOk;
    if (p.what & 1) {
        int part[kMpuMaxObservations], P = 0;      // the entries that take part, in order
        for (int e = 0; e < n; e++)
            if (!(a.obsFlags && (a.obsFlags[off0 + e] & 1))) part[P++] = e;
        if (P == 0) status = kMpuNoDescriptor;
        else {
            auto row = [&](int i) { return (const uint4*)(a.desc + ((long long)frames[part[i]] * p.capacity + rows[part[i]]) * 32); };
            int bestKey = 0x7fffffff;
            for (int i = 0; i < P; i++) {
                for (int j = 0; j < P; j++) dist[j] = i == j ? 0 : hamming256(row(i)[0], row(i)[1], row(j)[0], row(j)[1]);
                const int median = mpuRankSelect(mpuNeed(P), [&](int v) { int c = 0; for (int j = 0; j < P; j++) c += dist[j] <= v; return c; });
                bestKey = min(bestKey, median << 16 | i);
            }
            const int b = bestKey & 0xffff;
            std::memcpy(a.mpDesc + slot * 32, row(b), 32);
            a.best[m] = b; a.bestMedian[m] = bestKey >> 16;
        }
    }
    if (p.what & 2) {
        const float pos[3] = {a.mpWorld[3 * slot], a.mpWorld[3 * slot + 1], a.mpWorld[3 * slot + 2]};
        for (int e = 0; e < n; e++) {
            float Ow[3], t[3];
            mpuCentre<TwoEyes>(a.poses, p, frames[e], false, Ow);
            mpuUnit(pos, Ow, t);
            for (int c = 0; c < 3; c++) unit[3 * e + c] = t[c];
        }
        mpuNormalAndDepth<TwoEyes>(a, p, n, off0, ref, slot, pos, (const float*)unit);
    }
    a.status[m] = (uint8_t)status;
}
#endif

}  // namespace orbx
