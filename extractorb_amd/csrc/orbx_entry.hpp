// orbx_entry.hpp - the plain statements the C entry points of orbx_rows.cpp share: argument predicates, the LDS budget, the fills of the kernels'
// parameter blocks (templates over the block: no layout is named here), the level-table padding rules, and the order of "free, then allocate
// all or nothing" of a growable set of buffers.  Host only, no HIP, allocates nothing: tests/cpp/entry_check.cpp compiles it with g++ behind
// tests/cpp/host_shim and tests/test_entry_helpers.py compares every function with an independent statement.
#pragma once
#include <cmath>
#include <cstddef>
#include <initializer_list>

#include "orbx.h"
#include "orbx_geometry.hpp"
#include "orbx_params.hpp"

namespace orbx {

// ---- predicates -------------------------------------------------------------------------------------------------------------------
// written so that a NaN bound is empty
inline bool emptyBounds(const float* bounds4) { return !(bounds4[1] > bounds4[0]) || !(bounds4[3] > bounds4[2]); }
// The entries name the frames (keyframes, MapPoint lists) of pair p as first + p * step.  Two rules exist and they differ on negative steps:
// the walk rule lets a step be negative as long as no pair's index is (BoW, triangulation, Fuse, Sim3, frustum) ...
inline bool negativeWalk(int first, int step, int n) { return first < 0 || first + (long long)(n - 1) * step < 0; }
// ... the older rule refuses every negative step (SearchForInitialization, the frame-to-frame and local-map projection searches)
inline bool negativeFirstOrStep(int first, int step) { return first < 0 || step < 0; }

// orbx_fuse_two_eyes_device's `eyes`: bit 0 the left search, bit 1 the right; the loop-closing overload (reproj_check = 0) has no right-eye form
inline bool badFuseEyes(int eyes, int reprojCheck) { return eyes < 1 || eyes > 3 || (!reprojCheck && eyes != 1); }

// orbx_update_map_points*_device's `what`: bit 0 the descriptor, bit 1 normal and depth; one of them at least, nothing else
inline bool badUpdateWhat(int what) { return what < 1 || what > 3; }

// ---- limits -----------------------------------------------------------------------------------------------------------------------
constexpr size_t kLdsBudget = 160 * 1024 - 512;      // dynamic + static LDS a workgroup of the LDS-resident searches may ask for (160 KB per CU)
inline bool fitsLds(size_t bytes) { return bytes <= kLdsBudget; }
// orbx_search_by_bow_device alone keeps a bound of its own, NOT kLdsBudget: the 150 KB its launch wrapper (k_bow_match.hip) chooses its staged
// form with.  The one-camera BoW search predates kLdsBudget and which capacities it accepts is behaviour
constexpr size_t kBowMatchLdsBudget = 150 * 1024;
inline int clampDistance(int d) { return d < 255 ? d : 255; }      // no descriptor distance exceeds 255: a larger bound accepts the same matches

// orbx_detect_candidates_device: both kernels' tables must fit (k_place_recognition.hip).  160 KB - 512 holds 12 bytes for each of 13610 query
// words, and 12 * 8192 + 4 * 8192 + 80 bytes of lists for 8192 rows; 8193 rows need a sort of 16384 slots, which does not fit
inline bool placeFits(int nDb, int qCapacity) { return fitsLds(prPairLdsBytes(qCapacity)) && fitsLds(prQueryLdsBytes(nDb)); }
// ... and what it refuses as ORBX_ERR_BAD_ARGUMENT, the handle apart: the pointers as the entry was given them.  The database's arrays and
// d_score may be NULL when n_db == 0, d_loop / d_merge when n_candidates == 0, d_cand when cand_capacity == 0; d_connected and
// d_common_words are optional.  n_candidates stays below 2^30 (k_place_query packs a list position beside two flag bits)
inline bool placeBadArgument(const void* v, int mode, int nDb, const void* dbIds, const void* dbW, const void* dbN, int capacity, const void* dbMap,
                             const void* dbFlags, const void* dbCovis, int nQueries, int qFirst, int qStep, const void* qIds, const void* qW,
                             const void* qN, int qCapacity, const void* qMap, int nCandidates, const void* score, const void* result, const void* loop,
                             const void* merge, const void* cand, int candCapacity) {
    const bool nBest = mode == ORBX_PLACE_N_BEST;
    return !v || (mode != ORBX_PLACE_N_BEST && mode != ORBX_PLACE_RELOCALIZATION) || nDb < 0 || nQueries < 1 || nQueries > 65535 || capacity < 1 ||
           qCapacity < 1 || !qIds || !qW || !qN || !qMap || !result || negativeWalk(qFirst, qStep, nQueries) ||
           (nDb > 0 && (!dbIds || !dbW || !dbN || !dbMap || !dbFlags || !dbCovis || !score)) ||
           (nBest && (nCandidates < 0 || nCandidates > 0x3fffffff || (nCandidates > 0 && (!loop || !merge)) || (long long)nQueries * nCandidates > 0x7fffffffLL)) ||
           (!nBest && (candCapacity < 0 || (candCapacity > 0 && !cand) || (long long)nQueries * candCapacity > 0x7fffffffLL)) ||
           (long long)nQueries * nDb > 0x7fffffffLL;
}
// ... and as ORBX_ERR_UNSUPPORTED: a scoring other than L1_NORM (0), a database or a query capacity past the LDS bounds
inline bool placeUnsupported(int scoring, int nDb, int qCapacity) { return scoring != 0 || !placeFits(nDb, qCapacity); }
static_assert(prQueryLdsBytes(kPrMaxDb) <= kLdsBudget && prQueryLdsBytes(kPrMaxDb + 1) > kLdsBudget, "kPrMaxDb is the LDS bound on n_db");
static_assert(prPairLdsBytes(kPrMaxQueryWords) <= kLdsBudget && prPairLdsBytes(kPrMaxQueryWords + 1) > kLdsBudget, "kPrMaxQueryWords is the LDS bound on q_capacity");

// orbx_covisibility_device: k_covis_vote holds 8 bytes of sort key per list slot - a power of two of slots, every frame may be listed - and a
// counter word per frame: 12 * 8192 + 48 bytes for 8192 frames; 8193 frames need a sort of 16384 slots (131072 + 32772 + 48 bytes), which
// does not fit 160 KB - 512.  conn_capacity takes no LDS: the lists are written from the counters and the sorted keys
inline bool covisFits(int nFrames) { return nFrames <= kCvMaxFrames && fitsLds(cvVoteLdsBytes(nFrames)); }
// ... what it refuses as ORBX_ERR_BAD_ARGUMENT, the handle apart.  UPDATE_CONNECTIONS reads the three arrays of its self and map tests and
// writes the ordered block; LOCAL_KEYFRAMES reads and writes none of them.  The list blocks may be NULL when conn_capacity == 0
inline bool covisBadArgument(int mode, int nPoints, const void* obsOff, const void* obs, const void* mpFlags, int nFrames, const void* kfFlags,
                             const void* kfMap, const void* kfKey, int nSubjects, const void* subjectMp, const void* subjectN, int capacity,
                             const void* subjectKf, const void* subjectMap, int connCapacity, const void* counterKf, const void* counterW,
                             const void* orderedKf, const void* orderedW, const void* result) {
    const bool update = mode == ORBX_COVIS_UPDATE_CONNECTIONS;
    return (mode != ORBX_COVIS_UPDATE_CONNECTIONS && mode != ORBX_COVIS_LOCAL_KEYFRAMES) || nPoints < 0 || nFrames < 1 || nSubjects < 1 ||
           nSubjects > 65535 || capacity < 1 || connCapacity < 0 || !obsOff || !obs || !mpFlags || !kfFlags || !kfKey || !subjectMp || !subjectN ||
           !result || (update && (!kfMap || !subjectKf || !subjectMap)) || (connCapacity > 0 && (!counterKf || !counterW)) ||
           (update && connCapacity > 0 && (!orderedKf || !orderedW)) || (long long)nSubjects * capacity > 0x7fffffffLL ||
           (long long)nSubjects * connCapacity > 0x7fffffffLL;
}
inline bool covisUnsupported(int nFrames) { return !covisFits(nFrames); }
static_assert(cvVoteLdsBytes(kCvMaxFrames) <= kLdsBudget && cvVoteLdsBytes(kCvMaxFrames + 1) > kLdsBudget, "kCvMaxFrames is the LDS bound on n_frames");

// orbx_keyframe_redundancy_device: a state byte per slot (rounded up to a dword) and 48 bytes of scratch words: capacity <= 163280
inline bool redundancyFits(int capacity) { return capacity <= kRdMaxCapacity && fitsLds(rdLdsBytes(capacity)); }
// ... what it refuses as ORBX_ERR_BAD_ARGUMENT.  d_mp_nobs and d_slot_state are optional; d_depth / d_th_depth are read when monocular == 0.
// A NaN redundant_th is refused: no keyframe could be redundant
inline bool redundancyBadArgument(int nPoints, const void* obsOff, const void* obs, const void* mpFlags, int nFrames, const void* kfFlags,
                                  const void* kpsUn, const void* nOut, const void* depth, const void* thDepth, int nSubjects, const void* subjectMp,
                                  const void* subjectN, int capacity, const void* subjectKf, int monocular, float redundantTh, const void* result) {
    return nPoints < 0 || nFrames < 1 || nSubjects < 1 || nSubjects > 65535 || capacity < 1 || !obsOff || !obs || !mpFlags || !kfFlags || !kpsUn ||
           !nOut || !subjectMp || !subjectN || !subjectKf || !result || (!monocular && (!depth || !thDepth)) || redundantTh != redundantTh ||
           (long long)nSubjects * capacity > 0x7fffffffLL;
}
inline bool redundancyUnsupported(int capacity) { return !redundancyFits(capacity); }
static_assert(rdLdsBytes(kRdMaxCapacity) <= kLdsBudget && rdLdsBytes(kRdMaxCapacity + 1) > kLdsBudget, "kRdMaxCapacity is the LDS bound on capacity");

// Sim3Solver::SetRansacParameters' nIterations for N correspondences, before max(1, min(., maxIterations)) (reference src/Sim3Solver.cc:
// 137-147): epsilon is a FLOAT, pow / log / ceil run in double, minInliers == N gives 1.  The reference assigns the double to an int: a value
// outside the int range (epsilon^3 below 2^-53 gives log(1) = 0 and an infinite quotient) converts as its x86-64 build does, to INT_MIN.
// N < 1 has no epsilon; such a problem never iterates and the entry stores 1.
inline int sim3RansacIterations(double probability, int minInliers, int N) {
    if (N < 1 || minInliers == N) return 1;
    const float epsilon = (float)minInliers / N;
    const double v = std::ceil(std::log(1 - probability) / std::log(1 - std::pow(epsilon, 3)));
    return (v > -2147483649.0 && v < 2147483648.0) ? (int)v : (-2147483647 - 1);
}

// ---- fills of a parameter block ---------------------------------------------------------------------------------------------------
template <class P> inline void fillGridInverses(P& p, const float* bounds4) {
    p.wInv = (float)kGridCols / (bounds4[1] - bounds4[0]);      // mfGridElementWidthInv  (Frame.cc:339)
    p.hInv = (float)kGridRows / (bounds4[3] - bounds4[2]);      // mfGridElementHeightInv (Frame.cc:340)
}
template <class P> inline void fillGrid(P& p, const float* bounds4) {
    p.minX = bounds4[0]; p.minY = bounds4[2];
    fillGridInverses(p, bounds4);
}
// Frame's own float bounds, compared as they are (Frame.cc:520-523, :1213-1216, ORBmatcher.cc:2209-2212)
template <class P> inline void fillBounds(P& p, const float* bounds4) {
    p.minX = bounds4[0]; p.maxX = bounds4[1]; p.minY = bounds4[2]; p.maxY = bounds4[3];
}
// KeyFrame's mnMinX .. mnMaxY are const int (inc/KeyFrame.h:484) initialised from Frame's floats (KeyFrame.cc:58): truncated toward zero.
// IsInImage (:816-819) and GetFeaturesInArea (:778-790) compare with and subtract the truncated values, but scale by Frame's inverses, made
// from the untruncated floats and copied as they are (KeyFrame.cc:50): a KeyFrame's block takes this and fillGridInverses
template <class P> inline void fillBoundsTruncated(P& p, const float* bounds4) {
    p.minX = truncf(bounds4[0]); p.maxX = truncf(bounds4[1]); p.minY = truncf(bounds4[2]); p.maxY = truncf(bounds4[3]);
}
template <class P> inline void fillPinhole(P& p, const orbx_camera& cam) { p.fx = cam.fx; p.fy = cam.fy; p.cx = cam.cx; p.cy = cam.cy; }
// KannalaBrandt8::mvParameters
inline void fillKb8(float (&dst)[8], const orbx_camera_kb8& cam) {
    dst[0] = cam.fx; dst[1] = cam.fy; dst[2] = cam.cx; dst[3] = cam.cy; dst[4] = cam.k1; dst[5] = cam.k2; dst[6] = cam.k3; dst[7] = cam.k4;
}
// MapPoint::PredictScale's nlevels - 1 breakpoints; the elements from nlevels - 1 on stay what they are (zero in a block made with {})
template <class P> inline void fillBreaks(P& p, const float* breaks, int nlevels) {
    for (int l = 0; l + 1 < nlevels; l++) p.breaks[l] = breaks[l];
}

// ---- level tables: one function per padding rule.  dst is a block's table of kMaxLevels, src the handle's (ScaleTables) ------------------------
// Whether the rules need to differ is not decided here; each is what its kernels have always been given, the elements past nlevels included.
// stereo: 1 past nlevels
inline void levelsPaddedWithOne(float (&dst)[kMaxLevels], const float* src, int nlevels) {
    for (int l = 0; l < kMaxLevels; l++) dst[l] = l < nlevels ? src[l] : 1.f;
}
// the two project_last entries: the coarsest level's value past nlevels (CurrentFrame.mvScaleFactors)
inline void levelsPaddedWithLast(float (&dst)[kMaxLevels], const float* src, int nlevels) {
    for (int l = 0; l < kMaxLevels; l++) dst[l] = l < nlevels ? src[l] : src[nlevels - 1];
}
// triangulation: all kMaxLevels elements of the handle's table, whatever it holds past nlevels (makeScaleTables leaves zeros)
inline void levelsWholeTable(float (&dst)[kMaxLevels], const float* src) {
    for (int l = 0; l < kMaxLevels; l++) dst[l] = src[l];
}
// Fuse, Sim3, the frustum entries: the first nlevels; the rest stays what it is (zero in a block made with {})
inline void levelsOnly(float (&dst)[kMaxLevels], const float* src, int nlevels) {
    for (int l = 0; l < nlevels; l++) dst[l] = src[l];
}

// ---- growable buffers -------------------------------------------------------------------------------------------------------------
// Frees and nulls every item, then allocates all of them.  alloc(void** p, size_t bytes) returns false on failure; on the first failure
// what was obtained is freed again, every pointer is null and the result is false: the caller never holds a part of the set.
struct GrowItem { void** ptr; size_t bytes; };
template <class Alloc, class Free>
inline bool regrow(std::initializer_list<GrowItem> items, Alloc alloc, Free release) {
    auto drop = [&] { for (const GrowItem& it : items) { if (*it.ptr) release(*it.ptr); *it.ptr = nullptr; } };
    drop();
    for (const GrowItem& it : items)
        if (!alloc(it.ptr, it.bytes)) { *it.ptr = nullptr; drop(); return false; }
    return true;
}

}  // namespace orbx
