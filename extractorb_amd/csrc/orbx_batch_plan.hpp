// orbx_batch_plan.hpp - the launch policy of the extraction path as plain data and pure functions (host only: no HIP, no handle, no allocation
// outside buildBlurTables).  orbx_api.cpp asks here WHICH launch forms a geometry and a call take (planGeometry once per image size, planBatch
// once per call, planFront / planBack once per part of a call) and then only enqueues them; tests/cpp/batch_plan_check.cpp prints the same
// plans without a device.  The forms are result-identical: nothing decided here can change a result or make a call fail.
#pragma once
#include "orbx_geometry.hpp"

namespace orbx {

// the blur forms orbx_debug_last_forms reports (include/orbx.h; 2 and 4 named forms that round 6 removed)
enum BlurForm {
    kBlurLevels = 0,        // k_blur writes every blurred level
    kBlurInFast = 1,        // the blur's lanes ride in the FAST launch (small batches)
    kBlurPerKeypoint = 3,   // k_describe<PB> blurs every keypoint's patch itself: no blurred level exists
    kBlurSplitByLevel = 5,  // per keypoint below the split level, k_blur + k_describe<plain> from it on
};
inline bool blursPerKeypoint(int form) { return form == kBlurPerKeypoint || form == kBlurSplitByLevel; }
// the pyramid forms of the same report
enum PyrForm { kPyrRegionMajor = 0, kPyrPerLevel = 1 };

enum { kStageFront = 1, kStageBack = 2 };      // front: pyramid (+ blur) = ComputePyramid; back: FAST, quad-tree, orientation, descriptors

// What orbx_create reads once (the launch-policy switches, orbx_debug_policy) and the facts of the device.
struct LaunchPolicy {
    int numCUs = 256;
    int nfeatures = 0;
    int pyrCols = -1;                   // ORBX_PYR_COLS: 1 = the region-major pyramid for every batch it fits, 0 = never, default: the smallest batches
    int fastWide = -1;                  // ORBX_FAST_WIDE: 1 = a workgroup per FAST cell (k_fast_wide) whatever the batch, 0 = never, default: while a call holds few cells
    int patchBlur = -1;                 // ORBX_PATCH_BLUR: 1 = k_describe blurs each keypoint's patch itself (no blurred levels), 0 = never, default: by features per pixel (planBatch)
    int blurSplit = -1;                 // ORBX_BLUR_SPLIT=L: where the blur is per keypoint, only levels < L are (k_describe<PB>); levels >= L are blurred by k_blur and
                                        // described from the blurred level (the patches of the coarse levels hold more pixels than the levels); 0 = no split; default: planGeometry
    int colsShape = -1;                 // test aid "pyr_cols_shape": workgroup shape of k_pyr_cols (launchPyrCols: 1, 4 or 6; default: by the grid size)
    int splitMode = 1;                  // ORBX_SPLIT: 1 (default) = large batches overlap their blur with FAST + quad-tree on a side stream (the largest also stagger
                                        // their tails: planBatch); 0 = no overlap of any kind; 3 = staggered tails for every large batch
    bool fuseSmall = true;              // ORBX_FUSE_SMALL=0: small batches keep the blur as a launch of its own
    long long splitMinPixels = 0;       // ORBX_SPLIT_MIN_MPX: smallest half (pyramid pixels) worth its own kernels
    int leafFrames = 0;                 // frames covered by the leaf tables (ORBX_LEAF_FRAMES, default 128; 0 = off)
    int octThreadsForced = 0;           // ORBX_OCT_THREADS
    bool octRoomyForced = false;        // ORBX_OCT_ROOMY: the 128-VGPR variants whatever the batch (tests reach every variant with it)
    bool resizeBytewise = false;        // ORBX_RESIZE_BYTEWISE: force the byte-gather resize (diagnostic)
    bool octArena = false;              // the quad-tree's node arrays live in an HBM arena (too large for LDS): k_octree_1024g
};

// ---- per geometry -------------------------------------------------------------------------------------------------------------------

// The automatic split level of the per-keypoint blur (planGeometry): k_blur takes the levels whose patches hold more than kSplitRatioNum /
// kSplitRatioDen of the level's pixels.  Measured (round 6, A/B in one call, us per step): 512 x 640x480 x 1000 - no split 1696-1699, split at level
// 2 (patches 1.36 of the level) 1667-1668, at 3 (1.63) 1656-1666, at 4 (1.96) 1664-1674, at 5 1674-1680, k_blur for every level 1707-1710; 128 x
// 1080p x 2000, where the coarsest level's patches reach 0.99 of it: no split 2290, at 7 2316-2321, at 6 2318-2331, at 4 2355-2367 - so the
// levels past 1.5.
constexpr int kSplitRatioNum = 3, kSplitRatioDen = 2;

// The blur tables of a geometry: [0] 32-row blocks of every level, [1] 8-row blocks (small batches), [2] 32-row blocks of the levels >= splitLevel
// (the blur split by level; empty without a split).
constexpr int kBlurTableRows[3] = {kBlurBlockRows, kBlurBlockRowsSmall, kBlurBlockRows};
// the items of table v in table order: f(level, first row, lanes of the row block)
template <class F>
inline void forEachBlurItem(const FrameGeom& g, int v, int splitLevel, F f) {
    if (v == 2 && splitLevel == 0) return;
    for (int l = 0; l < g.nlevels; l++) {
        if (v == 2 && l < splitLevel) continue;               // the finest levels are blurred per keypoint
        for (int y0 = 0; y0 < g.lv[l].h; y0 += kBlurTableRows[v]) f(l, y0, (g.lv[l].w + 3) / 4);
    }
}

struct GeometryPlan {
    int splitLevel = 0;                 // the level table [2] starts at (0: no such table)
    int octThreads = 256;               // quad-tree workgroup size of queued launches (one size for all levels, chosen by the image area - separate
                                        // launches per size measured slower)
    int nBlurLanes[3] = {0, 0, 0}, nBlurItems[3] = {0, 0, 0};
    size_t blurItemOff[3] = {0, 0, 0}, blurLaneOff[3] = {0, 0, 0};      // first item / first lane of each table in the two arrays of buildBlurTables
};

inline GeometryPlan planGeometry(const FrameGeom& g, const LaunchPolicy& p) {
    GeometryPlan gp;
    // The blur split by level (round 6): where the blur is done per keypoint (k_describe<PB>), the patches of a coarse level hold more pixels than the
    // level itself - quota x 37 x 36 (the disc of the 43 x 37 horizontal pass + the 37 x 37 vertical one) against w x h; 640x480 x 1000: 0.94 of the
    // level's pixels at level 0, 1.63 at level 3, 3.4 at level 7 - so from the first level whose patches exceed kSplitRatio x its pixels on, k_blur
    // blurs the level (table [2]) and k_describe reads the blurred level.  ORBX_BLUR_SPLIT=L pins the level, 0 turns the split off.
    int splitLevel = 0;
    if (p.blurSplit > 0) splitLevel = p.blurSplit;
    else if (p.blurSplit < 0 && kSplitRatioNum > 0) {
        for (int l = 1; l < g.nlevels && !splitLevel; l++)
            if ((long long)g.lv[l].quota * 37 * 36 * kSplitRatioDen > (long long)kSplitRatioNum * g.lv[l].w * g.lv[l].h) splitLevel = l;
        // ... if those levels hold a quarter of the features: two more launches for the coarsest level alone cost more than its patches (128 x
        // 1280x720 x 1500, where only level 7 - 6 % of the features - is past 1.5: 1146 us per step split, 1128 unsplit)
        int tail = 0;
        for (int l = splitLevel; splitLevel && l < g.nlevels; l++) tail += g.lv[l].quota;
        if (4 * tail < p.nfeatures) splitLevel = 0;
    }
    if (splitLevel >= g.nlevels) splitLevel = 0;
    gp.splitLevel = splitLevel;
    size_t items = 0, lanes = 0;
    for (int v = 0; v < 3; v++) {
        gp.blurItemOff[v] = items; gp.blurLaneOff[v] = lanes;
        forEachBlurItem(g, v, splitLevel, [&](int, int, int n) { gp.nBlurItems[v]++; gp.nBlurLanes[v] += n; });
        items += gp.nBlurItems[v]; lanes += gp.nBlurLanes[v];
    }
    const long long px = (long long)g.lv[0].w * g.lv[0].h;
    gp.octThreads = px <= 500000 ? 256 : (px <= 1200000 ? 512 : 1024);   // measured: 640x480 -> 256, 1280x720 -> 512, 1920x1080 -> 1024 (512 equal)
    if (p.octThreadsForced == 256 || p.octThreadsForced == 512 || p.octThreadsForced == 1024) gp.octThreads = p.octThreadsForced;
    return gp;
}

// The blur item / lane tables of the plan, table after table: items[blurItemOff[v]].count holds table v's item count, laneItem the item (counted
// from its table's first) of every lane.  False: a table holds more items than a lane's 16-bit item number can name.
inline bool buildBlurTables(const FrameGeom& g, const GeometryPlan& gp, std::vector<BlurItem>& items, std::vector<unsigned short>& laneItem) {
    items.clear(); laneItem.clear();
    for (int v = 0; v < 3; v++) {
        if (gp.nBlurItems[v] > 65535) return false;
        const size_t t0 = items.size();
        int lanes = 0;
        forEachBlurItem(g, v, gp.splitLevel, [&](int l, int y0, int n) {
            laneItem.insert(laneItem.end(), (size_t)n, (unsigned short)(items.size() - t0));
            items.push_back(BlurItem{lanes, 0, (short)l, (short)y0});
            lanes += n;
        });
        if (items.size() > t0) items[t0].count = (int)(items.size() - t0);
    }
    return true;
}

// ---- per call -----------------------------------------------------------------------------------------------------------------------

// What the earlier call left on the handle and what the caller switched on.
struct CallState {
    int lastBlurForm = -1, lastSplitLevel = 0;      // the blur form (and its split level) of the last front part
    bool blurOwed = false;                          // that front part left the blur to the FAST launch that follows
    bool profiling = false;                         // event profiling (orbx_profile_enable): one kernel at a time
};

inline bool smallFrame(const FrameGeom& g) { return (long long)g.rows * g.cols <= 512 * 1024; }      // frames up to half a megapixel
// what k_fast / k_fast_wide hold of a cell's ROI (k_fast.hip: fastCanCarryBlur states the same limit for the blur's lanes)
inline bool roiFitsFastTile(const FrameGeom& g) { return g.maxRoiW <= 45 && g.maxRoiH <= 45; }
// blur: throughput form (32-row blocks, table [0]) once the grid fills the chip, else the short-chain form (8-row blocks, table [1]) ...
inline int blurVariant(const GeometryPlan& gp, const LaunchPolicy& p, int Bn) { return (long long)gp.nBlurLanes[0] * Bn >= 64LL * 2 * 4 * p.numCUs ? 0 : 1; }   // two waves per SIMD of 32-row lanes
// ... which in unprofiled small batches rides in the FAST launch (back) instead of being a launch of its own
inline bool blurRidesWithFast(const FrameGeom& g, const GeometryPlan& gp, const LaunchPolicy& p, const CallState& s, int Bn) {
    return blurVariant(gp, p, Bn) == 1 && !s.profiling && p.fuseSmall && roiFitsFastTile(g) && !g.big;
}

struct BatchPlan {
    bool bigBatch = false;      // the call holds ORBX_SPLIT_MIN_MPX of pyramid pixels
    bool patchBlur = false;     // k_describe<PB> blurs per keypoint ...
    int splitL = 0;             // ... the levels below this one (0: all of them); k_blur + k_describe<plain> from it on
    bool blurSide = false;      // the blur runs on the side stream beside FAST and the quad-tree
    bool stagger = false;       // FAST in two halves, the first half's tails on the internal stream
    int B0 = 0;                 // frames of the first half
};

inline BatchPlan planBatch(const FrameGeom& g, const GeometryPlan& gp, const LaunchPolicy& p, const CallState& s, int B, int stages) {
    BatchPlan b;
    const bool doFront = (stages & kStageFront) != 0, doBack = (stages & kStageBack) != 0;
    const bool rides = blurRidesWithFast(g, gp, p, s, B);
    // Patch blur (k_describe<PB>): no blurred levels at all - every keypoint's 37 x 37 patch is blurred out of its raw 43 x 43 tile.  It pays where
    // the keypoints' patches are not a much larger job than the whole pyramid (nfeatures x 43 x 37 pixels of horizontal pass against the pyramid's
    // pixels) and the blur would be a launch of its own (not the small-batch form that rides in the FAST launch) - k_describe is bound by its sparse
    // patch reads at large frames, and the one raw tile is fewer bytes than a raw + a blurred one.  Measured (us per step, k_blur beside FAST ->
    // patch blur): 128 x 1920x1080 x 2000 (ratio 0.50) 3041-3052 -> 2717-2723; 128 x 1280x720 x 1500 (0.84) 1448-1455 -> 1358-1364; 512 x 640x480 x
    // 1000 (1.67) 1929-1937 -> 1993-2000: taken up to a ratio of 1.25.  ORBX_PATCH_BLUR=1 / 0 forces / forbids it.
    // Round 5: ... and up to a ratio of 1.75 once the batch is large (>= 240 Mpx of pyramid: 256 frames of 640x480 x 1000).  Since round 4's
    // instruction work the two forms are level there (512 x 640x480 x 1000: 1725-1729 us with k_blur beside FAST, 1735 with the patch blur, A/B in
    // one gpurun call, -0.4 ... -0.6 %; 256 / 1024 frames the same; 64 frames -1.5 %, 1200 features per frame -3.5 %: not taken there), and the
    // patch blur moves 4.75 MB per frame through HBM instead of 8.0 (no blurred level is written or re-read) and leaves the
    // blurred arena (1 MB per frame) untouched: where the clock says "equal", the bytes decide.
    // A back-only pass (orbx_compute_keypoints_octree) describes from what the front part of the EARLIER call left: if that call blurred per
    // keypoint (form 3) no blurred level exists and this pass must do the same, whatever its own frame count would choose; otherwise the blurred
    // levels exist (or are owed to the FAST launch: blurOwed) and are used.
    // (round 6: "big" from ORBX_SPLIT_MIN_MPX = 120 Mpx of pyramid per call, the same threshold as the per-keypoint blur below - rounds 4-5: twice
    // that -: 128 x 640x480 with the coarse levels' blur aside and staggered tails 457 -> 450 us)
    b.bigBatch = (long long)g.sumPixels * B >= p.splitMinPixels;
    const long long patchPx4 = (long long)p.nfeatures * 43 * 37 * 4;      // 4 x the patches' pixels of horizontal pass
    // Round 6: with the coarse levels split off to k_blur (planGeometry: splitLevel) the per-keypoint form also wins earlier and further - from
    // 120 Mpx of pyramid per call (128 x 640x480: 468 -> 459 us; 64 frames: 232 -> 248, not taken) and up to a ratio of 2.25 (512 x 640x480 x 1200
    // features, the stereo stream, 2.0: 1758 -> 1743 us).
    b.patchBlur = !doFront ? blursPerKeypoint(s.lastBlurForm)
                           : (p.patchBlur > 0 || (p.patchBlur < 0 && !rides && (patchPx4 <= 5LL * g.sumPixels || (b.bigBatch && patchPx4 <= 9LL * g.sumPixels))));
    // ... split by level: levels >= splitL are blurred by k_blur and described from the blurred level (planGeometry: splitLevel)
    b.splitL = !b.patchBlur ? 0 : (!doFront ? (s.lastBlurForm == kBlurSplitByLevel ? s.lastSplitLevel : 0)
                                            : (gp.splitLevel > 0 && gp.splitLevel < g.nlevels && gp.nBlurLanes[2] > 0 ? gp.splitLevel : 0));
    // Overlap inside one call (round 4): the blurred levels are read by k_description only, the LAST launch, so the blur of a large batch runs on
    // a side stream beside FAST and the quad-tree: pyramid -> {blur | FAST -> quad-tree} -> description.  k_blur is the one HBM-bound kernel of the
    // path (0.53 of the issue rate), k_fast sits at the issue ceiling with idle memory pipes: 512 x 640x480 2016-2040 us unsplit, 1981-1988 as two
    // halves side by side (round 2's form), 1915-1933 with the blur aside (two halves AND the blur aside: 1932-1937); 256 frames 1035-1055 / 1001-1014 /
    // 999-1007; 128 x 1080p 3094-3136 (halves) -> 3021-3029; 128 frames of 640x480 and fewer: no difference.  A low-priority side stream only starts
    // the blur when everything else is done (2022-2030).  ORBX_SPLIT=0: no overlap of any kind (profiling runs: one kernel at a time).  (Round 2's two
    // half-batches side by side - removed in round 4 - are the "halves" figures above; profiles/r02_split_sweep.md.)
    b.blurSide = p.splitMode != 0 && b.bigBatch && !s.profiling && doFront && doBack;
    // Staggered tails (the largest batches: 1.5 x the pixels of `bigBatch` - round 5: 384 x 640x480 1315-1324 -> 1301-1308 us, 256 frames no difference;
    // rounds 3-4: twice; ORBX_SPLIT=3: every big batch): FAST in two halves back to back on the
    // caller's stream; the first half's quad-tree and description (barrier- and latency-bound: 0.4-0.6 of the issue rate) run on the internal
    // stream under the second half's FAST.  512 x 640x480: 1913-1914 -> 1888-1894 us; 256 frames and 128 x 1080p: no difference (k_fast fills the chip;
    // what runs beside it mostly adds its own issue time)
    // (never with the blur riding in the FAST launch, the form of SMALL batches, which an ORBX_SPLIT_MIN_MPX=0 test run also counts as big: the
    // whole-batch pyramid would leave the blur to the FIRST half's FAST launch only — found by the batch-shape fuzz)
    // (round 6, with the blur split by level: every big batch of small frames - 256 x 640x480 880 -> 870 us, 320 frames 1085 -> 1063-1069; the stereo
    // stream at 256 frames equal; rounds 3-5 started at 1.5-2 x the pixels of `bigBatch`)
    b.stagger = (p.splitMode == 3 || (p.splitMode == 1 && b.bigBatch && smallFrame(g))) &&
                !s.profiling && B >= 2 && b.bigBatch && doFront && doBack && !rides;
    b.B0 = b.stagger ? (B + 1) / 2 : B;
    return b;
}

// ---- per part of a call: the front (pyramid + blur) of frames [f0, f0 + Bn) ------------------------------------------------------------
struct FrontPlan {
    int cut = -1;                   // the region-major pyramid's cut as an index into g.colSets; -1: one launch per level (k_pyr_first + k_resize)
    int colsShape = 0;              // launchPyrCols' workgroup shape (with a cut)
    const char* resizeKernel = "";  // what runs in the resize slot
    int blurForm = kBlurLevels;     // the form to record (BlurForm)
    int blurTable = -1;             // the blur table (GeometryPlan) this part launches as k_blur; -1: none
    int blurBlockRows = 0;          // ... and its block rows
    bool blurOwed = false;          // the back part of this call - or orbx_compute_keypoints_octree later - brings the blur, in its FAST launch
    int pyrForm() const { return cut >= 0 ? kPyrRegionMajor : kPyrPerLevel; }
};

inline FrontPlan planFront(const FrameGeom& g, const GeometryPlan& gp, const LaunchPolicy& p, const CallState& s, const BatchPlan& b, int Bn) {
    FrontPlan f;
    // The pyramid region by region: one workgroup takes a region of the image through every level (k_pyr_cols; the coarsest cut that still
    // gives the chip ~3/4 workgroup per CU, else the finest).  Frames up to half a megapixel: for every batch size (512 frames of 640x480:
    // 2016 -> 1979 us per call against one launch per level, whose tiles are poorly filled on such small levels); larger frames: while the
    // coarsest cut stays below ~12 workgroups per CU - 1280x720: 16 frames 236 -> 226 us, 32: equal, 64: 767 vs 788; 1920x1080: 16 frames
    // 431 -> 422, 64: 1530 vs 1582, 128: 3119 vs 3222.  (Round 2's per-tile chains, k_pyr_chain, lost to it at every size and were removed in
    // round 4; a geometry whose regions do not fit the kernel's staging - none of the tested ones - takes one launch per level.)
    if (p.pyrCols != 0 && g.colsPacked && !p.resizeBytewise)      // (its steps are the packed ones: the regions carry quad records)
        for (size_t i = 0; i < g.colSets.size(); i++) {
            const FrameGeom::ColumnSet& c = g.colSets[i];
            if (!c.fit || c.ldsBytes > 60 * 1024) continue;
            if (f.cut < 0 || (long long)c.columns.size() * Bn >= 3LL * p.numCUs / 4) f.cut = (int)i;
        }
    if (f.cut >= 0 && p.pyrCols < 0 && !smallFrame(g) && (long long)g.colSets[f.cut].columns.size() * Bn > 12LL * p.numCUs) f.cut = -1;
    if (f.cut >= 0) {
        // workgroup shape (launchPyrCols): while every workgroup has a CU to itself, more threads shorten its levels - 1024 (512 derive, 512
        // write) for the fine cuts, 768 (256 + 512) for the coarse ones, whose levels write more than they derive; else 512 (256 + 256).
        // One frame 40.9 -> 39.8 us, two 45.8 -> 44.6, four 58.3 -> 55.7, eight 71.5 -> 67.1; from 32 frames on the small shape wins
        const FrameGeom::ColumnSet& c = g.colSets[f.cut];
        f.colsShape = p.colsShape > 0 ? p.colsShape : ((long long)c.columns.size() * Bn <= p.numCUs ? (c.px <= 56 ? 6 : 4) : 1);
    }
    f.resizeKernel = f.cut >= 0 ? "k_pyr_cols" : "k_resize";
    // blur: throughput form (32-row blocks) once the grid fills the chip, else the short-chain form (8-row blocks), which in
    // unprofiled small batches rides in the FAST launch (back) instead of being a launch of its own
    const bool rides = blurRidesWithFast(g, gp, p, s, Bn);
    f.blurForm = b.patchBlur ? (b.splitL ? kBlurSplitByLevel : kBlurPerKeypoint) : (rides ? kBlurInFast : kBlurLevels);
    f.blurOwed = !b.patchBlur && rides;
    if (b.patchBlur) {
        if (b.splitL) { f.blurTable = 2; f.blurBlockRows = kBlurTableRows[2]; }      // the coarse levels; levels < splitL: k_describe blurs per keypoint, no blurred level is written
    } else if (!rides) {
        f.blurTable = blurVariant(gp, p, Bn);
        f.blurBlockRows = kBlurTableRows[f.blurTable];
    }
    return f;
}

// ---- ... and the back (FAST, quad-tree, description) of frames [f0, f0 + Bn) ----------------------------------------------------------
struct BackPlan {
    bool leafTables = false;        // k_fast's emit does the quad-tree's first sweep (leaf counters and best keys in L2); k_octree loads and clears them
    bool carry = false;             // the FAST launch carries the owed blur's lanes
    bool blurFirst = false;         // the owed blur is a launch of its own (table [1]) in front of FAST
    bool wide = false;              // a workgroup per FAST cell
    const char* fastKernel = "";
    int octT[kMaxLevels] = {};      // quad-tree workgroup size per level
    bool roomy = false;             // its scratch-free build
    const char* octKernel = "";
};

// the quad-tree builds by rocprofv3's name: [256 | 512 | 1024 threads][queued | roomy][one- | two-dword candidates], and the HBM-arena build
constexpr const char* kOctKernelNames[3][2][2] = {{{"k_octree_256", "k_octree_256b"}, {"k_octree_256r", "k_octree_256rb"}},
                                                  {{"k_octree_512", "k_octree_512b"}, {"k_octree_512r", "k_octree_512rb"}},
                                                  {{"k_octree_1024", "k_octree_1024b"}, {"k_octree_1024r", "k_octree_1024rb"}}};
constexpr const char* kOctArenaKernelNames[2] = {"k_octree_1024g", "k_octree_1024gb"};

// blurOwed: what the front part of this call, or else the earlier call, left owed (CallState::blurOwed at the time of this part's FAST launch)
inline BackPlan planBack(const FrameGeom& g, const GeometryPlan& gp, const LaunchPolicy& p, const CallState& s, int f0, int Bn, bool blurOwed) {
    BackPlan k;
    // small batches: k_fast's emit does the quad-tree's first sweep (leaf counters and best keys in L2); k_octree loads and clears them
    k.leafTables = p.leafFrames && f0 + Bn <= p.leafFrames && !g.big;
    k.carry = blurOwed && blurRidesWithFast(g, gp, p, s, Bn);
    k.blurFirst = blurOwed && !k.carry;      // (a front part that counted on this launch, and a back part that cannot carry the blur: event profiling switched on in between)
    k.wide = !g.big && (p.fastWide > 0 || (p.fastWide < 0 && (long long)g.cells.size() * Bn <= 4LL * p.numCUs));
    k.fastKernel = k.wide && roiFitsFastTile(g) ? "k_fast_wide" : "k_fast";
    // small batches: while every (frame, level) workgroup is resident at once, the largest workgroup that still lets
    // them all be resident finishes a level soonest (640x480, one frame: 73 us with 1024 threads, 104 us with 256)
    // (the "resident" variants are compiled for 4 waves per SIMD = 128 VGPRs, no scratch: 1024 threads per CU-SIMD set)
    // (... the 1024-thread one; the 512- and 256-thread resident variants are compiled for 3 waves per SIMD - no scratch -: a CU then holds
    // THREE 256-thread workgroups (one wave per SIMD each) but only ONE of 512 threads (two waves per SIMD each: a second would need four) -
    // counted as 768 threads per CU, a third of the "resident" 512-thread workgroups queued)
    const long long wgs = (long long)Bn * g.nlevels;
    // one 1024-thread workgroup per CU (the 512-thread build is reached from here through `need` below, also one per CU), else three of 256
    int residentT = wgs <= p.numCUs ? 1024 : (wgs * 256 <= 768LL * p.numCUs ? 256 : 0);
    if (residentT < gp.octThreads || p.octThreadsForced) residentT = 0;   // never fewer threads than the image size asks for
    if (g.big) residentT = wgs <= p.numCUs ? 1024 : 0;      // (frames beyond 4096 px: the 1024-thread builds are the ones that read two-dword candidates)
    // ... but with the first sweep done by k_fast (leaf tables) what is left of a level is a chain of barriers over a list of at most
    // quota + 3 nodes: when 256 threads still give every node of the list its own thread (the short pass forms) the small workgroup
    // has the cheapest barriers (one frame: 1024 threads 16.7 us, 256 threads 13.6)
    if (residentT && k.leafTables) {
        int q = 0;
        for (int l = 0; l < g.nlevels; l++) q = g.lv[l].quota > q ? g.lv[l].quota : q;
        // (nfeatures 1200, level-0 quota 261: 512 threads 14.1 us, 1024 threads 15.1 - its last pass ranks up to 256 multi-key nodes
        // against each other, one packed key per node; before the packed key the larger workgroup won, 18.0 vs 19.3)
        int need = q + 4 <= 256 ? 256 : (q + 4 <= 512 ? 512 : residentT);
        if (need < residentT) residentT = need;
    }
    // queued launches whose first sweep k_fast has done: the same chain of barriers, and the 256-thread workgroup wins at every frame size
    // (128 x 1080p: 87 us with 1024 threads, 57 with 512, 50 with 256; 64 x 1080p: 49 / 34 / 28; 128 x 720p: 87 / 57 / 46) - the sizes by
    // image area were measured with the sweep inside the kernel, where a level-0 workgroup reads ~60 k candidates
    const int queuedT = k.leafTables && !p.octThreadsForced ? 256 : 0;
    for (int l = 0; l < g.nlevels; l++) k.octT[l] = g.big ? 1024 : (residentT ? residentT : (queuedT ? queuedT : gp.octThreads));
    // ... in its scratch-free build (three workgroups per CU instead of six) while the launch is at most four workgroups per CU: little queues
    // behind the first round, and no spilled register is touched.  Round 6, A/B in one call (k_octree_256 -> _256r, us per launch; step): 128 x
    // 1080p 51 -> 33 (2291-2294 -> 2271-2278), 64 x 1080p 28 -> 20, 128 x 720p 47 -> 32 (1167-1171 -> 1151-1157), 128 x 640x480 30 -> 28.5
    // (472-473 -> 468); 256 x 640x480 equal; 512 x 640x480 112 -> 118 (1663 -> 1699: the spilling build keeps its place there, six per CU)
    k.roomy = residentT != 0 || p.octRoomyForced || (queuedT == 256 && wgs <= 4LL * p.numCUs);
    k.octKernel = p.octArena ? kOctArenaKernelNames[g.big] : kOctKernelNames[k.octT[0] == 256 ? 0 : (k.octT[0] == 512 ? 1 : 2)][k.roomy][g.big];
    return k;
}

}  // namespace orbx
