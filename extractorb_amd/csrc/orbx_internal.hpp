// orbx_internal.hpp - what the host files of liborbx.so share: the launch wrappers the kernel files define, the handle, the error / profiling
// helpers.  orbx_api.cpp holds the extraction path (create, geometry installation, the launch sequence, the extract entry points, the pyramid),
// orbx_rows.cpp the rows behind it (stereo matching, Frame finishing, the window searches, the vocabulary and ComputeBoW / SearchByBoW),
// orbx_mapping_two_eyes.cpp Fuse on two-camera keyframes, orbx_mapping.cpp CreateNewMapPoints' triangulation on one-camera keyframes, orbx_debug.cpp the introspection, profiling and test aids.  The entry points' plain statements (predicates, parameter fills, padding rules) are
// in orbx_entry.hpp, which needs no HIP; what they need of the handle or the runtime is at the end of this file.  The extraction path's launch
// policy - which forms a geometry, a call and each part of a call take - is orbx_batch_plan.hpp, host only as well.  Not installed: callers see
// include/orbx.h only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <mutex>
#include <string>
#include <vector>

#include "orbx.h"
#include "orbx_entry.hpp"
#include "orbx_geometry.hpp"
#include "orbx_batch_plan.hpp"
#include "orbx_params.hpp"
#include "orbx_lds_pollute.hpp"

namespace orbx {
// launch wrappers and LDS sizes, defined in the k_*.hip files (the parameter blocks they take: orbx_params.hpp)
void launchPyrFirst(hipStream_t, const uint8_t*, long long, long long, const LevelGeom&, const LevelGeom*, int, int, int, int,
                    const ResizeX*, const QuadRec*, const ResizeX*, const TileFoot*, uint8_t*, int, int, bool, int, int);
void launchResize(hipStream_t, const LevelGeom&, const LevelGeom&, int, int, const ResizeX*, const QuadRec*, const ResizeX*, const TileFoot*,
                  uint8_t*, int, int, bool, int, int);
size_t bowMatchLdsBytes(int capacity, bool stageDesc);
void launchSearchBow(hipStream_t, const uint32_t*, const uint32_t*, const int*, const uint8_t*, const uint8_t*, const Keypoint*, const uint8_t*, const int*, const BowMatchParams&, int*, int*, int, LdsPolluter);
size_t bowTwoEyesLdsBytes(int capacity, bool stage);
void launchSearchBowTwoEyes(hipStream_t, const uint32_t*, const uint32_t*, const int*, const uint8_t*, const Keypoint*, const uint8_t*, const int*, const BowTwoEyesParams&, bool, int*, int*, int, LdsPolluter);
size_t triMatchLdsBytes(int capacity, bool stage);
void launchSearchTriangulation(hipStream_t, const uint32_t*, const uint32_t*, const int*, const uint8_t*, const uint8_t*, const Keypoint*, const float*, const uint8_t*, const int*, const float*, const float*, const TriMatchParams&, bool, int*, int*, int*, int, LdsPolluter);
void launchFuse(hipStream_t, const float*, const float*, const float*, const uint8_t*, const int*, const uint8_t*, const float*, const Keypoint*, const float*, const uint8_t*, const int*, const int*, const int*, const FuseParams&, int*, int*, uint8_t*, int*, int, LdsPolluter);
void launchFuseTwoEyes(hipStream_t, const float*, const float*, const float*, const uint8_t*, const int*, const uint8_t*, const float*, const Keypoint*, const uint8_t*, const int*, const int*, const int*, const FuseTwoEyesParams&, int*, int*, uint8_t*, int*, int, LdsPolluter);
size_t triMatchTwoEyesLdsBytes(int capacity, bool stage);
void launchSearchTriangulationTwoEyes(hipStream_t, const uint32_t*, const uint32_t*, const int*, const uint8_t*, const uint8_t*, const float*, const Keypoint*, const uint8_t*, const int*, const TriMatchTwoEyesParams&, bool, int*, int*, int*, int, LdsPolluter);
void launchKb8Unproject(hipStream_t, const float*, const float*, int, float*, LdsPolluter);
void launchKb8Triangulate(hipStream_t, const float*, const float*, const Kb8TriangulateParams&, float*, float*, LdsPolluter);
int stereoFisheyeTiles(int capacity);
void launchStereoFisheye(hipStream_t, const Keypoint*, const uint8_t*, const int*, const int*, const StereoFisheyeParams&, int*, int*, float*, float*, int*, int*, int, LdsPolluter);
int newMapPointsTiles(int listCapacity);
void launchNewMapPoints(hipStream_t, bool, const int*, const int*, const float*, const Keypoint*, const Keypoint*, const float*, const float*, const int*, const NewMapPointsParams&, uint8_t*, float*, int*, uint8_t*, uint8_t*, int, LdsPolluter);
void launchMapPointUpdate(hipStream_t, bool, const MapPointUpdateArrays&, const MapPointUpdateParams&, LdsPolluter);
void launchTwoView(hipStream_t, const Keypoint*, const int*, int*, int*, const int*, const TwoViewParams&, const TvWork&, void*, float*, uint8_t*, int, LdsPolluter);
void launchSim3Solve(hipStream_t, const void*, const float*, const float*, const int*, const int*, const int*, const Sim3SolveParams&, const SsWork&, void*, uint8_t*, int, int, LdsPolluter);
void launchPoseOptimization(hipStream_t, const void*, const Keypoint*, const int*, const float*, const int*, const float*, const PoseOptParams&, float*, uint8_t*, void*, int, LdsPolluter);
void launchPlaceRecognition(hipStream_t, const PlaceArrays&, const PlaceParams&, LdsPolluter);
void launchCovisibility(hipStream_t, const CovisArrays&, const CovisParams&, LdsPolluter);
void launchKeyFrameRedundancy(hipStream_t, const CovisArrays&, const CovisParams&, LdsPolluter);
size_t sim3SettleLdsBytes(int capacity, int mpCapacity);
size_t sim3RecordBytes();
void launchSim3Search(hipStream_t, const float*, const float*, const float*, const uint8_t*, const int*, const uint8_t*, const float*, const Keypoint*, const uint8_t*, const int*, const int*, const int*, const uint8_t*, const Sim3SearchParams&, void*, int*, int*, int*, uint8_t*, int*, int, LdsPolluter);
void launchLdsPollute(hipStream_t, int, int, unsigned*);
void launchPyrCols(hipStream_t, const uint8_t*, long long, long long, int, const PyrColumn*, int, const ColLevels*, int, const ResizeX*, int, uint8_t*, int, int, bool, int, int, int);
void launchBlur(hipStream_t, const BlurItem*, const unsigned short*, int, int, const LevelGeom*, const uint8_t*, uint8_t*, int, int);
void launchFast(hipStream_t, const CellDesc*, int, const LevelGeom*, int, const uint8_t*, int, int, unsigned*, unsigned*,
                int, int, int, int, const BlurItem*, const unsigned short*, int, uint8_t*, LeafTables, bool, bool);
bool fastCanCarryBlur(int, int);
size_t octreeLdsBytes(int M, int P, int R, int XT);
void launchOctree(hipStream_t, const LevelGeom*, int, const CellDesc*, int, const unsigned*, const unsigned*, int*, unsigned*,
                  unsigned*, unsigned short*, uint2*, int, int*, int*, const int*, int, int, int, int, const int*, bool, int, int, uint8_t*, LeafTables, bool);
void launchDescribe(hipStream_t, const DescLevels&, const uint8_t*, const uint8_t*, const uint2*, int, const int*,
                    const int*, Keypoint*, uint8_t*, int, int*, int*, Keypoint*, int*, bool, int, int, int, int, int, int, int);
bool checkUmax(const int* umax16);
void describeTables(unsigned* pb384, unsigned* plain256);
hipError_t runPackedSelfTest(hipStream_t, unsigned*, unsigned*);
void launchFrameFinish(hipStream_t, const Keypoint*, const int*, const FrameFinishParams&, Keypoint*, int*, int*, int*, int, LdsPolluter);
void launchStereo(hipStream_t, const LevelGeom*, const uint8_t*, const Keypoint*, const uint8_t*, const int*, const StereoParams&,
                  int, int*, unsigned short*, float*, float*, int*, int*, int, LdsPolluter);
size_t initMatchLdsBytes(int capacity, int slotCapacity);
int initMatchSlotCapacity(int capacity);
void launchSearchInit(hipStream_t, const Keypoint*, const uint8_t*, const int*, const int*, const int*, const InitMatchParams&,
                      float*, int*, int*, int, LdsPolluter);
size_t projSearchLdsBytes(int capacity, int queryCapacity, bool topList);
void launchProjectLast(hipStream_t, const Keypoint*, const Keypoint*, const int*, const uint8_t*, const float*, const float*, const ProjectParams&,
                       ProjQuery*, int, LdsPolluter);
void launchSearchProj(hipStream_t, const ProjQuery*, const uint8_t*, const int*, const Keypoint*, const uint8_t*, const int*, const int*,
                      const int*, const float*, uint8_t*, const ProjSearchParams&, int*, int*, int, LdsPolluter);
void launchFrustum(hipStream_t, const float*, const float*, const float*, const uint8_t*, const float*, const int*, const uint8_t*, const float*, const FrustumParams&, ProjQuery*, uint8_t*, int*, int*, TrackRecord*, int*, int, LdsPolluter);
int frustumTwoEyesGroups(int mpCapacity);
void launchFrustumTwoEyes(hipStream_t, const float*, const float*, const float*, const uint8_t*, const int*, const uint8_t*, const float*, const float*,
                          const FrustumTwoEyesParams&, int*, ProjQuery*, uint8_t*, int*, int*, int*, TrackRecord*, int*, int, LdsPolluter);
size_t twoEyesSearchLdsBytes(int capacity, int queryCapacity);
void launchSearchProjTwoEyes(hipStream_t, const ProjQuery*, const uint8_t*, const int*, const Keypoint*, const uint8_t*, const int*, const int*,
                             const int*, const int*, const int*, uint8_t*, const TwoEyesSearchParams&, int*, int*, int, LdsPolluter);
size_t lastTwoEyesLdsBytes(int capacity);
void launchKb8Project(hipStream_t, const float*, const float*, int, float*, LdsPolluter);
void launchProjectLastTwoEyes(hipStream_t, const Keypoint*, const int*, const uint8_t*, const float*, const float*, const ProjectTwoEyesParams&,
                              ProjQuery*, int, LdsPolluter);
void launchSearchLastTwoEyes(hipStream_t, const ProjQuery*, const uint8_t*, const Keypoint*, const uint8_t*, const int*, const int*, const int*,
                             uint8_t*, const LastTwoEyesSearchParams&, int*, int*, int, LdsPolluter);
void launchBow(hipStream_t, const VocabDevice&, const uint8_t*, const int*, int, int, uint32_t*, double*, uint32_t*, uint32_t*, double*, int*,
               uint32_t*, uint32_t*, int*, int, LdsPolluter);
void launchStereoFromRgbd(hipStream_t, const Keypoint*, const Keypoint*, const int*, const uint8_t*, const RgbdParams&, float*, float*, int, LdsPolluter);
void launchGray(hipStream_t, const uint8_t*, uint8_t*, const GrayParams&, int, LdsPolluter);
void launchClockProbe(hipStream_t, unsigned long long*, int, int, unsigned);
void launchCopyOut(hipStream_t, const void*, void*, size_t, int);
}  // namespace orbx

using namespace orbx;

extern double g_hostT[8];
extern long g_hostN;
extern const bool g_hostTiming;      // ORBX_HOST_TIMING (tools/host_call_anatomy.py)
static inline double nowSec() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }

// Test aids (tests/ only).  They are NOT reachable from the environment: a test sets them through orbx_debug_set_option() before orbx_create,
// so nothing in a deployed process's environment can poison an extractor's memory or make a call fail.
struct TestAids {
    int poison = -1;          // "poison": byte every device allocation of orbx_create is filled with (no kernel may depend on what hipMalloc returns)
    int ldsPollute = -1;      // "lds_pollute": byte every CU's LDS is filled with in front of every kernel
    int colsShape = -1;       // "pyr_cols_shape": pins the workgroup shape of k_pyr_cols (1, 4, 6) so that the parity tests reach every one
    long long sharedUploadBytes = -1;      // "shared_upload_bytes": input copies of at least this size go through the device's shared copy queue (-1: 16 MiB)
    int failAfterFast = 0;    // "fail_after_fast": the next handle's first call with leaf tables returns between k_fast and k_octree (one shot)
    int twoEyesBowStage = -1; // "two_eyes_bow_stage": 0 = the two-eye BoW search reads the frame pair's descriptors from L2 whatever the capacity (the form of large capacities)
    int describeSums = -1;    // "describe_sums": pins the form of k_describe's level sums (0: the scalar form of a full chip, 1: the lane form of small launches)
    int twoEyesWalk = 0;      // "two_eyes_walk": 1 = the two-eye projection search settles every pair by its walk instead of the fixed point
};
extern TestAids g_aids;
enum Slot { S_LEVEL0 = 0, S_RESIZE, S_BLUR, S_FAST, S_OCTREE, S_DESCRIBE, S_MISC, S_TOTAL, S_STEREO, S_FRAME };
extern const char* const kSlotNames[ORBX_NUM_KERNELS];
extern thread_local std::string g_createError;

struct EventPair { hipEvent_t a, b; int slot; };

struct orbx_handle {
    int device = 0;
    int nlevels = 0, iniTh = 0, minTh = 0;
    LaunchPolicy launch;   // the launch-policy switches as orbx_create read them, nfeatures and the facts of the device (orbx_batch_plan.hpp)
    float scaleFactor = 0;
    int maxW = 0, maxH = 0, maxB = 0;
    ScaleTables tabs;
    FrameGeom geom;        // geometry of the image size of the last call
    GeometryPlan geomPlan; // ... and what the launch policy makes of it (installGeometry: split level, quad-tree size, blur tables)
    FrameGeom maxGeom;     // geometry of max_width x max_height (sizes the arenas)
    hipStream_t stream = nullptr;
    bool ownStream = false;
    std::string err;

    // arenas (sized once)
    size_t pyrBytes = 0, blurBytes = 0, candEntries = 0, selEntries = 0, cellCap = 0, rxCap = 0, tileCap = 0;
    uint8_t *d_input = nullptr, *d_pyr = nullptr, *d_blur = nullptr;
    unsigned *d_candPos = nullptr, *d_candSeg = nullptr;   // packed (x,y,response): compacted / per-cell segments
    unsigned* d_cellCount = nullptr;                      // [frame][cell] candidates emitted by k_fast
    int* d_cellOff = nullptr;                             // [frame][cell] offset of the cell in the compacted array
    unsigned short* d_nodeOf = nullptr;
    unsigned* d_candCount = nullptr;
    unsigned* d_sink = nullptr;         // written by the LDS polluter (test aid)
    uint2* d_sel = nullptr;
    int *d_levelCount = nullptr, *d_levelLap = nullptr, *d_lap = nullptr;
    LevelGeom* d_lv = nullptr;
    DescLevels descLevels = {};         // what k_describe takes of the level table, by value (installGeometry fills it beside d_lv)
    CellDesc* d_cells = nullptr;
    ResizeX *d_rx = nullptr, *d_ry = nullptr;
    QuadRec* d_xq = nullptr;            // per level: the tile resize's dword-column records (FrameGeom::xq)
    size_t xqCap = 0, xqOff[kMaxLevels] = {};
    PyrColumn* d_cols = nullptr;        // regions of the region-major pyramid (k_pyr_cols)
    size_t colsCap = 0, colsOff[4] = {};   // first column of each cut of the geometry in d_cols
    ResizeX* d_colCoef = nullptr;       // the regions' coefficient lists, cut after cut
    size_t colCoefCap = 0, colCoefOff[4] = {};
    ColLevels* d_colLevels = nullptr;
    int colPx = 0;                      // ORBX_PYR_COL_PX: side of its regions in level-0 pixels (0: default)
    TileFoot* d_foot = nullptr;
    size_t footCap = 0, footOff[kMaxLevels] = {};
    BlurItem* d_tiles = nullptr;   // row-block items of the blur kernel: [0] blocks of kBlurBlockRows rows, [1] of kBlurBlockRowsSmall rows
    unsigned short* d_laneItem = nullptr;   // item of every lane of the blur grid, both tables
    size_t laneCap = 0;
    size_t rxOff[kMaxLevels] = {}, ryOff[kMaxLevels] = {};
    size_t octArenaSlice = 0;      // > 0: node arrays of the quad-tree live in d_octArena (too large for LDS)
    uint8_t* d_octArena = nullptr;
    int octM = 0, octP = 0, octR = 0, octXT = 0;   // quad-tree LDS: max nodes, sort size, roots covered by the dense phase
    // small batches: per-(frame, level, root) leaf counters / best keys filled by k_fast's emit, consumed and cleared by k_octree
    // (orbx_device.hpp: LeafTables); d_leafCode = [2][nlevels][octXT] host-built x / y path codes of the current geometry
    int* d_leafHist = nullptr;
    unsigned* d_leafBest = nullptr;
    uint8_t* d_leafCode = nullptr;
    // outputs of the host path: ONE result slab [n | mono | level counts | keypoints | descriptors | per-level keypoints], section-major for the
    // frames of the call (outLayout), on the device (d_out) and in pinned host memory (h_out).  A batch comes back with ONE D2H copy of the part the
    // caller asked for; ONE frame per call (the reference's call shape, Frame.cc:419-427) has no copy at all: the kernels write the slab in
    // pinned host memory themselves (tools/host_zero_copy.py: +3.8 us on the kernels against 4-6 copy commands of ~10 us each)
    int outCap = 0;
    uint8_t *d_out = nullptr, *h_out = nullptr;
    size_t outBytes = 0;
    bool zeroCopy = true;              // ORBX_ZERO_COPY=0: a single frame also goes through d_out and the D2H copy
    // pinned staging
    int* h_lap = nullptr;
    std::vector<int> lapCached;
    uint8_t* h_in = nullptr;           // pageable input of a few frames is gathered here (tight rows), then ONE asynchronous H2D copy
    size_t hInBytes = 0;
    uint8_t* h_pyr = nullptr;          // orbx_fetch_pyramid: one frame's bordered levels (allocated on first use)
    size_t hPyrBytes = 0;
    uint8_t* h_tab = nullptr;          // installGeometry: the geometry's tables, packed, copied to the device arenas on the handle's stream
    size_t hTabBytes = 0;
    // where the results of the last host-buffer batch are: as the kernels see them (dev: d_out, or h_out when written zero-copy) and on the host
    struct OutView { Keypoint* k = nullptr; uint8_t* d = nullptr; int* n = nullptr; int* mono = nullptr; Keypoint* lk = nullptr; int* lc = nullptr; };
    OutView dev, host;
    bool pyramidOnly = false;          // the last call was orbx_compute_pyramid: the handle holds a pyramid (and blurred levels) but no results
    bool blurOwed = false;             // the pyramid part of a call left the blur to the FAST launch that follows
    bool testFailAfterFast = false;    // test aid "fail_after_fast" (orbx_debug_set_option)
    bool leafDirty = false;            // k_fast has filled the leaf tables and k_octree has not been enqueued to clear them
    int lastPyrForm = -1, lastPyrCut = 0, lastBlurForm = -1, lastSplitLevel = 0;      // orbx_debug_last_forms
    std::string lastKernel[ORBX_NUM_KERNELS];                      // the kernel (rocprofv3's name, without template arguments) that last ran in each profile slot
    int lastB = 0;
    int lastHostB = 0;           // frames whose results the handle itself holds (the result slab: h->dev / h->host): set by the host-buffer path only
    int pendingB = 0;            // frames of the batch begun with orbx_extract_batch_begin and not yet ended
    bool pendingLevels = false;
    int ldsPollute = -1;               // test aid "lds_pollute" (orbx_debug_set_option): every CU's LDS is filled with the byte in front of every kernel
    int ldsPollutions = 0;             // pollution launches since orbx_create (orbx_debug_lds_pollutions)
    std::string policy;                // the launch-policy switches as read at orbx_create (orbx_debug_policy)
    // the internal stream and the events of the two-half overlap (enqueueBatch)
    hipStream_t aux = nullptr;
    hipEvent_t evFork = nullptr, evJoin = nullptr;
    long long sharedUploadBytes = -1;      // test aid "shared_upload_bytes" as orbx_create read it (-1: the default limit, uploadFrames)
    bool twoEyesBowStage = true;       // test aid "two_eyes_bow_stage" as orbx_create read it
    bool twoEyesWalk = false;          // test aid "two_eyes_walk" as orbx_create read it
    int describeSums = -1;             // test aid "describe_sums" as orbx_create read it (-1: by the launch's size)
    hipEvent_t evUp[2] = {nullptr, nullptr};      // uploadFrames: the handle's stream -> the device's shared input-copy queue -> back
    hipStream_t aux2 = nullptr;        // the blur's side stream (pyramid -> {blur, FAST -> quad-tree} -> description), events per half-batch
    hipEvent_t evPyr[2] = {nullptr, nullptr}, evBlur[2] = {nullptr, nullptr};
    // ComputeBoW scratch (allocated on first use): per-feature word id / weight / node
    size_t bowEntries = 0;
    uint32_t *d_bowWord = nullptr, *d_bowNode = nullptr;
    double* d_bowWeight = nullptr;
    // MapPoint::PredictScale's breakpoints for (scaleFactor, nlevels) (orbx_fuse_device computes them on its first call)
    float scaleBreaks[kMaxLevels] = {};
    bool scaleBreaksReady = false;
    // the Sim3 projection search's records (allocated on first use): the key list, the candidate count and the window of every (pair, MapPoint)
    size_t sim3Entries = 0;
    void* d_sim3Rec = nullptr;
    // the two-eye frustum requests' workspace (allocated on first use): a (slot count, in-view count) pair per workgroup of k_frustum_two_eyes_check
    size_t frustumCountEntries = 0;
    int* d_frustumCounts = nullptr;
    // the two-view reconstruction's workspace (allocated on first use): what TvWork names, sized for (pairs, capacity, iterations)
    struct TwoViewShape { size_t pairs = 0, cap = 0, iters = 0; } twoView;
    TvWork twoViewWork = {};
    // the Sim3 solver's workspace (allocated on first use): what SsWork names, sized for (problems, capacity, max_iterations); sim3Its is
    // the table its[N] as last uploaded, for (sim3ItsProb, sim3ItsMin)
    struct Sim3SolveShape { size_t problems = 0, cap = 0, iters = 0; } sim3Solve;
    SsWork sim3SolveWork = {};
    std::vector<int> sim3Its;
    double sim3ItsProb = 0.0;
    int sim3ItsMin = 0;
    // place recognition's workspace (allocated on first use): a shared-word count, a smallest shared word id and a score per (query, row)
    size_t placeEntries = 0;
    int* d_placeWords = nullptr;
    uint32_t* d_placeFirst = nullptr;
    float* d_placeScore = nullptr;
    // the covisibility vote's workspace (allocated on first use): frame -> rank of its key, rank -> frame, and a word per 256 frames "two keys are equal"
    size_t covisFrames = 0;
    int *d_covisRank = nullptr, *d_covisByRank = nullptr, *d_covisDup = nullptr;
    // stereo matching (allocated on first use)
    struct StereoShape { int pairs = 0, cap = 0, rows = 0; } stereo;      // what the six buffers below are sized for
    int *d_rowOff = nullptr, *d_sadDist = nullptr, *d_nMatched = nullptr;
    unsigned short* d_rowList = nullptr;
    float *d_uRight = nullptr, *d_depth = nullptr;
    // clock probe (orbx_debug_clock_probe: bench.py's sustained-load figure), allocated on first use
    hipStream_t probeStream = nullptr;
    unsigned long long* d_clock = nullptr;
    // profiling
    bool profiling = false;
    std::vector<EventPair> pending;
    double profMs[ORBX_NUM_KERNELS] = {};
    long profN[ORBX_NUM_KERNELS] = {};
};


#define HIP_TRY(h, expr)                                                                                 \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) {                                                                          \
            (h)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                                \
            return ORBX_ERR_HIP;                                                                         \
        }                                                                                                \
    } while (0)

inline int fail(orbx_handle* h, int code, const std::string& msg) {
    h->err = msg;
    return code;
}

inline int nextPow2(int v) { int p = 1; while (p < v) p <<= 1; return p; }

// Byte offsets of the sections of the result slab for a call of B frames (capacity cap per frame).  What every caller wants comes first, so
// that the D2H copy of a batch is one contiguous range: [0, noLevels) without the per-level arrays, [0, all) with them.
struct OutLayout { size_t n, mono, counts, kps, desc, levelK, noLevels, all; };
inline OutLayout outLayout(int B, int cap, int nlevels) {
    auto up = [](size_t v) { return (v + 63) & ~(size_t)63; };
    OutLayout o;
    o.n = 0;
    o.mono = up(sizeof(int) * (size_t)B);
    o.counts = o.mono + up(sizeof(int) * (size_t)B);
    o.kps = o.counts + up(sizeof(int) * (size_t)B * nlevels);
    o.desc = o.kps + up(sizeof(Keypoint) * (size_t)cap * B);
    o.noLevels = o.desc + up((size_t)32 * cap * B);
    o.levelK = o.noLevels;
    o.all = o.levelK + up(sizeof(Keypoint) * (size_t)cap * B);
    return o;
}
inline orbx_handle::OutView outView(uint8_t* base, const OutLayout& o) {
    orbx_handle::OutView v;
    v.n = (int*)(base + o.n); v.mono = (int*)(base + o.mono); v.lc = (int*)(base + o.counts);
    v.k = (Keypoint*)(base + o.kps); v.d = base + o.desc; v.lk = (Keypoint*)(base + o.levelK);
    return v;
}

struct Prof {
    orbx_handle* h; int slot; hipStream_t st; hipEvent_t a = nullptr, b = nullptr;
    Prof(orbx_handle* h_, int s, hipStream_t st_ = nullptr) : h(h_), slot(s), st(st_ ? st_ : h_->stream) {
        if (h->profiling) {
            (void)hipEventCreate(&a); (void)hipEventCreate(&b);
            (void)hipEventRecord(a, st);
        }
    }
    ~Prof() {
        if (h->profiling) {
            (void)hipEventRecord(b, st);
            h->pending.push_back(EventPair{a, b, slot});
        }
    }
};

// The test aid "lds_pollute" of a handle: what a launch* function takes as its last parameter, and the one statement in front of a kernel
// that a host file launches itself.  Nothing is enqueued unless h->ldsPollute >= 0.
inline LdsPolluter ldsPolluter(orbx_handle* h) { return LdsPolluter{h->ldsPollute >= 0 ? &launchLdsPollute : nullptr, h->launch.numCUs, h->ldsPollute, h->d_sink, &h->ldsPollutions}; }
inline void polluteLds(orbx_handle* h, hipStream_t st) { ldsPolluter(h)(st); }

// makeFrameGeom says why it refuses an image size; the code is read off that sentence
inline int geometryRefusalCode(const std::string& why) {
    return why.find("small") != std::string::npos ? ORBX_ERR_IMAGE_TOO_SMALL : ORBX_ERR_UNSUPPORTED;
}

// The device orbx_create / orbx_vocabulary_create is to use: *device < 0 names the current one.  A refusal leaves its sentence, with the
// entry's name in front, in g_createError (there is no handle yet to hold it).
inline int selectDevice(const char* entry, int* device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        g_createError = std::string(entry) + ": no HIP device (this library has no CPU path)";
        return ORBX_ERR_NO_DEVICE;
    }
    if (*device < 0) {
        const hipError_t e = hipGetDevice(device);
        if (e != hipSuccess) { g_createError = std::string("hipGetDevice(&device): ") + hipGetErrorString(e); return ORBX_ERR_HIP; }
    }
    if (*device >= ndev) { g_createError = std::string(entry) + ": device index out of range"; return ORBX_ERR_BAD_ARGUMENT; }
    return ORBX_OK;
}

// ---- what the entry points of orbx_rows.cpp share and that needs the handle or the runtime (the rest: orbx_entry.hpp) ----------------------
constexpr const char* kCapacityAbove32767Msg = "capacity above 32767 keypoints per frame";

// Grows a set of handle-owned device buffers (scratch allocated on first use).  The kernels in flight may still read the old ones: the stream
// drains first.  The recorded capacity says "nothing" from the moment the old buffers go until every new one is there, so a failed
// allocation leaves null pointers beside a capacity that makes the next call allocate again.
template <class Cap>
inline int growDevice(orbx_handle* h, Cap& recorded, const Cap& wanted, std::initializer_list<GrowItem> items) {
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    recorded = Cap{};
    hipError_t e = hipSuccess;
    if (!regrow(items, [&](void** p, size_t bytes) { return (e = hipMalloc(p, bytes)) == hipSuccess; }, [](void* p) { (void)hipFree(p); })) {
        h->err = std::string("hipMalloc (growDevice): ") + hipGetErrorString(e);
        return ORBX_ERR_HIP;
    }
    recorded = wanted;
    return ORBX_OK;
}

// the vocabulary is orbx_rows.cpp's: what another entry file needs of it (orbx_place_recognition.cpp: only L1_NORM is built)
int vocabularyScoring(const orbx_vocabulary* v);
int vocabularyDeviceIndex(const orbx_vocabulary* v);

// MapPoint::PredictScale's breakpoints for the handle's (scaleFactor, nlevels), computed by the first entry that needs them
inline int ensureScaleBreaks(orbx_handle* h) {
    if (h->scaleBreaksReady) return ORBX_OK;
    if (orbx_predict_scale_breakpoints(h->scaleFactor, h->nlevels, h->scaleBreaks) != ORBX_OK)
        return fail(h, ORBX_ERR_BAD_ARGUMENT, "no PredictScale breakpoints for the handle's scale factor");
    h->scaleBreaksReady = true;
    return ORBX_OK;
}

// the nlevels an entry is given must be the handle's
inline int sameLevels(orbx_handle* h, int nlevels) {
    if (nlevels != h->nlevels)
        return fail(h, ORBX_ERR_BAD_ARGUMENT, "nlevels differs from the handle's: the scale tables and PredictScale's breakpoints are the handle's");
    return ORBX_OK;
}

// the tail of every entry, after its Prof scope has closed: a launch that the runtime refused shows here
inline int finishLaunch(orbx_handle* h) {
    HIP_TRY(h, hipGetLastError());
    return ORBX_OK;
}
