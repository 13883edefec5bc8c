// orbx_params.hpp - the parameter blocks the kernels take BY VALUE and the records host and device exchange: the one definition of each.  The
// host files fill them (through orbx_internal.hpp), the k_* files read them; a field added here reaches both sides or neither.  Plain data only:
// compiles for the host (the CPU suite's builds behind tests/cpp/host_shim included) and the device.  A new entry adds its block here.
#pragma once
#include <stdint.h>

#include "orbx_device.hpp"

namespace orbx {

// ---- records mirrored by include/orbx.h ------------------------------------------------------------------------------------------
struct ProjQuery { float u, v, ur, radius; int minLevel, maxLevel, flags; float angle; };      // == orbx_proj_query
static_assert(sizeof(ProjQuery) == 32, "orbx_proj_query layout");
struct TrackRecord { float projX, projY, projXR, depth, viewCos; int level, exit; };             // == orbx_track_record
static_assert(sizeof(TrackRecord) == 28, "orbx_track_record layout");

// ---- in front of and behind the extractor ----------------------------------------------------------------------------------------
struct GrayParams {              // k_gray.hip
    int rows, cols, channels, redFirst, aligned;
    long long srcStride, srcFrame, dstStride, dstFrame;
};

struct StereoParams {            // k_stereo.hip
    float scale[kMaxLevels], invScale[kMaxLevels];
    float bf, b;
    int nlevels, capacity, rowCap;   // rowCap: entries of one pair's row-list arena
};

struct CameraParams { float fx, fy, cx, cy, k1, k2, p1, p2, k3; };
struct FrameFinishParams {       // k_frame.hip
    CameraParams cam;
    float minX, minY, wInv, hInv;   // mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv
    int capacity;
    int rawGrid;                    // the Nleft != -1 branch of AssignFeaturesToGrid (:404-414): the cells come from mvKeys / mvKeysRight, not from mvKeysUn
};

struct RgbdParams {              // k_frame.hip (k_stereo_from_rgbd)
    int capacity, rows, cols, isU16, scale;     // scale: convertTo runs (a 16-bit map always, a float map when factor != 1)
    long long stride, frame;                    // bytes
    float factor, mbf;
};

struct VocabDevice {            // k_bow.hip: plain arrays of the tree (TemplatedVocabulary::m_nodes)
    const int* childOff;        // [nNodes + 1] children of node n: childList[childOff[n] .. childOff[n + 1])  (in m_nodes[n].children order)
    const int* childList;
    const uint32_t* desc;       // [nNodes][8]  node descriptors
    const double* weight;       // [nNodes]
    const uint32_t* wordId;     // [nNodes]     valid for leaves
    int nNodes, k, L, scoring, weighting;
};

// ---- the matchers ----------------------------------------------------------------------------------------------------------------
struct InitMatchParams {         // k_match.hip
    float minX, minY, wInv, hInv;   // mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv of frame 2
    float r, nnRatio;               // windowSize as float (Frame.cc:660-661), mfNNratio
    int checkOrientation, capacity;
    int slotCapacity;               // level-0 keypoints of frame 2 the LDS tables hold (a multiple of 4)
    int f1First, f1Step, f2First, f2Step;
};

struct ProjectParams {           // k_project.hip (k_project_last)
    float fx, fy, cx, cy, minX, maxX, minY, maxY;
    float scale[kMaxLevels];
    float mbf, mb, th;
    int mono, capacity, lastFirst, lastStep, curFirst, curStep;
};

struct ProjSearchParams {        // k_project.hip (k_search_proj)
    float minX, minY, wInv, hInv, nnRatio;
    int ratioMode, checkOrientation, capacity, queryCapacity, curFirst, curStep, descFirst, descStep, maxDist;
};

struct TwoEyesSearchParams {     // k_project_two_eyes.hip
    float minX, minY, wInv, hInv, nnRatio;
    int capacity, queryCapacity, pairFirst, pairStep, descFirst, descStep, maxDist, forceWalk;
};

struct ProjectTwoEyesParams {    // k_last_frame_two_eyes.hip (k_project_last_two_eyes) / k_project_last_two_eyes_point.hpp
    float cam[8];                   // KannalaBrandt8::mvParameters: fx, fy, cx, cy, k1, k2, k3, k4
    float minX, maxX, minY, maxY;
    float scale[kMaxLevels];        // CurrentFrame.mvScaleFactors
    float trl[12];                  // CurrentFrame.mTrl, 3x4 row-major
    float mb, th;
    int mono, capacity, lastFirst, lastStep, curFirst, curStep;      // first / step: RIG frames (device frames 2r, 2r + 1)
};

struct LastTwoEyesSearchParams { // k_last_frame_two_eyes.hip (k_search_last_two_eyes)
    float minX, minY, wInv, hInv;
    int checkOrientation, capacity, curFirst, curStep, maxDist;
};

struct BowMatchParams {          // k_bow_match.hip
    float nnRatio;
    int thLow, checkOrientation, capacity, kfFirst, kfStep, curFirst, curStep;
    int twoKeyFrames;      // SearchByBoW(pKF1, pKF2, vpMatches12): candidates must hold a MapPoint, strict threshold, result indexed by pKF1's keypoints
};

struct BowTwoEyesParams {        // k_bow_match_two_eyes.hip
    float nnRatio;
    int thLow, checkOrientation, capacity, kfFirst, kfStep, curFirst, curStep;
};

struct TriMatchParams {          // k_triangulate_match.hip
    float scale[kMaxLevels], sigma2[kMaxLevels];      // mvScaleFactors, mvLevelSigma2 of the handle
    int nlevels, thLow, checkOrientation, onlyStereo, coarse, capacity, kf1First, kf1Step, kf2First, kf2Step;
};

struct FuseParams {              // k_fuse.hip
    float fx, fy, cx, cy, minX, maxX, minY, maxY, wInv, hInv;
    float scale[kMaxLevels], invSigma2[kMaxLevels];      // mvScaleFactors, mvInvLevelSigma2 of the handle
    float breaks[kMaxLevels];                            // [k - 1]: smallest ratio whose predicted level is >= k (k = 1 .. nlevels - 1)
    float mbf, th;
    int nlevels, thLow, reprojCheck, capacity, mpCapacity, kfFirst, kfStep, mpFirst, mpStep;
};

struct FuseTwoEyesParams {       // k_fuse_two_eyes.hip
    float cam[2][8];                                     // KannalaBrandt8::mvParameters of mpCamera (left eye) and mpCamera2 (right eye)
    float minX, maxX, minY, maxY, wInv, hInv;            // KeyFrame's truncated bounds and the Frame's inverses, as FuseParams; the same for both eyes
    float scale[kMaxLevels], invSigma2[kMaxLevels];      // mvScaleFactors, mvInvLevelSigma2 of the handle
    float breaks[kMaxLevels];                            // PredictScale's breakpoints, as FuseParams
    float tlr[12];                                       // KeyFrame::mTlr, 3x4 row-major: the right eye's getters derive everything from it alone
    float th;
    int nlevels, thLow, reprojCheck, eyes, capacity, mpCapacity;
    int kfFirst, kfStep, mpFirst, mpStep;                // kf: RIG keyframes (device frames 2r, 2r + 1; d_poses holds one pose per rig)
};

struct TriMatchTwoEyesParams {   // k_triangulate_match_two_eyes.hip
    float cam[2][8];                                     // KannalaBrandt8::mvParameters of mpCamera (left eye) and mpCamera2 (right eye)
    float sigma2[kMaxLevels];                            // mvLevelSigma2 of the handle
    float tlr[12];                                       // KeyFrame::mTlr, 3x4 row-major
    int nlevels, thLow, checkOrientation, onlyStereo, coarse, capacity;
    int kf1First, kf1Step, kf2First, kf2Step;            // RIG keyframes (device frames 2X, 2X + 1; d_poses holds one pose per rig)
    int countStats;                                      // orbx_debug_search_triangulation_two_eyes_enable: add this launch's counts to g_triTwoEyesStats
};

struct Kb8UnprojectParams { float k[8]; int n; };   // k_kb8_unproject: KannalaBrandt8::mvParameters by value

struct Kb8TriangulateParams {    // k_kb8_triangulate
    float cam1[8], cam2[8], R12[9], t12[3], sigma1, sigma2;
    int n;
};

struct StereoFisheyeParams {     // k_stereo_fisheye.hip
    float cam[2][8];                                     // KannalaBrandt8::mvParameters of mpCamera (left eye) and mpCamera2 (right eye)
    float sigma2[kMaxLevels];                            // mvLevelSigma2 of the handle
    float R12[9], t12[3];                                // Frame::mRlr (row-major) and mtlr: mTlr's rotation and last column, as they are
    int nlevels, capacity, rigFirst, rigStep;            // RIG frames (device frames 2r, 2r + 1)
    int tiles;                                           // workgroups per rig: ceil(capacity / rows per workgroup)
    int countStats;                                      // orbx_debug_stereo_fisheye_enable: add this launch's triangulations to g_stereoFisheyeStats
};

struct NewMapPointsParams {      // k_new_map_points.hip / k_new_map_points.hpp
    float cam[2][8];                                     // two eyes: KannalaBrandt8::mvParameters of mpCamera / mpCamera2; one camera: cam[0][0..3] = fx, fy, cx, cy (Pinhole)
    float scale[kMaxLevels], sigma2[kMaxLevels];         // mvScaleFactors, mvLevelSigma2 of the handle
    float tlr[12];                                       // KeyFrame::mTlr, 3x4 row-major (two eyes)
    float mb, mbf, thFarPoints;                          // pKF2->mb / mpCurrentKeyFrame->mb, mpCurrentKeyFrame->mbf, mThFarPoints (one rig has one of each)
    float ratioFactor;                                   // 1.5f * mfScaleFactor, a float product
    int nlevels, farPoints, mono;                        // mono: d_u_right is NULL, no feature is stereo
    int capacity;                                        // keypoints per batch frame (per eye)
    int listCapacity;                                    // entries of a pair's row of d_pairs / d_exit / d_x3d: capacity, or 2 * capacity for two eyes
    int kf1First, kf1Step, kf2First, kf2Step;            // batch frames (one camera) or RIG keyframes (two eyes: device frames 2X, 2X + 1; one pose per rig)
    int tiles;                                           // workgroups per pair: ceil(listCapacity / matches per workgroup)
    int countStats;                                      // orbx_debug_new_map_points_enable: add this launch's counts to g_newMapPointsStats
};

struct MapPointUpdateParams {    // k_map_point_update.hip / k_map_point_update.hpp
    float scale[kMaxLevels];                             // mvScaleFactors of the handle
    float tlr[12];                                       // KeyFrame::mTlr, 3x4 row-major (two eyes)
    int nlevels, capacity;                               // capacity: keypoints per batch frame (per eye)
    int nFrames;                                         // device frames of the batch (two eyes: 2 * rigs); an observation outside is BAD_INDEX
    int nPoints, what;                                   // what: bit 0 the descriptor, bit 1 normal and depth
};
struct MapPointUpdateArrays {    // the arrays of orbx_update_map_points*_device, as the entry was given them
    const int* obsOff; const int* obs; const uint8_t* obsFlags; const int* ref; const int* slot;
    const float* mpWorld; const float* poses; const Keypoint* kps; const uint8_t* desc; const int* nOut;
    uint8_t* mpDesc; float* mpNormal; float* mpDist; int* best; int* bestMedian; uint8_t* status;
};

struct TwoViewParams {           // k_two_view.hip / k_two_view.hpp
    float fx, fy, cx, cy;                                // Pinhole::toK()
    float sigma, minParallax, rhThreshold;
    int iterations, minTriangulated, prune, capacity;
    int f1First, f1Step, f2First, f2Step;
};

constexpr int kTvMaxIterations = 4096;                    // the cap on orbx_reconstruct_two_views_device's `iterations` (include/orbx.h)
// what the first kernel leaves for the other two, per pair: norm = meanX, sX, meanY, sY of frame 1, then of frame 2
struct TvPrep { int status, n, n1, n2; float norm[8]; float T1[9], T2[9], T2inv[9], T2t[9]; };
// the workspace: prep[pair]; first / second [pair*capacity + k] the compacted matches; score [(pair*2 + model)*iterations + it] and mats
// [.. * 9] (model 0 = H, 1 = F); inl / counted / cosv [pair*capacity + k]
struct TvWork { TvPrep* prep; int* first; int* second; float* score; float* mats; uint8_t* inl; uint8_t* counted; float* cosv; };

struct Sim3SolveParams { int capacity, maxIterations, minInliers, nlevels; };      // k_sim3_solver.hip / k_sim3_solver.hpp
constexpr int kSsMaxIterations = 4096;                    // the cap on orbx_sim3_solve_device's `max_iterations` (include/orbx.h)
constexpr int kSsPointFloats = 12;                        // per correspondence: X3Dc1[3] X3Dc2[3] P1im1[2] P2im2[2] max1 max2, component-major
// what the first kernel leaves for the other two, per problem
struct SsPrep { int status, n, maxIts, n1; };
// the workspace: prep[problem]; idx1 [problem*capacity + k] = mvnIndices1; pts [(problem*12 + c)*capacity + k] the twelve floats of
// correspondence k (k_sim3_solver.hpp); counts [problem*maxIterations + it]; its [N], N = 0 .. capacity (SetRansacParameters' iterations)
struct SsWork { SsPrep* prep; int* idx1; float* pts; int* counts; int* its; };

struct PoseOptParams {           // k_pose_optimization.hip / k_pose_optimization.hpp
    int capacity, eyes, nMapPoints, nlevels;
    int frameFirst, frameStep;                           // frames (eyes = 1) or RIG frames (eyes = 2: device frames 2r, 2r + 1; one pose per rig)
};

struct PlaceParams {             // k_place_recognition.hip / k_place_recognition.hpp
    int mode, nDb, capacity;                             // mode: orbx_place_mode; capacity: words per database row
    int nQueries, qFirst, qStep, qCapacity;              // query q is row qFirst + q * qStep of the query arrays, qCapacity words per row
    int nCandidates, candCapacity;                       // nNumCandidates (N_BEST); entries of a query's row of d_cand (RELOCALIZATION)
    int pairRows;                                        // database rows per workgroup of k_place_pairs (prPairRows): speed only
};
struct PlaceArrays {             // the arrays of orbx_detect_candidates_device, as the entry was given them, and the handle's workspace
    const uint32_t* dbIds; const double* dbW; const int* dbN; const int* dbMap; const uint8_t* dbFlags; const int* dbCovis;
    const uint32_t* qIds; const double* qW; const int* qN; const int* qMap; const uint8_t* connected;
    float* score; void* result; int* loop; int* merge; int* cand; int* commonWords;
    int* wsWords; uint32_t* wsFirst; float* wsScore;     // [q * nDb + k]: the pair's shared words, smallest shared word id, L1 score
};

constexpr int kPrScratchInts = 20;
constexpr int prPow2(int v) { int p = 1; while (p < v) p <<= 1; return p; }
// LDS of the two kernels.  k_place_pairs: the query's weights and ids, 12 bytes a word.  k_place_query: 8 bytes of key and 4 of pBestKF per
// list slot (a power of two of slots, for the sorts), 4 per row for the duplicate set, the scratch words
constexpr size_t prPairLdsBytes(int qCapacity) { return (size_t)12 * (size_t)qCapacity; }
constexpr size_t prQueryLdsBytes(int nDb) { return (size_t)12 * (size_t)prPow2(nDb) + (size_t)4 * (size_t)nDb + 4 * kPrScratchInts; }
// Database rows per workgroup of k_place_pairs: a multiple of its four waves.  Every workgroup stages the query again (as many bytes as one
// row), so many rows per workgroup save traffic and few give a small call enough workgroups for the chip: 4 rows while the call has fewer
// than 2048 workgroups of them, up to 32
constexpr int prPairRows(int nDb, int nQueries) {
    int rows = 4;
    while (rows < 32 && ((long long)nDb * nQueries + rows - 1) / rows > 2048) rows <<= 1;
    return rows;
}
constexpr int kPrMaxDb = 8192;                            // the largest n_db whose lists fit the LDS budget (orbx_entry.hpp: placeFits)
constexpr int kPrMaxQueryWords = 13610;                   // the largest q_capacity whose staged query does

struct CovisParams {             // k_covisibility.hip / k_covisibility.hpp: both entries
    int mode, nPoints, nFrames;                          // mode: orbx_covis_mode (the vote); MapPoints of the CSR; frames of the tables
    int nSubjects, capacity;                             // slots of a subject's row of d_subject_mp (and keypoints of a frame: redundancy)
    int th, connCapacity;                                // the vote: th of KeyFrame::UpdateConnections (15); entries of a subject's list blocks
    int monocular, thObs;                                // redundancy: mbMonocular; thObs (3)
    float redundantTh;                                   // redundancy: redundant_th (0.9f / 0.5f)
};
struct CovisArrays {             // the arrays of orbx_covisibility_device and orbx_keyframe_redundancy_device, and the handle's workspace
    const int* obsOff; const int* obs; const uint8_t* mpFlags; const int* mpNobs;
    const uint8_t* kfFlags; const int* kfMap; const uint64_t* kfKey;
    const Keypoint* kpsUn; const int* nOut; const float* depth; const float* thDepth;
    const int* subjectMp; const int* subjectN; const int* subjectKf; const int* subjectMap;
    int* counterKf; int* counterW; int* orderedKf; int* orderedW; void* result; uint8_t* slotState;
    int* wsRank; int* wsByRank; int* wsDup;              // frame -> rank of its key, rank -> frame, a word per kCvRankBlock frames: two keys equal
};

constexpr int kCvScratchInts = 12;
constexpr int kCvRankBlock = 4;                           // frames per workgroup of k_covis_rank (a wave each), and per word of wsDup
constexpr int cvRankBlocks(int nFrames) { return (nFrames + kCvRankBlock - 1) / kCvRankBlock; }
// LDS of the two per-subject kernels.  k_covis_vote: 8 bytes of sort key per list slot (a power of two of slots: every frame may be listed),
// a counter word per frame, the scratch words.  k_keyframe_redundancy: a state byte per slot (held back until every index of the subject
// has been checked), the scratch words
constexpr size_t cvVoteLdsBytes(int nFrames) { return (size_t)8 * (size_t)prPow2(nFrames) + (size_t)4 * (size_t)nFrames + 4 * kCvScratchInts; }
constexpr size_t rdLdsBytes(int capacity) { return (((size_t)capacity + 3) & ~(size_t)3) + 4 * kCvScratchInts; }
constexpr int kCvMaxFrames = 8192;                        // the largest n_frames whose lists fit the LDS budget (orbx_entry.hpp: covisFits)
constexpr int kRdMaxCapacity = 163280;                    // the largest capacity whose state bytes do (redundancyFits)

struct Sim3SearchParams {        // k_project_sim3.hip
    float fx, fy, cx, cy, minX, maxX, minY, maxY, wInv, hInv;
    float scale[kMaxLevels];       // mvScaleFactors of the handle
    float breaks[kMaxLevels];      // PredictScale's breakpoints
    float th;
    int nlevels, maxDist, projection, capacity, mpCapacity, kfFirst, kfStep, mpFirst, mpStep;
};

struct FrustumParams {           // k_frustum.hip / k_frustum_point.hpp
    float fx, fy, cx, cy, minX, maxX, minY, maxY;      // Frame's float bounds, as they are
    float scale[kMaxLevels];                           // mvScaleFactors of the handle
    float breaks[kMaxLevels];                          // [k - 1]: smallest ratio whose predicted level is >= k (k = 1 .. nlevels - 1)
    float mbf, viewCosLimit, th, thFarPoints;
    int nlevels, mode, farPoints, mpCapacity, curFirst, curStep, mpFirst, mpStep;
};

struct FrustumTwoEyesParams {    // k_frustum_two_eyes.hip / k_frustum_two_eyes_point.hpp
    float cam[2][8];                                   // KannalaBrandt8::mvParameters of mpCamera (left eye) and mpCamera2 (right eye)
    float minX, maxX, minY, maxY;                      // Frame's float bounds, as they are; the same four for both eyes
    float scale[kMaxLevels];                           // mvScaleFactors of the handle
    float breaks[kMaxLevels];                          // PredictScale's breakpoints, as FrustumParams
    float trl[12], tlr[12];                            // Frame::mTrl, Frame::mTlr, 3x4 row-major, as the Frame holds them
    float viewCosLimit, th, thFarPoints;
    int nlevels, farPoints, mpCapacity, queryCapacity;
    int groups;                                        // workgroups per pair: ceil(mpCapacity / MapPoints per workgroup)
    int curFirst, curStep, mpFirst, mpStep;            // cur: RIG frames (d_poses holds one pose per rig)
};

}  // namespace orbx
