/* orbx.h — C ABI of the MI355X-native ORB extractor (liborbx.so).
 *
 * Drop-in boundary for the reference's ORB_SLAM3::ORBextractor (reference
 * inc/ORBextractor.h:44-111): every entry point below names the reference interface it replaces.
 * The C++ shim include/orbx_extractor.hpp rebuilds the reference class on top of these calls;
 * INTEGRATION.md shows the binding a maintainer adds at Frame::ExtractORB (reference
 * src/Frame.cc:419-427).
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types; no exceptions cross this boundary
 *   - return value: ORBX_OK (0) or a negative orbx_status; orbx_last_error() gives the text
 *   - one handle == one camera == one HIP stream + its device buffers (the reference keeps one
 *     ORBextractor per camera: src/Tracking.cc:768-774).  Calls on one handle are serialised by
 *     the caller, calls on different handles may run concurrently (as Frame.cc:109-112 does)
 *   - "device" pointers are HIP device pointers valid on the handle's GPU
 */
#ifndef ORBX_H
#define ORBX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBX_ABI_VERSION 1
#define ORBX_MAX_LEVELS 16
#define ORBX_EDGE_THRESHOLD 19 /* reference ORBextractor.cc:72 */

typedef enum orbx_status {
    ORBX_OK = 0,
    ORBX_ERR_EMPTY_IMAGE = -1,    /* reference operator() returns -1 (ORBextractor.cc:1083-1084) */
    ORBX_ERR_BAD_ARGUMENT = -2,
    ORBX_ERR_CAPACITY = -3,       /* caller's output capacity too small */
    ORBX_ERR_IMAGE_TOO_LARGE = -4,/* exceeds max_width/max_height/max_batch given at create */
    ORBX_ERR_IMAGE_TOO_SMALL = -5,/* coarsest level narrower than one 30-px FAST cell (reference divides by 0) */
    ORBX_ERR_HIP = -6,            /* HIP runtime error, see orbx_last_error */
    ORBX_ERR_NO_DEVICE = -7,
    ORBX_ERR_UNSUPPORTED = -8
} orbx_status;

/* Layout-identical to cv::KeyPoint (28 bytes; reference consumers read pt/octave/angle/size/response:
 * src/Frame.cc:383-417, 748-782).  The shim memcpy's arrays of these into std::vector<cv::KeyPoint>. */
typedef struct orbx_keypoint {
    float x, y;     /* pt: level-0 pixel coordinates in the final arrays; level coordinates in per-level arrays */
    float size;     /* (int)(31 * scale[level])                         ORBextractor.cc:872,881 */
    float angle;    /* IC_Angle, degrees in [0,360)                      ORBextractor.cc:75-102 */
    float response; /* FAST-9 corner score                                ORBextractor.cc:818-819 */
    int32_t octave; /* pyramid level                                      ORBextractor.cc:880 */
    int32_t class_id; /* always -1 */
} orbx_keypoint;

typedef struct orbx_handle orbx_handle; /* opaque */

/* Replaces ORBextractor::ORBextractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST)
 * (inc/ORBextractor.h:50-51, ORBextractor.cc:408-475).  All device memory for images up to
 * max_width x max_height and batches up to max_batch frames is allocated here, once.
 * device < 0 selects the current HIP device.  The thresholds are 1 ... 254 each, in either order
 * (as the reference takes them: with ini_th_fast < min_th_fast the retry can add nothing). */
int orbx_create(orbx_handle** out, int nfeatures, float scale_factor, int nlevels, int ini_th_fast,
                int min_th_fast, int max_width, int max_height, int max_batch, int device);
void orbx_destroy(orbx_handle* h);
const char* orbx_last_error(const orbx_handle* h); /* h may be NULL: error of the last failed orbx_create */
int orbx_abi_version(void);

/* Replaces the getters inc/ORBextractor.h:63-83 (GetLevels, GetScaleFactor, GetScaleFactors,
 * GetInverseScaleFactors, GetScaleSigmaSquares, GetInverseScaleSigmaSquares) plus the public members
 * mnFeaturesPerLevel / umax (:103-105).  Arrays hold nlevels (umax: 16) entries.  Host-only. */
int orbx_get_levels(const orbx_handle* h);
float orbx_get_scale_factor(const orbx_handle* h);
int orbx_get_tables(const orbx_handle* h, float* scale_factors, float* inv_scale_factors,
                    float* level_sigma2, float* inv_level_sigma2, int* features_per_level, int* umax16);
/* Max keypoints one frame can produce: sum over levels of max(quota+3, 4*nIni) for the widest
 * supported aspect; callers size kps/desc with it (nfeatures + 3*nlevels for ordinary aspects). */
int orbx_max_keypoints(const orbx_handle* h);

/* Handle-free host helpers (no GPU touched; usable on a machine without one).
 * orbx_compute_tables: the constructor's tables for (nfeatures, scaleFactor, nlevels), ORBextractor.cc:419-474.
 * orbx_compute_level_sizes: pyramid level sizes of a cols x rows image, ORBextractor.cc:1171.
 * orbx_compute_cell_grid: FAST cell grid of one level (nCols, nRows, wCell, hCell: ORBextractor.cc:789-795),
 *   the number of cv::FAST calls the reference makes on it, the quad-tree root count nIni (:548) and the
 *   exact upper bound of FAST candidates the level can produce. */
int orbx_compute_tables(int nfeatures, float scale_factor, int nlevels, float* scale_factors,
                        float* inv_scale_factors, float* level_sigma2, float* inv_level_sigma2,
                        int* features_per_level, int* umax16);
int orbx_compute_level_sizes(float scale_factor, int nlevels, int rows, int cols, int* widths, int* heights);
int orbx_compute_cell_grid(float scale_factor, int nlevels, int rows, int cols, int level, int* n_cols,
                           int* n_rows, int* w_cell, int* h_cell, int* n_cells, int* n_ini, int* cand_cap);

/* Replaces int ORBextractor::operator()(image, mask, keypoints, descriptors, vLappingArea,
 * allLevelsKeypoints) (inc/ORBextractor.h:58-61, ORBextractor.cc:1078-1162) for one CV_8UC1 host image.
 *   img/rows/cols/stride : the cv::Mat (data, rows, cols, step); mask is ignored by the reference
 *   lap0, lap1           : vLappingArea[0], [1]
 *   kps, desc, capacity  : caller-owned outputs, desc is capacity x 32 bytes, row i <-> kps[i]
 *   *n_out               : number of keypoints == keypoints.size()
 *   *mono_out            : the reference's return value (monoIndex)
 *   level_kps, level_counts (optional, may be NULL): allLevelsKeypoints flattened level by level in
 *                          level coordinates (capacity entries), and the nlevels per-level counts
 * Returns ORBX_ERR_EMPTY_IMAGE (-1) for rows==0||cols==0||img==NULL exactly as the reference returns -1.
 * Synchronous: results are in host memory on return. */
int orbx_extract(orbx_handle* h, const uint8_t* img, int rows, int cols, ptrdiff_t stride, int lap0,
                 int lap1, orbx_keypoint* kps, uint8_t* desc, int capacity, int* n_out, int* mono_out,
                 orbx_keypoint* level_kps, int* level_counts);

/* The same call without the last copy: the results stay in the handle's pinned result slab and the caller gets pointers into it, valid
 * until the next result-producing call on this handle is MADE - its kernels write the same memory (the C++ shim copies them straight into the caller's std::vector / cv::Mat: one copy instead of
 * two).  want_levels != 0 also produces allLevelsKeypoints (level_kps flattened level by level, level_counts[nlevels]).  One frame per
 * call has NO copy command on the stream: the image goes through pinned staging in one H2D copy and the kernels write the slab in host
 * memory themselves. */
int orbx_extract_view(orbx_handle* h, const uint8_t* img, int rows, int cols, ptrdiff_t stride, int lap0, int lap1, int want_levels,
                      const orbx_keypoint** kps, const uint8_t** desc, int* n_out, int* mono_out, const orbx_keypoint** level_kps,
                      const int** level_counts);

/* Replaces the two public stage methods of the reference class (inc/ORBextractor.h:87-90: `protected:` is commented out so that callers
 * can use them; src/orb_extractor/main_orb_extractor.cpp:43-46 and main_whole_orb_extractor.cpp:44-46 do):
 *   void ORBextractor::ComputePyramid(cv::Mat image)                                        ORBextractor.cc:1164-1219
 *   void ORBextractor::ComputeKeyPointsOctTree(vector<vector<KeyPoint>>& allKeypoints)      ORBextractor.cc:773-888
 * orbx_compute_pyramid uploads one CV_8UC1 host image and builds the pyramid (mvImagePyramid: orbx_fetch_pyramid / orbx_get_level);
 * orbx_compute_keypoints_octree runs cell-grid FAST, DistributeOctTree, the (16,16) shift / octave / size fix-up and the orientation on
 * the pyramid the handle holds (from orbx_compute_pyramid or from any extract call: frame 0 of it) and returns allKeypoints flattened
 * level by level in LEVEL coordinates with angles set, exactly what operator() hands out as allLevelsKeypoints (:1094).  Both synchronous. */
int orbx_compute_pyramid(orbx_handle* h, const uint8_t* img, int rows, int cols, ptrdiff_t stride);
int orbx_compute_keypoints_octree(orbx_handle* h, orbx_keypoint* level_kps, int capacity, int* level_counts);

/* Batched form for a video stream or a stereo pair (the two std::threads of Frame.cc:109-112 become one
 * launch sequence).  All frames share rows/cols/stride; frame f starts at imgs + f*frame_stride.
 * Outputs are frame-major with a fixed per-frame capacity: kps[f*capacity + i], desc[(f*capacity+i)*32],
 * n_out[f], mono_out[f], level_counts[f*nlevels + l].  lap0/lap1 may be NULL (=> {0,1000}, the mono
 * default of Frame.cc:307) or hold one pair per frame: lap[2*f], lap[2*f+1]. */
int orbx_extract_batch(orbx_handle* h, int n_frames, const uint8_t* imgs, int rows, int cols,
                       ptrdiff_t stride, ptrdiff_t frame_stride, const int* lap, orbx_keypoint* kps,
                       uint8_t* desc, int capacity, int* n_out, int* mono_out, orbx_keypoint* level_kps,
                       int* level_counts);

/* Asynchronous host-buffer form.  _begin enqueues the H2D copy of the frames, the whole path and the D2H copy of
 * the results (into pinned staging owned by the handle) and returns without waiting; _end waits for that batch and
 * copies the results into the caller's arrays (same layout as orbx_extract_batch).  One batch in flight per handle:
 * two handles used alternately overlap the transfers of one batch with the kernels of the other (input copies of 16 MiB and more go through
 * ONE copy queue per device, shared by its handles, so that they run one after the other at the link's full rate: DESIGN.md).  The H2D copy is
 * only truly asynchronous from pinned memory (orbx_host_alloc).  want_levels != 0 also brings back the per-level
 * arrays.  orbx_extract_batch == _begin + _end. */
int orbx_extract_batch_begin(orbx_handle* h, int n_frames, const uint8_t* imgs, int rows, int cols, ptrdiff_t stride,
                             ptrdiff_t frame_stride, const int* lap, int want_levels);
int orbx_extract_batch_end(orbx_handle* h, orbx_keypoint* kps, uint8_t* desc, int capacity, int* n_out, int* mono_out,
                           orbx_keypoint* level_kps, int* level_counts);
/* Zero-copy variant of _end: waits, then hands out pointers into the handle's pinned result staging
 * (kps[f*capacity + i], desc[(f*capacity + i)*32], n_out[f], mono_out[f]).
 * Lifetime (same rule as orbx_extract_view): the pointers are valid until the NEXT CALL of any kind that produces results on this handle -
 * orbx_extract*, _begin, orbx_compute_keypoints_octree - is MADE, not until it completes: with one frame per call the kernels of that next
 * call write this very memory (there is no copy command whose completion would mark the overwrite).  Copy what you keep before calling again,
 * or alternate two handles. */
int orbx_extract_batch_end_view(orbx_handle* h, const orbx_keypoint** kps, const uint8_t** desc, int* capacity,
                                const int** n_out, const int** mono_out);
void* orbx_host_alloc(size_t bytes); /* pinned host memory (hipHostMalloc); NULL on failure */
void orbx_host_free(void* p);

/* Device-resident batched form: d_imgs and the outputs are device pointers; the work is enqueued on the
 * handle's stream and NOT synchronised (call orbx_synchronize or sync the stream yourself).  Same output
 * layout as orbx_extract_batch; d_level_kps/d_level_counts may be NULL.  lap is a HOST pointer (or NULL). */
int orbx_extract_batch_device(orbx_handle* h, int n_frames, const uint8_t* d_imgs, int rows, int cols,
                              ptrdiff_t stride, ptrdiff_t frame_stride, const int* lap,
                              orbx_keypoint* d_kps, uint8_t* d_desc, int capacity, int* d_n_out,
                              int* d_mono_out, orbx_keypoint* d_level_kps, int* d_level_counts);

/* Replaces reads of the public member mvImagePyramid (inc/ORBextractor.h:85; read by
 * Frame::ComputeStereoMatches, src/Frame.cc:820,910,929) after a call: copies level `level` of frame
 * `frame` of the last batch to host.  bordered==0: width x height pixels; bordered!=0: the
 * (width+38) x (height+38) buffer with the BORDER_REFLECT_101 frame of ORBextractor.cc:1193-1215. */
int orbx_get_level(orbx_handle* h, int frame, int level, int bordered, uint8_t* dst, ptrdiff_t dst_stride,
                   int* width, int* height);

/* All levels of frame `frame` of the last batch (or of orbx_compute_pyramid) in ONE device-to-host copy, for readers of mvImagePyramid
 * (Frame.cc:820,910,924,929): *base points into pinned staging owned by the handle (valid until the next orbx_fetch_pyramid on it);
 * level l is heights[l] rows of widths[l] pixels, pixel (0,0) at base[level_offset[l]], rows level_stride[l] bytes apart, and — as in the
 * reference, where mvImagePyramid[l] is a view into a bordered buffer (ORBextractor.cc:1173-1177) — the 19-px BORDER_REFLECT_101 frame
 * lies around it in the same buffer.  Arrays hold nlevels entries. */
int orbx_fetch_pyramid(orbx_handle* h, int frame, const uint8_t** base, size_t* level_offset, int* level_stride, int* widths, int* heights);

/* ---- next row beyond the extractor ------------------------------------------------------
 * Replaces Frame::ComputeStereoMatches() (reference src/Frame.cc:813-991) for stereo pairs extracted by ONE
 * batched call on this handle: frame 2p is the left eye, frame 2p+1 the right eye (n_frames = 2*n_pairs).
 * It consumes that call's keypoints/descriptors and the two eyes' image pyramids, which are still in HBM (the
 * reference reads mpORBextractorLeft/Right->mvImagePyramid for the 11x11 SAD refinement, Frame.cc:910,929).
 *   bf, b : Frame::mbf and Frame::mb (baseline*fx and baseline; minZ = b, maxD = bf/b, Frame.cc:843-845)
 *   u_right[p*capacity + i], depth[p*capacity + i] : mvuRight / mvDepth of left keypoint i (-1 = no match)
 *   n_matched[p] : matches that survive the median filter
 * orbx_stereo_match_device takes the device buffers an orbx_extract_batch_device call filled (and is asynchronous
 * on the handle's stream); orbx_stereo_match_last uses the results of the last orbx_extract_batch call, which the
 * handle keeps in HBM, and returns host arrays.
 * The median filter keeps one pair's SAD distances in the LDS of one CU: 4 * ((capacity + 3) & ~3) bytes beside
 * ORBX_STEREO_FILTER_STATIC_LDS_BYTES of its own.  A capacity (for _last: the handle's orbx_max_keypoints()) with
 *   4 * ((capacity + 3) & ~3) + ORBX_STEREO_FILTER_STATIC_LDS_BYTES > 160 * 1024 - 512      (capacity > 40568)
 * is refused with ORBX_ERR_UNSUPPORTED before anything is launched or allocated. */
#define ORBX_STEREO_FILTER_STATIC_LDS_BYTES 1056
int orbx_stereo_match_device(orbx_handle* h, int n_pairs, const orbx_keypoint* d_kps, const uint8_t* d_desc,
                             const int* d_n_out, int capacity, float bf, float b, float* d_u_right, float* d_depth,
                             int* d_n_matched);
int orbx_stereo_match_last(orbx_handle* h, int n_pairs, float bf, float b, float* u_right, float* depth, int capacity,
                           int* n_matched);

/* ---- the caller's side of the path: colour input ----------------------------------------------------------------
 * Replaces the cv::cvtColor(RGB2GRAY | BGR2GRAY | RGBA2GRAY | BGRA2GRAY) calls of Tracking::GrabImageMonocular / Stereo /
 * RGBD (src/Tracking.cc:915-941, 985-1001) for n_frames device-resident 8-bit frames of `channels` (3 or 4) interleaved
 * channels; red_first = Tracking::mbRGB.  gray = (R*4899 + G*9617 + B*1868 + 8192) >> 14 (OpenCV's 14-bit fixed point).
 * The result feeds orbx_extract_batch_device.  Asynchronous on the handle's stream. */
int orbx_gray_from_color_device(orbx_handle* h, int n_frames, const uint8_t* d_src, int rows, int cols, int channels, int red_first,
                                ptrdiff_t src_stride, ptrdiff_t src_frame_stride, uint8_t* d_gray, ptrdiff_t gray_stride,
                                ptrdiff_t gray_frame_stride);

/* ---- RGB-D frames: Frame::ComputeStereoFromRGBD (src/Frame.cc:994-1015) with the depth conversion of
 * Tracking::GrabImageRGBD (imDepth.convertTo(CV_32F, mDepthMapFactor), src/Tracking.cc:1003-1004) fused in.
 * d_depth: n_frames depth maps, float32 or uint16 (depth_is_u16); a uint16 map is always scaled by depth_map_factor
 * (= 1 / DepthMapFactor of the settings file, Tracking.cc:680-684), a float map only when |factor - 1| > 1e-5.
 * For keypoint i of frame f (d_kps: mvKeys, d_kps_un: mvKeysUn): d = depth(int(y), int(x)); d > 0 gives
 * d_depth_out = d and d_u_right = kpUn.x - mbf / d, else both are -1.  Slots past n_out[f] are filled with -1. */
int orbx_stereo_from_rgbd_device(orbx_handle* h, int n_frames, const orbx_keypoint* d_kps, const orbx_keypoint* d_kps_un,
                                 const int* d_n_out, int capacity, const void* d_depth, int depth_is_u16, int rows, int cols,
                                 ptrdiff_t depth_stride_bytes, ptrdiff_t depth_frame_stride_bytes, float depth_map_factor, float mbf,
                                 float* d_u_right, float* d_depth_out);

/* ---- next row: the rest of the Frame constructor ------------------------------------------
 * Frame::mK and Frame::mDistCoef as plain floats (fx, fy, cx, cy: src/Frame.cc:342-345; k1, k2, p1, p2[, k3]). */
typedef struct orbx_camera { float fx, fy, cx, cy, k1, k2, p1, p2, k3; } orbx_camera;
#define ORBX_GRID_COLS 64 /* FRAME_GRID_COLS, inc/Frame.h:40 */
#define ORBX_GRID_ROWS 48 /* FRAME_GRID_ROWS, inc/Frame.h:39 */

/* Replaces Frame::ComputeImageBounds (src/Frame.cc:784-811): bounds[4] = mnMinX, mnMaxX, mnMinY, mnMaxY of a
 * cols x rows image (the four corners undistorted when k1 != 0).  Host-only, no GPU touched. */
int orbx_compute_image_bounds(const orbx_camera* cam, int cols, int rows, float* bounds4);

/* Replaces Frame::UndistortKeyPoints (src/Frame.cc:748-782) and Frame::AssignFeaturesToGrid (:383-417, the
 * Nleft == -1 case; the other one: orbx_frame_finish_two_eyes_device below) + PosInGrid (:726-736) for n_frames frames of device-resident extraction results:
 *   d_kps_un[f*capacity + i]            : mvKeysUn
 *   d_grid_off[f*(64*48+1) + x*48 + y]  : first slot of mGrid[x][y]; [.. + 64*48] = keypoints inside the grid
 *   d_grid_idx[f*capacity + slot]       : keypoint indices, increasing inside a cell (push_back order)
 *   d_n_inside[f]
 * bounds4 as returned by orbx_compute_image_bounds.  Asynchronous on the handle's stream. */
int orbx_frame_finish_device(orbx_handle* h, int n_frames, const orbx_keypoint* d_kps, const int* d_n_out, int capacity,
                             const orbx_camera* cam, const float* bounds4, orbx_keypoint* d_kps_un, int* d_grid_off,
                             int* d_grid_idx, int* d_n_inside);
/* The Nleft != -1 branch of Frame::AssignFeaturesToGrid (src/Frame.cc:404-414; the two-camera Frame constructor, :1045-1122, which assigns BEFORE
 * it undistorts): for n_pairs pairs of a device-resident batch - frame 2p = the left eye (mvKeys), frame 2p + 1 = the right eye (mvKeysRight) -
 * the cells come from each eye's RAW keypoints: the left frame's CSR is mGrid (indices i < Nleft), the right frame's is mGridRight (indices
 * i - Nleft, i.e. the right eye's own); d_kps_un still receives UndistortKeyPoints' mvKeysUn of both eyes.  Same array layout as above, for
 * 2 * n_pairs frames.  (The camera model, matcher twins and frustum tests of that rig are out of scope: SURVEY.md §2 #13.) */
int orbx_frame_finish_two_eyes_device(orbx_handle* h, int n_pairs, const orbx_keypoint* d_kps, const int* d_n_out, int capacity,
                                      const orbx_camera* cam, const float* bounds4, orbx_keypoint* d_kps_un, int* d_grid_off,
                                      int* d_grid_idx, int* d_n_inside);

/* ---- next row: monocular initialisation matching ------------------------------------------
 * Replaces ORBmatcher::SearchForInitialization (src/ORBmatcher.cc:706-821; caller src/Tracking.cc:2065-2066 with
 * ORBmatcher(0.9, true) and windowSize 100) with Frame::GetFeaturesInArea (src/Frame.cc:655-724),
 * ORBmatcher::DescriptorDistance (:2349-2365) and ComputeThreeMaxima (:2303-2344), for n_pairs frame pairs of one
 * device-resident batch: pair p matches F1 = frame frame1_first + p*frame1_step against F2 = frame
 * frame2_first + p*frame2_step (a stream: 0,1,1,1; one initial frame against many: 0,0,1,1).
 *   d_kps_un, d_grid_off, d_grid_idx : as written by orbx_frame_finish_device (mvKeysUn, mGrid) for all frames
 *   d_desc, d_n_out                  : mDescriptors, N of all frames (orbx_extract_batch_device)
 *   d_prev_matched[(p*capacity + i)*2 + {0,1}] : vbPrevMatched of pair p, in/out (Tracking.cc:2029-2031 seeds it
 *                                      with F1.mvKeysUn[i].pt; matched entries become F2.mvKeysUn[match].pt, :815-817)
 *   d_matches12[p*capacity + i]      : vnMatches12, -1 = unmatched;  d_n_matches[p] : the return value
 * Frames of the initialisation extractor (ORBextractor(5 * nFeatures), src/Tracking.cc:774: capacity 5000 .. 10 000) are supported: only the
 * level-0 keypoints take part (:722-726: those of F1 ask, those of F2 inside the grid are candidates) and only they are kept on chip.  One
 * workgroup's table has as many entries for F1 as for F2 and takes 66 B per entry pair (56 B per level-0 keypoint of F2: descriptor, position,
 * cell, index, holder list; 10 B per level-0 keypoint of F1: index, two decision words) plus 608 B, in 160 KiB - 1 KiB of LDS:
 * (capacity + 3) & ~3 entries while that fits (capacity <= 2457), 2456 entries for every larger capacity.  The number bounds the level-0
 * keypoints of either frame: should F1 or F2 hold more (a one-level pyramid with thousands of features), the pair reports d_n_matches[p] = -1
 * and an all -1 table and leaves d_prev_matched as it was; the other pairs of the call are not affected.  Asynchronous on the handle's stream. */
int orbx_search_for_initialization_device(orbx_handle* h, int n_pairs, int frame1_first, int frame1_step, int frame2_first,
                                          int frame2_step, const orbx_keypoint* d_kps_un, const uint8_t* d_desc,
                                          const int* d_n_out, int capacity, const int* d_grid_off, const int* d_grid_idx,
                                          const float* bounds4, float* d_prev_matched, int window_size, float nn_ratio,
                                          int check_orientation, int* d_matches12, int* d_n_matches);

/* ---- monocular initialisation, second half: TwoViewReconstruction::Reconstruct ---------------------------------------
 * The statement behind SearchForInitialization in the tracker: mpCamera->ReconstructWithTwoViews (src/Tracking.cc:2081 ->
 * src/CameraModels/Pinhole.cpp:105-113 -> src/TwoViewReconstruction.cc:39-125) on the d_matches12 the search left on the device, and,
 * with prune != 0, the statement after it (src/Tracking.cc:2083-2090).  Pairs and arrays are numbered and shaped as
 * orbx_search_for_initialization_device's, so that entry's outputs go in unchanged.
 * How a pair left Reconstruct; every way out has a name: */
enum orbx_two_view_status {
    ORBX_TWO_VIEW_ACCEPTED_H = 0,            /* ReconstructH returned true (:724-732) */
    ORBX_TWO_VIEW_ACCEPTED_F = 1,            /* ReconstructF returned true (:526-571) */
    ORBX_TWO_VIEW_TOO_FEW_MATCHES = 2,       /* N < 8: the reference would call RandomInt(0, -1) */
    ORBX_TWO_VIEW_BAD_INDEX = 3,             /* a d_matches12[i] >= n of frame 2: nothing else is read; decides before TOO_FEW_MATCHES */
    ORBX_TWO_VIEW_ZERO_SCORES = 4,           /* SH + SF == 0 (:111) */
    ORBX_TWO_VIEW_H_DEGENERATE = 5,          /* d1/d2 < 1.00001 || d2/d3 < 1.00001 (:600) */
    ORBX_TWO_VIEW_H_AMBIGUOUS = 6,           /* the four conjuncts of :724, named by the first that fails in source order */
    ORBX_TWO_VIEW_H_LOW_PARALLAX = 7,
    ORBX_TWO_VIEW_H_FEW_POINTS = 8,
    ORBX_TWO_VIEW_H_BELOW_INLIER_SHARE = 9,
    ORBX_TWO_VIEW_F_FEW_POINTS = 10,         /* maxGood < nMinGood (:520) */
    ORBX_TWO_VIEW_F_AMBIGUOUS = 11,          /* nsimilar > 1 (:520) */
    ORBX_TWO_VIEW_F_LOW_PARALLAX = 12        /* the best motion's parallax is not above min_parallax (:526-571) */
};
/* One row per pair.  Every field computed before the exit holds its value, the rest is zero (best_it_* and chosen: -1). */
typedef struct orbx_two_view_result {
    int32_t status;                /* orbx_two_view_status */
    int32_t model;                 /* the model taken: 0 = H, 1 = F; -1 before the branch */
    int32_t n_matches;             /* N = the d_matches12[i] >= 0 of the pair */
    int32_t best_it_h, best_it_f;  /* the winning iteration of each model: the first with a strictly greater score (-1: no score above 0) */
    int32_t n_inliers;             /* vbMatchesInliers of the model taken */
    int32_t chosen;                /* the motion taken, an index into n_good / parallax */
    float SH, SF, RH;
    float H21[9], F21[9];          /* the winners, row-major */
    float R21[9], t21[3];          /* the accepted motion */
    int32_t n_good[8];             /* CheckRT of the motion hypotheses in the reference's order: eight for H, four for F (the rest zero) */
    float parallax[8];
} orbx_two_view_result;

/*   d_kps_un[f*capacity + i] : mvKeysUn of batch frame f; only .pt is read.  d_n_out[f] is clamped into [0, capacity].
 *   d_matches12[p*capacity + i], d_n_matches[p] : exactly what the search wrote.  With prune != 0 an ACCEPTED pair's entries
 *                     d_matches12[i] >= 0 with d_triangulated[i] == 0 become -1 and d_n_matches[p] is lowered by their number;
 *                     a rejected pair's table is left as it is.  prune == 0 writes neither.
 *   cam             : fx, fy, cx, cy, read as Pinhole::toK(); the distortion fields are not read.
 *   sigma, iterations : TwoViewReconstruction's constructor arguments (1.0f, 200: inc/TwoViewReconstruction.h:37); sigma > 0,
 *                     1 <= iterations <= 4096.  min_parallax, min_triangulated: 1.0f, 50 (:114-123).
 *   rh_threshold    : RH > rh_threshold takes the homography, compared in binary32; the reference has 0.50f (:117), its own comment
 *                     0.40-0.45.  Must lie in (0, 1): with SF == 0 and SH > 0, RH is 1 and H must be taken, as the F inliers are empty.
 *   d_rand[(p*iterations + it)*8 + j] : the raw rand() values, ints of [0, 2^31 - 1], that the reference's set loop (:79-96) would
 *                     draw: DUtils::Random::SeedRandOnce seeds once per PROCESS, so what the second Reconstruct call draws depends on
 *                     every rand() before it; the caller draws.  The device applies DUtils/Random.cpp:47-50 and the swap-remove of
 *                     :83-95 itself; a value outside the range is clamped onto the list.
 *   d_result[p]     : see above.  d_p3d[(p*capacity + i)*3] = vP3D and d_triangulated[p*capacity + i] = vbTriangulated, indexed by
 *                     the keypoint of frame 1 (CheckRT :811-812, :892-896): vP3D is written for every counted point, one with
 *                     cosParallax >= 0.99998 included, whose flag stays 0.  Both are zero for i < n of frame 1 on a rejecting status;
 *                     entries from n on are not touched.
 * cv::SVD and the cv::Mat kernels are the library's own definitions: the sign and order freedom of an SVD can
 * permute the 8 or 4 motion hypotheses against OpenCV's.  Asynchronous on the handle's stream; the workspace belongs to the handle.
 * Out of scope: KannalaBrandt8::ReconstructWithTwoViews' cv::fisheye::undistortPoints prelude (KannalaBrandt8.cpp:211-226) - a fisheye
 * caller passes undistorted points and the pinhole K of that prelude - and CreateInitialMapMonocular. */
int orbx_reconstruct_two_views_device(orbx_handle* h, int n_pairs, int frame1_first, int frame1_step, int frame2_first, int frame2_step,
                                      const orbx_keypoint* d_kps_un, const int* d_n_out, int capacity, int* d_matches12,
                                      int* d_n_matches, const orbx_camera* cam, float sigma, int iterations, float min_parallax,
                                      int min_triangulated, float rh_threshold, const int* d_rand, int prune,
                                      orbx_two_view_result* d_result, float* d_p3d, uint8_t* d_triangulated);

/* ---- loop closing, between SearchByBoW and SearchByProjection(pKF, Scw, ..): Sim3Solver ------------------------------------------
 * Per loop candidate the reference runs SearchByBoW (orbx_search_by_bow_*), Sim3Solver, SearchByProjection(pKF, Scw, ..)
 * (orbx_search_by_projection_sim3_device): src/LoopClosing.cc:595-760.  This entry is the middle link: Sim3Solver's constructor,
 * SetRansacParameters(probability, min_inliers, max_iterations) and the iterate(20, bNoMore, vbInliers, nInliers, bConverge) loop until it
 * converges or reports no more iterations (src/Sim3Solver.cc, call site LoopClosing.cc:673-684), for n_problems independent problems.
 * How a problem left the solver; every way out has a name: */
enum orbx_sim3_solve_status {
    ORBX_SIM3_SOLVE_CONVERGED = 0,                 /* an iteration counted more than min_inliers inliers (:277-285) */
    ORBX_SIM3_SOLVE_NO_MORE = 1,                   /* mRansacMaxIts iterations used up: the best Sim3 so far is returned, as the second overload does (:288-296) */
    ORBX_SIM3_SOLVE_TOO_FEW = 2,                   /* N < min_inliers (:228) */
    ORBX_SIM3_SOLVE_BAD_ARGUMENT = 3               /* what the reference would index out of bounds on: n1 outside [0, capacity], a model that is
                                              * neither, an octave outside [-1, nlevels), N >= min_inliers with fewer than 3 correspondences */
};
/* One row per problem, in device memory: what the caller reads off pKF1 and pKF2. */
typedef struct orbx_sim3_problem {
    int32_t n1;                    /* vpMatched12.size(): the slots of this problem, <= capacity */
    int32_t fix_scale;             /* bFixScale */
    int32_t model1, model2;        /* pKF1->mpCamera, pKF2->mpCamera: 0 = Pinhole (cam[0..3] = fx, fy, cx, cy), 1 = KannalaBrandt8
                                    * (cam = mvParameters as orbx_camera_kb8 lays them out); projectMat is virtual */
    float cam1[8], cam2[8];
    float Tcw1[12], Tcw2[12];      /* GetRotation() | GetTranslation() of pKF1, pKF2: 3x4 row-major */
    float level_sigma2[ORBX_MAX_LEVELS];     /* mvLevelSigma2 (the two keyframes of one system share it); the handle's nlevels entries are read */
} orbx_sim3_problem;
/* One row per problem.  Every field computed before the exit holds its value, the rest is zero (best_it: -1). */
typedef struct orbx_sim3_result {
    int32_t status;                /* orbx_sim3_solve_status */
    int32_t n;                     /* N, the correspondences: the present slots */
    int32_t max_its;               /* mRansacMaxIts after SetRansacParameters */
    int32_t iterations;            /* mnIterations at the return */
    int32_t best_it;               /* the iteration (from 0) whose Sim3 is returned: the converging one, or the LAST of the greatest count */
    int32_t n_inliers;             /* nInliers: the converging count, 0 otherwise */
    int32_t best_inliers;          /* mnBestInliers */
    float scale;                   /* mBestScale */
    float R[9], t[3];              /* mBestRotation (row-major), mBestTranslation */
    float T12[16];                 /* mBestT12, 4x4 row-major */
} orbx_sim3_result;

/*   d_problems[p]   : see above.
 *   d_x1w, d_x2w [(p*capacity + i)*3] : GetWorldPos() of pMP1 = pKF1's MapPoint i and of pMP2 = vpMatched12[i].
 *   d_octave1, d_octave2 [p*capacity + i] : the octave of kp1 = pKF1->mvKeysUn[indexKF1] and of kp2 = pKF2->mvKeysUn[indexKF2].  A slot is
 *                     ABSENT when either is -1: that stands for every `continue` of :73-91 - no match, no MapPoint, isBad, an index < 0.
 *                     isBad and GetIndexInKeyFrame stay with the caller.  With a non-empty vpKeyFrameMatchedMP, the only call in the
 *                     reference, bDifferentKFs is false and pKFm is ALWAYS pKF2 (:40-45, :84-85): indexKF2 is pMP2's index in pKF2, and a
 *                     point pKF2 does not observe is skipped.  Entries from n1 on are not read.
 *   probability, min_inliers, max_iterations : SetRansacParameters' arguments (0.99, 15, 300 at the call site); probability in [0, 1],
 *                     1 <= max_iterations <= 4096, n_problems * max_iterations < 2^31 (one workgroup per iteration).
 *   d_rand[(p*max_iterations + it)*3 + j] : the raw rand() values, ints of [0, 2^31 - 1], of iteration `it` (see
 *                     orbx_reconstruct_two_views_device: the caller draws).  The device applies DUtils/Random.cpp:47-50 and the swap-remove of
 *                     :251-262 itself; a value outside the range is clamped onto the list.  Iterations from max_its on are not read.
 *   d_result[p]     : see above.  d_inliers[p*capacity + i] = vbInliers[i1] (:280-282): all zero unless CONVERGED, as in the reference;
 *                     entries from n1 on are not touched (none at all when n1 is outside [0, capacity]).
 * cv::eigen, cv::Rodrigues and the cv::Mat expressions are the library's own definitions (k_sim3_solver.hpp states
 * each), and so are the double atan2 / sin / cos under them.  Three points that align exactly give the reference's NaN rotation: 0 inliers,
 * and every NaN of a result row is 0x7fc00000.  Asynchronous on the handle's stream.  The workspace belongs to the handle and grows to
 * 4*(13*n_problems*capacity + n_problems*max_iterations + capacity + 1) + 16*n_problems bytes; when it grows, or when (probability,
 * min_inliers) differ from the previous call's, the entry waits for the stream and uploads the table of SetRansacParameters' iteration
 * counts, computed with the host's libm.  No LDS.  What follows the solver - gScm * gSmw (LoopClosing.cc:720-723), OptimizeSim3 - is the
 * caller's.  Out of scope: the first iterate overload and find (no caller on this path; find's result follows from the same outputs). */
int orbx_sim3_solve_device(orbx_handle* h, int n_problems, const orbx_sim3_problem* d_problems, int capacity, const float* d_x1w,
                           const float* d_x2w, const int* d_octave1, const int* d_octave2, double probability, int min_inliers,
                           int max_iterations, const int* d_rand, orbx_sim3_result* d_result, uint8_t* d_inliers);

/* ---- tracking, between every pair of searches: Optimizer::PoseOptimization ---------------------------------------------------------
 * The motion-only bundle adjustment of src/Optimizer.cc:854-1168 - TrackReferenceKeyFrame after SearchByBoW (src/Tracking.cc:2333),
 * TrackWithMotionModel after the frame-to-frame SearchByProjection (:2492), TrackLocalMap after SearchLocalPoints (:2554-2560),
 * Relocalization around its SearchByProjection (:3285, :3301, :3316) - for n_problems independent problems, one per frame: everything from
 * :856 to the return at :1167.  The pose it writes is what orbx_frustum_requests_device and both frame-to-frame projection entries read as
 * d_poses; the flags are mvbOutlier.  How a problem left the function; every way out has a name: */
enum orbx_pose_optimization_status {
    ORBX_POSE_OPTIMIZATION_ALL_ROUNDS = 0,         /* the four optimisations ran (:1060-1157) */
    ORBX_POSE_OPTIMIZATION_FEW_EDGES = 1,          /* optimizer.edges().size() < 10 after round 0 (:1155): one round, the pose is round 0's */
    ORBX_POSE_OPTIMIZATION_TOO_FEW = 2,            /* nInitialCorrespondences < 3 (:1050): returns 0, the pose is untouched, the flags of the edges are 0 */
    ORBX_POSE_OPTIMIZATION_BAD_ARGUMENT = 3        /* what the reference would index out of bounds on: N outside [0, capacity], a camera model that is
                                                    * neither, a match outside [-1, n_map_points), an octave outside [0, nlevels) on a keypoint with a
                                                    * MapPoint.  Nothing but the result row is written */
};
/* One row per problem, in device memory: what the caller reads off the Frame. */
typedef struct orbx_pose_problem {
    int32_t model, model2;         /* mpCamera and, with eyes = 2, mpCamera2: 0 = Pinhole (cam[0..3] = fx, fy, cx, cy), 1 = KannalaBrandt8
                                    * (cam = mvParameters as orbx_camera_kb8 lays them out); project and projectJac are virtual */
    float cam[8], cam2[8];         /* the stereo edges read Frame::fx, fy, cx, cy from cam[0..3] */
    float mbf;                     /* Frame::mbf (stereo edges) */
    float Trl[12];                 /* Frame::mTrl, 3x4 row-major (right-eye edges) */
    float inv_level_sigma2[ORBX_MAX_LEVELS];      /* mvInvLevelSigma2; the handle's nlevels entries are read */
} orbx_pose_problem;
/* One row per problem.  Every field computed before the exit holds its value, the rest is zero. */
typedef struct orbx_pose_result {
    int32_t status;                /* orbx_pose_optimization_status */
    int32_t n_initial;             /* nInitialCorrespondences */
    int32_t n_bad;                 /* nBad of the last round run */
    int32_t n_inliers;             /* the return value: n_initial - n_bad, 0 for TOO_FEW */
    int32_t rounds;                /* optimisations run: 0, 1 or 4 */
    int32_t empty_rounds;          /* bit r: round r found NO edge at level 0 - initializeOptimization(0) builds no index mapping, optimize
                                    * returns -1 at once, the estimate stays the initial pose and every edge is classified there */
    int32_t its[4];                /* per round what optimize() returned: the LM iterations run, the terminating one included; -1 in an empty round */
    int32_t trials[4];             /* per round the trials (_levenbergIterations) over its iterations */
    double lambda[4], chi2[4];     /* per round _currentLambda and the robust chi2 (currentChi) when its last iteration ended */
} orbx_pose_result;

/*   frame_first, frame_step : problem p is frame f = frame_first + p*frame_step (no index may be negative).  eyes = 1: a one-camera frame
 *                     (monocular, rectified stereo, RGB-D).  eyes = 2: f is a RIG (mpCamera2 != 0): its eyes are device frames 2f and 2f + 1, its
 *                     rows of d_matches / d_outlier are 2p and 2p + 1, and d_poses holds one pose per rig.
 *   d_problems[p]   : see above.
 *   d_kps[f*capacity + i], d_n_out[f] : the observations and N.  eyes = 1: mvKeysUn (:911, :943).  eyes = 2: the RAW mvKeys of the left eye and
 *                     mvKeysRight of the right (:982, :1013).  x, y and octave are read.
 *   d_u_right[f*capacity + i] : mvuRight, or NULL (no stereo edge; required NULL with eyes = 2).  An entry that is NOT < 0 makes a stereo edge.
 *   d_matches[row*capacity + i] : the per-keypoint match rows the projection and BoW searches write, as indices into d_mp_world; -1 = the
 *                     keypoint holds no MapPoint.  d_mp_world[m*3] = GetWorldPos(), m < n_map_points.
 *   d_poses[f*12]   : in/out, Frame::mTcw rows 0..2 (3x4 row-major), the layout orbx_frustum_requests_device reads.  Written on ALL_ROUNDS and
 *                     FEW_EDGES; every NaN leaves as 0x7fc00000.
 *   d_outlier[row*capacity + i] : in/out, mvbOutlier.  Entries from N on are not touched; entries without a MapPoint are left as they were;
 *                     the others are written on every status but BAD_ARGUMENT.  Between the rounds they are the edges' level flags.
 *   d_result[p]     : see above.
 * g2o's and Eigen's arithmetic is the library's own definition (k_pose_optimization.hpp states each): the order of the
 * 28 double sums is a function of the edge index alone (256 slots, then one fixed tree), so the result does not depend on the launch; the
 * 6x6 system is solved by Cholesky, a pivot that is not positive fails the trial.  There is no depth test: a point behind the camera
 * contributes, a point with z == 0 makes the trial's chi2 non-finite and the trial is rejected.  The classification reads the error of the
 * LAST trial, rejected or not, as the reference's does.  Asynchronous on the handle's stream; one launch, one workgroup of 256 lanes per
 * problem, 896 bytes of static LDS (four waves' partial sums) and nothing staged per keypoint: the capacity has no LDS bound.  No workspace.
 * Out of scope: PoseInertialOptimization*, discarding the outlier MapPoints after the call (src/Tracking.cc:2336-2360: the caller's). */
int orbx_optimize_pose_device(orbx_handle* h, int n_problems, int frame_first, int frame_step, int eyes, const orbx_pose_problem* d_problems,
                              const orbx_keypoint* d_kps, const int* d_n_out, const float* d_u_right, int capacity, const int* d_matches,
                              const float* d_mp_world, int n_map_points, float* d_poses, uint8_t* d_outlier, orbx_pose_result* d_result);

/* ---- next row (second half): ORBmatcher::SearchByProjection ---------------------------------------
 * For Nleft == -1 frames (monocular, rectified stereo, RGB-D).  MapPoints, poses and frustum tests belong to the tracker and
 * the map (out of scope), so they enter as plain arrays.  One search request per MapPoint: */
typedef struct orbx_proj_query {
    float u, v;          /* projected position in the current frame: uv (ORBmatcher.cc:2003) / MapPoint::mTrackProjX, mTrackProjY (:58) */
    float ur;            /* predicted right-eye column: uv.x - mbf*invzc (:2043) / mTrackProjXR (:70); used only where mvuRight > 0 */
    float radius;        /* window half-size: th*mvScaleFactors[octave] (:2014) / RadiusByViewingCos(cos)[*th]*mvScaleFactors[level] (:52-58) */
    int32_t min_level, max_level;   /* GetFeaturesInArea's level range: (oct-1, oct+1) | (oct, -1) | (0, oct) (:2018-2023) / (level-1, level) (:58) */
    int32_t flags;       /* bit 0: search this request; bit 1: its MapPoint has Observations() > 0 (it then closes the keypoint it takes) */
    float angle;         /* LastFrame.mvKeysUn[i].angle for the rotation histogram (:2067); unused in ratio mode */
} orbx_proj_query;

/* Front half of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (src/ORBmatcher.cc:1961-2023, 2043): for pair p the
 * keypoints of frame last_first + p*last_step that hold a MapPoint are projected into frame cur_first + p*cur_step.
 *   d_kps / d_kps_un    : mvKeys (octave) / mvKeysUn (angle) of all frames          d_n_out : N of all frames
 *   d_mp_flags[f*capacity + i] : bit 0 = LastFrame.mvpMapPoints[i] != NULL && !mvbOutlier[i], bit 1 = Observations() > 0
 *   d_world[(f*capacity + i)*3]: MapPoint::GetWorldPos()
 *   d_poses[f*12]       : Frame::mTcw, rows 0..2 (3x4, row-major) of every frame
 *   cam (fx, fy, cx, cy): Pinhole::project;  bounds4: mnMinX, mnMaxX, mnMinY, mnMaxY;  mbf, mb: Frame::mbf, mb;  th, mono as passed
 *   d_queries[p*capacity + i]  : out, one request per keypoint of the last frame (flags = 0 where the reference `continue`s)
 * Asynchronous on the handle's stream. */
int orbx_project_last_frame_device(orbx_handle* h, int n_pairs, int last_first, int last_step, int cur_first, int cur_step,
                                   const orbx_keypoint* d_kps, const orbx_keypoint* d_kps_un, const int* d_n_out, int capacity,
                                   const uint8_t* d_mp_flags, const float* d_world, const float* d_poses, const orbx_camera* cam,
                                   const float* bounds4, float mbf, float mb, float th, int mono, orbx_proj_query* d_queries);

/* The search itself, for n_pairs frames cur_first + p*cur_step of one device-resident batch.
 *   ratio_mode 0: SearchByProjection(CurrentFrame, LastFrame, ...) (src/ORBmatcher.cc:2025-2175): best candidate, TH_HIGH = 100, rotation
 *                 histogram when check_orientation;
 *                 With max_distance = ORBdist, d_occupied = "mvpMapPoints[i2] != NULL", every request's flags bit 1 set and d_u_right = NULL
 *                 this is also SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:2179-2300, Relocalization):
 *                 the caller projects pKF's MapPoints (:2200-2226: bounds, distance invariance, PredictScale) into requests.
 *   max_distance: the acceptance bound on the best descriptor distance: ORBmatcher::TH_HIGH = 100 for the first two forms (:98, :2058)
 *   ratio_mode 1: SearchByProjection(F, vpMapPoints, th, ...) (src/ORBmatcher.cc:44-135): best and second best, the ratio nn_ratio applies
 *                 only when both lie on the same pyramid level; the caller passes only MapPoints with mbTrackInView that are not bad and
 *                 pass the far-point test (:50-59), in vpMapPoints order.
 *   d_queries[p*query_capacity + i], d_n_queries[p] (NULL: query_capacity requests per frame, unused ones have flags = 0)
 *   d_query_desc[((desc_first + p*desc_step)*query_capacity + i)*32] : MapPoint::GetDescriptor() of request i (desc_first / desc_step index
 *                 blocks of query_capacity descriptors: for frame-to-frame matching the last frames' blocks of a per-frame array)
 *   d_kps_un, d_desc, d_n_out, d_grid_off, d_grid_idx : mvKeysUn, mDescriptors, N, mGrid of all frames (orbx_frame_finish_device)
 *   d_u_right[f*capacity + i] : mvuRight of all frames, or NULL (monocular)
 *   d_occupied[p*capacity + i] : in/out or NULL (= all free): the keypoint already holds a MapPoint with Observations() > 0
 *   d_matches[p*capacity + i]  : out, request whose MapPoint the keypoint holds afterwards, -1 = none;  d_n_matches[p] : the return value
 * Asynchronous on the handle's stream. */
int orbx_search_by_projection_device(orbx_handle* h, int n_pairs, int cur_first, int cur_step, const orbx_proj_query* d_queries,
                                     const uint8_t* d_query_desc, int desc_first, int desc_step, const int* d_n_queries, int query_capacity,
                                     const orbx_keypoint* d_kps_un, const uint8_t* d_desc, const int* d_n_out, int capacity,
                                     const int* d_grid_off, const int* d_grid_idx, const float* bounds4, const float* d_u_right,
                                     uint8_t* d_occupied, int ratio_mode, float nn_ratio, int max_distance, int check_orientation,
                                     int* d_matches, int* d_n_matches);

/* ORBmatcher::SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) for TWO-CAMERA frames (src/ORBmatcher.cc:44-213 with
 * F.Nleft != -1; caller Tracking::SearchLocalPoints, src/Tracking.cc:2986), on the grids of orbx_frame_finish_two_eyes_device.  For pair q
 * the left eye is frame fL = 2*(pair_first + q*pair_step) (mvKeys, mGrid) and the right eye frame fL + 1 (mvKeysRight, mGridRight); each eye
 * has its own keypoint count d_n_out[f].  MapPoint i of pair q (the caller's vpMapPoints order, after the skips of :53-60) has two requests:
 *   d_queries[(q*query_capacity + i)*2 + 0]  left  (L, :62-140): u, v = mTrackProjX, mTrackProjY;
 *            radius = RadiusByViewingCos(mTrackViewCos) (2.5 if > 0.998, else 4.0) * th (only when th != 1) * mvScaleFactors[mnTrackScaleLevel];
 *            min_level, max_level = mnTrackScaleLevel - 1, mnTrackScaleLevel;  flags bit 0 = mbTrackInView
 *   d_queries[(q*query_capacity + i)*2 + 1]  right (R, :145-207): u, v = mTrackProjXR, mTrackProjYR;
 *            radius = RadiusByViewingCos(mTrackViewCosR) * mvScaleFactors[mnTrackScaleLevelR] - WITHOUT th (as the reference: :148);
 *            min_level, max_level = mnTrackScaleLevelR - 1, mnTrackScaleLevelR;  flags bit 0 = mbTrackInViewR && mnTrackScaleLevelR != -1
 *   flags bit 1 of both: Observations() > 0 (set it the same on both);  ur and angle are unused.
 *   d_query_desc[((desc_first + q*desc_step)*query_capacity + i)*32] : MapPoint::GetDescriptor(), one per MapPoint;
 *   d_n_queries[q] : MapPoints of pair q (NULL: query_capacity)
 *   d_kps, d_desc, d_n_out : the extraction's RAW keypoints (mvKeys / mvKeysRight), descriptors and counts, [f*capacity + i]
 *   d_grid_off, d_grid_idx, bounds4 : as written by / passed to orbx_frame_finish_two_eyes_device
 *   d_left_to_right[fL*capacity + i], d_right_to_left[(fL + 1)*capacity + j] : mvLeftToRightMatch / mvRightToLeftMatch
 *            (ComputeStereoFishEyeMatches: orbx_stereo_fisheye_match_device writes them in this layout), each read on its own branch as
 *            the reference does, not assumed inverse; NULL = all -1; an entry
 *            outside [0, N of the other eye) is taken as -1 (the reference would index out of bounds)
 *   d_occupied[(2q + eye)*capacity + i] : in/out or NULL (= all free): the keypoint holds a MapPoint with Observations() > 0
 *   nn_ratio : mfNNratio;  max_distance : TH_HIGH = 100
 *   d_matches[(2q + eye)*capacity + i] : out, the MapPoint the keypoint holds afterwards (the LAST one written to it), -1 = none written
 *   d_n_matches[q] : the return value: every write, 1 or 2 per accepted sub-search (the pairing writes count)
 * A pairing write writes what it is given (also onto a keypoint outside the grid, and without looking at what the keypoint holds: a
 * MapPoint without observations so written opens a closed keypoint again).  Supported: the tables of a pair live in LDS,
 *   100 * ((capacity + 3) & ~3) + 8 * query_capacity + 12 392 <= 163 328 bytes
 * (2 x orbx_max_keypoints() = 1302 of a 1200-feature extractor with query_capacity up to 2048, or capacity 1344 at 2048 MapPoints); a larger
 * call returns ORBX_ERR_UNSUPPORTED before anything is launched.  Asynchronous on the handle's stream. */
int orbx_search_by_projection_two_eyes_device(orbx_handle* h, int n_pairs, int pair_first, int pair_step, const orbx_proj_query* d_queries,
                                              const uint8_t* d_query_desc, int desc_first, int desc_step, const int* d_n_queries,
                                              int query_capacity, const orbx_keypoint* d_kps, const uint8_t* d_desc, const int* d_n_out,
                                              int capacity, const int* d_grid_off, const int* d_grid_idx, const float* bounds4,
                                              const int* d_left_to_right, const int* d_right_to_left, uint8_t* d_occupied, float nn_ratio,
                                              int max_distance, int* d_matches, int* d_n_matches);

/* ---- ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) for TWO-CAMERA frames (src/ORBmatcher.cc:1961-2177 with
 * CurrentFrame.Nleft != -1; caller Tracking::TrackWithMotionModel) -------------------------------------------------------------------
 * KannalaBrandt8::mvParameters[0..7] (src/CameraModels/KannalaBrandt8.cpp:28-44) as plain floats. */
typedef struct orbx_camera_kb8 { float fx, fy, cx, cy, k1, k2, k3, k4; } orbx_camera_kb8;

/* KannalaBrandt8::project(const cv::Point3f&) (src/CameraModels/KannalaBrandt8.cpp:28-44) over n device-resident points:
 *   d_xyz[i*3 + {0,1,2}] in, d_uv[i*2 + {0,1}] out.
 * Every operation is rounded in binary32 in the reference's order; atan2f is glibc 2.35's binary32 routine, cos(psi) / sin(psi) are taken
 * as cosf / sinf.  The projection by itself, for callers' own tests on such rigs; Frame::isInFrustumChecks (src/Frame.cc:1181-1254) over a
 * local map is orbx_frustum_requests_two_eyes_device, which projects inside its kernel.  Asynchronous on the handle's stream. */
int orbx_kb8_project_device(orbx_handle* h, int n, const float* d_xyz, const orbx_camera_kb8* cam, float* d_uv);

/* Front half (src/ORBmatcher.cc:1971-2023 and :2084-2101).  A rig frame r is device frames 2r (left eye, mvKeys) and 2r + 1 (right eye,
 * mvKeysRight), as in orbx_frame_finish_two_eyes_device.  For pair p the MapPoints of rig last_first + p*last_step are projected into rig
 * cur_first + p*cur_step.  MapPoint i of LastFrame (i < Nleft: left keypoint i; i >= Nleft: right keypoint i - Nleft) is request
 * j = eye*capacity + i, 2*capacity per pair, which keeps the reference's order.
 *   d_kps    : the RAW keypoints of all device frames (octave :2009-2010, angle :2066-2068)      d_n_out : Nleft / Nright per device frame
 *   d_mp_flags[f*capacity + i] : bit 0 = LastFrame.mvpMapPoints[..] != NULL && !mvbOutlier[..], bit 1 = Observations() > 0, per device frame f
 *   d_world[(f*capacity + i)*3]: MapPoint::GetWorldPos(), per device frame
 *   d_poses[r*12]       : Frame::mTcw, rows 0..2 (3x4, row-major), per RIG frame
 *   trl12               : CurrentFrame.mTrl (3x4, row-major; host memory): x3Dr = mTrl.R * x3Dc + mTrl.t as a cv::Mat product (:2084)
 *   cam                 : CurrentFrame.mpCamera.  The right request is projected with the LEFT camera's parameters too, as :2086 does
 *                         (mpCamera, not mpCamera2); it has no depth test and no bounds test.
 *   bounds4: mnMinX, mnMaxX, mnMinY, mnMaxY;  mb: Frame::mb;  th, mono as passed
 *   d_queries[(p*2*capacity + j)*2 + {0: L, 1: R}] : out.  flags bit 0 of L: the MapPoint exists, invzc >= 0 (:1999) and the left projection
 *            is inside the bounds (:2004-2007); bit 0 of R: the same condition; bit 1 of both: Observations() > 0.  radius = th *
 *            mvScaleFactors[octave]; min_level, max_level by bForward / bBackward (:2017-2022, :2096-2101); angle = the last keypoint's raw
 *            angle; ur is unused (0).  Where the reference `continue`s both records are all zero.
 * A last frame with Nleft == -1 against a two-camera current frame is not built.  Asynchronous on the handle's stream. */
int orbx_project_last_frame_two_eyes_device(orbx_handle* h, int n_pairs, int last_first, int last_step, int cur_first, int cur_step,
                                            const orbx_keypoint* d_kps, const int* d_n_out, int capacity, const uint8_t* d_mp_flags,
                                            const float* d_world, const float* d_poses, const float* trl12, const orbx_camera_kb8* cam,
                                            const float* bounds4, float mb, float th, int mono, orbx_proj_query* d_queries);

/* The search (src/ORBmatcher.cc:2013-2174) for n_pairs rigs cur_first + q*cur_step, on the grids of orbx_frame_finish_two_eyes_device.
 *   d_queries[(q*2*capacity + j)*2 + {0: L, 1: R}] : the requests above, or a caller's own; request j's L searches the left eye (mGrid, mvKeys),
 *            its R the right eye (mGridRight, mvKeysRight).  Requests are settled in the order of j, L before R.
 *   d_query_desc[(q*2*capacity + j)*32] : MapPoint::GetDescriptor() of request j
 *            (d_query_desc and d_desc are read 16 bytes at a time: both buffers must be 16-byte aligned, as hipMalloc's are)
 *   d_kps, d_desc, d_n_out : RAW keypoints, descriptors and counts of all device frames;  d_grid_off, d_grid_idx, bounds4 : as written by /
 *            passed to orbx_frame_finish_two_eyes_device
 *   d_occupied[(2q + eye)*capacity + i] : in/out or NULL (= all free): the keypoint holds a MapPoint with Observations() > 0
 *   max_distance : TH_HIGH = 100 (:2059, :2126);  check_orientation : ONE rotation histogram over both eyes (:2155-2174)
 *   d_matches[(2q + eye)*capacity + i] : out, the request j whose MapPoint the keypoint holds afterwards, -1 = none;  d_n_matches[q] : the return value
 * R is NOT run when its request's L has flags bit 0 set and L's GetFeaturesInArea result (cell window, level range, box test; closed
 * keypoints count) is empty: the `continue` of :2024 skips the rest of the MapPoint.  That rule belongs to this entry because it needs
 * the grid.  An L whose best distance is above max_distance, or whose candidates are all closed, does not stop R; an L with flags bit 0
 * clear is not run and does not stop an R whose own bit 0 is set.  Keypoints outside the grid never match.  A keypoint octave outside [0, 255]
 * (no extractor writes one) is taken as 0 or 255 when the frame is staged, where the reference compares the value as it is.  Supported: the tables of
 * a pair live in LDS,
 *   96 * ((capacity + 3) & ~3) + 12 * capacity + 12 496 <= 163 328 bytes
 * (capacity <= 1396: 2 x orbx_max_keypoints() = 1302 of a 1200-feature extractor is inside); a larger call returns ORBX_ERR_UNSUPPORTED
 * before anything is launched.  Asynchronous on the handle's stream. */
int orbx_search_last_frame_two_eyes_device(orbx_handle* h, int n_pairs, int cur_first, int cur_step, const orbx_proj_query* d_queries,
                                           const uint8_t* d_query_desc, const orbx_keypoint* d_kps, const uint8_t* d_desc, const int* d_n_out,
                                           int capacity, const int* d_grid_off, const int* d_grid_idx, const float* bounds4,
                                           uint8_t* d_occupied, int max_distance, int check_orientation, int* d_matches, int* d_n_matches);

/* ---- next row: Frame::ComputeBoW (src/Frame.cc:739-746) --------------------------------------------------
 * = DBoW2::TemplatedVocabulary<FORB>::transform(features, BowVector, FeatureVector, levelsup = 4)
 * (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1196, 1218-1262; BowVector.cpp:34-83; FeatureVector.cpp:31-46).
 * The vocabulary is an object of its own (System.cc:81-82 loads one per process and shares it between all frames). */
typedef struct orbx_vocabulary orbx_vocabulary;
/* Replaces ORBVocabulary::loadFromTextFile (TemplatedVocabulary.h:1338-1423): the ORBvoc.txt format ("k L scoring weighting", then one
 * node per line: parent, is-leaf, 32 descriptor bytes, weight).  device < 0: current HIP device.  Errors: ORBX_ERR_BAD_ARGUMENT (file). */
int orbx_vocabulary_load_text(orbx_vocabulary** out, const char* path, int device);
/* The same from arrays: node 0 is the root, node n >= 1 has parent[n] < n, is_leaf[n], desc[n*32 ..], weight[n]; word ids are given to the
 * leaves in node order, children are listed in node order (both as the loader does).  scoring: 0 L1_NORM .. 5 DOT_PRODUCT; weighting:
 * 0 TF_IDF, 1 TF, 2 IDF, 3 BINARY (BowVector.h:39-56). */
int orbx_vocabulary_create(orbx_vocabulary** out, int k, int L, int scoring, int weighting, int n_nodes, const int* parent,
                           const uint8_t* is_leaf, const uint8_t* desc, const double* weight, int device);
void orbx_vocabulary_destroy(orbx_vocabulary* v);
int orbx_vocabulary_info(const orbx_vocabulary* v, int* k, int* L, int* n_nodes, int* n_words);
/* mBowVec / mFeatVec of n_frames device-resident frames (d_desc, d_n_out: mDescriptors, N of orbx_extract_batch_device):
 *   d_word_ids[f*capacity + j], d_word_weights[f*capacity + j], d_n_words[f] : the BowVector (std::map<WordId, WordValue>) in key order
 *   d_feat_nodes[f*capacity + j], d_feat_idx[f*capacity + j], d_n_feat[f]    : the FeatureVector (std::map<NodeId, vector<unsigned>>)
 *                                                                               flattened in (node, feature index) order
 * Asynchronous on the handle's stream; the vocabulary must live on the handle's device. */
int orbx_compute_bow_device(orbx_handle* h, const orbx_vocabulary* v, int n_frames, const uint8_t* d_desc, const int* d_n_out, int capacity,
                            int levels_up, uint32_t* d_word_ids, double* d_word_weights, int* d_n_words, uint32_t* d_feat_nodes,
                            uint32_t* d_feat_idx, int* d_n_feat);

/* ---- the consumer of the BowVector: KeyFrameDatabase's place recognition -----------------------------------------------------------
 * KeyFrameDatabase::DetectNBestCandidates (src/KeyFrameDatabase.cc:612-780; LoopClosing::NewDetectCommonRegions, src/LoopClosing.cc:463:
 * the vpLoopBowCand / vpMergeBowCand that orbx_search_by_bow_keyframes_device -> orbx_sim3_solve_device ->
 * orbx_search_by_projection_sim3_device start from) and KeyFrameDatabase::DetectRelocalizationCandidates (:783-895;
 * Tracking::Relocalization, src/Tracking.cc:3192: the keyframes orbx_search_by_bow_device -> orbx_optimize_pose_device ->
 * orbx_frustum_requests_device(RELOCALIZATION) -> orbx_search_by_projection_device start from) for n_queries independent queries against
 * one database of n_db keyframe rows.  Who is in the database and who observes whom stays with the caller: the add / erase bookkeeping
 * is not built.  DetectLoopCandidates, DetectCandidates and DetectBestCandidates have no caller in the reference and are not built. */
enum orbx_place_mode {
    ORBX_PLACE_N_BEST = 0,                 /* DetectNBestCandidates(pKF, vpLoopCand, vpMergeCand, nNumCandidates) */
    ORBX_PLACE_RELOCALIZATION = 1          /* DetectRelocalizationCandidates(F, pMap) */
};
/* How a query left the function; every way out has a name: */
enum orbx_place_status {
    ORBX_PLACE_OK = 0,                     /* the function ran to its end */
    ORBX_PLACE_NO_SHARING = 1,             /* lKFsSharingWords.empty() (:655, :808): no row shares a word (N_BEST: no row that is not connected) */
    ORBX_PLACE_NONE_SCORED = 2,            /* lScoreAndMatch.empty() (:686, :839).  Unreachable - the row that holds maxCommonWords passes its own
                                            * threshold - and kept as a name */
    ORBX_PLACE_EMPTY_DATABASE = 3,         /* n_db == 0: NO_SHARING, named apart */
    ORBX_PLACE_EMPTY_QUERY = 4,            /* the query has no words: NO_SHARING, named apart */
    ORBX_PLACE_BAD_KEYFRAME = 5,           /* N_BEST: `if(pKFi->isBad()) continue;` (:735-736) advances neither i nor it - once a bad keyframe
                                            * reaches the front of the walk the reference never returns.  The entry stops there and writes what
                                            * was collected.  SetBadFlag erases a keyframe from the database, so only a caller's row with bit 0 of
                                            * its flags set gets here */
    ORBX_PLACE_TRUNCATED = 6               /* RELOCALIZATION: the list is longer than cand_capacity; its first cand_capacity entries are written,
                                            * n_loop holds the true count */
};
/* One row per query.  Every field computed before the exit holds its value, the rest is zero. */
typedef struct orbx_place_result {
    int32_t status;                /* orbx_place_status */
    int32_t n_sharing;             /* lKFsSharingWords.size() */
    int32_t max_common_words;      /* maxCommonWords */
    int32_t min_common_words;      /* minCommonWords = maxCommonWords*0.8f: a float product truncated to int; a row is scored when words > it */
    int32_t n_scored;              /* nscores = lScoreAndMatch.size() */
    float best_acc_score;          /* bestAccScore */
    int32_t n_loop;                /* N_BEST: vpLoopCand.size(); RELOCALIZATION: vpRelocCandidates.size(), whatever cand_capacity is */
    int32_t n_merge;               /* N_BEST: vpMergeCand.size() */
} orbx_place_result;

/*   v               : the vocabulary the BoW vectors were made with.  Only L1_NORM scoring (ORBvoc.txt's) is built: another scoring returns
 *                     ORBX_ERR_UNSUPPORTED before any launch.
 *   d_db_word_ids[k*capacity + j], d_db_word_weights[k*capacity + j], d_db_n_words[k] : the mBowVec of database row k, the layout
 *                     orbx_compute_bow_device writes (a keyframe's row is a copy of what that entry produced).  The n_db rows are IN THE ORDER
 *                     OF KeyFrameDatabase::add, erased keyframes removed: that is the order inside every mvInvertedFile[word] (:39-66).
 *   d_db_map_id[k]  : GetMap() as a number.  d_db_flags[k]: bit 0 = isBad(), bit 1 = GetMap()->IsBad().  Bit 1 is the MAP's: it must be the same
 *                     on every row of one map; the entry reads it from the candidate's own row.
 *   d_db_covis[k*10 + j] : GetBestCovisibilityKeyFrames(10) as database rows, in that function's order; -1 for a neighbour that is not in
 *                     the database or a list shorter than ten (a value outside [0, n_db) is skipped).
 *   q_first, q_step, d_q_word_ids, d_q_word_weights, d_q_n_words, q_capacity : query q is row q_first + q*q_step of these arrays (no index
 *                     may be negative): the frames orbx_compute_bow_device just wrote can be used directly.  d_q_map_id[q]: the map of pKF
 *                     (N_BEST), pMap (RELOCALIZATION).
 *   d_connected[q*n_db + k] : N_BEST: non-zero when row k is in pKF->GetConnectedKeyFrames() (:622, :638); NULL = none.  Such a row never
 *                     enters the list and never takes the query's id: it does not count towards maxCommonWords and is skipped as a
 *                     covisibility neighbour (:704).  Ignored in RELOCALIZATION mode, whose reference has no such test.
 *   n_candidates    : nNumCandidates (3 at the call site), N_BEST only; 0 returns no candidate.
 *   d_score[q*n_db + k] : IN AND OUT, mPlaceRecognitionScore / mRelocScore.  The reference writes the field only for the rows that pass the
 *                     word threshold (:681, :834) and reads it for every covisibility neighbour that carries the query's id (:707-711,
 *                     :860-864), rows that share a word but did not pass included: for those it reads what an EARLIER query left (the
 *                     constructor sets mPlaceRecognitionScore to 0 and leaves mRelocScore uninitialised, src/KeyFrame.cc:34-35, :52).  So
 *                     this is state, one row per query: the entry reads it, overwrites only the rows it scores and leaves the rest byte for
 *                     byte; a caller that replays the reference's sequence of queries hands each query the previous one's row.  The entry
 *                     promises "what the reference returns from this state".  Assumed: no database row carries the query's id before the
 *                     call (the reference's ids are unique and each is queried once).
 *   d_result[q]     : see above.
 *   d_loop[q*n_candidates + i], d_merge[..] : N_BEST: vpLoopCand / vpMergeCand as database rows; entries from n_loop / n_merge on are not
 *                     touched.  d_cand[q*cand_capacity + i]: RELOCALIZATION: vpRelocCandidates; entries from n_loop on are not touched.
 *   d_common_words[q*n_db + k] : optional (NULL), the words row k shares with query q, connected rows included.
 * Order: lKFsSharingWords is in order of first encounter - the query's words ascending, each word's inverted list in `add` order - which is
 * the order of (smallest shared word id, database row); lScoreAndMatch and lAccScoreAndMatch keep it.  RELOCALIZATION never sorts: that is
 * its output order.  N_BEST's list::sort(compFirst) is stable on a.first > b.first: equal accumulated scores stay in list order.  The
 * score is L1Scoring::score as written: a double 0, for every common word in ascending id score += fabs(vi - wi) - fabs(vi) - fabs(wi), a
 * SEQUENTIAL sum of three-rounding terms, then -score/2.0 narrowed to float.  accScore is a float sum in neighbour order, pBestKF the first
 * strictly greater score, bestAccScore starts at 0.  RELOCALIZATION keeps accScore > 0.75f*bestAccScore, skips another map's keyframe
 * before the duplicate set, then drops duplicates of pBestKF.  N_BEST walks on while either list is short; a keyframe enters the duplicate
 * set whether or not it was pushed (a same-map entry met when the loop list is full, a merge candidate of a bad map).
 * Two launches: k_place_pairs, one wave per (query, row) with the query's words staged in 12*q_capacity bytes of LDS, and k_place_query,
 * one workgroup per query with 12 bytes per list slot (a power of two of slots) and 4 per row.  Both must fit 160 KB - 512: q_capacity
 * <= 13610 and n_db <= 8192, else ORBX_ERR_UNSUPPORTED before anything is launched or allocated.  No bound depends on the data: every
 * list has room for all n_db rows.  n_queries <= 65535.  The pairs' workspace (12 bytes per query and row) belongs to the handle and
 * grows on first use.  ORBX_ERR_BAD_ARGUMENT is returned before any launch.  Asynchronous on the handle's stream; no CPU path. */
int orbx_detect_candidates_device(orbx_handle* h, const orbx_vocabulary* v, int mode, int n_db, const uint32_t* d_db_word_ids,
                                  const double* d_db_word_weights, const int* d_db_n_words, int capacity, const int* d_db_map_id,
                                  const uint8_t* d_db_flags, const int* d_db_covis, int n_queries, int q_first, int q_step,
                                  const uint32_t* d_q_word_ids, const double* d_q_word_weights, const int* d_q_n_words, int q_capacity,
                                  const int* d_q_map_id, const uint8_t* d_connected, int n_candidates, float* d_score, orbx_place_result* d_result,
                                  int* d_loop, int* d_merge, int* d_cand, int cand_capacity, int* d_common_words);

/* ---- covisibility: the lists of keyframes every chain above starts from ---------------------------------------------------------
 * One operation of the reference - walk a row of MapPoints, walk each MapPoint's observations, count per observing keyframe - in its
 * three places, for ONE-CAMERA keyframes (NLeft == -1) and a batch of independent subjects:
 *   KeyFrame::UpdateConnections (src/KeyFrame.cc:388-511): every new keyframe, after every Fuse, every keyframe loop closing touches;
 *   the voting half of Tracking::UpdateLocalKeyFrames (src/Tracking.cc:3030-3102): every tracked frame, between
 *     orbx_optimize_pose_device and orbx_frustum_requests_device;
 *   the test inside LocalMapping::KeyFrameCulling's loop (src/LocalMapping.cc:977-1043): orbx_keyframe_redundancy_device below.
 * The tables are the other entries': the observation CSR of orbx_update_map_points_device, the per-keypoint MapPoint row, d_kps_un,
 * d_n_out, the flags.  All integers (one float product in the redundancy test): the results are the reference's, byte for byte. */
enum orbx_covis_mode {
    ORBX_COVIS_UPDATE_CONNECTIONS = 0,     /* KeyFrame::UpdateConnections */
    ORBX_COVIS_LOCAL_KEYFRAMES = 1         /* Tracking::UpdateLocalKeyFrames up to :3102, before the neighbour expansion */
};
enum orbx_covis_status {
    ORBX_COVIS_OK = 0,
    ORBX_COVIS_EMPTY = 1,                  /* UPDATE_CONNECTIONS: KFcounter.empty() (:423) returns before anything is assigned: no list entry of
                                            * the subject is written.  (LOCAL_KEYFRAMES goes on with an empty list and pKFmax NULL: OK, n_counter 0,
                                            * kf_max -1) */
    ORBX_COVIS_TRUNCATED = 2,              /* a list is longer than conn_capacity: the row holds the true counts, the first conn_capacity entries
                                            * of each order are written */
    ORBX_COVIS_BAD_INDEX = 3,              /* a MapPoint index outside [-1, n_points), a list with d_obs_off[m] < 0, d_obs_off[m+1] < d_obs_off[m] or
                                            * d_obs_off[m+1] > d_obs_off[n_points], an observing frame outside [0, n_frames), d_subject_kf[s] outside
                                            * [-1, n_frames): the reference would index out of bounds.  Found before anything of the subject is
                                            * written; no list entry is.  (A bad MapPoint's list is not read and not checked) */
    ORBX_COVIS_DUPLICATE_KEY = 4           /* two of the n_frames keys are equal: the frames have no order.  A property of the CALL, said in every
                                            * subject's row; no list entry of any subject is written */
};
/* One row per subject.  EMPTY, BAD_INDEX and DUPLICATE_KEY rows hold zero counts and kf_max -1. */
typedef struct orbx_covis_result {
    int32_t status;                /* orbx_covis_status */
    int32_t n_counter;             /* UPDATE_CONNECTIONS: KFcounter.size() = mConnectedKeyFrameWeights.size(); LOCAL_KEYFRAMES:
                                    * mvpLocalKeyFrames.size() at :3102; whatever conn_capacity is */
    int32_t n_ordered;             /* UPDATE_CONNECTIONS: mvpOrderedConnectedKeyFrames.size(); LOCAL_KEYFRAMES: 0 */
    int32_t nmax;                  /* nmax (:440) / max (:3094) */
    int32_t kf_max;                /* pKFmax as a device frame: the FIRST strictly greater count in key order; -1 = NULL */
} orbx_covis_result;

/*   n_points, d_obs_off[n_points + 1], d_obs[o*2 + {0,1}] : exactly orbx_update_map_points_device's CSR of (device frame, keypoint row):
 *                     MapPoint m's mObservations.  Only the frame is read here.  A std::map holds a keyframe once: an entry is a vote.
 *   d_mp_flags[m]   : bit 0 = MapPoint::isBad().
 *   n_frames, d_kf_flags[f], d_kf_map_id[f] : bit 0 = KeyFrame::isBad(); GetMap() as a number (UPDATE_CONNECTIONS; may be NULL otherwise).
 *   d_kf_key[f]     : the KeyFrame* address, or any number in the same order.  std::map<KeyFrame*,int> iterates in address order and
 *                     std::sort on pair<int,KeyFrame*> breaks equal weights by address, so the address order is part of the reference's
 *                     result, and only the caller knows it.  Two frames with one key: ORBX_COVIS_DUPLICATE_KEY.
 *   d_subject_mp[s*capacity + i], d_subject_n[s] : mvpMapPoints of subject s as MapPoint indices, -1 for NULL - the row
 *                     orbx_optimize_pose_device takes as its matches; d_subject_n[s] is clamped into [0, capacity].
 *   d_subject_kf[s] : UPDATE_CONNECTIONS: the subject's own device frame (the mnId == mnId test of :415), -1 for none.  d_subject_map_id[s]:
 *                     mpMap.  Both may be NULL in LOCAL_KEYFRAMES mode, which has neither test.
 *   th              : 15 in the reference (:430).
 * UPDATE_CONNECTIONS: every slot i < N is visited - a MapPoint that stands in two slots votes twice, as :401 does.  Skipped: -1, a bad
 * MapPoint; an observer that is the subject itself, is bad, or lives in another map (:415).
 * LOCAL_KEYFRAMES: no self test and no map test; a bad observer IS counted into the map and skipped when the map is walked (:3091): it is
 * neither listed nor eligible as pKFmax.
 * Outputs, one block of conn_capacity entries per subject:
 *   d_counter_kf / d_counter_w [s*conn_capacity + j] : UPDATE_CONNECTIONS: mConnectedKeyFrameWeights, the WHOLE counter, counts below th
 *                     included, in key-ascending order: what GetConnectedKeyFrames / GetWeight - and orbx_detect_candidates_device's
 *                     d_connected - are made from.  LOCAL_KEYFRAMES: mvpLocalKeyFrames at :3102 and each one's count, key ascending, no
 *                     threshold, no sort.
 *   d_ordered_kf / d_ordered_w [s*conn_capacity + j] : UPDATE_CONNECTIONS only (may be NULL otherwise): mvpOrderedConnectedKeyFrames /
 *                     mvOrderedWeights - every count >= th, or if there is none the single pair (nmax, pKFmax) (:452-456) - after sort
 *                     ascending on (weight, key) and push_front: weight descending and, among equal weights, key DESCENDING.  Its first
 *                     ten are GetBestCovisibilityKeyFrames(10), a row of d_db_covis; its front is mpParent under mbFirstConnection.
 *   d_result[s]     : see above.  Entries of a block beyond the counts are never touched.
 * Stays with the caller: the reciprocal AddConnection(this, w) on each listed keyframe and its UpdateBestCovisibles (a sort of THAT
 * keyframe's weight list); AddChild / the parent bookkeeping; the neighbour expansion of UpdateLocalKeyFrames (:3104 onward); nulling a
 * frame's bad MapPoints (:3049).  Two-camera keyframes are not built: a rig's observation has two entries and would vote twice.
 * Two launches: k_covis_rank turns the keys into ranks (a wave per frame), k_covis_vote gives a workgroup per subject with a counter word
 * per frame and 8 bytes per sort slot (a power of two of slots) in LDS.  They must fit 160 KB - 512: n_frames <= 8192, else
 * ORBX_ERR_UNSUPPORTED before anything is launched or allocated.  conn_capacity takes no LDS and has no such bound.  n_subjects <= 65535.
 * The rank tables (8 bytes per frame) belong to the handle and grow on first use.  ORBX_ERR_BAD_ARGUMENT is returned before any launch.
 * Asynchronous on the handle's stream; no CPU path. */
int orbx_covisibility_device(orbx_handle* h, int mode, int n_points, const int* d_obs_off, const int* d_obs, const uint8_t* d_mp_flags, int n_frames,
                             const uint8_t* d_kf_flags, const int* d_kf_map_id, const uint64_t* d_kf_key, int n_subjects, const int* d_subject_mp,
                             const int* d_subject_n, int capacity, const int* d_subject_kf, const int* d_subject_map_id, int th, int conn_capacity,
                             int* d_counter_kf, int* d_counter_w, int* d_ordered_kf, int* d_ordered_w, orbx_covis_result* d_result);

enum orbx_redundancy_status {
    ORBX_REDUNDANCY_OK = 0,
    ORBX_REDUNDANCY_SKIPPED = 1,           /* the map's initial keyframe or a bad one (:977): nothing is counted, no slot state is written */
    ORBX_REDUNDANCY_BAD_INDEX = 2          /* as ORBX_COVIS_BAD_INDEX, and: d_subject_kf[s] outside [0, n_frames), an observation's keypoint row
                                            * outside [0, N_f).  Found before anything of the subject is written; no slot state is */
};
typedef struct orbx_redundancy_result {
    int32_t status;                /* orbx_redundancy_status */
    int32_t n_mps;                 /* nMPs */
    int32_t n_redundant;           /* nRedundantObservations */
    int32_t redundant;             /* 1 when nRedundantObservations > redundant_th*nMPs (:1043): (float)n_redundant > redundant_th*(float)n_mps,
                                    * ONE float product and a float compare, as the int/float expression evaluates */
} orbx_redundancy_result;

/* The test inside LocalMapping::KeyFrameCulling's loop (src/LocalMapping.cc:977-1043) for n_subjects one-camera keyframes, on the same
 * tables.  Subject s is device frame d_subject_kf[s]; d_subject_mp[s*capacity + i] / d_subject_n[s] are its GetMapPointMatches().
 *   d_mp_nobs[m]    : MapPoint::Observations(), which is NOT the list length (a stereo observation adds 2); NULL = the list length.
 *   d_kf_flags[f]   : bit 0 = isBad(), bit 1 = "is the map's initial keyframe" (mnId == GetMap()->GetInitKFid()): either gives SKIPPED.
 *   d_kps_un[f*capacity + i], d_n_out[f] : mvKeysUn of the n_frames frames; only octaves are read.  d_n_out[f] is clamped into [0, capacity].
 *   d_depth[f*capacity + i], d_th_depth[f] : mvDepth and mThDepth, read when monocular == 0 (:992-996; may be NULL otherwise).  The skip is
 *                     depth > th || depth < 0 as written: a NaN depth and -0.0 are counted.
 *   th_obs          : 3.  redundant_th: 0.9f, or 0.5f (inertial and not monocular).
 * Per slot i < N: NULL and bad MapPoints and far points are skipped; nMPs++; only if Observations() > th_obs the observers OTHER than the
 * subject whose octave is <= octave_i + 1 are counted - observers are NOT tested for isBad - and the slot is redundant when that count is
 * > th_obs (the reference's break changes nothing).
 *   d_slot_state[s*capacity + i] : optional (NULL); 0 = not counted, 1 = counted, 2 = redundant, for i < N of an OK subject.
 * Stays with the caller: SetBadFlag and its consequences - KeyFrameCulling culls INSIDE its loop, so a later keyframe of the same loop sees
 * the erased observations; the entry answers, per listed keyframe, what the reference computes from the tables AS THEY STAND, and a caller
 * who wants the exact sequence refreshes the tables after a cull -; the count > 20 && mbAbortBA / count > 100 cut; every inertial branch
 * (:1045-1076).  Two-camera keyframes are not built (:1003 reads mvKeysRight[i] with the unshifted i).
 * One launch, k_keyframe_redundancy, a workgroup per subject with a state byte per slot in LDS: capacity <= 163280, else
 * ORBX_ERR_UNSUPPORTED before anything is launched.  n_subjects <= 65535.  ORBX_ERR_BAD_ARGUMENT (a NaN redundant_th among the reasons) is
 * returned before any launch.  Asynchronous on the handle's stream; no CPU path. */
int orbx_keyframe_redundancy_device(orbx_handle* h, int n_points, const int* d_obs_off, const int* d_obs, const uint8_t* d_mp_flags, const int* d_mp_nobs,
                                    int n_frames, const uint8_t* d_kf_flags, const orbx_keypoint* d_kps_un, const int* d_n_out, const float* d_depth,
                                    const float* d_th_depth, int n_subjects, const int* d_subject_mp, const int* d_subject_n, int capacity,
                                    const int* d_subject_kf, int monocular, int th_obs, float redundant_th, orbx_redundancy_result* d_result,
                                    uint8_t* d_slot_state);

/* ---- the consumer of the FeatureVector: ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vpMapPointMatches) ------------------
 * (src/ORBmatcher.cc:269-471; Tracking::TrackReferenceKeyFrame, Tracking::Relocalization), Nleft == -1: for n_pairs pairs
 * (keyframe = frame kf_first + p*kf_step, current frame = frame cur_first + p*cur_step of one device-resident batch) the features of
 * the two frames that fell into the same vocabulary node are matched: nearest / second nearest by ORBmatcher::DescriptorDistance
 * among the frame's not yet matched features of the node, TH_LOW and the ratio test, rotation-histogram clean-up (ComputeThreeMaxima).
 *   d_feat_nodes, d_feat_idx, d_n_feat : mFeatVec of all frames as written by orbx_compute_bow_device (same capacity)
 *   d_kf_mp_flags[p*capacity + i]      : bit 0 = keypoint i of the keyframe holds a MapPoint that is not bad (:301-307)
 *   d_kps[f*capacity + i]              : mvKeys of all frames (only .angle is read: mvKeysUn keeps it, src/Frame.cc:776-780)
 *   d_desc, d_n_out                    : mDescriptors, N of all frames
 *   nn_ratio = mfNNratio, th_low = ORBmatcher::TH_LOW (50), check_orientation = mbCheckOrientation
 *   d_matches[p*capacity + i]          : out, the keyframe keypoint whose MapPoint keypoint i of the frame receives, -1 = none
 *   d_n_matches[p]                     : out, the return value
 * A FeatureVector index >= d_n_out of its frame names no feature (here and in orbx_search_by_bow_keyframes_device): a keyframe entry with
 * one is skipped before it searches or votes in the rotation histogram, a candidate with one is dropped.
 * Asynchronous on the handle's stream.  Errors: ORBX_ERR_UNSUPPORTED if the tables (22 bytes per slot of the capacity rounded up to 16, + 64) do not fit a workgroup's LDS
 * (with 64 more bytes per slot the descriptors are staged in LDS too; without them they are read from L2). */
int orbx_search_by_bow_device(orbx_handle* h, int n_pairs, int kf_first, int kf_step, int cur_first, int cur_step,
                              const uint32_t* d_feat_nodes, const uint32_t* d_feat_idx, const int* d_n_feat, const uint8_t* d_kf_mp_flags,
                              const orbx_keypoint* d_kps, const uint8_t* d_desc, const int* d_n_out, int capacity, float nn_ratio,
                              int th_low, int check_orientation, int* d_matches, int* d_n_matches);

/* ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vpMatches12) (src/ORBmatcher.cc:823-963; LoopClosing.cc:624): as above between two
 * keyframes — a keypoint of pKF2 is a candidate only if it holds a good MapPoint and has not been matched (:879-888), the threshold is strict
 * (bestDist1 < TH_LOW, :908), and the result is indexed by pKF1's keypoints:
 *   d_kf1_mp_flags / d_kf2_mp_flags[p*capacity + i] : bit 0 = keypoint i of keyframe 1 / 2 holds a MapPoint that is not bad
 *   d_matches12[p*capacity + i]                     : out, the keypoint of pKF2 whose MapPoint vpMatches12[i] names, -1 = NULL */
int orbx_search_by_bow_keyframes_device(orbx_handle* h, int n_pairs, int kf1_first, int kf1_step, int kf2_first, int kf2_step,
                                        const uint32_t* d_feat_nodes, const uint32_t* d_feat_idx, const int* d_n_feat,
                                        const uint8_t* d_kf1_mp_flags, const uint8_t* d_kf2_mp_flags, const orbx_keypoint* d_kps,
                                        const uint8_t* d_desc, const int* d_n_out, int capacity, float nn_ratio, int th_low,
                                        int check_orientation, int* d_matches12, int* d_n_matches);

/* ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vpMapPointMatches) for TWO-CAMERA frames (src/ORBmatcher.cc:269-471 with F.Nleft != -1:
 * the else branch :340-367 and :373-433; the function reads descriptors, the two FeatureVectors, keypoint angles and F.Nleft, and the
 * camera pair only as null tests).  Search p matches keyframe pair K = kf_first + p*kf_step against frame pair C = cur_first + p*cur_step;
 * a pair X is batch frame 2X (left eye: mvKeys, the first Nleft rows of mDescriptors) and 2X + 1 (right eye: mvKeysRight, the other rows),
 * Nleft = d_n_out[2X], Nright = d_n_out[2X + 1].  kf_step = 0 (one keyframe, many frames) and cur_step = 0 (relocalisation) are allowed.
 *   d_feat_nodes, d_feat_idx, d_n_feat : what orbx_compute_bow_device wrote PER EYE (frames 2X and 2X + 1), same capacity.  The mFeatVec of
 *                 the stacked descriptors is not needed: a node's list there is the left eye's list followed by the right eye's (+ Nleft),
 *                 and the entry walks them so.  (The pair's mBowVec, which orbx_detect_candidates_device reads and this matcher does not, is what
 *                 orbx_compute_bow_device gives for the two descriptor blocks packed back to back as one frame.)
 *   d_kf_mp_flags[(2p + eye)*capacity + i] : bit 0 = keypoint i of that eye of the KEYFRAME holds a MapPoint that is not bad (:301-307)
 *   d_kps[f*capacity + i] : the extraction's RAW keypoints of all frames; only .angle is read, of the eye the index falls in (:382-391,
 *                 :408-417).  A one-camera keyframe is the case d_n_out[2K + 1] == 0 (mvKeysUn keeps the angle).
 *   d_desc, d_n_out : descriptors and counts of all frames
 *   nn_ratio = mfNNratio;  th_low = ORBmatcher::TH_LOW (50), a value above 255 is taken as 255;  check_orientation = mbCheckOrientation
 *   d_matches[(2p + eye)*capacity + i] : out, for keypoint i of that eye of the FRAME the keyframe feature whose MapPoint it received, in
 *                 the index space of pKF->GetMapPointMatches() (i_kf for a left feature, Nleft of the keyframe + j_kf for a right one),
 *                 -1 = none; all capacity entries of both eyes are written
 *   d_n_matches[p] : out, the return value (= the number of entries >= 0)
 * As the reference: per keyframe feature the frame's open left and right candidates of the node are ranked separately; nothing happens
 * unless the LEFT best is within th_low; then the left keypoint is written if it passes the ratio test and, whether or not it did, the
 * right best if it is within th_low (its ratio test is disabled, :403).  One keyframe feature can so hand its MapPoint to two keypoints,
 * and a node without an open left candidate never matches a right one.  The rotation histogram takes the pushes of both eyes.
 * A FeatureVector index >= d_n_out of its eye names no feature: a keyframe entry with one is skipped before it searches or votes in the
 * rotation histogram, a candidate with one is dropped.
 * Supported: the tables of a search live in LDS,
 *   40 * ((capacity + 15) & ~15) + 64 <= 163 328 bytes      (capacity <= 4080; orbx_max_keypoints() = 1302 of a 1200-feature extractor is inside)
 * a larger call returns ORBX_ERR_UNSUPPORTED before anything is launched.  While 104 * ((capacity + 15) & ~15) + 64 <= 163 328
 * (capacity <= 1568) the frame pair's descriptors are staged in LDS as well ("Two-eye BoW search": measured times); above, they
 * are read from L2.  Asynchronous on the handle's stream. */
int orbx_search_by_bow_two_eyes_device(orbx_handle* h, int n_pairs, int kf_first, int kf_step, int cur_first, int cur_step,
                                       const uint32_t* d_feat_nodes, const uint32_t* d_feat_idx, const int* d_n_feat,
                                       const uint8_t* d_kf_mp_flags, const orbx_keypoint* d_kps, const uint8_t* d_desc, const int* d_n_out,
                                       int capacity, float nn_ratio, int th_low, int check_orientation, int* d_matches, int* d_n_matches);

/* ---- the mapping thread's matcher: ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, bCoarse) -----------
 * (src/ORBmatcher.cc:965-1206; LocalMapping::CreateNewMapPoints, src/LocalMapping.cc:456-463, once per neighbour keyframe; src/Tracking.cc:3702-3706)
 * for keyframes with NLeft == -1 and no mpCamera2 on either side (monocular, rectified stereo, RGB-D) and the Pinhole model
 * (Pinhole::epipolarConstrain, src/CameraModels/Pinhole.cpp:122-144).  The two-camera branches (:994-1004, :1099-1129;
 * KannalaBrandt8) are orbx_search_for_triangulation_two_eyes_device below.  NOT covered: the second overload (:1208-1397,
 * matchAndtriangulate), which nothing in the reference calls.
 * Pair p matches keyframe 1 = frame kf1_first + p*kf1_step against keyframe 2 = frame kf2_first + p*kf2_step of one device-resident batch;
 * kf1_step = 0 is LocalMapping's shape (one new keyframe against its neighbours), kf2_step = 0 is allowed as well.
 *   d_feat_nodes, d_feat_idx, d_n_feat : mFeatVec of all frames as written by orbx_compute_bow_device (same capacity)
 *   d_kf1_mp_flags / d_kf2_mp_flags[p*capacity + i] : bit 0 = GetMapPoint(i) of keyframe 1 / 2 of pair p is not NULL (:1033-1039, :1064-1068:
 *                 the pointer test alone, there is no isBad() here, unlike the SearchByBoW flags)
 *   d_kps_un[f*capacity + i]  : mvKeysUn of all frames (orbx_frame_finish_device); .pt, .octave and .angle are read
 *   d_u_right[f*capacity + i] : mvuRight of all frames (orbx_stereo_match_device / orbx_stereo_from_rgbd_device), >= 0 = stereo; NULL = no
 *                 feature is stereo (monocular)
 *   d_desc, d_n_out           : mDescriptors, N of all frames
 *   d_f12[p*9]                : F12 of pair p, row-major binary32, = K1^-T [t12]x R12 K2^-1 as Pinhole.cpp:124-127 builds it (the reference
 *                 ignores the F12 argument it is handed and rebuilds the matrix per candidate; its cv::Mat rounding is the caller's)
 *   d_epipole[p*2]            : ep of pair p (:972-977: keyframe 1's camera centre projected into keyframe 2)
 *   only_stereo = bOnlyStereo, coarse = bCoarse, th_low = ORBmatcher::TH_LOW (50), check_orientation = mbCheckOrientation
 *   d_matches12[p*capacity + i] : out, vMatches12: the keypoint of keyframe 2 chosen for keypoint i of keyframe 1, -1 = none; all capacity
 *                 entries are written
 *   d_pairs[(p*capacity + k)*2 + {0, 1}] : out, vMatchedPairs: entry k < d_n_matches[p] is (i, d_matches12[i]) in increasing i; entries from
 *                 d_n_matches[p] on are left as they were
 *   d_n_matches[p]            : out, the return value
 * As the reference: inside a node both FeatureVectors hold, every keyframe-1 feature without a MapPoint (and, under only_stereo, with
 * mvuRight >= 0) scans keyframe 2's features of the node in list order; a candidate is dropped if it holds a MapPoint, by the stereo filter,
 * if dist > th_low, if neither feature is stereo and it lies in the epipole's disc (distex^2 + distey^2 < 100 * mvScaleFactors[octave],
 * :1089-1097), and if it fails dsqr < 3.84 * mvLevelSigma2[octave] (binary32 up to dsqr, every operation rounded on its own, the compare
 * in double) unless coarse.  vbMatched2 is tested (:1067) but never set in this function, so a keyframe-1 feature never closes a candidate for
 * another: SEVERAL keyframe-1 features may choose the same keyframe-2 keypoint.  bestDist starts AT th_low and an equal distance replaces
 * the holder (:1057, :1080): of the passing candidates the smallest distance wins and of equal smallest distances the LAST in list order
 * (the opposite of SearchByBoW).  Rotation histogram and ComputeThreeMaxima as there (:1147-1157, :1174-1193).
 * The scale tables are the handle's (orbx_get_tables).  An octave outside [0, nlevels) is CLAMPED into the tables (the reference would
 * index past them).  d_n_feat[f] and d_n_out[f] are clamped into [0, capacity].  A FeatureVector index >= d_n_out of its frame (a stale
 * count beside an older FeatureVector; orbx_compute_bow_device writes none) names no feature: a keyframe-1 entry with one is skipped
 * before it searches or votes in the rotation histogram, a keyframe-2 candidate with one is dropped, and both launch forms answer alike.
 * Supported: the tables of a pair live in LDS,
 *   28 * ((capacity + 15) & ~15) + 64 <= 163 328 bytes      (capacity <= 5824)
 * a larger call returns ORBX_ERR_UNSUPPORTED before anything is launched.  While 60 * ((capacity + 15) & ~15) + 64 <= 163 328
 * (capacity <= 2720; orbx_max_keypoints() of a 2000-feature extractor is inside) keyframe 2's descriptors are staged in LDS as well; above,
 * they are read from L2.  Asynchronous on the handle's stream. */
int orbx_search_for_triangulation_device(orbx_handle* h, int n_pairs, int kf1_first, int kf1_step, int kf2_first, int kf2_step,
                                         const uint32_t* d_feat_nodes, const uint32_t* d_feat_idx, const int* d_n_feat,
                                         const uint8_t* d_kf1_mp_flags, const uint8_t* d_kf2_mp_flags, const orbx_keypoint* d_kps_un,
                                         const float* d_u_right, const uint8_t* d_desc, const int* d_n_out, int capacity, const float* d_f12,
                                         const float* d_epipole, int only_stereo, int coarse, int th_low, int check_orientation,
                                         int* d_matches12, int* d_pairs, int* d_n_matches);

/* ---- the mapping thread's second matcher: the search half of ORBmatcher::Fuse (LocalMapping::SearchInNeighbors, src/LocalMapping.cc:729-837) ----
 * MapPoint::PredictScale(currentDist, pKF) (src/MapPoint.cc:514-529) on the host, through the host libm:
 *   ratio = max_distance / dist;  ceil(log(ratio) / mfLogScaleFactor) clamped to [0, nlevels - 1]
 * with log, / and ceil in binary32 (`using namespace std` is in scope there) and mfLogScaleFactor = log(scale_factor) in binary32
 * (src/Frame.cc:99).  Where the reference is undefined (the int conversion of +inf / NaN): a ratio of +inf gives nlevels - 1, NaN (and a negative
 * ratio) gives 0; a ratio of 0 gives 0.  Returns the level, or ORBX_ERR_BAD_ARGUMENT (nlevels < 1, scale_factor not a finite number above 1). */
int orbx_predict_scale(float max_distance, float dist, float scale_factor, int nlevels);
/* The same as a table: as a function of ratio the expression is a monotone step function with nlevels - 1 steps;
 *   breakpoints[k - 1] (k = 1 .. nlevels - 1) = the smallest positive float r with ceil(logf(r) / logf(scale_factor)) >= k,
 * found by bisection over float bit patterns with the expression itself (the steps sit a few ulp above scale_factor^k - 1.20000017,
 * 1.44000018 for 1.2 - a table of powers would be wrong).  The predicted level of `ratio` is the number of breakpoints <= ratio (+inf: all,
 * NaN: none).  Host-only, no GPU touched.  breakpoints may be NULL when nlevels == 1. */
int orbx_predict_scale_breakpoints(float scale_factor, int nlevels, float* breakpoints /* nlevels - 1 */);

/* Where a MapPoint left Fuse (d_exit of orbx_fuse_device): the reference's own count_* names at src/ORBmatcher.cc:1430 */
enum orbx_fuse_exit {
    ORBX_FUSE_FLAG = 0,           /* count_notMP / count_bad / count_isinKF: bit 0 of its flag is clear (or it lies beyond d_n_mp) */
    ORBX_FUSE_NEG_DEPTH = 1,      /* count_negdepth (:1459) */
    ORBX_FUSE_NOT_IN_IMAGE = 2,   /* count_notinim (:1473) */
    ORBX_FUSE_DISTANCE = 3,       /* count_dist (:1487) */
    ORBX_FUSE_NORMAL = 4,         /* count_normal (:1496) */
    ORBX_FUSE_EMPTY_WINDOW = 5,   /* count_notidx (:1509): GetFeaturesInArea returned nothing */
    ORBX_FUSE_ABOVE_TH_LOW = 6,   /* count_thcheck (:1594): no candidate passed, or the best distance is above th_low */
    ORBX_FUSE_FUSED = 7           /* nFused++ (:1591) */
};

/* ORBmatcher::Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, th, bRight = false) (src/ORBmatcher.cc:1399-1609; reproj_check = 1) and
 * the loop-closing overload Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) (:1611-1733; reproj_check = 0: the same search without the
 * reprojection test of :1533-1557), for keyframes with NLeft == -1 and the Pinhole model (monocular, rectified stereo, RGB-D).  NOT covered:
 * bRight = true and NLeft != -1 (:1404-1410, :1524-1526, :1559: mpCamera2, the KannalaBrandt8 pair) - those keyframes go through
 * orbx_fuse_two_eyes_device below.
 * THE SEARCH HALF ONLY.  Everything up to bestIdx / bestDist (:1455-1570, :1643-1712) reads the MapPoint's position, normal, distance bounds and
 * descriptor and the keyframe's pose, keypoints, grid, mvuRight and descriptors; only the tail (:1573-1592, :1715-1729: Replace /
 * AddObservation / AddMapPoint) touches the map, and it closes no keypoint for later MapPoints.  So all MapPoints of all keyframes are searched
 * in one launch, and the CALLER replays the tail on the host, keyframe by keyframe and in list order, re-testing isBad() and IsInKeyFrame(pKF)
 * at replay time (an earlier Replace may have changed them): INTEGRATION.md, "SearchInNeighbors".
 * WHERE THAT IS EXACT.  A call with ONE keyframe (n_pairs = 1: SearchInNeighbors' second half, LoopClosing's Fuse) plus the replay is the
 * reference's Fuse: the MapPoint that survives a Replace is in pKF afterwards and is not searched there again.  A call with SEVERAL keyframes
 * and one list (mp_step = 0) is exact for every list entry whose descriptor is still the uploaded one when the replay reaches the keyframe:
 * MapPoint::Replace ends with ComputeDistinctiveDescriptors() on the survivor (src/MapPoint.cc:296-298, :330-403), which may rewrite
 * mDescriptor, and the reference searches that entry in the LATER keyframes with the new descriptor (GetDescriptor(), :1517).  Position, normal
 * and distances are not touched by Replace.  So before replaying keyframe p the caller compares GetDescriptor() of the list entries that
 * survived a Replace in keyframes 0 .. p-1 with what it uploaded, and searches the changed ones again in keyframe p (one more call with
 * n_pairs = 1 and bit 0 set for them alone); with that the sequence is the reference's.  INTEGRATION.md shows the loop, and
 * tests/test_fuse.py holds it against the sequential Fuse on a map model with descriptors.
 * Pair p fuses MapPoint list mp_first + p*mp_step into keyframe kf_first + p*kf_step of one device-resident batch: mp_step = 0 is
 * SearchInNeighbors' first half (the current keyframe's MapPoints into every neighbour), n_pairs = 1 with a long list its second half;
 * kf_step = 0 is allowed as well.
 *   per MapPoint, in blocks of mp_capacity per list (m = list*mp_capacity + i):
 *   d_mp_world[m*3], d_mp_normal[m*3] : GetWorldPos(), GetNormal()
 *   d_mp_dist[m*3]             : GetMinDistanceInvariance(), GetMaxDistanceInvariance() (0.8f * mfMinDistance, 1.2f * mfMaxDistance: the bounds of
 *                 :1487) and mfMaxDistance ITSELF, which PredictScale divides (src/MapPoint.cc:519; dividing the second by 1.2f is not bit-exact)
 *   d_mp_desc[m*32]            : GetDescriptor() (16-byte aligned, as d_desc)
 *   d_n_mp[list]               : MapPoints of the list, NULL = mp_capacity
 *   d_mp_flags[p*mp_capacity + i] : per PAIR; bit 0 = pMP && !pMP->isBad() && !pMP->IsInKeyFrame(pKF) (:1435-1452); for reproj_check = 0
 *                 bit 0 = !pMP->isBad() && !spAlreadyFound.count(pMP) (:1639)
 *   d_poses[f*12]              : rows 0..2 of the keyframe's Tcw (3x4, row-major: Rcw | tcw) of every frame, as orbx_project_last_frame_device
 *                 takes them; for reproj_check = 0 the caller's sRcw/scw | tcw/scw (:1620-1623).  Ow = -Rcw.t()*tcw is computed here.
 *   d_kps_un, d_desc, d_n_out, d_grid_off, d_grid_idx : mvKeysUn, mDescriptors, N, mGrid of all frames (orbx_frame_finish_device)
 *   bounds4                    : Frame's FLOAT mnMinX, mnMaxX, mnMinY, mnMaxY (orbx_compute_image_bounds), the ones the grid was built with.  KeyFrame's
 *                 own mnMinX .. mnMaxY are const int (inc/KeyFrame.h:484) initialised from them (src/KeyFrame.cc:58), so truncated toward zero,
 *                 while its mfGridElementWidthInv / HeightInv are copies of Frame's, made from the floats (:50).  The entry does the same:
 *                 IsInImage and the window subtract (float)(int)bounds4[i], the window scales by 64 / (bounds4[1] - bounds4[0]) and
 *                 48 / (bounds4[3] - bounds4[2]).  With a distorted camera the bounds are no integers and the two differ near the edge.
 *   d_u_right[f*capacity + i]  : mvuRight of all frames, NULL = monocular (all -1)
 *   cam (fx, fy, cx, cy), mbf  : Pinhole::project, pKF->mbf;  th : 3.0 at both callers;  th_low : ORBmatcher::TH_LOW (50), above 255 taken as 255
 *   nlevels                    : pKF->mnScaleLevels; must equal orbx_get_levels(h) - mvScaleFactors, mvInvLevelSigma2 and PredictScale's
 *                 breakpoints are the handle's (orbx_get_tables, orbx_predict_scale_breakpoints); else ORBX_ERR_BAD_ARGUMENT
 *   d_best_idx[p*mp_capacity + i]  : out, bestIdx, the keyframe's keypoint, if bestDist <= th_low; else -1
 *   d_best_dist[p*mp_capacity + i] : out, bestDist; 256 where no candidate passed (in both modes; :1693 starts at INT_MAX)
 *   d_exit[p*mp_capacity + i]      : out or NULL, an orbx_fuse_exit
 *   d_n_fused[p]                   : out, the return value under the flags as passed (the number of ORBX_FUSE_FUSED)
 * All mp_capacity entries of every pair are written.  Arithmetic as the reference's x86-64 build, every operation rounded on its own:
 * p3Dc and Ow as cv::gemm (products and sums in double, one rounding to float), z < 0.0f rejected (z == 0 leaves by IsInImage), invz a FLOAT
 * division (:1465), IsInImage with strict upper bounds on the truncated bounds (src/KeyFrame.cc:816-819), dist3D = (float)sqrt of squares summed in double, PO.dot(Pn) in
 * double against 0.5 * (double)dist3D, KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:770-814: NOT Frame's - no level filter, four early
 * returns, fabs(dx) < r && fabs(dy) < r, ix outer / iy inner / push order = the CSR order of d_grid_idx), kpLevel in [level - 1, level],
 * (float)(e2 * invSigma2) promoted and compared with 7.8 (mvuRight >= 0) / 5.99, DescriptorDistance with strict <: of equal distances the
 * FIRST in visit order wins.  A keypoint octave of -1 that passes the level filter (level 0) is CLAMPED into the table (the reference would
 * index past it).  No table lives in LDS: there is no capacity bound and no ORBX_ERR_UNSUPPORTED case.  Asynchronous on the handle's stream. */
int orbx_fuse_device(orbx_handle* h, int n_pairs, int kf_first, int kf_step, int mp_first, int mp_step, const float* d_mp_world,
                     const float* d_mp_normal, const float* d_mp_dist, const uint8_t* d_mp_desc, const int* d_n_mp, int mp_capacity,
                     const uint8_t* d_mp_flags, const float* d_poses, const orbx_keypoint* d_kps_un, const float* d_u_right,
                     const uint8_t* d_desc, const int* d_n_out, int capacity, const int* d_grid_off, const int* d_grid_idx,
                     const float* bounds4, const orbx_camera* cam, int nlevels, float mbf, float th, int th_low, int reproj_check,
                     int* d_best_idx, int* d_best_dist, uint8_t* d_exit, int* d_n_fused);

/* ORBmatcher::Fuse for TWO-CAMERA keyframes (NLeft != -1, a KannalaBrandt8 pair): Fuse(pKF, vpMapPoints, th, bRight = false) and
 * Fuse(pKF, vpMapPoints, th, bRight = true) (src/ORBmatcher.cc:1399-1609 with :1404-1410, :1524-1528, :1559), as
 * LocalMapping::SearchInNeighbors calls them one after the other (src/LocalMapping.cc:787-788, :816-817), and the loop-closing overload
 * (:1611-1733; reproj_check = 0) on such a keyframe.  THE SEARCH HALF ONLY, under orbx_fuse_device's contract: the caller replays the tails on
 * the host and searches the changed survivors again (above; INTEGRATION.md, "SearchInNeighbors", the two-camera loop).  What differs:
 * FRAMES.  Rig keyframe r is device frames 2r (left eye: mvKeys, mGrid, the left rows of mDescriptors) and 2r + 1 (right eye: mvKeysRight,
 * mGridRight, the right rows), the layout of orbx_frame_finish_two_eyes_device.  Pair p fuses list mp_first + p*mp_step into RIG
 * kf_first + p*kf_step.  d_kps holds the RAW keypoints of both eyes: the reference reads mvKeys / mvKeysRight for position and octave
 * (:1524-1528, src/KeyFrame.cc:801-803), not mvKeysUn.  d_poses[r*12] is one pose per rig, as orbx_frustum_requests_two_eyes_device takes it.
 * POSES.  Left eye: Rcw | tcw of the pose, Ow = -Rcw.t()*tcw.  Right eye: KeyFrame's getters (src/KeyFrame.cc:1232-1262), which derive
 * everything from mTlr ALONE (tlr12, 3x4 row-major; Frame's mTrl has no part here): Rrl = mTlr.R.t(); Rrw = Rrl*Rlw, a 3x3 product;
 * trl = -Rrl*mTlr.t, one gemm with alpha = -1; trw = Rrl*tlw + trl, one gemm with the addend; twr = Rwl*mTlr.t + Ow, one gemm with the float Ow
 * as addend.  cv::Mat products as everywhere here (products and sums in double, one rounding to float): parity unpinned, as Fuse's.
 * CAMERAS.  uv = KannalaBrandt8::project with THAT EYE's camera (cam_left = mpCamera, cam_right = mpCamera2; :1409, :1416), libm's atan2f,
 * sqrtf, sinf, cosf restated for the device (orbx_kb8_project_device).  z < 0.0f leaves (:1459); z == 0 does NOT leave by itself as it does
 * under the pinhole model: atan2f(r, 0) is pi / 2, the projection is finite and the MapPoint goes on (z = -0.0f as well).
 * FLAGS.  d_mp_flags[p*mp_capacity + i] is per pair, bit 0 as orbx_fuse_device, and serves BOTH eyes.  The reference's right call sees
 * IsInKeyFrame after the left call's tail; that re-test belongs to the replay, as it does across keyframes.
 * eyes: bit 0 = the left search, bit 1 = the right; 1, 2 or 3, anything else is ORBX_ERR_BAD_ARGUMENT.  reproj_check = 0 (the loop-closing
 * overload) has no right-eye form and requires eyes == 1.  A call with eyes = 2 is the re-search between the eyes of one keyframe.
 * THE REPROJECTION TEST is always the monocular one, (float)(e2 * invSigma2) promoted against 5.99: mvuRight of a two-camera keyframe has
 * Nleft entries, all -1 (src/Frame.cc:1150), so ur, invz and mbf have no observable effect and are no arguments.  The reference indexes
 * mvuRight with the right eye's OWN index (:1533, before :1559), out of bounds where Nright > Nleft: the entry takes -1 there.
 *   d_mp_world .. d_mp_desc, d_n_mp (clamped to 0 .. mp_capacity, NULL = mp_capacity), the d_mp_dist triples, nlevels, th, th_low : as orbx_fuse_device
 *   d_kps, d_desc, d_n_out, d_grid_off, d_grid_idx : of all device frames; bounds4 : Frame's FLOAT bounds, the same for both eyes, truncated for
 *                 IsInImage and the window's subtraction, untruncated for the grid inverses, as orbx_fuse_device
 *   d_best_idx[(p*2 + eye)*mp_capacity + i]  : out, bestIdx in the KEYFRAME's numbering (:1559) if bestDist <= th_low, else -1: a left keypoint i is
 *                 i, a right keypoint i is NLeft + i with NLeft = d_n_out[2r] clamped to 0 .. capacity; GetMapPoint(bestIdx) and
 *                 AddObservation(pKF, bestIdx) take it as it is.  The descriptor of right keypoint i is row i of device frame 2r + 1.
 *   d_best_dist[(p*2 + eye)*mp_capacity + i] : out, bestDist; 256 where no candidate passed (in both modes)
 *   d_exit[(p*2 + eye)*mp_capacity + i]      : out or NULL, an orbx_fuse_exit (the same eight codes)
 *   d_n_fused[p*2 + eye]                     : out, the number of ORBX_FUSE_FUSED of that eye under the flags as passed
 * All mp_capacity entries of every eye asked for are written; the entries of an eye not asked for are left untouched.  After (u, v) the
 * arithmetic is orbx_fuse_device's, line by line: IsInImage, the distance and normal tests, PredictScale by breakpoints, radius =
 * th * mvScaleFactors[level], KeyFrame::GetFeaturesInArea(u, v, r, bRight) on that eye's grid and raw keypoints (four early returns, ix outer /
 * iy inner / CSR order), kpLevel in [level - 1, level] from the raw octave (-1 CLAMPED into the table), strict <: the FIRST of equal
 * distances in visit order stays; fused when bestDist <= th_low.  No table lives in LDS: no capacity bound and no ORBX_ERR_UNSUPPORTED case.
 * ORBX_ERR_BAD_ARGUMENT is returned before any launch.  Asynchronous on the handle's stream. */
int orbx_fuse_two_eyes_device(orbx_handle* h, int n_pairs, int kf_first, int kf_step, int mp_first, int mp_step, const float* d_mp_world,
                              const float* d_mp_normal, const float* d_mp_dist, const uint8_t* d_mp_desc, const int* d_n_mp, int mp_capacity,
                              const uint8_t* d_mp_flags, const float* d_poses, const float* tlr12, const orbx_camera_kb8* cam_left,
                              const orbx_camera_kb8* cam_right, const orbx_keypoint* d_kps, const uint8_t* d_desc, const int* d_n_out,
                              int capacity, const int* d_grid_off, const int* d_grid_idx, const float* bounds4, int nlevels, float th,
                              int th_low, int reproj_check, int eyes, int* d_best_idx, int* d_best_dist, uint8_t* d_exit, int* d_n_fused);

/* ---- ORBmatcher::SearchForTriangulation for TWO-CAMERA keyframes (src/ORBmatcher.cc:965-1206 with mpCamera2 on both sides: the branches
 * :994-1004 and :1099-1129; a KannalaBrandt8 pair; LocalMapping::CreateNewMapPoints, src/LocalMapping.cc:456-463) and the camera math it
 * stands on, as entries of their own ------------------------------------------------------------------------------------------------------
 * KannalaBrandt8::unproject(const cv::Point2f&) (src/CameraModels/KannalaBrandt8.cpp:103-130) over n device-resident pixels:
 *   d_uv[i*2 + {0,1}] in, d_rays[i*3 + {0,1,2}] out (x, y, 1).
 * Every operation is rounded in binary32 in the reference's order: the clamp of theta_d against (float)(CV_PI / 2), the compare with 1e-8 in
 * double, ten Newton steps with the early exit at `const float precision` = 1e-6, std::tan as glibc 2.35's binary32 tanf.  Asynchronous on
 * the handle's stream. */
int orbx_kb8_unproject_device(orbx_handle* h, int n, const float* d_uv, const orbx_camera_kb8* cam, float* d_rays);

/* KannalaBrandt8::TriangulateMatches(pCamera2, kp1, kp2, R12, t12, sigmaLevel, unc, p3D) (src/CameraModels/KannalaBrandt8.cpp:336-405, with
 * Triangulate, :424-437) over n device-resident keypoint pairs under ONE relative pose:
 *   d_kp1 / d_kp2[i*2 + {0,1}] : kp1.pt under cam1 (this), kp2.pt under cam2 (pCamera2)
 *   r12_9, t12_3               : R12 (row-major) and t12, host pointers;  sigma1 = sigmaLevel, sigma2 = unc
 *   d_z[i]                     : out, the return value: z1, or -1 (parallax above 0.9998, z1 <= 0, z2 <= 0, a reprojection error above
 *                                5.991 * sigma); epipolarConstrain (:237-240) is d_z[i] > 0.0001f
 *   d_x3d[i*3 + {0,1,2}]       : out, x3D in camera 1 (zeros when the parallax test left; the reference leaves p3D untouched on every -1)
 * vt.row(3) of cv::SVD::compute is the library's own one-sided Jacobi in binary32 (cv::SVD is OpenCV's Jacobi or
 * LAPACK's sgesdd by its build, parity unpinned), the cv::Mat / cv::MatExpr roundings are listed there.  A zero fourth component flows
 * through as infinity or NaN, on which every test is false; NaN > 0.0001f rejects.  Asynchronous on the handle's stream. */
int orbx_kb8_triangulate_device(orbx_handle* h, int n, const float* d_kp1, const float* d_kp2, const orbx_camera_kb8* cam1,
                                const orbx_camera_kb8* cam2, const float* r12_9, const float* t12_3, float sigma1, float sigma2, float* d_z,
                                float* d_x3d);

/* The search.  Pair p matches rig keyframe K1 = kf1_first + p*kf1_step against K2 = kf2_first + p*kf2_step; a rig keyframe X is batch frames
 * 2X (left eye: mvKeys, the first NLeft rows of mDescriptors) and 2X + 1 (right eye: mvKeysRight), NLeft = d_n_out[2X], as in
 * orbx_search_by_bow_two_eyes_device.  kf1_step = 0 is LocalMapping's shape.
 *   d_feat_nodes, d_feat_idx, d_n_feat : what orbx_compute_bow_device wrote PER EYE (same capacity); a node's list of the stacked mFeatVec
 *                 is the left eye's list followed by the right eye's (+ NLeft), and the entry walks them so
 *   d_kf1_mp_flags / d_kf2_mp_flags[(2p + eye)*capacity + i] : bit 0 = GetMapPoint of that keypoint of keyframe 1 / 2 of pair p is not NULL
 *   d_poses[X*12] : Tcw of rig keyframe X (3x4 row-major);  tlr12 : mTlr (3x4, host);  cam_left / cam_right : mpCamera / mpCamera2 (host),
 *                 as orbx_fuse_two_eyes_device takes them: the eyes' rotations and translations are KeyFrame's getters
 *                 (src/KeyFrame.cc:1232-1262), the four (R12, t12) are :995-1003 as cv::gemm rows
 *   d_kps[f*capacity + i] : the RAW keypoints of all frames (:1048-1050, :1083-1085: mvKeys / mvKeysRight, not mvKeysUn); .pt, .octave,
 *                 .angle are read;  d_desc, d_n_out : descriptors and counts of all frames;  nlevels : the handle's
 *   only_stereo = bOnlyStereo: bStereo1 is false on such keyframes (:1041), so 1 returns no match;  coarse = bCoarse: accepts without the
 *                 geometric test (:1132);  th_low = TH_LOW (50);  check_orientation = mbCheckOrientation
 *   d_matches12[(2p + eye)*capacity + i] : out, keyframe 2's keypoint chosen for keypoint i of that eye of keyframe 1 in the STACKED
 *                 numbering (a right keypoint j is NLeft + j), -1 = none; all capacity entries of both eyes are written
 *   d_pairs[(p*2*capacity + k)*2 + {0, 1}] : out, vMatchedPairs in stacked numbering, increasing; entries from d_n_matches[p] on are left
 *   d_n_matches[p] : out, the return value
 * As the reference: there is no stereo filter and no epipole disc on such keyframes (:1070, :1089), F12 and the epipole are not read; the
 * geometric test is pCamera1->epipolarConstrain(pCamera2, kp1, kp2, R12, t12, mvLevelSigma2[kp1.octave], mvLevelSigma2[kp2.octave]) with the
 * cameras and (R12, t12) of the candidate's eye combination; of the passing candidates within th_low the smallest distance wins and of
 * equal distances the LAST in list order; vbMatched2 is never set.  An octave outside [0, nlevels) is CLAMPED into the table.
 * A FeatureVector index >= d_n_out of its eye names no feature: a keyframe-1 entry with one is skipped before it searches or votes in the
 * rotation histogram, a keyframe-2 candidate with one is dropped.
 * Supported: the tables of a pair live in LDS, capacity counted over both eyes,
 *   62 * ((capacity + 15) & ~15) + 1024 <= 163 328 bytes      (capacity <= 2608 per eye; 2 x 1302 of a 1200-feature extractor are inside)
 * a larger call returns ORBX_ERR_UNSUPPORTED before anything is launched.  While 126 * ((capacity + 15) & ~15) + 1024 <= 163 328
 * (capacity <= 1280 per eye) keyframe 2's descriptors are staged in LDS as well; above, they are read from L2.  Asynchronous on the
 * handle's stream. */
int orbx_search_for_triangulation_two_eyes_device(orbx_handle* h, int n_pairs, int kf1_first, int kf1_step, int kf2_first, int kf2_step,
                                                  const uint32_t* d_feat_nodes, const uint32_t* d_feat_idx, const int* d_n_feat,
                                                  const uint8_t* d_kf1_mp_flags, const uint8_t* d_kf2_mp_flags, const float* d_poses,
                                                  const float* tlr12, const orbx_camera_kb8* cam_left, const orbx_camera_kb8* cam_right,
                                                  const orbx_keypoint* d_kps, const uint8_t* d_desc, const int* d_n_out, int capacity, int nlevels,
                                                  int only_stereo, int coarse, int th_low, int check_orientation, int* d_matches12, int* d_pairs,
                                                  int* d_n_matches);

/* ---- Frame::ComputeStereoFishEyeMatches (src/Frame.cc:1139-1179; the two-camera Frame constructor, :1108): the per-frame stereo matches of a
 * fisheye rig, the counterpart of orbx_stereo_match_device (rectified stereo) --------------------------------------------------------------
 * Rig r = rig_first + q*rig_step is batch frames 2r (left eye: mvKeys, mDescriptors) and 2r + 1 (right eye), as every two-eye entry numbers
 * them.
 *   d_kps, d_desc, d_n_out, d_mono_out : what orbx_extract_batch_device wrote: the RAW keypoints, descriptors, Nleft / Nright and monoLeft /
 *                 monoRight of every batch frame.  N is clamped into [0, capacity] and mono into [0, N] (the reference would index out of
 *                 bounds).  The lapping rows are [mono, N) of each eye.
 *   tlr12       : mTlr (3x4 row-major, host): R12 = mRlr is its rotation and t12 = mtlr its last column, handed to TriangulateMatches as
 *                 they are (:1169);  cam_left / cam_right : mpCamera / mpCamera2 (host);  nlevels : the handle's
 *   d_left_to_right[(2r)*capacity + i]      : out, mvLeftToRightMatch: the RAW right index (trainIdx + monoRight), -1 = none
 *   d_right_to_left[(2r + 1)*capacity + j]  : out, mvRightToLeftMatch: the raw left index, -1 = none
 *   d_depth[(2r)*capacity + i]              : out, mvDepth (-1 = none)
 *   d_x3d[((2r)*capacity + i)*3 + {0,1,2}]  : out, mvStereo3Dpoints[i] in the left camera.  The reference leaves an empty cv::Mat where
 *                 nothing matched: here that is zeros, VALID ONLY where d_left_to_right >= 0
 *   d_n_matches[q]      : out, nMatches;   d_n_desc_matches[q] : out or NULL, descMatches (the rows that passed the ratio test)
 * All capacity entries of the rows a rig owns are written on every call (-1, -1, -1.0f, zeros); the rows of the other eye in each array
 * (d_left_to_right of frame 2r + 1, d_right_to_left, d_depth and d_x3d of the other frame) are not touched.  The layout is what
 * orbx_search_by_projection_two_eyes_device reads.  mvuRight stays all -1 on this path (:1150): the caller's constant, not an output.
 * The definitions (OpenCV is not available to this project: parity unpinned, as the cv::SVD ones):
 *   * BFMatcher(NORM_HAMMING).knnMatch(left lapping rows, right lapping rows, 2) is OpenCV's batchDistance insertion over the right rows in
 *     increasing index: a candidate enters only if strictly smaller than the current second and moves in front only if strictly smaller
 *     than the first.  [0] is the FIRST index of the smallest distance, [1] the smallest remaining distance, which may equal [0]'s.  With
 *     fewer than two right lapping rows nothing matches (size() >= 2).
 *   * (*it)[0].distance < (*it)[1].distance * 0.7 (a float times a double, compared in double) equals 10*d0 < 7*d1 on every pair of
 *     distances 0 .. 256 (enumerated by tests/test_stereo_fisheye.py); equal distances never pass.
 *   * accepted when KannalaBrandt8::TriangulateMatches(mpCamera2, mvKeys[i], mvKeysRight[j], mRlr, mtlr, mvLevelSigma2[octave_i],
 *     mvLevelSigma2[octave_j]) > 0.0001f, as orbx_kb8_triangulate_device computes it on both RAW points; NaN and -1 reject, +inf accepts.
 *     An octave outside [0, nlevels) is CLAMPED into the table.
 *   * the reference walks the left rows in increasing index: mvRightToLeftMatch[j] ends as the LARGEST accepted left row that chose j,
 *     while each of them keeps its own mvLeftToRightMatch = j.  The two arrays are NOT inverse.
 * No table depends on the capacity: there is no ORBX_ERR_UNSUPPORTED case.  ORBX_ERR_BAD_ARGUMENT is returned before any launch.
 * Asynchronous on the handle's stream; no CPU path. */
int orbx_stereo_fisheye_match_device(orbx_handle* h, int n_rigs, int rig_first, int rig_step, const orbx_keypoint* d_kps, const uint8_t* d_desc,
                                     const int* d_n_out, const int* d_mono_out, int capacity, const float* tlr12, const orbx_camera_kb8* cam_left,
                                     const orbx_camera_kb8* cam_right, int nlevels, int* d_left_to_right, int* d_right_to_left, float* d_depth,
                                     float* d_x3d, int* d_n_matches, int* d_n_desc_matches);

/* ---- the mapping thread's triangulation: the loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:481-707) --------------------------
 * Between orbx_search_for_triangulation_device / orbx_search_for_triangulation_two_eyes_device, which write vMatchedIndices (d_pairs,
 * d_n_matches), and orbx_fuse_device / orbx_fuse_two_eyes_device, which read MapPoint positions: every matched pair becomes a world point
 * or is rejected, from reading vMatchedIndices[ikp] (:483) to the last `continue` of the scale-consistency test (:707).  The map-changing
 * tail (:709-723: new MapPoint, AddObservation, ComputeDistinctiveDescriptors, UpdateNormalAndDepth) stays with the caller, as for Fuse, and
 * so does the per-neighbour prelude (:436-456: baseline, median depth, ComputeF12): the caller passes only the pairs it wants.
 * How a match left the loop (d_exit): three accepting codes name the branch that made the point, every `continue` has its own. */
enum orbx_new_point_exit {
    ORBX_NEW_POINT_TRIANGULATED = 0,     /* accepted; the linear triangulation (:593-611) */
    ORBX_NEW_POINT_STEREO_1 = 1,         /* accepted; mpCurrentKeyFrame->UnprojectStereo(idx1) (:614) */
    ORBX_NEW_POINT_STEREO_2 = 2,         /* accepted; pKF2->UnprojectStereo(idx2) (:618) */
    ORBX_NEW_POINT_ZERO_W = 3,           /* x3D.at<float>(3) == 0 (:605) */
    ORBX_NEW_POINT_LOW_PARALLAX = 4,     /* no stereo and very low parallax (:622); a NaN pose ends here */
    ORBX_NEW_POINT_EMPTY_STEREO = 5,     /* x3Dt.empty() (:627): UnprojectStereo with mvDepth <= 0 */
    ORBX_NEW_POINT_BEHIND_1 = 6,         /* z1 <= 0 (:630) */
    ORBX_NEW_POINT_BEHIND_2 = 7,         /* z2 <= 0 (:634) */
    ORBX_NEW_POINT_REPROJ_1 = 8,         /* the reprojection error in the first keyframe (:649 / :661) */
    ORBX_NEW_POINT_REPROJ_2 = 9,         /* ... in the second (:675 / :686) */
    ORBX_NEW_POINT_ZERO_DIST = 10,       /* dist1 == 0 || dist2 == 0 (:697) */
    ORBX_NEW_POINT_FAR = 11,             /* mbFarPoints && a distance >= mThFarPoints (:700) */
    ORBX_NEW_POINT_SCALE = 12,           /* the scale-consistency test (:706) */
    ORBX_NEW_POINT_BAD_INDEX = 13        /* an index outside its keyframe's [0, N): nothing is read (the reference would index out of bounds) */
};

/* One-camera keyframes (NLeft == -1, no mpCamera2; monocular, rectified stereo, RGB-D) with the Pinhole model.  Pair p triangulates the
 * matches of keyframe 1 = frame kf1_first + p*kf1_step and keyframe 2 = frame kf2_first + p*kf2_step, numbered as
 * orbx_search_for_triangulation_device numbers them; kf1_step = 0 is LocalMapping's shape.
 *   d_pairs[(p*capacity + k)*2 + {0, 1}], d_n_matches[p] : exactly what the search wrote; d_n_matches[p] is clamped into [0, capacity]
 *   d_poses[f*12]   : Tcw of batch frame f, 3x4 row-major.  Rwc = Rcw.t(), Ow = -Rwc*tcw and Twc = [Rwc | Ow] are derived on the device
 *                     (src/KeyFrame.cc:111-125) as cv::gemm rows
 *   cam             : fx, fy, cx, cy (host); Pinhole::unproject / project are src/CameraModels/Pinhole.cpp:59-62, :30-33.  The distortion
 *                     fields are not read: mvKeysUn are undistorted
 *   d_kps_un[f*capacity + i] : mvKeysUn of all frames; .pt and .octave are read
 *   d_kps[f*capacity + i]    : the RAW mvKeys; read only by UnprojectStereo (src/KeyFrame.cc:821-834, which uses mvKeys, not mvKeysUn)
 *   d_u_right, d_depth [f*capacity + i] : mvuRight, mvDepth as orbx_stereo_match_device / orbx_stereo_from_rgbd_device write them.  NULL
 *                     d_u_right = monocular: no feature is stereo, and d_kps / d_depth may be NULL then (and only then)
 *   d_n_out[f]      : N of all frames, clamped into [0, capacity]
 *   mb, mbf         : the reference reads pKF2->mb for the second keyframe and mpCurrentKeyFrame->mb / ->mbf for the first and for BOTH
 *                     gates (:583, :585, :656, :681); the keyframes of one call are one rig's, which has one of each
 *   far_points, th_far_points : mbFarPoints, mThFarPoints;  nlevels : the handle's.  mvScaleFactors / mvLevelSigma2 are the handle's,
 *                     ratioFactor = 1.5f * the handle's scale factor in binary32 (:424); an octave outside [0, nlevels) is CLAMPED
 *   d_exit[p*capacity + k]              : out, orbx_new_point_exit of match k < d_n_matches[p], in the order of d_pairs
 *   d_x3d[(p*capacity + k)*3 + {0,1,2}] : out, the world point; ZEROS on every rejecting exit
 *   d_n_new[p]      : out, the accepted matches of pair p (a pair named twice in one call gives the same count twice)
 *   d_mark1 / d_mark2 : NULL, or flag rows laid out like d_kf1_mp_flags / d_kf2_mp_flags of the search ([p*capacity + i]): for every
 *                     accepted match bit 0 of the entry of idx1 / idx2 is SET; nothing is ever cleared.  The bit is set with an atomic OR
 *                     on the containing 32-bit word: the arrays start 4-byte aligned and their length is a multiple of 4 bytes
 * Entries of d_exit / d_x3d from d_n_matches[p] on are left as they were, as d_pairs is.
 * The marks serve the reference's walk over the neighbours: a keypoint that received a MapPoint from neighbour i is skipped by the search
 * of neighbour i + 1 (src/ORBmatcher.cc:1033-1039).  A caller that wants exactly that runs search and triangulation with n_pairs = 1 per
 * neighbour on the handle's stream and passes the flag row the next search reads as d_mark1; a batched call
 * (n_pairs > 1) is the approximation in which all neighbours see the flags of before.
 * What is kept of the reference, each asserted by tests/test_new_map_points.py against the sequential walk:
 *   * bStereo1 = mvuRight[idx1] >= 0, bStereo2 likewise (:490, :499); pose and camera are the keyframes' own for every match;
 *   * cosParallaxRays = ray1.dot(ray2) / (norm(ray1)*norm(ray2)) in double, rounded to float once; ray = Rwc*xn one cv::gemm row each;
 *   * cosParallaxStereo = cosParallaxRays + 1 in float; cosParallaxStereo1 is replaced if bStereo1, ELSE IF bStereo2
 *     cosParallaxStereo2: with both stereo only the first is (:582-585).  cos(2*atan2(mb/2, depth)) is binary32 throughout (`using namespace
 *     std` is in scope through TemplatedVocabulary.h:36: the float overloads), as glibc's atan2f and cosf evaluate it;
 *   * the branch test (:590-591): cosParallaxRays < cosParallaxStereo compares floats, > 0 an int, < 0.9998 compares in double; mbInertial
 *     changes nothing, both alternatives are the same test;
 *   * A's rows are xn.x*Tcw.row(2) - Tcw.row(0) etc., each product and difference rounded in float; vt.row(3) is the library's own Jacobi
 *     (orbx_kb8_triangulate_device); x3D[3] == 0 is an explicit exit here; x3D = v[0..2] / v[3] a float division per element;
 *   * UnprojectStereo: (u - cx)*z*invfx rounded per operation in float with invfx = 1.0f / fx, Twc.R*x3Dc + Twc.t one cv::gemm row per element;
 *   * z1, x1, y1 ... = Rcw.row(r).dot(x3Dt) + tcw[r]: products and sums in double, rounded to float once; invz = 1.0 / z in double, rounded;
 *   * the monocular gate is > 5.991*sigma2, the stereo gate > 7.8*sigma2 with the third error u - mbf*invz - kp_ur; both compare in double;
 *   * dist = (float)cv::norm(x3D - Ow), the difference in float, the norm in double; dist == 0 rejects;
 *   * ratioDist*ratioFactor < ratioOctave || ratioDist > ratioOctave*ratioFactor, all in float.
 * The cv::Mat roundings are the library's definitions (parity unpinned).  No table depends on the capacity: there is
 * no ORBX_ERR_UNSUPPORTED case; ORBX_ERR_BAD_ARGUMENT is returned before any launch.  Asynchronous on the handle's stream; no CPU path. */
int orbx_create_new_map_points_device(orbx_handle* h, int n_pairs, int kf1_first, int kf1_step, int kf2_first, int kf2_step, const int* d_pairs,
                                      const int* d_n_matches, const float* d_poses, const orbx_camera* cam, const orbx_keypoint* d_kps_un,
                                      const orbx_keypoint* d_kps, const float* d_u_right, const float* d_depth, const int* d_n_out,
                                      int capacity, int nlevels, float mb, float mbf, int far_points, float th_far_points, uint8_t* d_exit,
                                      float* d_x3d, int* d_n_new, uint8_t* d_mark1, uint8_t* d_mark2);

/* Two-camera keyframes (NLeft != -1, mpCamera2 on both sides, a KannalaBrandt8 pair).  Rig keyframes, batch frames 2X / 2X + 1 and the
 * stacked numbering (a right keypoint j is NLeft + j, NLeft = d_n_out[2X]) as orbx_search_for_triangulation_two_eyes_device.
 *   d_pairs[(p*2*capacity + k)*2 + {0, 1}], d_n_matches[p] : exactly what that search wrote; d_n_matches[p] is clamped into [0, 2*capacity]
 *   d_poses[X*12], tlr12, cam_left, cam_right, d_kps (the RAW keypoints of both eyes; .pt and .octave are read), d_n_out : as there
 *   d_exit[p*2*capacity + k], d_x3d[(p*2*capacity + k)*3 + {0,1,2}], d_n_new[p] : out, as above
 *   d_mark1 / d_mark2 : NULL, or flag rows laid out like that search's d_kf1_mp_flags / d_kf2_mp_flags ([(2p + eye)*capacity + i])
 * What differs from the one-camera form:
 *   * pose and camera are RE-PICKED PER MATCH from bRight1 = idx1 >= NLeft1 and bRight2 (:503-568): GetRotation / GetTranslation / GetPose /
 *     GetCameraCenter and mpCamera, or GetRightRotation / GetRightTranslation / GetRightPose / GetRightCameraCenter
 *     (src/KeyFrame.cc:1232-1262, from mTlr alone, as orbx_fuse_two_eyes_device derives them) and mpCamera2.  All four branches assign
 *     everything, so nothing carries over from the match before;
 *   * bStereo1 = bStereo2 = false always (:490, :499: mpCamera2 is set): no stereo branch, no stereo gate, STEREO_1 / STEREO_2 /
 *     EMPTY_STEREO never appear; mb and mbf are not inputs;
 *   * unproject / project are KannalaBrandt8's (orbx_kb8_unproject_device, orbx_kb8_project_device).
 * Asynchronous on the handle's stream; no CPU path. */
int orbx_create_new_map_points_two_eyes_device(orbx_handle* h, int n_pairs, int kf1_first, int kf1_step, int kf2_first, int kf2_step,
                                               const int* d_pairs, const int* d_n_matches, const float* d_poses, const float* tlr12,
                                               const orbx_camera_kb8* cam_left, const orbx_camera_kb8* cam_right, const orbx_keypoint* d_kps,
                                               const int* d_n_out, int capacity, int nlevels, int far_points, float th_far_points,
                                               uint8_t* d_exit, float* d_x3d, int* d_n_new, uint8_t* d_mark1, uint8_t* d_mark2);

/* ---- MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:330-403) and MapPoint::UpdateNormalAndDepth (:427-494) on observation lists:
 * the last link between "a point was made or fused" and "the next search reads it".  The mapping thread calls both on every new point
 * (src/LocalMapping.cc:718-720), on every tracked point of a new keyframe (:317-318), on every point of the current keyframe after fusing
 * (:829-830) and on the survivor of every Replace (src/MapPoint.cc:298); the optimizer calls the second alone after every bundle
 * adjustment.  Both are pure functions of the observation list, the observing keyframes' descriptors, poses and one keypoint octave, all of
 * which live on the device; what they write are exactly the rows orbx_fuse*_device, orbx_frustum_requests*_device and the projection
 * searches read.  The bookkeeping (who observes what, who survived, mpRefKF) stays with the caller, who supplies it as lists.
 * The longest list the entries take.  1024 descriptors are 32 KB of LDS, so that several workgroups fit on a CU: a CHOICE, not a
 * measurement.  A longer list is refused per point (ORBX_MAP_POINT_TOO_LONG) and stays with the host. */
#define ORBX_MAX_OBSERVATIONS 1024

/* How a listed MapPoint left the update (d_status) */
enum orbx_map_point_update {
    ORBX_MAP_POINT_OK = 0,
    ORBX_MAP_POINT_EMPTY = 1,          /* N == 0: the early returns of :344 / :442.  No table row is written */
    ORBX_MAP_POINT_NO_DESCRIPTOR = 2,  /* every entry's keyframe isBad() (:366): the descriptor row is untouched; normal and depth ARE written */
    ORBX_MAP_POINT_BAD_INDEX = 3,      /* a frame outside the batch, a row outside [0, N_f), d_ref[m] outside the list, a negative d_obs_off[m]
                                          or d_slot[m]: the reference would index out of bounds.  No table row is written */
    ORBX_MAP_POINT_TOO_LONG = 4        /* N > ORBX_MAX_OBSERVATIONS.  No table row is written */
};

/* One-camera keyframes (NLeft == -1).  For n_points MapPoints:
 *   d_obs_off[n_points + 1] : a CSR over observations; MapPoint m owns the entries [d_obs_off[m], d_obs_off[m+1]) of d_obs; its length N is
 *                 clamped at 0 from below
 *   d_obs[o*2 + {0,1}]      : (device frame, keypoint row in that frame), ONE ENTRY PER DESCRIPTOR, in the reference's iteration order of
 *                 mObservations - the order of std::map<KeyFrame*, ...>, which is the caller's to supply.  BestIdx' tie rule and the
 *                 rounding of the normal's sum depend on it
 *   d_obs_flags[o]          : or NULL (no flag set); bit 0 = pKF->isBad().  Such an entry is left out of the descriptor selection (:353) but IS
 *                 counted in the normal: UpdateNormalAndDepth has no such test
 *   d_ref[m]                : the position within MapPoint m's list of the observation in mpRefKF, whose keypoint gives `level` (:471-482)
 *   d_slot[m]               : or NULL (= m); the row of the MapPoint tables this point reads (d_mp_world) and writes, so that only changed points
 *                 need to be listed.  Rows no listed point names are never touched.  Two listed points must not name one row
 *   d_mp_world[slot*3]      : GetWorldPos(), as orbx_fuse_device takes it
 *   d_poses[f*12], n_frames : Tcw (3x4 row-major) of the n_frames frames of the batch; Ow = -Rcw.t()*tcw is computed here
 *   d_kps_un[f*capacity + i]: mvKeysUn; only the octave of the reference entry's keypoint is read (:475)
 *   d_desc, d_n_out, capacity : mDescriptors and N of all frames; d_n_out[f] is clamped into [0, capacity]
 *   nlevels                 : must equal orbx_get_levels(h): mvScaleFactors are the handle's
 *   what                    : bit 0 = the descriptor, bit 1 = normal and depth; 1, 2 or 3, anything else is ORBX_ERR_BAD_ARGUMENT.  The rows of a
 *                 half not asked for are not touched
 *   d_mp_desc[slot*32]      : out, mDescriptor (16-byte aligned)
 *   d_mp_normal[slot*3]     : out, mNormalVector
 *   d_mp_dist[slot*3]       : out, orbx_fuse_device's triple: 0.8f*mfMinDistance, 1.2f*mfMaxDistance, mfMaxDistance
 *   d_best[m]               : out, BestIdx as a position in the list counting only the entries that took part; -1 where no descriptor was
 *                 chosen (what without bit 0 included)
 *   d_best_median[m]        : out, BestMedian; -1 beside d_best = -1
 *   d_status[m]             : out, an orbx_map_point_update.  d_best, d_best_median and d_status are written for EVERY listed point
 * Every entry of a list is checked (flagged ones as well, and whatever `what` asks for) before anything of the point is written.  What the
 * entry cannot check is the caller's: d_obs holds d_obs_off[n_points] entries and the tables hold every row d_slot names.
 * THE DESCRIPTOR HALF is integers, bit-exact against the reference: Distances[i][i] = 0, DescriptorDistance elsewhere; median =
 * sorted(row)[int(0.5*(N-1))], the element of rank (N-1)/2 of the N values with the row's own 0 among them (N = 1 and N = 2 give 0); BestIdx
 * the FIRST row with the smallest median (strict <, :393); the output is a copy of that row's 32 bytes.
 * THE NORMAL AND DEPTH HALF is cv::Mat arithmetic, the library's definitions (parity unpinned): normali = Pos - Owi a
 * float subtraction per element; cv::norm the sum of squares and the root in double; normal + normali/norm is cv::scaleAdd, normal[c] =
 * normali[c]*(float)(1.0/norm) + normal[c] with both operations rounded in float, accumulated SEQUENTIALLY in list order; normal/n =
 * normal[c]*(float)(1.0/(double)n); dist = (float)cv::norm(Pos - Ow_ref); mfMaxDistance = dist*mvScaleFactors[level], mfMinDistance =
 * mfMaxDistance/mvScaleFactors[nlevels-1], the invariance bounds their products with 0.8f and 1.2f, all float operations.  An octave outside
 * [0, nlevels) is CLAMPED into the table.
 * ORBX_ERR_BAD_ARGUMENT (a NULL pointer other than d_obs_flags / d_slot, capacity or n_frames < 1, negative n_points, `what`, nlevels) is
 * returned before any launch; n_points = 0 does nothing.  Asynchronous on the handle's stream; no CPU path. */
int orbx_update_map_points_device(orbx_handle* h, int n_points, const int* d_obs_off, const int* d_obs, const uint8_t* d_obs_flags,
                                  const int* d_ref, const int* d_slot, const float* d_mp_world, const float* d_poses, int n_frames,
                                  const orbx_keypoint* d_kps_un, const uint8_t* d_desc, const int* d_n_out, int capacity, int nlevels, int what,
                                  uint8_t* d_mp_desc, float* d_mp_normal, float* d_mp_dist, int* d_best, int* d_best_median, uint8_t* d_status);

/* Two-camera keyframes (NLeft != -1).  Rig keyframe r is device frames 2r (left eye) and 2r + 1 (right eye), d_poses[r*12] holds one pose
 * per rig and tlr12 is mTlr, exactly as orbx_fuse_two_eyes_device lays them out; n_rigs rigs make 2*n_rigs device frames.  What differs:
 *   d_obs     : a right keypoint NLeft + j is (2r + 1, j).  For a rig keyframe with both indices set the caller writes the left entry and
 *               then the right entry (:357-362, :454-465)
 *   centres   : an entry of frame 2r counts GetCameraCenter(), one of frame 2r + 1 GetRightCameraCenter() = Rwl*mTlr.t + Ow (one cv::gemm
 *               row with the float Ow as addend, src/KeyFrame.cc:1232-1240), as orbx_fuse_two_eyes_device derives it
 *   d_ref[m]  : the left entry of mpRefKF if leftIndex != -1, otherwise its right entry (:477-482).  The reference centre is ALWAYS
 *               GetCameraCenter(), the LEFT centre of that entry's rig (:468), also for a right entry
 *   d_kps     : the RAW keypoints of both eyes (mvKeys / mvKeysRight, :478, :481); only the reference entry's octave is read
 * Everything else as above. */
int orbx_update_map_points_two_eyes_device(orbx_handle* h, int n_points, const int* d_obs_off, const int* d_obs, const uint8_t* d_obs_flags,
                                           const int* d_ref, const int* d_slot, const float* d_mp_world, const float* d_poses,
                                           const float* tlr12, int n_rigs, const orbx_keypoint* d_kps, const uint8_t* d_desc,
                                           const int* d_n_out, int capacity, int nlevels, int what, uint8_t* d_mp_desc, float* d_mp_normal,
                                           float* d_mp_dist, int* d_best, int* d_best_median, uint8_t* d_status);

/* ---- loop closing's matcher: the two Sim3 overloads of ORBmatcher::SearchByProjection ----------------------------------------------------
 * Where a MapPoint left the search (d_exit of orbx_search_by_projection_sim3_device); 0 .. 5 are orbx_fuse_exit's */
enum orbx_sim3_search_exit {
    ORBX_SIM3_SEARCH_FLAG = 0,           /* bit 0 of its flag is clear (isBad() or in spAlreadyFound, :501 / :617), or it lies beyond d_n_mp */
    ORBX_SIM3_SEARCH_NEG_DEPTH = 1,      /* :511 / :627 */
    ORBX_SIM3_SEARCH_NOT_IN_IMAGE = 2,   /* :522 / :639 */
    ORBX_SIM3_SEARCH_DISTANCE = 3,       /* :531 / :648 */
    ORBX_SIM3_SEARCH_NORMAL = 4,         /* :537 / :654 */
    ORBX_SIM3_SEARCH_EMPTY_WINDOW = 5,   /* vIndices.empty() (:547 / :664), tested before any keypoint state */
    ORBX_SIM3_SEARCH_NO_MATCH = 6,       /* every candidate was closed, failed the level filter or was above the bound */
    ORBX_SIM3_SEARCH_MATCHED = 7         /* nmatches++ (:580 / :697) */
};

/* The acceptance bestDist <= TH_LOW*ratioHamming (src/ORBmatcher.cc:577, :694) compares an int with a float product.  Host-only: the largest
 * integer d in [0, 255] with (float)d <= (float)th_low * ratio_hamming; -1 if the product is negative or NaN (nothing matches).  A product
 * of 256 or more gives 255: there the reference would accept bestDist = 256 of a MapPoint WITHOUT a candidate and write vpMatched[-1];
 * the entry CLAMPS to 255 instead, so such a MapPoint never matches.  (50, 1.5) -> 75, (50, 1.0) -> 50, (50, 0.999) -> 49. */
int orbx_sim3_hamming_bound(int th_low, float ratio_hamming);

/* ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th, ratioHamming) (src/ORBmatcher.cc:473-586; projection = 0; called at
 * src/LoopClosing.cc:755 with th 5, ratio 1.0 and at :1008 with th 3, ratio 1.5) and SearchByProjection(pKF, Scw, vpPoints, vpPointsKFs,
 * vpMatched, vpMatchedKF, th, ratioHamming) (:588-704; projection = 1; called at src/LoopClosing.cc:730 with th 8, ratio 1.5), for
 * keyframes with NLeft == -1 and the Pinhole model.  NOT covered: the KannalaBrandt8 model.  (ORBmatcher::SearchBySim3, :1735-1959, has no
 * caller in the reference and is not built.)
 * Up to the window the search is the Sim3 overload of Fuse (orbx_fuse_device with reproj_check = 0) and shares its front end.  What is
 * new: a match CLOSES its keypoint for every later MapPoint of the list (vpMatched[bestIdx] = pMP, :579 / :696, is read back at :558 /
 * :675), so the MapPoints of a pair are a sequential chain.  The entry computes exactly what that chain computes - as a parallel fixed
 * point ("Sim3 projection search") - including which of several MapPoints that want the same keypoint gets it (the first in
 * list order) and what the others fall back to.
 * Pair p searches MapPoint list mp_first + p*mp_step in keyframe kf_first + p*kf_step of one device-resident batch.  kf_step = 0 is the
 * normal case: several loop candidates, each with its own Sim3 and point list, searched in the same current keyframe.
 *   d_mp_world, d_mp_normal, d_mp_dist, d_mp_desc, d_n_mp, mp_capacity : as orbx_fuse_device (d_mp_dist holds GetMinDistanceInvariance(),
 *                 GetMaxDistanceInvariance() and mfMaxDistance ITSELF)
 *   d_mp_flags[p*mp_capacity + i] : bit 0 = !pMP->isBad() && !spAlreadyFound.count(pMP) (:501, :617); static, the reference builds
 *                 spAlreadyFound once before the loop (:490, :605)
 *   d_poses[p*12]              : PER PAIR, not per frame: rows of sRcw/scw | tcw/scw as the caller's cv::Mat code computes them (:483-486,
 *                 :598-601), the convention of orbx_fuse_device with reproj_check = 0.  Ow = -Rcw.t()*tcw (:487) is computed here.
 *   d_kps_un, d_desc, d_n_out, capacity, d_grid_off, d_grid_idx, bounds4, cam, nlevels : as orbx_fuse_device (bounds4 truncated for
 *                 IsInImage and the window, the grid inverses from the floats; nlevels must be the handle's)
 *   projection                 : 0 = pKF->mpCamera->project (:519): u = fx*x/z + cx;  1 = the second overload's own lines (:631-636):
 *                 invz = 1/z; x = X*invz; u = fx*x + cx.  Every operation is rounded on its own; the two differ in the last bit.
 *   th                         : the reference's int th, multiplied as (float)th * mvScaleFactors[level] (:543, :660); 8, 5, 3 at the callers
 *   th_low, ratio_hamming      : ORBmatcher::TH_LOW (50) and ratioHamming; the bound is orbx_sim3_hamming_bound(th_low, ratio_hamming)
 *   d_occupied[p*capacity + idx] : vpMatched[idx] != NULL on entry, or NULL = all free
 *   d_matches[p*capacity + idx]  : out, the list index i of the MapPoint the keypoint holds afterwards (vpMatched[idx] = vpPoints[i]), -1 =
 *                 none; a keypoint occupied on entry stays -1 (the caller keeps its old entry).  vpMatchedKF[idx] of the second overload is
 *                 vpPointsKFs[d_matches[idx]]: the caller derives it.
 *   d_match_idx[p*mp_capacity + i]  : out, the keypoint MapPoint i received, -1 = none
 *   d_match_dist[p*mp_capacity + i] : out, the accepted distance; 256 where nothing was accepted
 *   d_exit[p*mp_capacity + i]       : out or NULL, an orbx_sim3_search_exit
 *   d_n_matches[p]                  : out, the return value
 * All entries of every pair are written (entries past d_n_mp as FLAG, -1, 256).  Arithmetic, IsInImage, PredictScale, GetFeaturesInArea
 * and the tie rule (of equal distances the FIRST in visit order) as orbx_fuse_device.  Errors: ORBX_ERR_BAD_ARGUMENT as orbx_fuse_device
 * (and for a projection other than 0 / 1).  Supported: the settling workgroup of a pair keeps one int per keypoint and one per MapPoint
 * in LDS, and a key holds the keypoint's grid slot in 16 bits:
 *   4 * (capacity + mp_capacity) + 64 <= 163 328 bytes  and  capacity <= 65 536      (capacity 2720 with mp_capacity 16384 is inside)
 * a larger call returns ORBX_ERR_UNSUPPORTED before anything is launched or allocated.  The key lists (48 bytes per pair and MapPoint)
 * are the handle's, allocated on first use.  Asynchronous on the handle's stream. */
int orbx_search_by_projection_sim3_device(orbx_handle* h, int n_pairs, int kf_first, int kf_step, int mp_first, int mp_step,
                                          const float* d_mp_world, const float* d_mp_normal, const float* d_mp_dist, const uint8_t* d_mp_desc,
                                          const int* d_n_mp, int mp_capacity, const uint8_t* d_mp_flags, const float* d_poses,
                                          const orbx_keypoint* d_kps_un, const uint8_t* d_desc, const int* d_n_out, int capacity,
                                          const int* d_grid_off, const int* d_grid_idx, const float* bounds4, const orbx_camera* cam, int nlevels,
                                          int projection, float th, int th_low, float ratio_hamming, const uint8_t* d_occupied, int* d_matches,
                                          int* d_match_idx, int* d_match_dist, uint8_t* d_exit, int* d_n_matches);

/* ---- the tracker's front half of the two map-to-frame projection searches: the frustum test and the request lists -------------------------
 * Which statement orbx_frustum_requests_device applies to a MapPoint */
enum orbx_frustum_mode {
    ORBX_FRUSTUM_LOCAL_MAP = 0,       /* Frame::isInFrustum (src/Frame.cc:493-570) + the matcher's prelude (src/ORBmatcher.cc:50-73) */
    ORBX_FRUSTUM_RELOCALIZATION = 1   /* the projection of pKF's MapPoints (src/ORBmatcher.cc:2183-2230) */
};
/* Where a MapPoint left it (orbx_track_record.exit) */
enum orbx_frustum_exit {
    ORBX_FRUSTUM_FLAG = 0,            /* bit 0 of its flag is clear (src/Tracking.cc:2945-2948 / src/ORBmatcher.cc:2199-2201), or it lies beyond d_n_mp */
    ORBX_FRUSTUM_NEG_DEPTH = 1,       /* PcZ < 0.0f (src/Frame.cc:513); never in the relocalisation mode, which has no depth test */
    ORBX_FRUSTUM_NOT_IN_IMAGE = 2,    /* src/Frame.cc:520-523 / src/ORBmatcher.cc:2209-2212 */
    ORBX_FRUSTUM_DISTANCE = 3,        /* src/Frame.cc:535 / src/ORBmatcher.cc:2222 */
    ORBX_FRUSTUM_VIEW_COS = 4,        /* viewCos < viewingCosLimit (src/Frame.cc:547); local map only */
    ORBX_FRUSTUM_FAR = 5,             /* isInFrustum returned true, the matcher skips it: bFarPoints && mTrackDepth > thFarPoints (src/ORBmatcher.cc:56) */
    ORBX_FRUSTUM_REQUEST = 6          /* it became a request */
};
/* What Frame::isInFrustum leaves in the MapPoint (src/Frame.cc:497-499, :526-527, :556-565), one per list entry.  mbTrackInView is
 * exit >= ORBX_FRUSTUM_FAR.  proj_x / proj_y are -1 until the bounds test has passed and uv from there on (the reference assigns them at
 * :526-527 even when it returns false later).  Fields the reference does not assign on the entry's path are 0 and level is -1 (proj_xr,
 * depth, view_cos and level are assigned only when isInFrustum returns true), so every byte is defined; an entry that was not looked at
 * (ORBX_FRUSTUM_FLAG) carries -1, -1, 0, 0, 0, -1, 0.  Relocalisation mode: proj_x / proj_y as above, level = nPredictedLevel of a request
 * (src/ORBmatcher.cc:2225), proj_xr = depth = view_cos = 0. */
typedef struct orbx_track_record {
    float proj_x, proj_y;   /* mTrackProjX, mTrackProjY */
    float proj_xr;          /* mTrackProjXR = uv.x - mbf*invz (:558) */
    float depth;            /* mTrackDepth = Pc_dist = cv::norm(Pc) (:508, :560) */
    float view_cos;         /* mTrackViewCos (:545, :565) */
    int32_t level;          /* mnTrackScaleLevel (:551, :564) */
    int32_t exit;           /* an orbx_frustum_exit */
} orbx_track_record;

/* Tracking::SearchLocalPoints' loop over the local map (src/Tracking.cc:2941-2959) and the front half of Relocalization's projection search,
 * on the device: MapPoint lists and frame poses in, the request lists of orbx_search_by_projection_device out.  For frames with Nleft == -1 and
 * the Pinhole model.  NOT covered here: isInFrustum's Nleft != -1 branch (src/Frame.cc:571 on: isInFrustumChecks, mpCamera2 - the KannalaBrandt8
 * pair), which is orbx_frustum_requests_two_eyes_device below; the relocalisation mode has no two-camera form.
 * Pair p projects MapPoint list mp_first + p*mp_step into frame cur_first + p*cur_step (mp_step = 0: one local map into several frames).
 *   per MapPoint, in blocks of mp_capacity per list (m = list*mp_capacity + i), the conventions of orbx_fuse_device:
 *   d_mp_world[m*3], d_mp_normal[m*3] : GetWorldPos(), GetNormal() (the normals are read in mode 0 only and may be NULL in mode 1)
 *   d_mp_dist[m*3]             : GetMinDistanceInvariance(), GetMaxDistanceInvariance() and mfMaxDistance ITSELF (src/MapPoint.cc:519)
 *   d_mp_desc[m*32]            : GetDescriptor() (16-byte aligned)
 *   d_mp_angle[m]              : mode 1: pKF->mvKeysUn[i].angle of the keypoint that holds the MapPoint (src/ORBmatcher.cc:2264); NULL is allowed in mode 0
 *   d_n_mp[list]               : MapPoints of the list, NULL = mp_capacity
 *   d_mp_flags[p*mp_capacity + i] : per PAIR.  mode 0: bit 0 = pMP->mnLastFrameSeen != mCurrentFrame.mnId && !pMP->isBad()
 *                 (src/Tracking.cc:2945-2948), bit 1 = Observations() > 0.  mode 1: bit 0 = pMP && !pMP->isBad() && !sAlreadyFound.count(pMP)
 *                 (src/ORBmatcher.cc:2199-2201)
 *   d_poses[f*12]              : Frame::mTcw, rows 0..2 (3x4, row-major: Rcw | tcw) of every frame, as orbx_project_last_frame_device takes them
 *   cam (fx, fy, cx, cy)       : Pinhole::project (src/CameraModels/Pinhole.cpp:30-33): u = fx*x/z + cx
 *   bounds4                    : Frame's FLOAT mnMinX, mnMaxX, mnMinY, mnMaxY, compared as they are and NON-STRICTLY (uv.x < mnMinX || uv.x >
 *                 mnMaxX leaves, src/Frame.cc:520-523): a projection exactly on a bound passes.  Not KeyFrame's truncated, strict bounds of orbx_fuse_device.
 *   nlevels                    : must equal orbx_get_levels(h) (mvScaleFactors and PredictScale's breakpoints are the handle's); else ORBX_ERR_BAD_ARGUMENT
 * mode = ORBX_FRUSTUM_LOCAL_MAP: Frame::isInFrustum(pMP, view_cos_limit) (src/Frame.cc:493-570; the caller passes 0.5, src/Tracking.cc:2950),
 * every operation rounded on its own: Pc = mRcw*P + mtcw as cv::gemm (products and sums in double, one rounding to float); Pc_dist =
 * cv::norm(Pc) (squares summed in double in element order, one square root, then float, :508); PcZ < 0.0f leaves (:513); invz = 1.0f/PcZ is a
 * float division (:512) and z == 0 is NOT rejected: it goes on to Pinhole::project and +-inf leaves by the bounds (:520-523); mOw =
 * -mRcw.t()*mtcw (src/Frame.cc:466-472); PO = P - mOw in float (:532); dist = cv::norm(PO) (:533); dist < min || dist > max leaves (:535: both
 * ends pass); viewCos = (float)(PO.dot(Pn) / (double)dist) - Mat::dot accumulates a double in element order and the quotient is a double
 * division stored to float (:545; NOT Fuse's dot < 0.5*dist: a quotient below 0.5 that rounds to 0.5f passes here); viewCos < view_cos_limit
 * leaves (:547); PredictScale(dist, this) as the count of breakpoints at or below mfMaxDistance/dist (:551, src/MapPoint.cc:531-546);
 * mTrackProjXR = uv.x - mbf*invz (:558); mTrackDepth = Pc_dist (:560).  Then the prelude of ORBmatcher::SearchByProjection(F, vpMapPoints, th,
 * bFarPoints, thFarPoints) (src/ORBmatcher.cc:50-73): far_points && mTrackDepth > th_far_points leaves (:56); r = RadiusByViewingCos(viewCos)
 * (:216-222: the float against the DOUBLE literal 0.998, which is viewCos >= 0.998f - a viewCos equal to 0.998f gets 2.5, not 4.0); th !=
 * 1.0f multiplies it (:48, :69-70); the request is u, v = uv, ur = mTrackProjXR, radius = r*mvScaleFactors[level], min_level, max_level =
 * level - 1, level (:73), flags = 1 | (bit 1 of the input flag), angle = 0.
 * mode = ORBX_FRUSTUM_RELOCALIZATION: src/ORBmatcher.cc:2183-2230.  x3Dc = Rcw*x3Dw + tcw (:2205), project (:2207), the four bounds tests
 * (:2209-2212) - there is NO depth test: a point behind the camera that projects inside the bounds becomes a request, as in the reference -,
 * Ow (:2185), PO, dist3D (:2215-2216), the invariance test (:2222), PredictScale (:2225); the request is u, v = uv, ur = 0, radius =
 * th*mvScaleFactors[level] (:2228), min_level, max_level = level - 1, level + 1 (:2230), flags = 3, angle = d_mp_angle[m].  d_mp_normal, mbf,
 * view_cos_limit, far_points and th_far_points are unused.
 *   d_queries[p*mp_capacity + k], d_query_desc[(p*mp_capacity + k)*32], d_query_src[p*mp_capacity + k], k < d_n_queries[p] : out, the requests
 *                 of pair p COMPACTED IN LIST ORDER (the same order in every run: no atomic decides a position), their descriptors (16-byte
 *                 aligned) and the list index i each came from.  They are what orbx_search_by_projection_device takes with query_capacity =
 *                 mp_capacity, desc_first = 0, desc_step = 1 and d_n_queries as it is; vpMapPoints[d_query_src[d_matches[i2]]] is the match.
 *                 (With n_pairs = 1 any query_capacity at or above d_n_queries[0] addresses the same slots, and the search's LDS grows with it.)
 *                 Slots k >= d_n_queries[p] get an all-zero request and src = -1; their descriptor slots are left untouched.
 *   d_track[p*mp_capacity + i] : out, an orbx_track_record per list entry; entries beyond d_n_mp carry ORBX_FRUSTUM_FLAG
 *   d_n_in_view[p]             : out, nToMatch (src/Tracking.cc:2950-2954): the entries with exit >= ORBX_FRUSTUM_FAR, counted BEFORE the far test -
 *                 the caller's IncreaseVisible() set and mmProjectPoints.  In mode 1 it equals d_n_queries[p].
 * Errors: ORBX_ERR_BAD_ARGUMENT as orbx_fuse_device (null pointer, nlevels, a mode other than 0 / 1, negative sizes or indices).  Nothing lives in
 * LDS tables: there is no capacity bound and no ORBX_ERR_UNSUPPORTED case.  Asynchronous on the handle's stream. */
int orbx_frustum_requests_device(orbx_handle* h, int n_pairs, int cur_first, int cur_step, int mp_first, int mp_step, const float* d_mp_world,
                                 const float* d_mp_normal, const float* d_mp_dist, const uint8_t* d_mp_desc, const float* d_mp_angle,
                                 const int* d_n_mp, int mp_capacity, const uint8_t* d_mp_flags, const float* d_poses, const orbx_camera* cam,
                                 const float* bounds4, int nlevels, int mode, float mbf, float view_cos_limit, float th, int far_points,
                                 float th_far_points, orbx_proj_query* d_queries, uint8_t* d_query_desc, int* d_query_src, int* d_n_queries,
                                 orbx_track_record* d_track, int* d_n_in_view);

/* Tracking::SearchLocalPoints' loop over the local map (src/Tracking.cc:2941-2959) for TWO-CAMERA rigs (Nleft != -1, a KannalaBrandt8 pair), on
 * the device: MapPoint lists and rig poses in, the request lists of orbx_search_by_projection_two_eyes_device out.  The statement is
 * Frame::isInFrustum's else branch (src/Frame.cc:571-581): Frame::isInFrustumChecks (:1181-1254) once per eye, then the prelude of
 * ORBmatcher::SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) for F.Nleft != -1 (src/ORBmatcher.cc:50-73, :145-151, :216-222).
 * Pair p projects MapPoint list mp_first + p*mp_step into RIG frame cur_first + p*cur_step.  The list / pair indexing, the d_mp_dist triples,
 * d_n_mp (clamped to 0 .. mp_capacity, NULL = mp_capacity), d_mp_flags per pair (bit 0 = pMP->mnLastFrameSeen != mCurrentFrame.mnId &&
 * !pMP->isBad(), bit 1 = Observations() > 0) and nlevels are those of orbx_frustum_requests_device.
 *   d_poses[r*12]              : Frame::mTcw, rows 0..2 (3x4, row-major: Rcw | tcw), per RIG frame, as orbx_project_last_frame_two_eyes_device
 *   trl12, tlr12               : Frame::mTrl and Frame::mTlr (3x4, row-major; host memory), BOTH as the Frame holds them: neither is derived from the other
 *   cam_left, cam_right        : mpCamera and mpCamera2.  The right eye is projected with ITS OWN eight parameters (:1210) - unlike the
 *                 frame-to-frame search, which uses the left camera for both eyes
 *   bounds4                    : Frame's FLOAT mnMinX, mnMaxX, mnMinY, mnMaxY, the same four for both eyes, compared NON-STRICTLY in the
 *                 reference's form (uv.x < mnMinX || uv.x > mnMaxX leaves, :1213-1216): a projection on a bound passes, and so does a NaN
 *   d_mp_prev_depth[p*mp_capacity + i] : mTrackDepth as an earlier frame left it in the MapPoint; may be NULL (= 0 everywhere).  It decides only for a
 *                 MapPoint that the right eye sees and the left eye does not (below)
 * Rig invariants, once per pair: left eye mR = Rcw, mt = tcw, twc = mOw = -Rcw.t()*tcw; right eye mR = Rrl*Rcw (a 3x3 cv::Mat product: every
 * element one row-by-column sum in double, rounded to float once), mt = Rrl*tcw + trl (ONE gemm with the addend), twc = mRwc*mTlr.col(3) + mOw
 * (one gemm of the transposed Rcw with the float mOw as addend) (:1186-1197).  These cv::Mat roundings are parity unpinned, as orbx_fuse_device's.
 * Per eye, every operation rounded on its own: Pc = mR*P + mt as cv::gemm; Pc_dist = cv::norm(Pc) (squares summed in double in element order,
 * one square root, then float); PcZ < 0.0f leaves, z == 0 goes on (:1205); uv = KannalaBrandt8::project(Pc) with that eye's camera, as
 * orbx_kb8_project_device; the bounds (:1213-1216); PO = P - twc in float; dist = cv::norm(PO); dist < min || dist > max leaves (:1224);
 * viewCos = (float)(PO.dot(Pn) / (double)dist) (:1230); viewCos < view_cos_limit leaves (:1232); level = PredictScale(dist) (:1236).  A check
 * that returns false assigns NOTHING - unlike the one-camera branch there is no mTrackProjX = uv.x in front of the distance test and no invz.
 * Per MapPoint: mbTrackInView = L, mbTrackInViewR = R; nToMatch counts L || R (src/Tracking.cc:2950-2954).  The matcher skips the MapPoint when
 * neither eye is in view (:53) and when far_points && mTrackDepth > th_far_points (:56).  mTrackDepth is the LEFT eye's Pc_dist; when the left
 * check failed nothing assigned it in this frame, the reference reads what an earlier frame left there, and the entry takes that value from
 * d_mp_prev_depth (NULL or 0: never far).  Left request: radius = RadiusByViewingCos(mTrackViewCos) (viewCos >= 0.998f gives 2.5, else 4.0),
 * times th only when th != 1.0f (:69-70), times mvScaleFactors[level]; levels level - 1, level (:73).  Right request: radius =
 * RadiusByViewingCos(mTrackViewCosR) * mvScaleFactors[levelR], WITHOUT th (:148); levels levelR - 1, levelR (:151).  flags of each request =
 * (that eye in view ? 1 : 0) | (bit 1 of the input flag); a request whose eye is not in view is all zero apart from that bit 1; ur and angle
 * are 0.  A MapPoint becomes a slot (two requests, one descriptor) when L || R and it is not far.
 *   d_track[(p*mp_capacity + i)*2 + eye] : out, one orbx_track_record per eye.  L: proj_x / proj_y = mTrackProjX / Y, depth = mTrackDepth,
 *                 view_cos = mTrackViewCos, level = mnTrackScaleLevel.  R: proj_x / proj_y = mTrackProjXR / YR, depth = mTrackDepthR, view_cos =
 *                 mTrackViewCosR, level = mnTrackScaleLevelR.  proj_xr is 0 in both.  A record whose check returned false, or that was not looked
 *                 at, is -1, -1, 0, 0, 0, -1 (the level src/Frame.cc:574-575 leave) plus its exit, an orbx_frustum_exit per eye: every byte
 *                 is defined.  In view is exit >= ORBX_FRUSTUM_FAR; ORBX_FRUSTUM_FAR is set on every in-view eye of a far MapPoint.
 *   d_queries[(p*query_capacity + k)*2 + {0: L, 1: R}], d_query_desc[(p*query_capacity + k)*32], d_query_src[p*query_capacity + k],
 *   k < d_n_queries[p]         : out, the slots of pair p COMPACTED IN LIST ORDER (the same order in every run: no atomic decides a position),
 *                 their descriptors (16-byte aligned, as d_mp_desc) and the list index each came from.  They are what
 *                 orbx_search_by_projection_two_eyes_device takes with the same query_capacity, desc_first = 0, desc_step = 1 and d_n_queries
 *                 as it is.  Slots k >= d_n_queries[p] get two all-zero requests and src = -1; their descriptor slots are left untouched.
 *   query_capacity             : 1 .. mp_capacity, a stride of its own (the search keeps 8 bytes per request in LDS: a 4096-point local map with
 *                 half of its points in view need not force 4096 on a multi-pair call).  Slots beyond it are dropped from the END of the list:
 *                 d_n_queries[p] is the number written, d_n_wanted[p] (may be NULL) the number the list produced.
 *   d_n_in_view[p]             : out, nToMatch: the MapPoints with L || R, counted BEFORE the far test
 * Two launches on the handle's stream (the statement and one slot count per workgroup; the placement), a list spread over ceil(mp_capacity / 256)
 * workgroups per pair; the counts live in a workspace of the handle that grows on first use.  Errors: ORBX_ERR_BAD_ARGUMENT before any launch
 * (null pointer, nlevels, n_pairs outside 1 .. 65535, query_capacity outside 1 .. mp_capacity, negative sizes or indices).  Nothing lives in
 * LDS tables: there is no capacity bound and no ORBX_ERR_UNSUPPORTED case.  Asynchronous on the handle's stream. */
int orbx_frustum_requests_two_eyes_device(orbx_handle* h, int n_pairs, int cur_first, int cur_step, int mp_first, int mp_step,
                                          const float* d_mp_world, const float* d_mp_normal, const float* d_mp_dist, const uint8_t* d_mp_desc,
                                          const int* d_n_mp, int mp_capacity, const uint8_t* d_mp_flags, const float* d_mp_prev_depth,
                                          const float* d_poses, const float* trl12, const float* tlr12, const orbx_camera_kb8* cam_left,
                                          const orbx_camera_kb8* cam_right, const float* bounds4, int nlevels, float view_cos_limit, float th,
                                          int far_points, float th_far_points, int query_capacity, orbx_proj_query* d_queries,
                                          uint8_t* d_query_desc, int* d_query_src, int* d_n_queries, int* d_n_wanted, orbx_track_record* d_track,
                                          int* d_n_in_view);

/* Stream control.  By default the handle owns a stream; orbx_set_stream adopts a caller stream
 * (hipStream_t passed as void*, e.g. torch.cuda.current_stream().cuda_stream) so the caller's events
 * and graphs see the work. */
int orbx_set_stream(orbx_handle* h, void* hip_stream);
void* orbx_get_stream(const orbx_handle* h);
int orbx_synchronize(orbx_handle* h);

/* ---- introspection used by tests and bench.py (not part of the reference surface) ------------- */
/* rounds the fixed-point projection search of the last launch needed for pair 0, and 100-MHz ticks of its staging / first scan / rounds */
int orbx_debug_search_rounds(int* out4);
/* the two-eye projection search (orbx_search_by_projection_two_eyes_device): out4[0] rounds the fixed point of the last launch's pair 0
 * needed, [1] 1 if pair 0 was settled by the walk (forced, or a MapPoint without observations reopened a keypoint), [2] pairs settled by the
 * walk since the last read (the read resets it), [3] 100-MHz ticks of pair 0's workgroup.  Returns 0, or a negative orbx_status. */
int orbx_debug_two_eyes_search_stats(int* out4);
/* the two-eye frame-to-frame search (orbx_search_last_frame_two_eyes_device), the last launch's pair 0: out4[0] rounds of the fixed point,
 * out4[1..3] 100 MHz ticks of staging, of the first scan and of the rounds */
int orbx_debug_last_frame_two_eyes_stats(int* out4);
/* the two-camera triangulation search (orbx_search_for_triangulation_two_eyes_device): counters are kept only after
 * orbx_debug_search_triangulation_two_eyes_enable(1) (process-wide; off by default, a launch then pays nothing for them).  The last counted
 * launch, all pairs: out2[0] calls of KannalaBrandt8::TriangulateMatches, out2[1] candidates without a MapPoint and with dist <= th_low.
 * The read waits for the whole device (hipDeviceSynchronize), whatever stream the handle uses. */
int orbx_debug_search_triangulation_two_eyes_enable(int on);
int orbx_debug_search_triangulation_two_eyes_stats(int* out2);
/* orbx_stereo_fisheye_match_device: the counter is kept only after orbx_debug_stereo_fisheye_enable(1) (process-wide; off by default, a launch
 * then pays nothing for it).  The last counted launch, all rigs: out1[0] calls of KannalaBrandt8::TriangulateMatches (= d_n_desc_matches
 * summed).  The read waits for the whole device (hipDeviceSynchronize), whatever stream the handle uses. */
int orbx_debug_stereo_fisheye_enable(int on);
int orbx_debug_stereo_fisheye_stats(int* out1);
/* orbx_create_new_map_points_device / _two_eyes_device: the counters are kept only after orbx_debug_new_map_points_enable(1) (process-wide;
 * off by default, a launch then pays nothing for them).  The last counted launch, all pairs: out2[0] matches that took the SVD branch
 * (:590-611), out2[1] matches that took an UnprojectStereo branch (:612-619).  The read waits for the whole device. */
int orbx_debug_new_map_points_enable(int on);
/* orbx_reconstruct_two_views_device: which of its two hypothesis kernels the next launches take (process-wide): 1 = the rows of the 16x9 /
 * 8x9 system over the lanes of the wave (the default), 0 = one lane out of LDS.  The results are the same bit for bit. */
int orbx_debug_two_view_shape(int shape);
/* orbx_sim3_solve_device: which of its three kernels the next calls launch (process-wide; tools/sim3_solver_rate.py times the steps by
 * difference): 1 = prepare, 3 = prepare + hypotheses, 7 = all (the default).  Anything but 7 leaves the result rows unfinished. */
int orbx_debug_sim3_solve_steps(int mask);
/* orbx_optimize_pose_device has ONE launch form: the launches of its kernel so far in this process (one per accepted call). */
int orbx_debug_pose_optimization_launches(void);
/* orbx_detect_candidates_device has ONE launch form of two kernels: the launches so far in this process of k_place_pairs (which = 0; none for
 * a call with n_db == 0) and of k_place_query (which = 1; one per accepted call). */
int orbx_debug_place_recognition_launches(int which);
/* orbx_covisibility_device has ONE launch form of two kernels, orbx_keyframe_redundancy_device of one: the launches so far in this process
 * of k_covis_rank (which = 0) and k_covis_vote (1), one each per accepted call of the vote, and of k_keyframe_redundancy (2), one per
 * accepted call of the redundancy test.  Another `which` returns ORBX_ERR_BAD_ARGUMENT. */
int orbx_debug_covisibility_launches(int which);
int orbx_debug_new_map_points_stats(int* out2);

/* the Sim3 projection search (orbx_search_by_projection_sim3_device): out4[0] rounds the fixed point of the last launch's pair 0 needed
 * (the last one changes nothing), [1] requests of the last launch whose decision came from scanning the window again (every key of a
 * truncated list was closed), [2] 100-MHz ticks of pair 0's settling workgroup, [3] 0.  Returns 0, or a negative orbx_status. */
int orbx_debug_sim3_search_stats(int* out4);
/* keys the window kernel of that search keeps per MapPoint (tests plant a window that holds more) */
int orbx_debug_sim3_search_list_length(void);

/* Which launch forms the last call took (results never depend on them; the parity tests assert the form they mean to cover and the
 * published timings name theirs): pyramid_form 0 = k_pyr_cols (region-major, *pyramid_cut_px = side of its regions), 1 = k_pyr_first +
 * one k_resize per level; blur_form 0 = k_blur, 1 = lanes of the FAST launch, 3 = per keypoint inside k_describe (no blurred level exists:
 * orbx_debug_get_blurred has nothing to show), 5 = split by level: per keypoint below orbx_debug_last_split_level(), k_blur from that level on
 * (only those blurred levels exist).  (2 and 4 named forms that rounds 4 / 5 measured slower and round 6 removed.) */
int orbx_debug_last_forms(const orbx_handle* h, int* pyramid_form, int* pyramid_cut_px, int* blur_form);
/* the first level the last call blurred with k_blur when its blur form was 5; 0 otherwise */
int orbx_debug_last_split_level(const orbx_handle* h);
/* Launches of the LDS polluter (test aid "lds_pollute", below) on this handle since orbx_create: one in front of EVERY kernel a call enqueues,
 * the second and later kernels of an entry included, so a test reads off the difference how many kernels an entry call launched behind a
 * pollution.  0 for ever with the aid off.  NULL handle: ORBX_ERR_BAD_ARGUMENT. */
int orbx_debug_lds_pollutions(const orbx_handle* h);

/* Test aids.  They cannot be set from the environment: a test calls this BEFORE orbx_create and the handles created afterwards carry the
 * setting.  name = "poison" (byte every device allocation of orbx_create is filled with; -1 = off), "lds_pollute" (byte every CU's LDS is
 * filled with in front of every kernel; -1 = off), "fail_after_fast" (1: the next handle's first small-batch call returns ORBX_ERR_HIP
 * between the FAST and the quad-tree launch, once), "pyr_cols_shape" (1, 4 or 6: pins the workgroup shape of k_pyr_cols; -1 = by the grid
 * size), "shared_upload_bytes" (host-buffer batches whose input is at least this large copy it through the device's shared copy queue
 * and bring the results back by DMA, smaller ones use the handle's stream and a copy kernel; -1 = 16 MiB), "two_eyes_walk" (1: the two-eye
 * projection search settles every pair by its walk instead of the fixed point; 0 = by the decisions), "two_eyes_bow_stage" (0: the two-eye
 * BoW search reads the frame pair's descriptors from L2 whatever the capacity; -1 = staged in LDS where they fit), "describe_sums" (pins how the
 * description kernels sum a frame's per-level counts: 0 = the scalar form of large launches, 1 = the lane form of small ones; -1 = by the
 * launch's size).  Unknown name: ORBX_ERR_BAD_ARGUMENT. */
int orbx_debug_set_option(const char* name, int value);

/* IC_Angle's weight words, the static tables the description kernels fill their LDS copy from: pb384 = [2][16][12] words over the 44-byte tile
 * row of the patch-blur form (byte t <-> u = t - 22), plain256 = [2][16][8] words over the 32 bytes from the patch's first column on (byte k <->
 * u = k - 15); plane 0 holds u + 16 inside the disc's row (|u| <= umax[|v|], |u| <= 15), plane 1 holds 1 there, both 0 outside.  The host's copy
 * of the array the device's is initialised from: needs no device. */
int orbx_debug_describe_tables(unsigned* pb384, unsigned* plain256);

/* The level table the description kernels take by value, beside the per-level geometry it is filled from, for a rows x cols image on a handle
 * of max_batch frames: both as [11][16] 64-bit values, rows = first selection slot, width, height, pyramid row stride, blurred row stride, pyramid
 * offset, pyramid bytes per frame, blurred offset, blurred bytes per frame, scale factor (the float's bits), keypoint size; columns = levels.  In
 * desc176 a level >= nlevels has INT_MAX as its first slot (no slot lies in it) and 0 elsewhere; in geom176 it is all 0.  Needs no device. */
int orbx_debug_describe_levels(int nfeatures, float scale_factor, int nlevels, int rows, int cols, int max_batch, int* desc_nlevels,
                               long long* desc176, long long* geom176);

/* The launch-policy switches as orbx_create read them, "NAME=value" separated by blanks, "(env)" behind a value that came from an ORBX_<NAME>
 * environment variable (read once, at orbx_create; they choose between result-identical launch forms), and the test aids in force, if any.
 * bench.py prints it as config.policy. */
const char* orbx_debug_policy(const orbx_handle* h);

/* The shader clock while the handle's work is running (bench.py: secondary.sustained).  orbx_debug_clock_probe enqueues, on a stream of
 * its own and without waiting, one sleeping wave per CU that reads the shader-clock and the 100-MHz real-time counters 50 us apart, into
 * slot 0..63; orbx_debug_clock_read waits for the probes launched so far and returns GHz per slot (0 for a slot never probed). */
int orbx_debug_clock_probe(orbx_handle* h, int slot);
int orbx_debug_clock_read(orbx_handle* h, int n_slots, double* ghz);

/* ORBX_HOST_TIMING=1 in the environment: wall seconds of the one-frame host call (orbx_extract_view) accumulated per phase since the last read:
 * out8[0] enqueue (staging + copy + launches), [1] wait, [2] pointer query, [3] staging memcpy, [4] staging + H2D enqueue; *calls = calls summed. */
int orbx_debug_host_timing(double* out8, long* calls);

/* Stage outputs of frame `frame` of the last batch, copied to host.  Candidates are the reference's
 * vToDistributeKeys of one level (ORBextractor.cc:786-864) in rectangle coordinates; their order is
 * unspecified (the octree result does not depend on it), sort before comparing. */
int orbx_debug_num_candidates(orbx_handle* h, int frame, int level, int* n);
int orbx_debug_get_candidates(orbx_handle* h, int frame, int level, orbx_keypoint* out, int capacity);
/* The 7x7 sigma-2 blurred level (ORBextractor.cc:1126-1127), width x height. */
int orbx_debug_get_blurred(orbx_handle* h, int frame, int level, uint8_t* dst, ptrdiff_t dst_stride);

/* Per-kernel timing with HIP events on the handle's stream.  enable=1 brackets every kernel launch of
 * subsequent extract calls with events (adds launch overhead: use for attribution, not for fps). */
#define ORBX_NUM_KERNELS 10
int orbx_profile_enable(orbx_handle* h, int enable);
int orbx_profile_reset(orbx_handle* h);
/* Resolves pending events; fills total milliseconds and launch counts per kernel slot. */
int orbx_profile_read(orbx_handle* h, double* total_ms, long* launches);
const char* orbx_profile_kernel_name(int slot);
/* ... and the kernel that last ran in that slot on this handle, by the name rocprofv3 prints (without template arguments): slot 1 is
 * k_pyr_cols or k_resize, slot 3 k_fast or k_fast_wide, slot 4 k_octree_256 / _512 / _1024 (+ r: the 128-VGPR build, g: node arrays in HBM).
 * bench.py keys roofline.kernel_ms_per_step with these, so that the line can be read next to profiles/ *_kernel_stats.md. */
const char* orbx_profile_kernel_name_of(const orbx_handle* h, int slot);

/* Algorithmic HBM bytes of one frame at this geometry (P0 + 2*S + 60*n_out). */
long orbx_algorithmic_bytes(const orbx_handle* h, int rows, int cols, int n_out);

#ifdef __cplusplus
}
#endif
#endif /* ORBX_H */
