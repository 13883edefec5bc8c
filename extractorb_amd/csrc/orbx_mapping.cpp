// orbx_mapping.cpp - the C ABI of the mapping thread's triangulation on ONE-CAMERA keyframes (include/orbx.h): the loop of
// LocalMapping::CreateNewMapPoints behind SearchForTriangulation (k_new_map_points.hip), and MapPoint::ComputeDistinctiveDescriptors /
// UpdateNormalAndDepth on the observation lists of such keyframes (k_map_point_update.hip; its rejections are held by
// tests/test_map_point_update_gpu.py).  Thin, as the entries of orbx_rows.cpp are: argument
// checks, the parameter block, the counters' launch and one launch.  The checks and fills are orbx_entry.hpp's and orbx_internal.hpp's.  A file
// of its own: tests/test_entry_rejections_gpu.py holds a table of exactly the *_device entries of orbx_rows.cpp, and the rejections of the
// entry here are held by tests/test_new_map_points_gpu.py.  The two-camera form is in orbx_mapping_two_eyes.cpp.
// No CPU path.
#include "orbx_internal.hpp"

extern "C" {

int orbx_create_new_map_points_device(orbx_handle* h, int n_pairs, int kf1_first, int kf1_step, int kf2_first, int kf2_step, const int* d_pairs,
                                      const int* d_n_matches, const float* d_poses, const orbx_camera* cam, const orbx_keypoint* d_kps_un,
                                      const orbx_keypoint* d_kps, const float* d_u_right, const float* d_depth, const int* d_n_out,
                                      int capacity, int nlevels, float mb, float mbf, int far_points, float th_far_points, uint8_t* d_exit,
                                      float* d_x3d, int* d_n_new, uint8_t* d_mark1, uint8_t* d_mark2) {
    if (!h) return ORBX_ERR_BAD_ARGUMENT;
    // d_mark1 and d_mark2 may be NULL; d_u_right NULL = monocular, and only then may d_kps and d_depth be NULL
    if (!d_pairs || !d_n_matches || !d_poses || !cam || !d_kps_un || !d_n_out || !d_exit || !d_x3d || !d_n_new ||
        (d_u_right && (!d_kps || !d_depth)) || capacity < 1 || n_pairs < 1 || negativeWalk(kf1_first, kf1_step, n_pairs) ||
        negativeWalk(kf2_first, kf2_step, n_pairs) || (long long)n_pairs * newMapPointsTiles(capacity) > 0x7fffffffLL)
        return fail(h, ORBX_ERR_BAD_ARGUMENT, "null pointer (d_kps and d_depth are needed beside d_u_right), capacity/n_pairs < 1, a negative "
                                              "frame index or more than 2^31 - 1 workgroups");
    if (int rc = sameLevels(h, nlevels)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    NewMapPointsParams p{};
    p.cam[0][0] = cam->fx; p.cam[0][1] = cam->fy; p.cam[0][2] = cam->cx; p.cam[0][3] = cam->cy;      // Pinhole::mvParameters
    levelsWholeTable(p.scale, h->tabs.scale);
    levelsWholeTable(p.sigma2, h->tabs.sigma2);
    p.ratioFactor = 1.5f * h->scaleFactor;      // LocalMapping.cc:424, a float product
    p.mb = mb; p.mbf = mbf; p.thFarPoints = th_far_points; p.farPoints = far_points ? 1 : 0; p.mono = d_u_right ? 0 : 1;
    p.nlevels = std::max(1, std::min(h->nlevels, (int)kMaxLevels));
    p.capacity = capacity; p.listCapacity = capacity;
    p.kf1First = kf1_first; p.kf1Step = kf1_step; p.kf2First = kf2_first; p.kf2Step = kf2_step;
    {
        Prof pr(h, S_FRAME);
        launchNewMapPoints(h->stream, false, d_pairs, d_n_matches, d_poses, (const Keypoint*)d_kps_un, (const Keypoint*)d_kps, d_u_right, d_depth,
                           d_n_out, p, d_exit, d_x3d, d_n_new, d_mark1, d_mark2, n_pairs, ldsPolluter(h));
    }
    return finishLaunch(h);
}

int orbx_update_map_points_device(orbx_handle* h, int n_points, const int* d_obs_off, const int* d_obs, const uint8_t* d_obs_flags,
                                  const int* d_ref, const int* d_slot, const float* d_mp_world, const float* d_poses, int n_frames,
                                  const orbx_keypoint* d_kps_un, const uint8_t* d_desc, const int* d_n_out, int capacity, int nlevels, int what,
                                  uint8_t* d_mp_desc, float* d_mp_normal, float* d_mp_dist, int* d_best, int* d_best_median, uint8_t* d_status) {
    if (!h) return ORBX_ERR_BAD_ARGUMENT;
    // d_obs_flags and d_slot may be NULL
    if (!d_obs_off || !d_obs || !d_ref || !d_mp_world || !d_poses || !d_kps_un || !d_desc || !d_n_out || !d_mp_desc || !d_mp_normal ||
        !d_mp_dist || !d_best || !d_best_median || !d_status || capacity < 1 || n_frames < 1 || n_points < 0 || badUpdateWhat(what))
        return fail(h, ORBX_ERR_BAD_ARGUMENT, "null pointer, capacity/n_frames < 1, negative n_points or what outside 1 .. 3");
    if (int rc = sameLevels(h, nlevels)) return rc;
    if (n_points == 0) return ORBX_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    MapPointUpdateParams p{};
    levelsOnly(p.scale, h->tabs.scale, h->nlevels);
    p.nlevels = h->nlevels; p.capacity = capacity; p.nFrames = n_frames; p.nPoints = n_points; p.what = what;
    const MapPointUpdateArrays a{d_obs_off, d_obs, d_obs_flags, d_ref, d_slot, d_mp_world, d_poses, (const Keypoint*)d_kps_un, d_desc, d_n_out,
                                 d_mp_desc, d_mp_normal, d_mp_dist, d_best, d_best_median, d_status};
    {
        Prof pr(h, S_FRAME);
        launchMapPointUpdate(h->stream, false, a, p, ldsPolluter(h));
    }
    return finishLaunch(h);
}

}  // extern "C"
