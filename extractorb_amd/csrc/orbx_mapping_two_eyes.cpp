// orbx_mapping_two_eyes.cpp - the C ABI of the mapping thread's matchers on TWO-CAMERA keyframes (NLeft != -1; include/orbx.h): the search half
// of ORBmatcher::Fuse with bRight false and true (k_fuse_two_eyes.hip), SearchForTriangulation on such keyframes and the KannalaBrandt8
// unprojection and triangulation it stands on (k_triangulate_match_two_eyes.hip), and the two-camera Frame constructor's
// ComputeStereoFishEyeMatches, which stands on the same camera header (k_stereo_fisheye.hip), and the two-camera form of CreateNewMapPoints'
// triangulation loop (k_new_map_points.hip; its one-camera form is orbx_mapping.cpp), and the two-camera form of the MapPoint update
// (k_map_point_update.hip; tests/test_map_point_update_gpu.py holds its rejections).  Thin, as the entries of orbx_rows.cpp are: argument
// checks, the parameter block, a memset of the counters asked for and one launch.  The checks and fills are orbx_entry.hpp's and
// orbx_internal.hpp's.  A file of its own: tests/test_entry_rejections_gpu.py holds a table of exactly the *_device entries of orbx_rows.cpp,
// and the rejections of the entries here are held by tests/test_fuse_two_eyes_gpu.py, tests/test_search_triangulation_two_eyes_gpu.py and
// tests/test_stereo_fisheye_gpu.py.
// No CPU path.
#include "orbx_internal.hpp"

extern "C" {

int orbx_fuse_two_eyes_device(orbx_handle* h, int n_pairs, int kf_first, int kf_step, int mp_first, int mp_step, const float* d_mp_world,
                              const float* d_mp_normal, const float* d_mp_dist, const uint8_t* d_mp_desc, const int* d_n_mp, int mp_capacity,
                              const uint8_t* d_mp_flags, const float* d_poses, const float* tlr12, const orbx_camera_kb8* cam_left,
                              const orbx_camera_kb8* cam_right, const orbx_keypoint* d_kps, const uint8_t* d_desc, const int* d_n_out,
                              int capacity, const int* d_grid_off, const int* d_grid_idx, const float* bounds4, int nlevels, float th,
                              int th_low, int reproj_check, int eyes, int* d_best_idx, int* d_best_dist, uint8_t* d_exit, int* d_n_fused) {
    if (!h) return ORBX_ERR_BAD_ARGUMENT;
    // d_n_mp and d_exit may be NULL
    if (!d_mp_world || !d_mp_normal || !d_mp_dist || !d_mp_desc || !d_mp_flags || !d_poses || !tlr12 || !cam_left || !cam_right || !d_kps ||
        !d_desc || !d_n_out || !d_grid_off || !d_grid_idx || !bounds4 || !d_best_idx || !d_best_dist || !d_n_fused || capacity < 1 ||
        mp_capacity < 1 || n_pairs < 1 || n_pairs > 65535 || negativeWalk(kf_first, kf_step, n_pairs) || negativeWalk(mp_first, mp_step, n_pairs) ||
        th_low < 0 || emptyBounds(bounds4) || badFuseEyes(eyes, reproj_check))
        return fail(h, ORBX_ERR_BAD_ARGUMENT, "null pointer, capacity/mp_capacity/n_pairs < 1, more than 65535 pairs, a negative rig or list index, "
                                              "negative th_low, empty bounds, eyes outside 1 .. 3 or reproj_check = 0 with eyes != 1");
    if (int rc = sameLevels(h, nlevels)) return rc;
    if (int rc = ensureScaleBreaks(h)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    FuseTwoEyesParams p{};
    fillKb8(p.cam[0], *cam_left);         // mpCamera, mpCamera2 (ORBmatcher.cc:1409, :1416)
    fillKb8(p.cam[1], *cam_right);
    fillBoundsTruncated(p, bounds4);      // a KeyFrame's bounds and the Frame's inverses, as orbx_fuse_device; the same for both eyes
    fillGridInverses(p, bounds4);
    levelsOnly(p.scale, h->tabs.scale, h->nlevels);
    levelsOnly(p.invSigma2, h->tabs.invSigma2, h->nlevels);
    fillBreaks(p, h->scaleBreaks, h->nlevels);
    for (int i = 0; i < 12; i++) p.tlr[i] = tlr12[i];
    p.th = th; p.nlevels = h->nlevels; p.thLow = clampDistance(th_low); p.reprojCheck = reproj_check ? 1 : 0; p.eyes = eyes;
    p.capacity = capacity; p.mpCapacity = mp_capacity; p.kfFirst = kf_first; p.kfStep = kf_step; p.mpFirst = mp_first; p.mpStep = mp_step;
    {
        Prof pr(h, S_FRAME);
        // the counters of the eyes asked for: [p*2 + eye]; those of an eye not asked for stay what they are
        if (eyes == 3) HIP_TRY(h, hipMemsetAsync(d_n_fused, 0, sizeof(int) * 2 * (size_t)n_pairs, h->stream));
        else HIP_TRY(h, hipMemset2DAsync(d_n_fused + (eyes - 1), 2 * sizeof(int), 0, sizeof(int), (size_t)n_pairs, h->stream));
        launchFuseTwoEyes(h->stream, d_mp_world, d_mp_normal, d_mp_dist, d_mp_desc, d_n_mp, d_mp_flags, d_poses, (const Keypoint*)d_kps, d_desc,
                          d_n_out, d_grid_off, d_grid_idx, p, d_best_idx, d_best_dist, d_exit, d_n_fused, n_pairs, ldsPolluter(h));
    }
    return finishLaunch(h);
}

int orbx_search_for_triangulation_two_eyes_device(orbx_handle* h, int n_pairs, int kf1_first, int kf1_step, int kf2_first, int kf2_step,
                                                  const uint32_t* d_feat_nodes, const uint32_t* d_feat_idx, const int* d_n_feat,
                                                  const uint8_t* d_kf1_mp_flags, const uint8_t* d_kf2_mp_flags, const float* d_poses,
                                                  const float* tlr12, const orbx_camera_kb8* cam_left, const orbx_camera_kb8* cam_right,
                                                  const orbx_keypoint* d_kps, const uint8_t* d_desc, const int* d_n_out, int capacity, int nlevels,
                                                  int only_stereo, int coarse, int th_low, int check_orientation, int* d_matches12, int* d_pairs,
                                                  int* d_n_matches) {
    if (!h) return ORBX_ERR_BAD_ARGUMENT;
    if (!d_feat_nodes || !d_feat_idx || !d_n_feat || !d_kf1_mp_flags || !d_kf2_mp_flags || !d_poses || !tlr12 || !cam_left || !cam_right ||
        !d_kps || !d_desc || !d_n_out || !d_matches12 || !d_pairs || !d_n_matches || capacity < 1 || n_pairs < 1 ||
        negativeWalk(kf1_first, kf1_step, n_pairs) || negativeWalk(kf2_first, kf2_step, n_pairs))
        return fail(h, ORBX_ERR_BAD_ARGUMENT, "null pointer, capacity/n_pairs < 1 or a negative rig index");
    if (int rc = sameLevels(h, nlevels)) return rc;
    if (!fitsLds(triMatchTwoEyesLdsBytes(capacity, false)))
        return fail(h, ORBX_ERR_UNSUPPORTED, "capacity too large for the LDS-resident two-camera triangulation search (62 bytes per slot of the "
                                             "per-eye capacity rounded up to 16, + 1024: 160 KB per CU)");
    HIP_TRY(h, hipSetDevice(h->device));
    TriMatchTwoEyesParams p{};
    fillKb8(p.cam[0], *cam_left);         // mpCamera, mpCamera2 of both keyframes (one rig)
    fillKb8(p.cam[1], *cam_right);
    levelsWholeTable(p.sigma2, h->tabs.sigma2);
    for (int i = 0; i < 12; i++) p.tlr[i] = tlr12[i];
    p.nlevels = std::max(1, std::min(h->nlevels, (int)kMaxLevels));
    p.thLow = th_low; p.checkOrientation = check_orientation ? 1 : 0; p.onlyStereo = only_stereo ? 1 : 0; p.coarse = coarse ? 1 : 0;
    p.capacity = capacity; p.kf1First = kf1_first; p.kf1Step = kf1_step; p.kf2First = kf2_first; p.kf2Step = kf2_step;
    const bool stage = fitsLds(triMatchTwoEyesLdsBytes(capacity, true));
    {
        Prof pr(h, S_FRAME);
        launchSearchTriangulationTwoEyes(h->stream, d_feat_nodes, d_feat_idx, d_n_feat, d_kf1_mp_flags, d_kf2_mp_flags, d_poses, (const Keypoint*)d_kps,
                                         d_desc, d_n_out, p, stage, d_matches12, d_pairs, d_n_matches, n_pairs, ldsPolluter(h));
    }
    return finishLaunch(h);
}

int orbx_kb8_unproject_device(orbx_handle* h, int n, const float* d_uv, const orbx_camera_kb8* cam, float* d_rays) {
    if (!h) return ORBX_ERR_BAD_ARGUMENT;
    if (!d_uv || !cam || !d_rays || n < 1) return fail(h, ORBX_ERR_BAD_ARGUMENT, "null pointer or n < 1");
    HIP_TRY(h, hipSetDevice(h->device));
    float k[8];
    fillKb8(k, *cam);
    {
        Prof pr(h, S_FRAME);
        launchKb8Unproject(h->stream, d_uv, k, n, d_rays, ldsPolluter(h));
    }
    return finishLaunch(h);
}

int orbx_kb8_triangulate_device(orbx_handle* h, int n, const float* d_kp1, const float* d_kp2, const orbx_camera_kb8* cam1,
                                const orbx_camera_kb8* cam2, const float* r12_9, const float* t12_3, float sigma1, float sigma2, float* d_z,
                                float* d_x3d) {
    if (!h) return ORBX_ERR_BAD_ARGUMENT;
    if (!d_kp1 || !d_kp2 || !cam1 || !cam2 || !r12_9 || !t12_3 || !d_z || !d_x3d || n < 1)
        return fail(h, ORBX_ERR_BAD_ARGUMENT, "null pointer or n < 1");
    HIP_TRY(h, hipSetDevice(h->device));
    Kb8TriangulateParams p{};
    fillKb8(p.cam1, *cam1);
    fillKb8(p.cam2, *cam2);
    for (int i = 0; i < 9; i++) p.R12[i] = r12_9[i];
    for (int i = 0; i < 3; i++) p.t12[i] = t12_3[i];
    p.sigma1 = sigma1; p.sigma2 = sigma2; p.n = n;
    {
        Prof pr(h, S_FRAME);
        launchKb8Triangulate(h->stream, d_kp1, d_kp2, p, d_z, d_x3d, ldsPolluter(h));
    }
    return finishLaunch(h);
}

int orbx_stereo_fisheye_match_device(orbx_handle* h, int n_rigs, int rig_first, int rig_step, const orbx_keypoint* d_kps, const uint8_t* d_desc,
                                     const int* d_n_out, const int* d_mono_out, int capacity, const float* tlr12, const orbx_camera_kb8* cam_left,
                                     const orbx_camera_kb8* cam_right, int nlevels, int* d_left_to_right, int* d_right_to_left, float* d_depth,
                                     float* d_x3d, int* d_n_matches, int* d_n_desc_matches) {
    if (!h) return ORBX_ERR_BAD_ARGUMENT;
    // d_n_desc_matches may be NULL.  The grid folds the rigs into x: n_rigs times the workgroups of a rig has to fit a launch
    if (!d_kps || !d_desc || !d_n_out || !d_mono_out || !tlr12 || !cam_left || !cam_right || !d_left_to_right || !d_right_to_left || !d_depth ||
        !d_x3d || !d_n_matches || capacity < 1 || n_rigs < 1 || negativeWalk(rig_first, rig_step, n_rigs) ||
        (long long)n_rigs * stereoFisheyeTiles(capacity) > 0x7fffffffLL)
        return fail(h, ORBX_ERR_BAD_ARGUMENT, "null pointer, capacity/n_rigs < 1, a negative rig index or more than 2^31 - 1 workgroups");
    if (int rc = sameLevels(h, nlevels)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    StereoFisheyeParams p{};
    fillKb8(p.cam[0], *cam_left);         // mpCamera, mpCamera2 (Frame.cc:1169)
    fillKb8(p.cam[1], *cam_right);
    levelsWholeTable(p.sigma2, h->tabs.sigma2);
    for (int r = 0; r < 3; r++) {         // mRlr, mtlr (Frame.cc:1100-1101), handed to TriangulateMatches as they are
        for (int c = 0; c < 3; c++) p.R12[3 * r + c] = tlr12[4 * r + c];
        p.t12[r] = tlr12[4 * r + 3];
    }
    p.nlevels = std::max(1, std::min(h->nlevels, (int)kMaxLevels));
    p.capacity = capacity; p.rigFirst = rig_first; p.rigStep = rig_step;
    {
        Prof pr(h, S_FRAME);
        launchStereoFisheye(h->stream, (const Keypoint*)d_kps, d_desc, d_n_out, d_mono_out, p, d_left_to_right, d_right_to_left, d_depth, d_x3d,
                            d_n_matches, d_n_desc_matches, n_rigs, ldsPolluter(h));
    }
    return finishLaunch(h);
}

int orbx_create_new_map_points_two_eyes_device(orbx_handle* h, int n_pairs, int kf1_first, int kf1_step, int kf2_first, int kf2_step,
                                               const int* d_pairs, const int* d_n_matches, const float* d_poses, const float* tlr12,
                                               const orbx_camera_kb8* cam_left, const orbx_camera_kb8* cam_right, const orbx_keypoint* d_kps,
                                               const int* d_n_out, int capacity, int nlevels, int far_points, float th_far_points,
                                               uint8_t* d_exit, float* d_x3d, int* d_n_new, uint8_t* d_mark1, uint8_t* d_mark2) {
    if (!h) return ORBX_ERR_BAD_ARGUMENT;
    // d_mark1 and d_mark2 may be NULL.  The grid folds the pairs into x: n_pairs times the workgroups of a pair has to fit a launch
    if (!d_pairs || !d_n_matches || !d_poses || !tlr12 || !cam_left || !cam_right || !d_kps || !d_n_out || !d_exit || !d_x3d || !d_n_new ||
        capacity < 1 || capacity > 0x3fffffff || n_pairs < 1 || negativeWalk(kf1_first, kf1_step, n_pairs) ||
        negativeWalk(kf2_first, kf2_step, n_pairs) || (long long)n_pairs * newMapPointsTiles(2 * capacity) > 0x7fffffffLL)
        return fail(h, ORBX_ERR_BAD_ARGUMENT, "null pointer, capacity/n_pairs < 1, a negative rig index or more than 2^31 - 1 workgroups");
    if (int rc = sameLevels(h, nlevels)) return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    NewMapPointsParams p{};
    fillKb8(p.cam[0], *cam_left);         // mpCamera, mpCamera2 of both keyframes (one rig)
    fillKb8(p.cam[1], *cam_right);
    levelsWholeTable(p.scale, h->tabs.scale);
    levelsWholeTable(p.sigma2, h->tabs.sigma2);
    for (int i = 0; i < 12; i++) p.tlr[i] = tlr12[i];
    p.ratioFactor = 1.5f * h->scaleFactor;      // LocalMapping.cc:424, a float product
    p.thFarPoints = th_far_points; p.farPoints = far_points ? 1 : 0; p.mono = 1;      // bStereo1 = bStereo2 = false (:490, :499)
    p.nlevels = std::max(1, std::min(h->nlevels, (int)kMaxLevels));
    p.capacity = capacity; p.listCapacity = 2 * capacity;
    p.kf1First = kf1_first; p.kf1Step = kf1_step; p.kf2First = kf2_first; p.kf2Step = kf2_step;
    {
        Prof pr(h, S_FRAME);
        launchNewMapPoints(h->stream, true, d_pairs, d_n_matches, d_poses, (const Keypoint*)d_kps, nullptr, nullptr, nullptr, d_n_out, p, d_exit,
                           d_x3d, d_n_new, d_mark1, d_mark2, n_pairs, ldsPolluter(h));
    }
    return finishLaunch(h);
}

int orbx_update_map_points_two_eyes_device(orbx_handle* h, int n_points, const int* d_obs_off, const int* d_obs, const uint8_t* d_obs_flags,
                                           const int* d_ref, const int* d_slot, const float* d_mp_world, const float* d_poses,
                                           const float* tlr12, int n_rigs, const orbx_keypoint* d_kps, const uint8_t* d_desc,
                                           const int* d_n_out, int capacity, int nlevels, int what, uint8_t* d_mp_desc, float* d_mp_normal,
                                           float* d_mp_dist, int* d_best, int* d_best_median, uint8_t* d_status) {
    if (!h) return ORBX_ERR_BAD_ARGUMENT;
    // d_obs_flags and d_slot may be NULL
    if (!d_obs_off || !d_obs || !d_ref || !d_mp_world || !d_poses || !tlr12 || !d_kps || !d_desc || !d_n_out || !d_mp_desc || !d_mp_normal ||
        !d_mp_dist || !d_best || !d_best_median || !d_status || capacity < 1 || n_rigs < 1 || n_rigs > 0x3fffffff || n_points < 0 ||
        badUpdateWhat(what))
        return fail(h, ORBX_ERR_BAD_ARGUMENT, "null pointer, capacity/n_rigs < 1, negative n_points or what outside 1 .. 3");
    if (int rc = sameLevels(h, nlevels)) return rc;
    if (n_points == 0) return ORBX_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    MapPointUpdateParams p{};
    levelsOnly(p.scale, h->tabs.scale, h->nlevels);
    for (int i = 0; i < 12; i++) p.tlr[i] = tlr12[i];
    p.nlevels = h->nlevels; p.capacity = capacity; p.nFrames = 2 * n_rigs; p.nPoints = n_points; p.what = what;
    const MapPointUpdateArrays a{d_obs_off, d_obs, d_obs_flags, d_ref, d_slot, d_mp_world, d_poses, (const Keypoint*)d_kps, d_desc, d_n_out,
                                 d_mp_desc, d_mp_normal, d_mp_dist, d_best, d_best_median, d_status};
    {
        Prof pr(h, S_FRAME);
        launchMapPointUpdate(h->stream, true, a, p, ldsPolluter(h));
    }
    return finishLaunch(h);
}

}  // extern "C"
