// orbx_covisibility.cpp - the C ABI of the covisibility vote and the keyframe redundancy test (include/orbx.h): KeyFrame::UpdateConnections
// (reference src/KeyFrame.cc:388-511), the voting half of Tracking::UpdateLocalKeyFrames (src/Tracking.cc:3030-3102) and the test inside
// LocalMapping::KeyFrameCulling's loop (src/LocalMapping.cc:977-1043) for a batch of subjects (k_covisibility.hip).  Thin, as
// orbx_place_recognition.cpp is: the argument checks, which are plain functions of orbx_entry.hpp (covisBadArgument, covisUnsupported,
// redundancyBadArgument, redundancyUnsupported: the CPU suite runs every rejection), the rank tables through growDevice, one launch wrapper
// each.  tests/test_covisibility_gpu.py holds the same rejections through the C ABI.  No CPU path.
#include "orbx_internal.hpp"

static int g_covisLaunches[3] = {0, 0, 0};

extern "C" {

// launches so far in this process of k_covis_rank (which = 0), k_covis_vote (1) and k_keyframe_redundancy (2): each entry has ONE form - the
// vote both of its kernels once per accepted call, the redundancy test its one
int orbx_debug_covisibility_launches(int which) { return which >= 0 && which <= 2 ? g_covisLaunches[which] : ORBX_ERR_BAD_ARGUMENT; }

int orbx_covisibility_device(orbx_handle* h, int mode, int n_points, const int* d_obs_off, const int* d_obs, const uint8_t* d_mp_flags, int n_frames,
                             const uint8_t* d_kf_flags, const int* d_kf_map_id, const uint64_t* d_kf_key, int n_subjects, const int* d_subject_mp,
                             const int* d_subject_n, int capacity, const int* d_subject_kf, const int* d_subject_map_id, int th, int conn_capacity,
                             int* d_counter_kf, int* d_counter_w, int* d_ordered_kf, int* d_ordered_w, orbx_covis_result* d_result) {
    static_assert(sizeof(orbx_covis_result) == 20, "orbx_covis_result layout");
    if (!h) return ORBX_ERR_BAD_ARGUMENT;
    if (covisBadArgument(mode, n_points, d_obs_off, d_obs, d_mp_flags, n_frames, d_kf_flags, d_kf_map_id, d_kf_key, n_subjects, d_subject_mp, d_subject_n,
                         capacity, d_subject_kf, d_subject_map_id, conn_capacity, d_counter_kf, d_counter_w, d_ordered_kf, d_ordered_w, d_result))
        return fail(h, ORBX_ERR_BAD_ARGUMENT, "null pointer, a mode other than 0 / 1, n_points < 0, n_frames or capacity < 1, n_subjects outside 1 .. 65535, "
                                              "conn_capacity < 0 or more than 2^31 - 1 entries");
    if (covisUnsupported(n_frames))
        return fail(h, ORBX_ERR_UNSUPPORTED, "n_frames above 8192 (the counters and the sort keys do not fit a workgroup's LDS)");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t need = (size_t)n_frames;
    if (need > h->covisFrames)
        if (int rc = growDevice(h, h->covisFrames, need, {{(void**)&h->d_covisRank, need * sizeof(int)}, {(void**)&h->d_covisByRank, need * sizeof(int)},
                                                         {(void**)&h->d_covisDup, (size_t)cvRankBlocks(n_frames) * sizeof(int)}}))
            return rc;
    const bool update = mode == ORBX_COVIS_UPDATE_CONNECTIONS;
    CovisParams p{};
    p.mode = mode; p.nPoints = n_points; p.nFrames = n_frames; p.nSubjects = n_subjects; p.capacity = capacity; p.th = th; p.connCapacity = conn_capacity;
    CovisArrays a{};
    a.obsOff = d_obs_off; a.obs = d_obs; a.mpFlags = d_mp_flags; a.kfFlags = d_kf_flags; a.kfMap = d_kf_map_id; a.kfKey = d_kf_key;
    a.subjectMp = d_subject_mp; a.subjectN = d_subject_n; a.subjectKf = update ? d_subject_kf : nullptr; a.subjectMap = update ? d_subject_map_id : nullptr;
    a.counterKf = d_counter_kf; a.counterW = d_counter_w; a.orderedKf = update ? d_ordered_kf : nullptr; a.orderedW = update ? d_ordered_w : nullptr;
    a.result = d_result; a.wsRank = h->d_covisRank; a.wsByRank = h->d_covisByRank; a.wsDup = h->d_covisDup;
    {
        Prof pr(h, S_FRAME);
        launchCovisibility(h->stream, a, p, ldsPolluter(h));
        g_covisLaunches[0]++;
        g_covisLaunches[1]++;
    }
    return finishLaunch(h);
}

int orbx_keyframe_redundancy_device(orbx_handle* h, int n_points, const int* d_obs_off, const int* d_obs, const uint8_t* d_mp_flags, const int* d_mp_nobs,
                                    int n_frames, const uint8_t* d_kf_flags, const orbx_keypoint* d_kps_un, const int* d_n_out, const float* d_depth,
                                    const float* d_th_depth, int n_subjects, const int* d_subject_mp, const int* d_subject_n, int capacity,
                                    const int* d_subject_kf, int monocular, int th_obs, float redundant_th, orbx_redundancy_result* d_result,
                                    uint8_t* d_slot_state) {
    static_assert(sizeof(orbx_redundancy_result) == 16, "orbx_redundancy_result layout");
    if (!h) return ORBX_ERR_BAD_ARGUMENT;
    if (redundancyBadArgument(n_points, d_obs_off, d_obs, d_mp_flags, n_frames, d_kf_flags, d_kps_un, d_n_out, d_depth, d_th_depth, n_subjects, d_subject_mp,
                              d_subject_n, capacity, d_subject_kf, monocular, redundant_th, d_result))
        return fail(h, ORBX_ERR_BAD_ARGUMENT, "null pointer, n_points < 0, n_frames or capacity < 1, n_subjects outside 1 .. 65535 or more than 2^31 - 1 slots, "
                                              "a NaN redundant_th");
    if (redundancyUnsupported(capacity))
        return fail(h, ORBX_ERR_UNSUPPORTED, "capacity above 163280 (the slot states do not fit a workgroup's LDS)");
    HIP_TRY(h, hipSetDevice(h->device));
    CovisParams p{};
    p.nPoints = n_points; p.nFrames = n_frames; p.nSubjects = n_subjects; p.capacity = capacity; p.monocular = monocular ? 1 : 0; p.thObs = th_obs;
    p.redundantTh = redundant_th;
    CovisArrays a{};
    a.obsOff = d_obs_off; a.obs = d_obs; a.mpFlags = d_mp_flags; a.mpNobs = d_mp_nobs; a.kfFlags = d_kf_flags; a.kpsUn = (const Keypoint*)d_kps_un;
    a.nOut = d_n_out; a.depth = monocular ? nullptr : d_depth; a.thDepth = monocular ? nullptr : d_th_depth; a.subjectMp = d_subject_mp;
    a.subjectN = d_subject_n; a.subjectKf = d_subject_kf; a.result = d_result; a.slotState = d_slot_state;
    {
        Prof pr(h, S_FRAME);
        launchKeyFrameRedundancy(h->stream, a, p, ldsPolluter(h));
        g_covisLaunches[2]++;
    }
    return finishLaunch(h);
}

}  // extern "C"
