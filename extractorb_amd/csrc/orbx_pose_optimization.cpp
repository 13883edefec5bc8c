// orbx_pose_optimization.cpp - the C ABI of the tracker's motion-only bundle adjustment (include/orbx.h): Optimizer::PoseOptimization
// (reference src/Optimizer.cc:854-1168) on a batch of frames (k_pose_optimization.hip).  Thin, as orbx_sim3_solver.cpp is: argument checks
// and one launch; no workspace, no table, no CPU path.  The rejections of the entry here are held by tests/test_pose_optimization_gpu.py.
#include "orbx_internal.hpp"

static int g_poseOptLaunches = 0;

extern "C" {

// launches of k_pose_optimization so far in this process: the entry has ONE launch form, one launch per call
int orbx_debug_pose_optimization_launches(void) { return g_poseOptLaunches; }

int orbx_optimize_pose_device(orbx_handle* h, int n_problems, int frame_first, int frame_step, int eyes, const orbx_pose_problem* d_problems,
                              const orbx_keypoint* d_kps, const int* d_n_out, const float* d_u_right, int capacity, const int* d_matches,
                              const float* d_mp_world, int n_map_points, float* d_poses, uint8_t* d_outlier, orbx_pose_result* d_result) {
    static_assert(sizeof(orbx_pose_result) == 120 && sizeof(orbx_pose_problem) == 188, "orbx_pose_result / orbx_pose_problem layout");
    if (!h) return ORBX_ERR_BAD_ARGUMENT;
    if (!d_problems || !d_kps || !d_n_out || !d_matches || !d_mp_world || !d_poses || !d_outlier || !d_result || capacity < 1 || n_problems < 1 ||
        n_map_points < 0 || eyes < 1 || eyes > 2 || (eyes == 2 && d_u_right) || negativeWalk(frame_first, frame_step, n_problems) ||
        (long long)capacity * eyes > 0x7fffffffLL)
        return fail(h, ORBX_ERR_BAD_ARGUMENT, "null pointer, capacity/n_problems < 1, n_map_points < 0, eyes outside 1 .. 2, d_u_right with two eyes, "
                                              "a negative frame index or eyes * capacity above 2^31 - 1");
    HIP_TRY(h, hipSetDevice(h->device));
    const PoseOptParams p{capacity, eyes, n_map_points, h->nlevels, frame_first, frame_step};
    {
        Prof pr(h, S_FRAME);
        launchPoseOptimization(h->stream, d_problems, (const Keypoint*)d_kps, d_n_out, d_u_right, d_matches, d_mp_world, p, d_poses, d_outlier, d_result, n_problems, ldsPolluter(h));
        g_poseOptLaunches++;
    }
    return finishLaunch(h);
}

}  // extern "C"
