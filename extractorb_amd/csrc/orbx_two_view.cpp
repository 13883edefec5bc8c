// orbx_two_view.cpp - the C ABI of the monocular initialisation's reconstruction (include/orbx.h): TwoViewReconstruction::Reconstruct on
// the match tables of orbx_search_for_initialization_device (k_two_view.hip).  Thin, as the entries of orbx_rows.cpp are: argument checks
// through orbx_entry.hpp, the workspace through growDevice, the parameter block, one launch wrapper.  A file of its own: tests/
// test_entry_rejections_gpu.py holds a table of exactly the *_device entries of orbx_rows.cpp, and the rejections of the entry here are
// held by tests/test_two_view_rejections_gpu.py.  No CPU path.
#include "orbx_internal.hpp"

extern "C" {

int orbx_reconstruct_two_views_device(orbx_handle* h, int n_pairs, int frame1_first, int frame1_step, int frame2_first, int frame2_step,
                                      const orbx_keypoint* d_kps_un, const int* d_n_out, int capacity, int* d_matches12,
                                      int* d_n_matches, const orbx_camera* cam, float sigma, int iterations, float min_parallax,
                                      int min_triangulated, float rh_threshold, const int* d_rand, int prune,
                                      orbx_two_view_result* d_result, float* d_p3d, uint8_t* d_triangulated) {
    static_assert(sizeof(orbx_two_view_result) == 224, "orbx_two_view_result layout");
    if (!h) return ORBX_ERR_BAD_ARGUMENT;
    // written so that a NaN sigma or threshold is refused
    if (!d_kps_un || !d_n_out || !d_matches12 || !d_n_matches || !cam || !d_rand || !d_result || !d_p3d || !d_triangulated || capacity < 1 ||
        n_pairs < 1 || negativeFirstOrStep(frame1_first, frame1_step) || negativeFirstOrStep(frame2_first, frame2_step) || iterations < 1 ||
        iterations > kTvMaxIterations || !(sigma > 0.0f) || !(rh_threshold > 0.0f && rh_threshold < 1.0f) ||
        (long long)n_pairs * 2 * iterations > 0x7fffffffLL)
        return fail(h, ORBX_ERR_BAD_ARGUMENT, "null pointer, capacity/n_pairs < 1, negative frame index/step, iterations outside 1 .. 4096, sigma <= 0, "
                                              "rh_threshold outside (0, 1) or more than 2^31 - 1 workgroups");
    HIP_TRY(h, hipSetDevice(h->device));
    const size_t pairs = (size_t)n_pairs, cap = (size_t)capacity, iters = (size_t)iterations;
    if (pairs > h->twoView.pairs || cap > h->twoView.cap || iters > h->twoView.iters) {
        const orbx_handle::TwoViewShape want{std::max(pairs, h->twoView.pairs), std::max(cap, h->twoView.cap), std::max(iters, h->twoView.iters)};
        TvWork& w = h->twoViewWork;
        const size_t entries = want.pairs * want.cap, hyps = want.pairs * 2 * want.iters;
        if (int rc = growDevice(h, h->twoView, want,
                                {{(void**)&w.prep, want.pairs * sizeof(TvPrep)}, {(void**)&w.first, entries * sizeof(int)},
                                 {(void**)&w.second, entries * sizeof(int)}, {(void**)&w.score, hyps * sizeof(float)},
                                 {(void**)&w.mats, hyps * 9 * sizeof(float)}, {(void**)&w.inl, entries}, {(void**)&w.counted, entries},
                                 {(void**)&w.cosv, entries * sizeof(float)}}))
            return rc;
    }
    TwoViewParams p{};
    fillPinhole(p, *cam);
    p.sigma = sigma; p.minParallax = min_parallax; p.rhThreshold = rh_threshold;
    p.iterations = iterations; p.minTriangulated = min_triangulated; p.prune = prune != 0; p.capacity = capacity;
    p.f1First = frame1_first; p.f1Step = frame1_step; p.f2First = frame2_first; p.f2Step = frame2_step;
    {
        Prof pr(h, S_FRAME);
        launchTwoView(h->stream, (const Keypoint*)d_kps_un, d_n_out, d_matches12, d_n_matches, d_rand, p, h->twoViewWork, d_result, d_p3d,
                      d_triangulated, n_pairs, ldsPolluter(h));
    }
    return finishLaunch(h);
}

}  // extern "C"
