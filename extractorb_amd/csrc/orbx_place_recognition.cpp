// orbx_place_recognition.cpp - the C ABI of place recognition (include/orbx.h): KeyFrameDatabase::DetectNBestCandidates and
// DetectRelocalizationCandidates (reference src/KeyFrameDatabase.cc:612-780, :783-895; call sites src/LoopClosing.cc:463 and
// src/Tracking.cc:3192) for a batch of queries (k_place_recognition.hip).  Thin, as orbx_sim3_solver.cpp is: the argument checks, which are
// plain functions of orbx_entry.hpp (placeBadArgument, placeUnsupported: the CPU suite runs every rejection), the workspace through
// growDevice, one launch wrapper.  tests/test_place_recognition_gpu.py holds the same rejections through the C ABI.  No CPU path.
#include "orbx_internal.hpp"

static int g_placeLaunches[2] = {0, 0};

extern "C" {

// launches so far in this process of k_place_pairs (which = 0) and k_place_query (which = 1): the entry has ONE form - both kernels once per
// accepted call, k_place_pairs not at all when n_db == 0
int orbx_debug_place_recognition_launches(int which) { return which == 0 || which == 1 ? g_placeLaunches[which] : ORBX_ERR_BAD_ARGUMENT; }

int orbx_detect_candidates_device(orbx_handle* h, const orbx_vocabulary* v, int mode, int n_db, const uint32_t* d_db_word_ids,
                                  const double* d_db_word_weights, const int* d_db_n_words, int capacity, const int* d_db_map_id,
                                  const uint8_t* d_db_flags, const int* d_db_covis, int n_queries, int q_first, int q_step,
                                  const uint32_t* d_q_word_ids, const double* d_q_word_weights, const int* d_q_n_words, int q_capacity,
                                  const int* d_q_map_id, const uint8_t* d_connected, int n_candidates, float* d_score, orbx_place_result* d_result,
                                  int* d_loop, int* d_merge, int* d_cand, int cand_capacity, int* d_common_words) {
    static_assert(sizeof(orbx_place_result) == 32, "orbx_place_result layout");
    if (!h) return ORBX_ERR_BAD_ARGUMENT;
    if (placeBadArgument(v, mode, n_db, d_db_word_ids, d_db_word_weights, d_db_n_words, capacity, d_db_map_id, d_db_flags, d_db_covis, n_queries, q_first,
                         q_step, d_q_word_ids, d_q_word_weights, d_q_n_words, q_capacity, d_q_map_id, n_candidates, d_score, d_result, d_loop, d_merge, d_cand,
                         cand_capacity))
        return fail(h, ORBX_ERR_BAD_ARGUMENT, "null pointer, a mode other than 0 / 1, n_db < 0, n_queries outside 1 .. 65535, capacity/q_capacity < 1, a "
                                              "negative query index, n_candidates outside 0 .. 2^30 - 1, cand_capacity < 0 or more than 2^31 - 1 entries");
    if (vocabularyDeviceIndex(v) != h->device) return fail(h, ORBX_ERR_BAD_ARGUMENT, "the vocabulary lives on another device than the handle");
    if (placeUnsupported(vocabularyScoring(v), n_db, q_capacity))
        return fail(h, ORBX_ERR_UNSUPPORTED, "a scoring other than L1_NORM, n_db above 8192 or q_capacity above 13610 (the lists or the staged query do not "
                                             "fit a workgroup's LDS)");
    HIP_TRY(h, hipSetDevice(h->device));
    const bool nBest = mode == ORBX_PLACE_N_BEST;
    const size_t need = (size_t)n_queries * (size_t)n_db;
    if (need > h->placeEntries)
        if (int rc = growDevice(h, h->placeEntries, need, {{(void**)&h->d_placeWords, need * sizeof(int)}, {(void**)&h->d_placeFirst, need * sizeof(uint32_t)},
                                                          {(void**)&h->d_placeScore, need * sizeof(float)}}))
            return rc;
    const PlaceParams p{mode, n_db, capacity, n_queries, q_first, q_step, q_capacity, nBest ? n_candidates : 0, nBest ? 0 : cand_capacity, prPairRows(n_db, n_queries)};
    const PlaceArrays a{d_db_word_ids, d_db_word_weights, d_db_n_words, d_db_map_id, d_db_flags, d_db_covis, d_q_word_ids, d_q_word_weights, d_q_n_words,
                        d_q_map_id, nBest ? d_connected : nullptr, d_score, d_result, d_loop, d_merge, d_cand, d_common_words,
                        h->d_placeWords, h->d_placeFirst, h->d_placeScore};
    {
        Prof pr(h, S_FRAME);
        launchPlaceRecognition(h->stream, a, p, ldsPolluter(h));
        if (n_db > 0) g_placeLaunches[0]++;
        g_placeLaunches[1]++;
    }
    return finishLaunch(h);
}

}  // extern "C"
