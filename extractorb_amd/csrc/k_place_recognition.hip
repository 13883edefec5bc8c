// k_place_recognition.hip - KeyFrameDatabase::DetectNBestCandidates and DetectRelocalizationCandidates (reference src/KeyFrameDatabase.cc
// :612-780, :783-895) for a batch of queries: TWO kernels.  What they compute is k_place_recognition.hpp's, which the CPU suite compiles for
// the host.
//   k_place_pairs   grid (ceil(n_db / rows), n_queries), four waves; rows = 4 .. 32 by the size of the call (orbx_params.hpp: prPairRows).
//                   The workgroup stages its query's weights and word ids in LDS (12 bytes a word); a wave takes database rows w, w + 4, ..
//                   of the workgroup's and runs prPair: 64 of the row's ids per step, each lane a binary search in the staged ids, the hits
//                   by ballot, the terms by a sequential chain of v_readlane reads.  Lane 0 writes the pair's shared-word count, smallest
//                   shared id and score into the handle's workspace;
//   k_place_query   one workgroup of 256 lanes per query runs prQuery: the maximum and the threshold, the score write-back, the scored rows
//                   sorted by (smallest shared word, row) - a bitonic sort of 64-bit keys in LDS -, the neighbour accumulation a list entry
//                   per lane, then the selection: an ordered compaction (RELOCALIZATION) or a second sort, by descending accumulated score
//                   and list position, and the walk as two ordered counts (N_BEST).  12 bytes per list slot and 4 per row of LDS.
// No launch depends on the data: every list has room for all n_db rows.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orbx_lds_pollute.hpp"
#include "k_place_recognition.hpp"

namespace orbx {

__global__ __launch_bounds__(kPrThreads) void k_place_pairs(PlaceArrays a, PlaceParams p) {
    ORBX_DYNAMIC_LDS(lds);
    double* sW = (double*)lds;
    uint32_t* sIds = (uint32_t*)(lds + (size_t)8 * p.qCapacity);
    const int q = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long frame = p.qFirst + (long long)q * p.qStep;
    const int nq = prClampWords(a.qN[frame], p.qCapacity);
    for (int i = tid; i < nq; i += kPrThreads) {
        sW[i] = a.qW[frame * p.qCapacity + i];
        sIds[i] = a.qIds[frame * p.qCapacity + i];
    }
    __syncthreads();
    const int k0 = blockIdx.x * p.pairRows, k1 = k0 + p.pairRows < p.nDb ? k0 + p.pairRows : p.nDb;
    for (int k = k0 + wave; k < k1; k += kPrThreads / 64) {
        int words;
        uint32_t first;
        float score;
        prPair(lane, sIds, sW, nq, a.dbIds + (size_t)k * p.capacity, a.dbW + (size_t)k * p.capacity, prClampWords(a.dbN[k], p.capacity), words, first, score);
        if (lane == 0) {
            const size_t at = (size_t)q * p.nDb + k;
            a.wsWords[at] = words; a.wsFirst[at] = first; a.wsScore[at] = score;
            if (a.commonWords) a.commonWords[at] = words;
        }
    }
}

__global__ __launch_bounds__(kPrThreads) void k_place_query(PlaceArrays a, PlaceParams p) {
    ORBX_DYNAMIC_LDS(lds);
    prQuery(threadIdx.x, blockIdx.x, a, p, lds);
}

void launchPlaceRecognition(hipStream_t st, const PlaceArrays& a, const PlaceParams& p, LdsPolluter pollute) {
    if (p.nDb > 0) {
        pollute(st);
        hipLaunchKernelGGL(k_place_pairs, dim3((unsigned)((p.nDb + p.pairRows - 1) / p.pairRows), (unsigned)p.nQueries), dim3(kPrThreads),
                           prPairLdsBytes(p.qCapacity), st, a, p);
    }
    pollute(st);
    hipLaunchKernelGGL(k_place_query, dim3((unsigned)p.nQueries), dim3(kPrThreads), prQueryLdsBytes(p.nDb), st, a, p);
}

}  // namespace orbx
