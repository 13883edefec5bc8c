// k_sim3_decide.hpp - the per-request decision rule of the Sim3 projection search's fixed point (k_project_sim3.hip), as one
// __host__ __device__ function: the settling kernel and the CPU suite's emulated rounds (tests/cpp/sim3_host_check.cpp) run this source.
// A key is (distance << 16 | CSR slot of the keypoint in the keyframe's grid): ascending keys = ascending distance and, among equal
// distances, the reference's visit order (ix outer, iy inner, push order inside a cell), so the smallest key is what the strict "<" of
// reference src/ORBmatcher.cc:570 / :687 keeps.
#pragma once

namespace orbx {

constexpr int kSim3Top = 4;                  // keys k_sim3_window keeps per request (orbx_debug_sim3_search_list_length)
constexpr int kSim3NoKey = 0x7fffffff;       // "no candidate": above every key (a key is below 2^24)

// A DECISION as the settling keeps it per request: a key, with kSim3First set if it is the request's smallest key; kSim3NoKey = none this
// round; kSim3Dead = the request has no key at all and never decides.
constexpr int kSim3Dead = 0x7ffffffe;
constexpr int kSim3First = 1 << 30;
__host__ __device__ inline bool sim3IsNone(int d) { return d >= kSim3Dead; }
__host__ __device__ inline int sim3Slot(int d) { return d & 0xFFFF; }
__host__ __device__ inline int sim3Dist(int d) { return (d >> 16) & 0xFF; }
// The round's shortcut, from the previous decision alone (no key list is read): a dead request stays dead, and a request that holds its
// smallest key keeps it while no j < i decides for that slot - sim3Decide would return keys[0] again.
__host__ __device__ inline bool sim3Stays(int prev, const int* closedBy, int i) {
    return prev == kSim3Dead || (!sim3IsNone(prev) && (prev & kSim3First) && !(closedBy[sim3Slot(prev)] < i));
}

// Request i sees a keypoint closed iff a request j < i currently decides for it: closedBy[slot] = the smallest request index deciding for
// the slot under the decisions of the previous round (INT_MAX: nobody).  keys: the request's kSim3Top smallest keys, ascending, kSim3NoKey
// behind the last; count: how many candidates its window held in all (they all passed the static tests: level, distance bound, not
// occupied on entry).  Returns the key the request decides for, or kSim3NoKey.  *rescan: every key of a TRUNCATED list is closed - the
// answer lies among the candidates the list dropped, and the caller scans the window again under closedBy.
__host__ __device__ inline int sim3Decide(const int (&keys)[kSim3Top], int count, const int* closedBy, int i, bool* rescan) {
    *rescan = false;
    for (int k = 0; k < kSim3Top; k++) {
        if (keys[k] == kSim3NoKey) return kSim3NoKey;
        if (!(closedBy[keys[k] & 0xFFFF] < i)) return keys[k];
    }
    *rescan = count > kSim3Top;
    return kSim3NoKey;
}

}  // namespace orbx
