// match_helpers_check.cpp - extractorb_amd/csrc/k_match_helpers.hpp compiled for the HOST (tests/cpp/host_shim/hip/hip_runtime.h stands in for
// the device vocabulary) as a stand-alone program: the shared statements of DescriptorDistance, GetFeaturesInArea's cell window, the rotation
// bin, ComputeThreeMaxima and the sorted key list, called directly.  tests/test_match_helpers.py feeds it cases on standard input, one per
// line, and compares the answers with an independent statement.  Floats travel as their bit patterns (hexadecimal): nothing is rounded on the way.
//   M h0 .. h29                      -> ind1 ind2 ind3
//   B angle1 angle2                  -> bin
//   W u v r minX minY wInv hInv      -> inside minCX maxCX minCY maxCY   (frameCellWindow, built on cellWindowMin / cellWindowMax)
//   I N n k1 .. kn                   -> the N keys after inserting k1 .. kn into a list of N empty (INT_MAX) entries; N is 2 or 4
//   H a0 .. a7 x0 .. x7              -> the Hamming distance of two 256-bit descriptors (eight hexadecimal words each)
//   V frames f capacity  nOut[frames]  gridOff[frames * (kGridCells + 1)]  gridIdx[frames * capacity]  (x y octave)[frames * capacity]
//     u v r level minCX maxCX minCY maxCY
//                                    -> any nIn n s1 idx1 .. sn idxn   (keyFrameView of frame f and keyFrameVisitArea of k_keyframe_project.hpp:
//                                       the (slot, index) pairs in the order the body was called; every table has exactly the size given)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "../../extractorb_amd/csrc/k_keyframe_project.hpp"
#include "../../extractorb_amd/csrc/k_match_helpers.hpp"

using namespace orbx;

static float bitsToFloat(unsigned u) { float f; std::memcpy(&f, &u, 4); return f; }
struct Window { float minX, minY, wInv, hInv; };

template <int N>
static void insertAll(int n) {
    int keys[N];
    for (int t = 0; t < N; t++) keys[t] = 0x7fffffff;
    for (int j = 0; j < n; j++) { int k; if (std::scanf("%d", &k) != 1) std::abort(); sortedInsert(keys, k); }
    for (int t = 0; t < N; t++) std::printf("%d%c", keys[t], t + 1 < N ? ' ' : '\n');
}

int main() {
    char op[4];
    while (std::scanf("%3s", op) == 1) {
        if (op[0] == 'M') {
            int* hist = new int[kHistoLength];      // exact size: a read past the bins is reported by the sanitizer
            for (int i = 0; i < kHistoLength; i++) if (std::scanf("%d", &hist[i]) != 1) return 2;
            const ThreeMaxima m = computeThreeMaxima(hist);
            std::printf("%d %d %d\n", m.ind1, m.ind2, m.ind3);
            delete[] hist;
        } else if (op[0] == 'B') {
            unsigned a, b;
            if (std::scanf("%x %x", &a, &b) != 2) return 2;
            std::printf("%d\n", rotationBin(bitsToFloat(a), bitsToFloat(b)));
        } else if (op[0] == 'W') {
            unsigned v[7];
            for (unsigned& x : v) if (std::scanf("%x", &x) != 1) return 2;
            const Window p{bitsToFloat(v[3]), bitsToFloat(v[4]), bitsToFloat(v[5]), bitsToFloat(v[6])};
            int minCX, maxCX, minCY, maxCY;
            const bool in = frameCellWindow(bitsToFloat(v[0]), bitsToFloat(v[1]), bitsToFloat(v[2]), p, minCX, maxCX, minCY, maxCY);
            std::printf("%d %d %d %d %d\n", (int)in, minCX, maxCX, minCY, maxCY);
        } else if (op[0] == 'I') {
            int N, n;
            if (std::scanf("%d %d", &N, &n) != 2 || (N != 2 && N != 4)) return 2;
            if (N == 2) insertAll<2>(n); else insertAll<4>(n);
        } else if (op[0] == 'H') {
            uint32_t w[16];
            for (uint32_t& x : w) if (std::scanf("%x", &x) != 1) return 2;
            const uint4 a{w[0], w[1], w[2], w[3]}, b{w[4], w[5], w[6], w[7]}, x{w[8], w[9], w[10], w[11]}, y{w[12], w[13], w[14], w[15]};
            std::printf("%d\n", hamming256(a, b, x, y));
        } else if (op[0] == 'V') {
            int frames, f, capacity;
            if (std::scanf("%d %d %d", &frames, &f, &capacity) != 3 || frames < 1 || f < 0 || f >= frames || capacity < 1) return 2;
            // exact sizes, on the heap: a read past any of them is reported by the sanitizer
            int* nOut = new int[frames];
            int* gridOff = new int[(size_t)frames * (kGridCells + 1)];
            int* gridIdx = new int[(size_t)frames * capacity];
            Keypoint* kps = new Keypoint[(size_t)frames * capacity];
            uint8_t* desc = new uint8_t[(size_t)frames * capacity * 32];
            for (int i = 0; i < frames; i++) if (std::scanf("%d", &nOut[i]) != 1) return 2;
            for (int i = 0; i < frames * (kGridCells + 1); i++) if (std::scanf("%d", &gridOff[i]) != 1) return 2;
            for (int i = 0; i < frames * capacity; i++) if (std::scanf("%d", &gridIdx[i]) != 1) return 2;
            for (int i = 0; i < frames * capacity; i++) {
                unsigned x, y;
                int octave;
                if (std::scanf("%x %x %d", &x, &y, &octave) != 3) return 2;
                kps[i] = Keypoint{bitsToFloat(x), bitsToFloat(y), 31.f, 0.f, 0.f, octave, -1};
            }
            unsigned w[3];
            KfProjection q;
            if (std::scanf("%x %x %x %d %d %d %d %d", &w[0], &w[1], &w[2], &q.level, &q.minCX, &q.maxCX, &q.minCY, &q.maxCY) != 8) return 2;
            q.u = bitsToFloat(w[0]); q.v = bitsToFloat(w[1]); q.r = bitsToFloat(w[2]); q.invz = 0.f;
            const KeyFrameView kf = keyFrameView(f, kps, desc, nOut, gridOff, gridIdx, capacity);
            if (kf.nIn != keyFrameSlotsInGrid(f, nOut, gridOff, capacity)) return 3;
            std::vector<int> seen;
            const bool any = keyFrameVisitArea(kf, q, [&](int s, int idx, float kx, float ky) {
                if (kx != kf.K[idx].x || ky != kf.K[idx].y) std::abort();
                seen.push_back(s); seen.push_back(idx);
            });
            std::printf("%d %d %d", (int)any, kf.nIn, (int)seen.size() / 2);
            for (int t : seen) std::printf(" %d", t);
            std::printf("\n");
            delete[] nOut; delete[] gridOff; delete[] gridIdx; delete[] kps; delete[] desc;
        } else {
            return 2;
        }
    }
    return 0;
}
