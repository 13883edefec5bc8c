// match_helpers_check.cpp - extractorb_amd/csrc/k_match_helpers.hpp compiled for the HOST (tests/cpp/host_shim/hip/hip_runtime.h stands in for
// the device vocabulary) as a stand-alone program: the shared statements of DescriptorDistance, GetFeaturesInArea's cell window, the rotation
// bin, ComputeThreeMaxima and the sorted key list, called directly.  tests/test_match_helpers.py feeds it cases on standard input, one per
// line, and compares the answers with an independent statement.  Floats travel as their bit patterns (hexadecimal): nothing is rounded on the way.
//   M h0 .. h29                      -> ind1 ind2 ind3
//   B angle1 angle2                  -> bin
//   W u v r minX minY wInv hInv      -> inside minCX maxCX minCY maxCY   (frameCellWindow, built on cellWindowMin / cellWindowMax)
//   I N n k1 .. kn                   -> the N keys after inserting k1 .. kn into a list of N empty (INT_MAX) entries; N is 2 or 4
//   H a0 .. a7 x0 .. x7              -> the Hamming distance of two 256-bit descriptors (eight hexadecimal words each)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>

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
        } else {
            return 2;
        }
    }
    return 0;
}
