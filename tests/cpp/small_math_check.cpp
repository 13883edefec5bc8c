// small_math_check.cpp - extractorb_amd/csrc/k_small_math.hpp and the Jacobi pair of k_small_svd.hpp compiled for the HOST
// (tests/cpp/host_shim stands in for the device vocabulary) as a stand-alone program: the draw without replacement, the pair rotation and
// the canonical NaN, called directly.  tests/test_small_math.py feeds it cases on standard input, one per line, and compares the answers
// with an independent statement.  Floats and doubles travel as their bit patterns (hexadecimal): nothing is rounded on the way.
//   D K N r0 .. r(K-1)                        -> idx0 .. idx(K-1)                     (drawSet<K>, K is 3 or 8; r are raw rand() ints)
//   J N ai[N] aj[N] vi[N] vj[N]               -> rotated ai[N] aj[N] vi[N] vj[N]      (jacobiPair<N>, N is 3 or 4)
//   C x                                       -> canonNaN(float x), then quietNaN()
//   E x                                       -> canonNaN(double x)
#include "host_shim/triangulation_two_eyes_shim.h"

#include <cstdio>
#include <cstring>

#include "../../extractorb_amd/csrc/k_small_math.hpp"
#include "../../extractorb_amd/csrc/k_small_svd.hpp"

using namespace orbx;

static float bitsToFloat(unsigned u) { float f; std::memcpy(&f, &u, 4); return f; }
static unsigned floatToBits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }

template <int K>
static int draw(int N) {
    int* raw = new int[K];      // exact size: a read past the values is reported by the sanitizer
    for (int j = 0; j < K; j++) if (std::scanf("%d", &raw[j]) != 1) { delete[] raw; return 2; }
    int idx[K];
    drawSet<K>(raw, N, idx);
    for (int j = 0; j < K; j++) std::printf("%d%c", idx[j], j + 1 < K ? ' ' : '\n');
    delete[] raw;
    return 0;
}

template <int N>
static int pair() {
    float col[4][N];
    for (int a = 0; a < 4; a++)
        for (int k = 0; k < N; k++) { unsigned u; if (std::scanf("%x", &u) != 1) return 2; col[a][k] = bitsToFloat(u); }
    bool rotated = false;
    jacobiPair<N>(col[0], col[1], col[2], col[3], rotated);
    std::printf("%d", (int)rotated);
    for (int a = 0; a < 4; a++)
        for (int k = 0; k < N; k++) std::printf(" %08x", floatToBits(col[a][k]));
    std::printf("\n");
    return 0;
}

int main() {
    char op[4];
    while (std::scanf("%3s", op) == 1) {
        int bad = 0;
        if (op[0] == 'D') {
            int K, N;
            if (std::scanf("%d %d", &K, &N) != 2 || (K != 3 && K != 8)) return 2;
            bad = K == 3 ? draw<3>(N) : draw<8>(N);
        } else if (op[0] == 'J') {
            int N;
            if (std::scanf("%d", &N) != 1 || (N != 3 && N != 4)) return 2;
            bad = N == 3 ? pair<3>() : pair<4>();
        } else if (op[0] == 'C') {
            unsigned u;
            if (std::scanf("%x", &u) != 1) return 2;
            std::printf("%08x %08x\n", floatToBits(canonNaN(bitsToFloat(u))), floatToBits(quietNaN()));
        } else if (op[0] == 'E') {
            unsigned long long u;
            if (std::scanf("%llx", &u) != 1) return 2;
            double d;
            std::memcpy(&d, &u, 8);
            d = canonNaN(d);
            std::memcpy(&u, &d, 8);
            std::printf("%016llx\n", u);
        } else {
            return 2;
        }
        if (bad) return bad;
    }
    return 0;
}
