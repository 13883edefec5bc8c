// entry_check.cpp - extractorb_amd/csrc/orbx_entry.hpp (the entry points' predicates, parameter fills, level-table padding rules and the
// all-or-nothing regrow) compiled for the HOST behind tests/cpp/host_shim as a stand-alone program.  tests/test_entry_helpers.py feeds it cases
// on standard input, one per line, and compares the answers with an independent statement.  Floats travel as their bit patterns (hexadecimal).
//   K                                -> kLdsBudget kBowMatchLdsBudget kMaxLevels
//   P first step n                   -> negativeWalk negativeFirstOrStep
//   E b0 b1 b2 b3                    -> emptyBounds
//   C d                              -> clampDistance
//   L bytes                          -> fitsLds
//   G b0 b1 b2 b3                    -> minX minY wInv hInv of fillGrid, then wInv hInv of fillGridInverses alone
//   B b0 b1 b2 b3                    -> minX maxX minY maxY of fillBounds, then of fillBoundsTruncated
//   Q c0 .. c8                       -> fx fy cx cy of fillPinhole (orbx_camera), then the eight of fillKb8 (orbx_camera_kb8 from c0 .. c7)
//   T rule nlevels s0 .. s15         -> the sixteen elements of a zeroed table after rule 1 (padded with one), 2 (padded with the last level),
//                                       3 (the whole table) or 4 (the levels only)
//   R nlevels r0 .. r15              -> the sixteen breaks of a zeroed block after fillBreaks
//   W k s0 s1 s2                     -> regrow of three items that hold old buffers, with an allocator that fails on its k-th call (0: never):
//                                       result, non-null pointers, live new buffers, frees of each old buffer (three), sizes of what the items hold
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

#include "../../extractorb_amd/csrc/orbx_entry.hpp"

using namespace orbx;

static float bitsToFloat(unsigned u) { float f; std::memcpy(&f, &u, 4); return f; }
static unsigned floatToBits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }
static bool readFloats(float* dst, int n) {
    for (int i = 0; i < n; i++) { unsigned u; if (std::scanf("%x", &u) != 1) return false; dst[i] = bitsToFloat(u); }
    return true;
}
static void printFloats(const float* v, int n, char last) {
    for (int i = 0; i < n; i++) std::printf("%08x%c", floatToBits(v[i]), i + 1 < n ? ' ' : last);
}

struct Block {      // the fields the fills name, as the parameter blocks of orbx_params.hpp spell them
    float fx, fy, cx, cy, minX, maxX, minY, maxY, wInv, hInv;
    float breaks[kMaxLevels];
};

// the counting allocator of the regrow cases: real heap blocks, so that the sanitizer sees a leak, a double free or a free of a stranger
static std::map<void*, size_t> g_live;
static int g_allocCalls = 0, g_failAt = 0;
static std::map<void*, int> g_freed;
static bool fakeAlloc(void** p, size_t bytes) {
    if (++g_allocCalls == g_failAt) return false;
    *p = std::malloc(bytes ? bytes : 1);
    g_live[*p] = bytes;
    return true;
}
static void fakeFree(void* p) {
    g_freed[p]++;
    g_live.erase(p);
    std::free(p);
}

int main() {
    char op[4];
    while (std::scanf("%3s", op) == 1) {
        if (op[0] == 'K') {
            std::printf("%zu %zu %d\n", kLdsBudget, kBowMatchLdsBudget, (int)kMaxLevels);
        } else if (op[0] == 'P') {
            int first, step, n;
            if (std::scanf("%d %d %d", &first, &step, &n) != 3) return 2;
            std::printf("%d %d\n", (int)negativeWalk(first, step, n), (int)negativeFirstOrStep(first, step));
        } else if (op[0] == 'E') {
            float* b = new float[4];      // exact size: a read past the four bounds is reported by the sanitizer
            if (!readFloats(b, 4)) return 2;
            std::printf("%d\n", (int)emptyBounds(b));
            delete[] b;
        } else if (op[0] == 'C') {
            int d;
            if (std::scanf("%d", &d) != 1) return 2;
            std::printf("%d\n", clampDistance(d));
        } else if (op[0] == 'L') {
            unsigned long long bytes;
            if (std::scanf("%llu", &bytes) != 1) return 2;
            std::printf("%d\n", (int)fitsLds((size_t)bytes));
        } else if (op[0] == 'G') {
            float b[4];
            if (!readFloats(b, 4)) return 2;
            Block p{}, q{};
            fillGrid(p, b);
            fillGridInverses(q, b);
            const float out[6] = {p.minX, p.minY, p.wInv, p.hInv, q.wInv, q.hInv};
            printFloats(out, 6, '\n');
        } else if (op[0] == 'B') {
            float b[4];
            if (!readFloats(b, 4)) return 2;
            Block p{}, q{};
            fillBounds(p, b);
            fillBoundsTruncated(q, b);
            const float out[8] = {p.minX, p.maxX, p.minY, p.maxY, q.minX, q.maxX, q.minY, q.maxY};
            printFloats(out, 8, '\n');
        } else if (op[0] == 'Q') {
            float c[9];
            if (!readFloats(c, 9)) return 2;
            const orbx_camera cam{c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7], c[8]};
            const orbx_camera_kb8 kb{c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]};
            Block p{};
            fillPinhole(p, cam);
            float k[8];
            fillKb8(k, kb);
            const float out[4] = {p.fx, p.fy, p.cx, p.cy};
            printFloats(out, 4, ' ');
            printFloats(k, 8, '\n');
        } else if (op[0] == 'T') {
            int rule, nlevels;
            float src[kMaxLevels], dst[kMaxLevels] = {};
            if (std::scanf("%d %d", &rule, &nlevels) != 2 || !readFloats(src, kMaxLevels)) return 2;
            if (rule == 1) levelsPaddedWithOne(dst, src, nlevels);
            else if (rule == 2) levelsPaddedWithLast(dst, src, nlevels);
            else if (rule == 3) levelsWholeTable(dst, src);
            else if (rule == 4) levelsOnly(dst, src, nlevels);
            else return 2;
            printFloats(dst, kMaxLevels, '\n');
        } else if (op[0] == 'R') {
            int nlevels;
            float src[kMaxLevels];
            if (std::scanf("%d", &nlevels) != 1 || !readFloats(src, kMaxLevels)) return 2;
            Block p{};
            fillBreaks(p, src, nlevels);
            printFloats(p.breaks, kMaxLevels, '\n');
        } else if (op[0] == 'W') {
            unsigned long long size[3];
            if (std::scanf("%d %llu %llu %llu", &g_failAt, &size[0], &size[1], &size[2]) != 4) return 2;
            g_allocCalls = 0; g_live.clear(); g_freed.clear();
            void* item[3];
            void* old[3];
            for (int i = 0; i < 3; i++) item[i] = old[i] = std::malloc(16);
            const bool ok = regrow({{&item[0], (size_t)size[0]}, {&item[1], (size_t)size[1]}, {&item[2], (size_t)size[2]}}, fakeAlloc, fakeFree);
            int nonNull = 0;
            for (void* p : item) nonNull += p != nullptr;
            std::printf("%d %d %zu %d %d %d", (int)ok, nonNull, g_live.size(), g_freed[old[0]], g_freed[old[1]], g_freed[old[2]]);
            for (void* p : item) std::printf(" %lld", p && g_live.count(p) ? (long long)g_live[p] : -1LL);
            std::printf("\n");
            for (void* p : item) if (p) fakeFree(p);      // what a success leaves is the caller's: given back here, so that a leak is regrow's
        } else {
            return 2;
        }
    }
    return 0;
}
