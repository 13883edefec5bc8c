// predict_scale_sweep.cpp - orbx_predict_scale_breakpoints against orbx_predict_scale (MapPoint::PredictScale, reference src/MapPoint.cc:514-529)
// over EVERY float of a range, for the three pyramids the tests use.  Stand-alone: it links extractorb_amd/csrc/orbx_predict_scale.cpp and
// nothing else (no HIP), so it also builds and runs under -fsanitize=address,undefined as a host program.
//   predict_scale_sweep          every float from 0.5 to twice the last breakpoint (about 3e7 per pyramid)
//   predict_scale_sweep RADIUS   RADIUS floats on either side of every breakpoint
// One line per pyramid; exit status 1 on any mismatch or any step down.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "orbx.h"

static uint32_t bitsOf(float f) { uint32_t b; std::memcpy(&b, &f, 4); return b; }
static float floatOf(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }

int main(int argc, char** argv) {
    const long radius = argc > 1 ? std::atol(argv[1]) : 0;
    const struct { float scale; int levels; } pyramids[] = {{1.2f, 8}, {1.1f, 12}, {2.0f, 4}};
    int bad = 0;
    for (const auto& py : pyramids) {
        std::vector<float> bp(py.levels - 1);
        if (orbx_predict_scale_breakpoints(py.scale, py.levels, bp.data()) != ORBX_OK) { std::printf("no breakpoints for %g\n", py.scale); return 2; }
        std::vector<std::pair<uint32_t, uint32_t>> ranges;      // inclusive bit ranges of positive floats
        if (radius > 0)
            for (float b : bp) ranges.push_back({bitsOf(b) - (uint32_t)radius, bitsOf(b) + (uint32_t)radius});
        else
            ranges.push_back({bitsOf(0.5f), bitsOf(2.0f * bp.back())});
        long floats = 0, mismatches = 0, stepsDown = 0;
        for (const auto& r : ranges) {
            int last = -1;
            for (uint32_t b = r.first; b <= r.second; b++) {
                const float ratio = floatOf(b);
                int byTable = 0;
                for (float x : bp) byTable += ratio >= x ? 1 : 0;
                const int byExpression = orbx_predict_scale(ratio, 1.0f, py.scale, py.levels);
                mismatches += byTable != byExpression;
                stepsDown += byExpression < last;
                last = byExpression;
                floats++;
            }
        }
        std::printf("scale %g levels %d floats %ld mismatches %ld non-monotone %ld\n", py.scale, py.levels, floats, mismatches, stepsDown);
        bad |= mismatches != 0 || stepsDown != 0;
    }
    return bad;
}
