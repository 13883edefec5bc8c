// orbx_predict_scale.cpp - MapPoint::PredictScale (reference src/MapPoint.cc:514-529) on the host, and its form for the device: a table of
// breakpoints.  No HIP here: the file also builds on its own (tests/cpp/predict_scale_sweep.cpp links nothing else).
//   nScale = ceil(log(ratio) / pKF->mfLogScaleFactor), clamped to [0, mnScaleLevels - 1]
// `using namespace std` is in scope there (the unqualified unique_lock<mutex> at :518), ratio and mfLogScaleFactor are float, so log, / and ceil
// are the binary32 overloads; mfLogScaleFactor = log(mfScaleFactor) in binary32 (src/Frame.cc:99).  As a function of ratio this is a monotone
// step function with nlevels - 1 steps.  The steps are found by bisection over float bit patterns WITH THIS EXPRESSION (they sit a few ulp
// above scale_factor^k - 1.20000017, 1.44000018 for 1.2 - so a table of powers would be wrong), and k_fuse only counts breakpoints <= ratio.
#include <cmath>
#include <cstdint>
#include <cstring>

#include "orbx.h"

namespace {
// ceil(log(ratio) / mfLogScaleFactor) before the clamp, as a float: NaN for a negative or NaN ratio, -inf for 0, +inf for +inf
inline float stepsOf(float ratio, float logScaleFactor) { return std::ceil(std::log(ratio) / logScaleFactor); }
inline float fromBits(uint32_t b) { float f; std::memcpy(&f, &b, 4); return f; }
}  // namespace

extern "C" {

int orbx_predict_scale(float max_distance, float dist, float scale_factor, int nlevels) {
    if (nlevels < 1 || !(scale_factor > 1.0f) || !std::isfinite(scale_factor)) return ORBX_ERR_BAD_ARGUMENT;
    const float ratio = max_distance / dist;                                     // MapPoint.cc:519
    const float c = stepsOf(ratio, std::log(scale_factor));                      // :522
    if (!(c >= 0.0f)) return 0;                                                  // :523-524 (and NaN, where the reference's int conversion is undefined)
    if (c >= (float)nlevels) return nlevels - 1;                                 // :525-526 (and +inf)
    return (int)c;
}

int orbx_predict_scale_breakpoints(float scale_factor, int nlevels, float* breakpoints) {
    if (nlevels < 1 || !(scale_factor > 1.0f) || !std::isfinite(scale_factor) || (nlevels > 1 && !breakpoints)) return ORBX_ERR_BAD_ARGUMENT;
    const float logScaleFactor = std::log(scale_factor);
    if (!(logScaleFactor > 0.0f)) return ORBX_ERR_BAD_ARGUMENT;
    for (int k = 1; k < nlevels; k++) {
        uint32_t lo = 0u, hi = 0x7f800000u;      // ratio 0 gives -inf (below every k), +inf gives +inf (not below any)
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (stepsOf(fromBits(mid), logScaleFactor) >= (float)k) hi = mid; else lo = mid;
        }
        breakpoints[k - 1] = fromBits(hi);
    }
    return ORBX_OK;
}

}  // extern "C"
