// k_rig_two_eyes.hpp - what KeyFrame's getters give for the two eyes of a rig keyframe (reference src/KeyFrame.cc:118, :1232-1262), from the
// rig's pose and mTlr alone.  Shared by the two-camera Fuse (k_fuse_two_eyes.hip) and the two-camera SearchForTriangulation
// (k_triangulate_match_two_eyes.hip).  Plain arithmetic on gemmRow: compiles for the host behind tests/cpp/host_shim.
#pragma once
#include "k_match_helpers.hpp"

namespace orbx {

constexpr int kRigEyeFloats = 15;      // one eye of a rig keyframe: mR (row-major) at 0..8, mt at 9..11, the camera centre at 12..14

// Element j = eye * kRigEyeFloats + k of the two records, from the rig's pose T (3x4 row-major, Rcw | tcw) and mTlr (3x4 row-major).
// eye 0: GetRotation, GetTranslation, GetCameraCenter = -Rcw.t()*tcw (KeyFrame.cc:118).  eye 1: GetRightRotation, GetRightTranslation,
// GetRightCameraCenter (KeyFrame.cc:1232-1262); row r of Rrl = mTlr.R.t() is column r of mTlr's rotation, row r of Rwl column r of Rcw.
__device__ __forceinline__ float fuseTwoEyesRigElement(const float* T, const float* tlr, int j) {
    const int eye = j >= kRigEyeFloats, k = j - eye * kRigEyeFloats;
    const float tcw[3] = {T[3], T[7], T[11]};
    const float tlr3[3] = {tlr[3], tlr[7], tlr[11]};
    if (k < 9) {                                                                     // mR
        const int r = k / 3, c = k - 3 * r;
        if (!eye) return T[4 * r + c];
        const float col[3] = {T[c], T[4 + c], T[8 + c]};
        return gemmRow(tlr[r], tlr[4 + r], tlr[8 + r], col, 1.0, 0.f, false);       // Rrw = Rrl*Rlw (:1247)
    }
    if (k < 12) {                                                                    // mt
        const int r = k - 9;
        if (!eye) return tcw[r];
        const float trl = gemmRow(tlr[r], tlr[4 + r], tlr[8 + r], tlr3, -1.0, 0.f, false);      // trl = -Rrl*mTlr.t (:1257)
        return gemmRow(tlr[r], tlr[4 + r], tlr[8 + r], tcw, 1.0, trl, true);         // trw = Rrl*tlw + trl (:1259)
    }
    const int r = k - 12;                                                            // the centre
    const float ow = gemmRow(T[r], T[4 + r], T[8 + r], tcw, -1.0, 0.f, false);
    if (!eye) return ow;
    return gemmRow(T[r], T[4 + r], T[8 + r], tlr3, 1.0, ow, true);                   // twr = Rwl*tlr + twl (:1238)
}

}  // namespace orbx
