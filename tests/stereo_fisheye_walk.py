"""The checker of orbx_stereo_fisheye_match_device: Frame::ComputeStereoFishEyeMatches (reference src/Frame.cc:1139-1179) as a sequential
statement, in the reference's control flow: the lapping rows cut out of both eyes, knnMatch(..., 2), the loop over `matches` in increasing
left index with Lowe's ratio, TriangulateMatches on the two RAW keypoints, and the four assignments with their overwrites in order.

OpenCV is not available to this project, so two of its routines are the project's definitions (include/orbx.h; parity
unpinned, as the cv::SVD ones):
  * cv::BFMatcher(NORM_HAMMING).knnMatch(query, train, matches, 2) is batchDistance's insertion over the train rows in increasing index:
    a candidate enters the list only if it is strictly smaller than the current last entry (or the list is shorter than 2), and moves in
    front of an entry only if that entry is strictly larger (knn2 below);
  * (*it)[0].distance < (*it)[1].distance * 0.7: DMatch::distance is a float, 0.7 a double, the product and the compare are in double.
KannalaBrandt8::unproject and TriangulateMatches are tests/triangulation_two_eyes_walk.py's (imported, not restated).  An octave outside
[0, nlevels) is clamped into mvLevelSigma2 and a mono count outside [0, N] into it: the reference would index out of bounds on either.

An eye is dict(kps (the RAW keypoints: x, y, octave), desc [n, 32])."""
import numpy as np

import triangulation_two_eyes_walk as W
from two_eyes_bow_walk import POPCOUNT

f32 = np.float32
WHY = {W.OK: "ok", W.PARALLAX: "parallax", W.Z1: "z1", W.Z2: "z2", W.ERROR1: "error1", W.ERROR2: "error2"}


def knn2(dists):
    """matches[i] of knnMatch(..., 2) for one query row: up to two (distance, trainIdx), from the row's distances to every train row"""
    best = []
    for j, d in enumerate(dists):
        if len(best) == 2:
            if not d < best[1][0]:
                continue
            best.pop()
        pos = len(best)
        while pos > 0 and best[pos - 1][0] > d:
            pos -= 1
        best.insert(pos, (int(d), j))
    return best


def ratio_passes(d0, d1):
    """(*it)[0].distance < (*it)[1].distance * 0.7: the float promoted, times the double"""
    return float(f32(d0)) < float(f32(d1)) * 0.7


def compute_stereo_fisheye_matches(m, left, right, mono_left, mono_right, tlr, cams, level_sigma2, trace=None):
    """Returns dict(left_to_right = mvLeftToRightMatch, right_to_left = mvRightToLeftMatch, depth = mvDepth, x3d = mvStereo3Dpoints (zeros
    where the reference leaves an empty Mat), n = nMatches, desc = descMatches, knn = the lists of knnMatch).  trace: a list that receives
    (left index, right index, accepted, depth, why TriangulateMatches left) of every row that passed the ratio test, in order."""
    sig2 = np.asarray(level_sigma2, f32)
    cams = [[f32(c) for c in cam] for cam in cams]
    tlr = np.asarray(tlr, f32).reshape(3, 4)
    R12, t12 = tlr[:, :3], tlr[:, 3]                               # mRlr, mtlr (:1100-1101)
    n_left, n_right = len(left["kps"]), len(right["kps"])
    mono_left = min(max(int(mono_left), 0), n_left); mono_right = min(max(int(mono_right), 0), n_right)
    desc_left = np.asarray(left["desc"], np.uint8).reshape(-1, 32)[mono_left:]          # :1144-1145
    desc_right = np.asarray(right["desc"], np.uint8).reshape(-1, 32)[mono_right:]
    l2r = [-1] * n_left; r2l = [-1] * n_right; depth = [f32(-1.0)] * n_left          # :1147-1151
    x3d = np.zeros((n_left, 3), f32)
    dist = POPCOUNT[desc_left[:, None, :] ^ desc_right[None, :, :]].sum(2) if len(desc_left) and len(desc_right) else np.zeros((len(desc_left), 0), int)
    matches = [knn2(row.tolist()) for row in dist]                 # :1157
    n_matches = desc_matches = 0

    def sigma(octave):
        return sig2[min(max(int(octave), 0), len(sig2) - 1)]

    for query, it in enumerate(matches):                           # :1163
        if len(it) >= 2 and ratio_passes(it[0][0], it[1][0]):
            desc_matches += 1
            i, j = query + mono_left, it[0][1] + mono_right
            k1, k2 = left["kps"][i], right["kps"][j]
            z, p3d, why = W.triangulate_matches(m, cams[0], cams[1], (k1["x"], k1["y"]), (k2["x"], k2["y"]), R12, t12, sigma(k1["octave"]),
                                                sigma(k2["octave"]))
            ok = bool(z > f32(0.0001))                             # :1170
            if trace is not None:
                trace.append((i, j, ok, z, WHY[why]))
            if ok:
                l2r[i] = j                                         # :1171-1175
                r2l[j] = i
                x3d[i] = p3d
                depth[i] = z
                n_matches += 1
    return dict(left_to_right=l2r, right_to_left=r2l, depth=np.array(depth, f32), x3d=x3d, n=n_matches, desc=desc_matches, knn=matches)
