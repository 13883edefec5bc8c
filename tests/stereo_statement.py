"""The checker of oracle_stereo_match and orbx_stereo_match_*: an independent per-feature statement of Frame::ComputeStereoMatches
(reference src/Frame.cc:813-991) in plain numpy.  It shares no code with oracle/orb_oracle.cpp: there are no row tables (every left keypoint
builds its candidate mask over all right keypoints), the Hamming distance comes from a byte table, the 11 SADs from one 11 x 21 strip, and
every binary32 step is a numpy float32 scalar operation, rounded once.

The pyramids are read from two oracle_lib.Oracle objects through level(l, bordered=True) (the 19-pixel BORDER_REFLECT_101 frame lies around
each level, as around the reference's mvImagePyramid views), so a window may hang over the level's edge as it does in the reference.

Exit codes, one per left keypoint, in the reference's order:
  OFF_IMAGE   (int)vL is no row of the image (the reference would index vRowIndices out of range; both restatements skip the keypoint)
  NO_ROW      vCandidates.empty(): no right keypoint's band covers the row                              (:857-858)
  MAXU_NEG    maxU < 0                                                                                  (:864-865)
  NO_100      no candidate inside the octave and u gates with a distance < TH_HIGH = 100                (:873-893)
  NOT_75      best distance in [75, 100)                                                                (:896)
  WIN_LEFT    iniu < 0                                                                                  (:919)
  WIN_RIGHT   endu >= cols of the right level                                                           (:919)
  SAD_END     the SAD minimum lies at a shift of -5 or +5                                               (:945)
  DELTA       deltaR outside [-1, 1]                                                                    (:955-956)
  RANGE       disparity outside [0, maxD)                                                               (:962)
  DROPPED     matched, then removed by the median filter                                                (:981-996)
  KEPT        matched and kept

DELTA is unreachable: the best shift is the FIRST minimum, so a = dist1 - dist2 > 0 and b = dist3 - dist2 >= 0, and
deltaR = (dist1 - dist3) / (2 (dist1 + dist3 - 2 dist2)) = (a - b) / (2 (a + b)) lies in [-0.5, 0.5]; all operands are integers below 2^24,
so binary32 computes it without rounding before the quotient.  The tests assert that its count is 0."""
import numpy as np

f32 = np.float32
EXITS = ("OFF_IMAGE", "NO_ROW", "MAXU_NEG", "NO_100", "NOT_75", "WIN_LEFT", "WIN_RIGHT", "SAD_END", "DELTA", "RANGE", "DROPPED", "KEPT")
OFF_IMAGE, NO_ROW, MAXU_NEG, NO_100, NOT_75, WIN_LEFT, WIN_RIGHT, SAD_END, DELTA, RANGE, DROPPED, KEPT = range(len(EXITS))
BITS = np.array([bin(v).count("1") for v in range(256)], np.int32)
EDGE = 19            # ORBextractor.cc: EDGE_THRESHOLD, the frame around every level
TH_HIGH, TH_LOW = 100, 50      # ORBmatcher.cc:36-37


def round_half_away(x):
    """std::round of a binary32: halves away from zero (|x| + 0.5 is exact in double)"""
    x = float(x)
    return f32(np.copysign(np.floor(abs(x) + 0.5), x))


def stereo_statement(o_left, o_right, kL, dL, kR, dR, bf, b):
    """Returns dict(u_right, depth [N] float32, kept = the return value, exit [N] codes, sad [N] pre-filter SAD (-1 = no match),
    shared [N]: the best Hamming distance (< 75) was held by more than one candidate, shared_apart: ... by candidates of different x,
    clamped [N]: the disparity <= 0 branch was taken, best_r [N] the chosen right index (-1 = none), median)."""
    N, Nr = len(kL), len(kR)
    dL = np.asarray(dL, np.uint8).reshape(-1, 32); dR = np.asarray(dR, np.uint8).reshape(-1, 32)
    scale, inv = np.asarray(o_left.scale_factors, np.float32), np.asarray(o_left.inv_scale_factors, np.float32)
    rows = o_left.level_size(0)[1]
    bf, b = f32(bf), f32(b)
    max_d = f32(bf / b)                                            # minZ = mb, minD = 0, maxD = mbf / minZ (:843-845)
    th_orb = (TH_HIGH + TH_LOW) // 2
    # the band of every right keypoint, in binary32 (:826-840)
    yR, xR, oR = kR["y"].astype(np.float32), kR["x"].astype(np.float32), kR["octave"].astype(np.int64)
    r = (f32(2.0) * scale[oR]).astype(np.float32) if Nr else np.zeros(0, np.float32)
    band_hi = np.ceil((yR + r).astype(np.float32)).astype(np.int64); band_lo = np.floor((yR - r).astype(np.float32)).astype(np.int64)
    levels_l, levels_r = {}, {}

    def level_of(cache, o, l):
        if l not in cache:
            cache[l] = o.level(l, bordered=True).astype(np.int32)
        return cache[l]

    u_right = np.full(N, -1, np.float32); depth = np.full(N, -1, np.float32)
    code = np.zeros(N, np.int32); sad = np.full(N, -1, np.int64); best_r = np.full(N, -1, np.int64)
    shared = np.zeros(N, bool); shared_apart = np.zeros(N, bool); clamped = np.zeros(N, bool)
    for i in range(N):
        uL, vL, lvl = f32(kL["x"][i]), f32(kL["y"][i]), int(kL["octave"][i])
        row = int(vL)                                              # truncation, as (size_t)vL of a non-negative value
        if row < 0 or row >= rows:
            code[i] = OFF_IMAGE; continue
        in_band = (band_lo <= row) & (row <= band_hi)
        if not in_band.any():
            code[i] = NO_ROW; continue
        min_u, max_u = f32(uL - max_d), f32(uL - f32(0))
        if max_u < 0:
            code[i] = MAXU_NEG; continue
        cand = np.flatnonzero(in_band & (oR >= lvl - 1) & (oR <= lvl + 1) & (xR >= min_u) & (xR <= max_u))     # increasing right index
        ham = BITS[dR[cand] ^ dL[i]].sum(1) if len(cand) else np.zeros(0, np.int32)
        if len(cand) == 0 or ham.min() >= TH_HIGH:
            code[i] = NO_100; continue
        best = int(ham.min())
        if best >= th_orb:
            code[i] = NOT_75; continue
        holders = cand[ham == best]
        j = int(holders[0])                                        # `dist < bestDist` keeps the first = lowest right index
        best_r[i] = j
        shared[i] = len(holders) > 1
        shared_apart[i] = len(np.unique(xR[holders])) > 1
        s_inv = inv[lvl]
        su_l, sv_l, su_r = round_half_away(f32(uL * s_inv)), round_half_away(f32(vL * s_inv)), round_half_away(f32(xR[j] * s_inv))
        w_r = o_right.level_size(lvl)[0]
        ini_u, end_u = f32(f32(su_r + f32(5)) - f32(5)), f32(f32(f32(su_r + f32(5)) + f32(5)) + f32(1))
        if ini_u < 0:
            code[i] = WIN_LEFT; continue
        if end_u >= w_r:
            code[i] = WIN_RIGHT; continue
        y0, xl0 = int(f32(sv_l - f32(5))), int(f32(su_l - f32(5)))
        img_l, img_r = level_of(levels_l, o_left, lvl), level_of(levels_r, o_right, lvl)
        win = img_l[EDGE + y0:EDGE + y0 + 11, EDGE + xl0:EDGE + xl0 + 11]
        assert win.shape == (11, 11), "left window outside the bordered level: keypoint %d" % i
        win = win - win[5, 5]
        x_first = int(f32(f32(su_r + f32(-5)) - f32(5)))          # the window's first column at incR = -5
        strip = img_r[EDGE + y0:EDGE + y0 + 11, EDGE + x_first:EDGE + x_first + 21]
        assert strip.shape == (11, 21)
        sads = np.array([np.abs(win - (strip[:, s:s + 11] - strip[5, s + 5])).sum() for s in range(11)], np.int64)
        dists = sads.astype(np.float32)
        k = int(np.argmin(sads))                                   # `dist < bestDist`: the first minimum
        if k == 0 or k == 10:
            code[i] = SAD_END; continue
        d1, d2, d3 = dists[k - 1], dists[k], dists[k + 1]
        delta = f32(f32(d1 - d3) / f32(f32(2.0) * f32(f32(d1 + d3) - f32(f32(2.0) * d2))))
        if delta < -1 or delta > 1:
            code[i] = DELTA; continue
        best_u = f32(scale[lvl] * f32(f32(su_r + f32(k - 5)) + delta))
        disparity = f32(uL - best_u)
        if not (disparity >= 0 and disparity < max_d):
            code[i] = RANGE; continue
        if disparity <= 0:
            disparity = f32(0.01); best_u = f32(float(uL) - 0.01); clamped[i] = True      # the one double-precision step (:962-966)
        depth[i] = f32(bf / disparity); u_right[i] = best_u; sad[i] = int(sads[k]); code[i] = KEPT
    matched = np.flatnonzero(sad >= 0)
    median = -1
    if len(matched):                                               # (:981-996); with no match the reference reads vDistIdx[0] of an empty vector
        median = int(np.sort(sad[matched])[len(matched) // 2])
        th = f32(f32(f32(1.5) * f32(1.4)) * f32(median))
        drop = matched[~(sad[matched].astype(np.float32) < th)]
        u_right[drop] = -1; depth[drop] = -1; code[drop] = DROPPED
    return dict(u_right=u_right, depth=depth, kept=int((code == KEPT).sum()), exit=code, sad=sad, shared=shared, shared_apart=shared_apart,
                clamped=clamped, best_r=best_r, median=median)


def counts(res):
    """exit name -> number of left keypoints"""
    return {name: int((res["exit"] == c).sum()) for c, name in enumerate(EXITS)}
