"""The checker of orbx_search_by_projection_sim3_device: a sequential restatement of the two Sim3 overloads of ORBmatcher::SearchByProjection
(reference src/ORBmatcher.cc:473-586 and :588-704; loop closing) for keyframes with NLeft == -1 and the Pinhole model: one MapPoint after the
other, one candidate after the other, MUTATING vpMatched - a match closes its keypoint for every later MapPoint (:579 / :696 read back at
:558 / :675).  The front-end pieces (cv::gemm rows, Ow, KeyFrame's truncated bounds, PredictScale through the host libm, KeyFrame::
GetFeaturesInArea) are tests/fuse_walk.py's; what is stated here is the loop, the two projection forms and the candidate loop.
  projection 0: pKF->mpCamera->project (:519)            u = fx*x/z + cx
  projection 1: the second overload's own lines (:631-636) invz = 1/z; x = X*invz; u = fx*x + cx
every operation rounded on its own.  The acceptance is the reference's: int bestDist against the FLOAT product TH_LOW*ratioHamming (:577); a
MapPoint without a candidate (bestDist 256, bestIdx -1) never matches (the entry clamps the bound to 255, include/orbx.h)."""
import numpy as np

import fuse_walk as W
from fuse_walk import f32, f64

EXIT_FLAG, EXIT_NEG_DEPTH, EXIT_NOT_IN_IMAGE, EXIT_DISTANCE, EXIT_NORMAL, EXIT_EMPTY_WINDOW, EXIT_NO_MATCH, EXIT_MATCHED = range(8)


def project(pc, cam, projection):
    """(u, v) of a camera-frame point in the form of the first (0) or the second (1) overload"""
    fx, fy, cx, cy = (f32(c) for c in cam[:4])
    with np.errstate(all="ignore"):
        if projection:
            invz = f32(1.0) / pc[2]
            x = pc[0] * invz; y = pc[1] * invz
            return fx * x + cx, fy * y + cy
        return fx * pc[0] / pc[2] + cx, fy * pc[1] / pc[2] + cy


def search(kf, pose, mps, flags, cam, bounds, tab, projection=0, th=3.0, th_low=50, ratio_hamming=1.0, occupied=None, n_mp=None, stats=None):
    """kf: dict(kps, desc, grid_off, grid_idx); pose [3, 4] f32 = sRcw/scw | tcw/scw; mps as fuse_walk.search; flags [M] bit 0; occupied [n] or
    None = vpMatched[idx] != NULL on entry.  Returns dict(matches [n]: the list index each keypoint holds afterwards or -1, match_idx [M],
    match_dist [M], exit [M], n_matches).  stats (a dict) counts what the candidates met."""
    M = len(mps["world"]); n = len(kf["kps"])
    n_mp = M if n_mp is None else max(0, min(int(n_mp), M))
    minx, maxx, miny, maxy = W.keyframe_bounds(bounds)[0]
    th = f32(th)
    pose = np.asarray(pose, f32)
    R, t = pose[:, :3], pose[:, 3]
    Ow = W.camera_centre(pose)
    kps, desc = kf["kps"], kf["desc"]
    bound = f32(th_low) * f32(ratio_hamming)
    held = np.full(n, -1, np.int64)                      # vpMatched as list indices; -2 = a MapPoint it held on entry
    if occupied is not None:
        held[np.asarray(occupied[:n]) != 0] = -2
    match_idx = np.full(M, -1, np.int32); match_dist = np.full(M, 256, np.int32); exits = np.zeros(M, np.uint8)
    bump = (lambda k: stats.__setitem__(k, stats.get(k, 0) + 1)) if stats is not None else (lambda k: None)
    nmatches = 0
    with np.errstate(all="ignore"):
        for i in range(M):
            if i >= n_mp or not (int(flags[i]) & 1):
                exits[i] = EXIT_FLAG; continue
            pw = mps["world"][i].astype(f32)
            pc = [W.gemm_row(R[r], pw, 1.0, t[r]) for r in range(3)]
            if pc[2] < f32(0.0):
                exits[i] = EXIT_NEG_DEPTH; continue
            u, v = project(pc, cam, projection)
            if not (u >= minx and u < maxx and v >= miny and v < maxy):
                exits[i] = EXIT_NOT_IN_IMAGE; continue
            PO = pw - Ow
            dist3d = f32(np.sqrt((f64(PO[0]) * f64(PO[0]) + f64(PO[1]) * f64(PO[1])) + f64(PO[2]) * f64(PO[2])))
            min_d, max_d, mf_max = (f32(d) for d in mps["dist"][i])
            if dist3d < min_d or dist3d > max_d:
                exits[i] = EXIT_DISTANCE; continue
            pn = mps["normal"][i].astype(f32)
            dot = (f64(PO[0]) * f64(pn[0]) + f64(PO[1]) * f64(pn[1])) + f64(PO[2]) * f64(pn[2])
            if dot < f64(0.5) * f64(dist3d):
                exits[i] = EXIT_NORMAL; continue
            level = W.predict_scale(mf_max, dist3d, tab["scale_factor"], tab["nlevels"])
            radius = th * tab["scale"][level]
            cand = W.features_in_area(kf, bounds, u, v, radius, stats)
            if not cand:
                exits[i] = EXIT_EMPTY_WINDOW; continue
            bd, bi = 256, -1
            closed_best = 256                              # the best distance among the candidates an earlier MapPoint closed
            for j in cand:
                lv = int(kps["octave"][j])
                if held[j] != -1:
                    if held[j] == -2:
                        bump("occupied_skip")
                    else:
                        bump("closed_skip")
                        if level - 1 <= lv <= level:
                            closed_best = min(closed_best, int(W.POPCOUNT[mps["desc"][i] ^ desc[j]].sum()))
                    continue
                if lv < level - 1 or lv > level:
                    bump("level_filter"); continue
                d = int(W.POPCOUNT[mps["desc"][i] ^ desc[j]].sum())
                if d < bd:
                    bd, bi = d, j
                elif d == bd:
                    bump("tie_kept_first")
            if bi >= 0 and f32(bd) <= bound:
                held[bi] = i; nmatches += 1
                match_idx[i] = bi; match_dist[i] = bd; exits[i] = EXIT_MATCHED
                if closed_best < bd:
                    bump("best_closed_worse_taken")
            else:
                exits[i] = EXIT_NO_MATCH
                if closed_best <= bound:
                    bump("only_closed_within_bound")
    return dict(matches=np.where(held >= 0, held, -1).astype(np.int32), match_idx=match_idx, match_dist=match_dist, exit=exits, n_matches=nmatches)
