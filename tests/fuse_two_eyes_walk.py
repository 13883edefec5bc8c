"""The checker of orbx_fuse_two_eyes_device: a sequential restatement of ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight) (reference
src/ORBmatcher.cc:1399-1609) and of the loop-closing overload (:1611-1733) for TWO-CAMERA keyframes (NLeft != -1, a KannalaBrandt8 pair), one
MapPoint after the other, one candidate after the other, built from what the one-camera checker has (tests/fuse_walk.py: gemm_row,
features_in_area, predict_scale, tables, build_grid, Map; its tail with the two-camera Observations()) and KannalaBrandt8::project of tests/last_frame_two_eyes_walk.py.  What is new:
  * keyframe_rig(pose, tlr): the three right-eye getters of KeyFrame (src/KeyFrame.cc:1232-1262), which derive everything from mTlr alone;
  * the projection with the eye's own camera, after which z == 0 does not leave by itself;
  * the eye's own grid and RAW keypoints (KeyFrame::GetFeaturesInArea(x, y, r, bRight), src/KeyFrame.cc:798-803; ORBmatcher.cc:1524-1528);
  * the reprojection test is always the monocular one (mvuRight is all -1, src/Frame.cc:1150);
  * bestIdx in the keyframe's numbering: a right keypoint i is NLeft + i (:1559);
  * the map model for keyframes whose observations are (left index, right index) pairs (src/MapPoint.cc:146-160, :249-301).
A rig keyframe is dict(pose [3, 4] f32 (Rcw | tcw), eyes = (left, right)); an eye is dict(kps (raw), desc [n, 32], grid_off, grid_idx).
OpenCV is not available to this project: the cv::Mat roundings are the project's restatement (parity unpinned)."""
import numpy as np

import fuse_walk as W
import last_frame_two_eyes_walk as K
from fuse_walk import (EXIT_ABOVE_TH_LOW, EXIT_DISTANCE, EXIT_EMPTY_WINDOW, EXIT_FLAG, EXIT_FUSED, EXIT_NEG_DEPTH, EXIT_NORMAL,  # noqa: F401
                       EXIT_NOT_IN_IMAGE, POPCOUNT, f32, f64, gemm_row)

LIBM = K.libm_math()


def keyframe_rig(pose, tlr):
    """((Rcw, tcw, Ow), (Rrw, trw, twr)): GetRotation / GetTranslation / GetCameraCenter and GetRightRotation / GetRightTranslation /
    GetRightCameraCenter of a KeyFrame with the pose `pose` and mTlr = `tlr` (both 3x4)"""
    pose = np.asarray(pose, f32); tlr = np.asarray(tlr, f32)
    Rlw, tlw = pose[:, :3], pose[:, 3]
    Ow = W.camera_centre(pose)                                                       # KeyFrame.cc:118
    Rrl = tlr[:, :3].T                                                               # mTlr.rowRange(0,3).colRange(0,3).t()
    t_lr = tlr[:, 3]
    Rrw = np.array([[gemm_row(Rrl[r], Rlw[:, c], 1.0) for c in range(3)] for r in range(3)], f32)      # :1247
    trl = np.array([gemm_row(Rrl[r], t_lr, -1.0) for r in range(3)], f32)           # :1257, one gemm with alpha = -1
    trw = np.array([gemm_row(Rrl[r], tlw, 1.0, trl[r]) for r in range(3)], f32)     # :1259, one gemm with the addend
    Rwl = Rlw.T
    twr = np.array([gemm_row(Rwl[r], t_lr, 1.0, Ow[r]) for r in range(3)], f32)     # :1238
    return (Rlw.copy(), tlw.copy(), Ow), (Rrw, trw, twr)


def project(rig_eye, cam, pw):
    """(p3Dc, u, v) of a world point in one eye: Rcw*p3Dw + tcw as cv::gemm, then KannalaBrandt8::project with that eye's camera"""
    R, t, _ = rig_eye
    pc = [gemm_row(R[r], np.asarray(pw, f32), 1.0, t[r]) for r in range(3)]
    u, v = K.kb8_project(LIBM, cam, pc[0], pc[1], pc[2])
    return pc, u, v


def cells_population(eye, bounds, x, y, r):
    """how many keypoints the cells of GetFeaturesInArea's window hold (for the statistics only: the box test's rejections)"""
    (minx, _, miny, _), w_inv, h_inv = W.keyframe_bounds(bounds)
    lo_x = max(0, int(np.floor((x - minx - r) * w_inv))); hi_x = min(W.COLS - 1, int(np.ceil((x - minx + r) * w_inv)))
    lo_y = max(0, int(np.floor((y - miny - r) * h_inv))); hi_y = min(W.ROWS - 1, int(np.ceil((y - miny + r) * h_inv)))
    if lo_x >= W.COLS or hi_x < 0 or lo_y >= W.ROWS or hi_y < 0:
        return 0
    off = eye["grid_off"]
    return sum(int(off[ix * W.ROWS + hi_y + 1] - off[ix * W.ROWS + lo_y]) for ix in range(lo_x, hi_x + 1) if hi_y >= lo_y)


def search(kf, right, mps, flags, tlr, cams, bounds, tab, th=3.0, th_low=50, reproj_check=True, n_mp=None, stats=None):
    """Fuse(pKF, vpMapPoints, th, bRight = right), the search half.  kf: a rig keyframe; mps / flags as fuse_walk.search; cams = (mpCamera,
    mpCamera2) as eight floats each.  Returns dict(best_idx (the keyframe's numbering), best_dist, exit, n_fused)."""
    M = len(mps["world"])
    n_mp = M if n_mp is None else max(0, min(int(n_mp), M))
    eye = kf["eyes"][1 if right else 0]
    n_left = len(kf["eyes"][0]["kps"])                                               # pKF->NLeft
    rig_eye = keyframe_rig(kf["pose"], tlr)[1 if right else 0]                       # :1404-1417
    Ow = rig_eye[2]
    cam = [f32(c) for c in cams[1 if right else 0]]
    minx, maxx, miny, maxy = W.keyframe_bounds(bounds)[0]
    th = f32(th)
    kps, desc = eye["kps"], eye["desc"]
    best_idx = np.full(M, -1, np.int32); best_dist = np.full(M, 256, np.int32); exits = np.zeros(M, np.uint8)
    bump = (lambda k, n=1: stats.__setitem__(k, stats.get(k, 0) + n)) if stats is not None else (lambda k, n=1: None)
    with np.errstate(all="ignore"):
        for i in range(M):
            if i >= n_mp or not (int(flags[i]) & 1):
                exits[i] = EXIT_FLAG; continue
            pw = mps["world"][i].astype(f32)
            pc, u, v = project(rig_eye, cam, pw)                                     # :1456, :1470
            if pc[2] < f32(0.0):                                                     # :1459; z == 0 and z == -0 go on
                exits[i] = EXIT_NEG_DEPTH; continue
            if pc[2] == 0:
                bump("z_is_zero")
            if not (u >= minx and u < maxx and v >= miny and v < maxy):              # KeyFrame::IsInImage
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
            cand = W.features_in_area(eye, bounds, u, v, radius, stats)              # GetFeaturesInArea(u, v, r, bRight): this eye's grid and raw keypoints
            if stats is not None:
                bump("box_test", cells_population(eye, bounds, u, v, radius) - len(cand))
            if not cand:
                exits[i] = EXIT_EMPTY_WINDOW; continue
            bd, bi = 256, -1
            for j in cand:
                lv = int(kps["octave"][j])                                           # mvKeys / mvKeysRight (:1524-1528)
                if lv < level - 1:
                    bump("level_too_low"); continue
                if lv > level:
                    bump("level_too_high"); continue
                if lv < 0:
                    bump("level_minus_one")
                if reproj_check:                                                     # mvuRight[idx] is -1 (Frame.cc:1150): :1547-1557
                    inv = tab["inv_sigma2"][min(max(lv, 0), tab["nlevels"] - 1)]
                    ex = u - f32(kps["x"][j]); ey = v - f32(kps["y"][j])
                    e2 = ex * ex + ey * ey
                    if f64(e2 * inv) > 5.99:
                        bump("reject_5_99"); continue
                    bump("pass_5_99")
                d = int(POPCOUNT[mps["desc"][i] ^ desc[j]].sum())                    # mDescriptors.row(idx + NLeft): this eye's row j
                if d < bd:
                    bd, bi = d, j
                elif d == bd:
                    bump("tie_kept_first")
            best_dist[i] = bd
            if bi >= 0 and bd <= min(th_low, 255):
                best_idx[i] = bi + (n_left if right else 0); exits[i] = EXIT_FUSED   # :1559
                if right and bi >= n_left:
                    bump("right_winner_at_or_above_nleft")
            else:
                exits[i] = EXIT_ABOVE_TH_LOW
    return dict(best_idx=best_idx, best_dist=best_dist, exit=exits, n_fused=int((exits == EXIT_FUSED).sum()))


# ---------------------------------------------------------------- the map model ----------------------------------------------------------------
class Map(W.Map):
    """fuse_walk.Map for keyframes with NLeft != -1.  A keyframe's slots and descriptors are in the keyframe's numbering (left keypoints, then
    NLeft + right keypoints); an observation is a pair (left index, right index), -1 = none (MapPoint::AddObservation, src/MapPoint.cc:146-160:
    idx >= NLeft goes to the right half).  IsInKeyFrame is true with either half, so the right call skips what the left call added.  Replace
    (src/MapPoint.cc:249-301) moves both halves.  ComputeDistinctiveDescriptors (:330-403) collects the left and the right descriptor of every
    observation."""

    def __init__(self, point_desc, kf_desc, n_left):
        super().__init__(point_desc, kf_desc)
        self.n_left = list(n_left)

    def copy(self):
        m = Map([], [], self.n_left)
        m.desc = [d.copy() for d in self.desc]; m.kf_desc = self.kf_desc
        m.obs = [dict(o) for o in self.obs]; m.bad = list(self.bad); m.slots = [list(s) for s in self.slots]; m.recomputed = set(self.recomputed)
        return m

    def add(self, mp, kf, idx):                       # AddObservation + AddMapPoint
        left, right = self.obs[mp].get(kf, (-1, -1))
        if idx >= self.n_left[kf]:
            right = idx
        else:
            left = idx
        self.obs[mp][kf] = (left, right)
        self.slots[kf][idx] = mp

    def observations(self, mp):                       # Observations(): nObs
        return sum(i != -1 for pair in self.obs[mp].values() for i in pair)

    def compute_distinctive_descriptors(self, mp):    # MapPoint.cc:330-403 with :357-362
        if self.bad[mp] or not self.obs[mp]:
            return
        ds = [self.kf_desc[kf][i] for kf, pair in sorted(self.obs[mp].items()) for i in pair if i != -1]
        n = len(ds)
        dist = [[int(POPCOUNT[a ^ b].sum()) for b in ds] for a in ds]
        best_median, best = 1 << 31, 0
        for i in range(n):
            median = sorted(dist[i])[int(0.5 * (n - 1))]
            if median < best_median:
                best_median, best = median, i
        self.desc[mp] = ds[best].copy()

    def replace(self, old, new):                      # old->Replace(new)
        if old == new:
            return
        obs = self.obs[old]; self.obs[old] = dict(); self.bad[old] = True
        for kf in sorted(obs):
            left, right = obs[kf]
            if not self.in_keyframe(new, kf):
                for i in (left, right):                # :279-286
                    if i != -1:
                        self.slots[kf][i] = new
                        self.add(new, kf, i)
            else:
                for i in (left, right):                # :289-294
                    if i != -1:
                        self.slots[kf][i] = -1
        self.compute_distinctive_descriptors(new)
        self.recomputed.add(new)


def tail(mp_map, kf, mp, best_idx):
    """:1573-1592 as fuse_walk.tail, with Observations() of a two-camera map: nObs counts every index of every observation (MapPoint.cc:162-165
    with mpCamera2 set), so a MapPoint seen by both eyes of a keyframe counts twice"""
    held = mp_map.slots[kf][best_idx]
    if held >= 0:
        if not mp_map.bad[held]:
            if mp_map.observations(held) > mp_map.observations(mp):
                mp_map.replace(mp, held)
            else:
                mp_map.replace(held, mp)
    else:
        mp_map.add(mp, kf, best_idx)


def fuse_sequential(mp_map, kf_index, kf, right, mp_list, mps, **kw):
    """the reference's one call Fuse(pKF, vpMapPoints, th, bRight): every search on the map as the earlier tails left it"""
    n = 0
    for i, mp in enumerate(mp_list):
        fl = W.flags_of(mp_map, kf_index, [mp])
        one = dict((k, v[i:i + 1]) for k, v in mps.items())
        if mp >= 0:
            one["desc"] = mp_map.desc[mp][None, :]
        r = search(kf, right, one, fl, **kw)
        if r["exit"][0] == EXIT_FUSED:
            tail(mp_map, kf_index, mp, int(r["best_idx"][0])); n += 1
    return n


def replay_tail(mp_map, kf_index, mp_list, result, uploaded_desc=None, search_again=None):
    """the batched form's host half for ONE EYE of one keyframe, as fuse_walk.replay_tail: first the list entries that survived a Replace
    earlier (in an earlier keyframe, or in this keyframe's other eye) and whose descriptor is no longer the uploaded one are searched again in
    this keyframe and eye (search_again(flags, descriptors) -> a search() result, flags set for them alone); then, in list order, isBad() /
    IsInKeyFrame are tested again - what the left tail put into the keyframe is skipped by the right - and the tail is applied.
    Returns (the count of tails applied, the list positions searched again)."""
    stale = []
    if search_again is not None:
        stale = [i for i, mp in enumerate(mp_list) if mp in mp_map.recomputed and not mp_map.bad[mp] and not mp_map.in_keyframe(mp, kf_index)
                 and not np.array_equal(mp_map.desc[mp], uploaded_desc[i])]
        if stale:
            fl = np.zeros(len(mp_list), np.uint8); fl[stale] = 1
            again = search_again(fl, W.list_descriptors(mp_map, mp_list))
            result = dict((k, np.array(result[k])) for k in ("best_idx", "best_dist", "exit"))
            for k in result:
                result[k][stale] = again[k][stale]
    n = 0
    for i, mp in enumerate(mp_list):
        if result["exit"][i] != EXIT_FUSED:
            continue
        if mp < 0 or mp_map.bad[mp] or mp_map.in_keyframe(mp, kf_index):
            continue
        tail(mp_map, kf_index, mp, int(result["best_idx"][i])); n += 1
    return n, stale
