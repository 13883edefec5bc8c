"""The checker of orbx_fuse_device: a sequential restatement of both ORBmatcher::Fuse overloads (reference src/ORBmatcher.cc:1399-1609 and
:1611-1733) for keyframes with NLeft == -1 and the Pinhole model, one MapPoint after the other, one candidate after the other, in numpy binary32 /
binary64 scalars with the reference's roundings:
  * cv::Mat products (Rcw*p3Dw+tcw, -Rcw.t()*tcw) as cv::gemm on CV_32F: products and sums in double, one rounding to float;
  * invz = 1/z, Pinhole::project (fx*x/z + cx), ur, PO, ratio, radius, the window arithmetic and the reprojection errors in float, each operation
    rounded on its own; cv::norm and Mat::dot accumulate in double in element order;
  * MapPoint::PredictScale (src/MapPoint.cc:514-529) through the HOST libm's logf (ctypes; numpy's float32 log is another implementation);
  * KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:770-814) with its four early returns, ix outer, iy inner, push order inside a cell;
  * KeyFrame's image bounds: mnMinX .. mnMaxY are const int there (inc/KeyFrame.h:484), initialised from Frame's floats (src/KeyFrame.cc:58) and so
    truncated toward zero, while mfGridElementWidthInv / HeightInv are copies of Frame's, made from the floats (:50).  IsInImage and the window
    use the truncated bounds and the untruncated inverses; the grid itself (build_grid) is Frame's and uses the floats.
search() is the search half (what the device entry computes, with an exit code per MapPoint and counters of what the candidates met); replay_tail()
and fuse_sequential() are the map-changing tails (:1573-1592, :1715-1729) on a tiny map model, for the batching licence of tests/test_fuse.py.
OpenCV is not available to this project: the cv::Mat roundings above are the project's restatement (parity unpinned)."""
import ctypes
import ctypes.util

import numpy as np

f32, f64 = np.float32, np.float64
COLS, ROWS = 64, 48
POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int32)
EXIT_FLAG, EXIT_NEG_DEPTH, EXIT_NOT_IN_IMAGE, EXIT_DISTANCE, EXIT_NORMAL, EXIT_EMPTY_WINDOW, EXIT_ABOVE_TH_LOW, EXIT_FUSED = range(8)
EXIT_NAMES = ("flag", "negdepth", "notinim", "dist", "normal", "notidx", "thcheck", "fused")

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]


def logf(x):
    return f32(_libm.logf(ctypes.c_float(float(x))))


def predict_scale(max_distance, dist, scale_factor, nlevels):
    """MapPoint::PredictScale; +inf -> nlevels - 1 and NaN -> 0 where the reference's int conversion is undefined (include/orbx.h)"""
    with np.errstate(all="ignore"):
        ratio = f32(max_distance) / f32(dist)
        c = np.ceil(f32(logf(ratio) / logf(f32(scale_factor))))
    if not c >= 0:
        return 0
    return nlevels - 1 if c >= nlevels else int(c)


def tables(scale_factor=1.2, nlevels=8):
    """mvScaleFactors, mvInvLevelSigma2 (ORBextractor.cc:416-436: float products of the float scale factor held in a double)"""
    sf = np.ones(nlevels, f32); s2 = np.ones(nlevels, f32)
    for i in range(1, nlevels):
        sf[i] = f32(f64(sf[i - 1]) * f64(f32(scale_factor)))
        s2[i] = sf[i] * sf[i]
    return dict(scale=sf, inv_sigma2=(f32(1.0) / s2).astype(f32), scale_factor=f32(scale_factor), nlevels=nlevels)


def c_round(t):
    """round() of <cmath> on a double: halves away from zero"""
    t = np.asarray(t, f64)
    return np.trunc(t + np.copysign(0.5, t)).astype(np.int64)


def build_grid(kps, bounds):
    """Frame::AssignFeaturesToGrid + PosInGrid (src/Frame.cc:383-417, :726-736) as CSR: offsets[64*48 + 1] over cells x*48 + y, indices in push order"""
    bounds = np.asarray(bounds, f32)
    w_inv = f32(COLS) / (bounds[1] - bounds[0]); h_inv = f32(ROWS) / (bounds[3] - bounds[2])
    px = c_round((kps["x"].astype(f32) - bounds[0]) * w_inv); py = c_round((kps["y"].astype(f32) - bounds[2]) * h_inv)
    inside = (px >= 0) & (px < COLS) & (py >= 0) & (py < ROWS)
    cell = np.where(inside, px * ROWS + py, COLS * ROWS)
    order = np.argsort(cell, kind="stable")
    order = order[:int(inside.sum())]
    off = np.zeros(COLS * ROWS + 1, np.int32)
    off[1:] = np.cumsum(np.bincount(cell[inside], minlength=COLS * ROWS))
    return off, order.astype(np.int32), np.where(inside, cell, -1)


def gemm_row(a, b, alpha, c=None):
    s = f64(a[0]) * f64(b[0])
    s = s + f64(a[1]) * f64(b[1])
    s = s + f64(a[2]) * f64(b[2])
    s = s * f64(alpha)
    if c is not None:
        s = s + f64(c)
    return f32(s)


def camera_centre(pose):
    """Ow = -Rcw.t()*tcw (src/KeyFrame.cc:118, src/ORBmatcher.cc:1624)"""
    R, t = pose[:, :3], pose[:, 3]
    return np.array([gemm_row(R[:, r], t, -1.0) for r in range(3)], f32)


def keyframe_bounds(bounds):
    """Frame's float bounds -> KeyFrame's (mnMinX, mnMaxX, mnMinY, mnMaxY) as floats of the truncated ints, and Frame's grid inverses"""
    b = np.asarray(bounds, f32)
    w_inv = f32(COLS) / (b[1] - b[0]); h_inv = f32(ROWS) / (b[3] - b[2])
    return tuple(f32(np.trunc(v)) for v in b), w_inv, h_inv


def features_in_area(kf, bounds, x, y, r, stats=None):
    """KeyFrame::GetFeaturesInArea(x, y, r): keypoint indices in visit order"""
    (minx, maxx, miny, maxy), w_inv, h_inv = keyframe_bounds(bounds)
    bump = (lambda k: stats.__setitem__(k, stats.get(k, 0) + 1)) if stats is not None else (lambda k: None)
    min_cx = max(0, int(np.floor((x - minx - r) * w_inv)))
    if min_cx >= COLS:
        bump("return_min_cell_x"); return []
    max_cx = min(COLS - 1, int(np.ceil((x - minx + r) * w_inv)))
    if max_cx < 0:
        bump("return_max_cell_x"); return []
    min_cy = max(0, int(np.floor((y - miny - r) * h_inv)))
    if min_cy >= ROWS:
        bump("return_min_cell_y"); return []
    max_cy = min(ROWS - 1, int(np.ceil((y - miny + r) * h_inv)))
    if max_cy < 0:
        bump("return_max_cell_y"); return []
    if (x - minx - r) * w_inv < 0: bump("window_past_left")
    if (x - minx + r) * w_inv > COLS - 1: bump("window_past_right")
    if (y - miny - r) * h_inv < 0: bump("window_past_top")
    if (y - miny + r) * h_inv > ROWS - 1: bump("window_past_bottom")
    out = []
    off, idx, kps = kf["grid_off"], kf["grid_idx"], kf["kps"]
    for ix in range(min_cx, max_cx + 1):
        for iy in range(min_cy, max_cy + 1):
            for s in range(off[ix * ROWS + iy], off[ix * ROWS + iy + 1]):
                j = int(idx[s])
                if abs(f32(kps["x"][j]) - x) < r and abs(f32(kps["y"][j]) - y) < r:
                    out.append(j)
    return out


def search(kf, mps, flags, cam, bounds, mbf, tab, th=3.0, th_low=50, reproj_check=True, n_mp=None, stats=None):
    """kf: dict(pose [3, 4] f32 (Rcw | tcw), kps (mvKeysUn), ur (mvuRight or None), desc [n, 32], grid_off, grid_idx);
    mps: dict(world [M, 3], normal [M, 3], dist [M, 3] (min invariance, max invariance, mfMaxDistance), desc [M, 32]); flags [M] bit 0.
    Returns dict(best_idx, best_dist, exit, n_fused).  stats (a dict) counts what the candidates met."""
    M = len(mps["world"])
    n_mp = M if n_mp is None else max(0, min(int(n_mp), M))
    fx, fy, cx, cy = (f32(c) for c in cam[:4])
    minx, maxx, miny, maxy = keyframe_bounds(bounds)[0]
    mbf, th = f32(mbf), f32(th)
    pose = np.asarray(kf["pose"], f32)
    R, t = pose[:, :3], pose[:, 3]
    Ow = camera_centre(pose)
    kps, ur_all, desc = kf["kps"], kf["ur"], kf["desc"]
    best_idx = np.full(M, -1, np.int32); best_dist = np.full(M, 256, np.int32); exits = np.zeros(M, np.uint8)
    bump = (lambda k: stats.__setitem__(k, stats.get(k, 0) + 1)) if stats is not None else (lambda k: None)
    with np.errstate(all="ignore"):
        for i in range(M):
            if i >= n_mp or not (int(flags[i]) & 1):
                exits[i] = EXIT_FLAG; continue
            pw = mps["world"][i].astype(f32)
            pc = [gemm_row(R[r], pw, 1.0, t[r]) for r in range(3)]
            if pc[2] < f32(0.0):
                exits[i] = EXIT_NEG_DEPTH; continue
            invz = f32(1.0) / pc[2]
            u = fx * pc[0] / pc[2] + cx
            v = fy * pc[1] / pc[2] + cy
            if not (u >= minx and u < maxx and v >= miny and v < maxy):
                exits[i] = EXIT_NOT_IN_IMAGE; continue
            ur = u - mbf * invz
            PO = pw - Ow
            dist3d = f32(np.sqrt((f64(PO[0]) * f64(PO[0]) + f64(PO[1]) * f64(PO[1])) + f64(PO[2]) * f64(PO[2])))
            min_d, max_d, mf_max = (f32(d) for d in mps["dist"][i])
            if dist3d < min_d or dist3d > max_d:
                exits[i] = EXIT_DISTANCE; continue
            pn = mps["normal"][i].astype(f32)
            dot = (f64(PO[0]) * f64(pn[0]) + f64(PO[1]) * f64(pn[1])) + f64(PO[2]) * f64(pn[2])
            if dot < f64(0.5) * f64(dist3d):
                exits[i] = EXIT_NORMAL; continue
            level = predict_scale(mf_max, dist3d, tab["scale_factor"], tab["nlevels"])
            radius = th * tab["scale"][level]
            cand = features_in_area(kf, bounds, u, v, radius, stats)
            if not cand:
                exits[i] = EXIT_EMPTY_WINDOW; continue
            bd, bi = 256, -1
            for j in cand:
                lv = int(kps["octave"][j])
                if lv < level - 1 or lv > level:
                    bump("level_filter"); continue
                if reproj_check:
                    inv = tab["inv_sigma2"][min(max(lv, 0), tab["nlevels"] - 1)]
                    ex = u - f32(kps["x"][j]); ey = v - f32(kps["y"][j])
                    kr = f32(-1.0) if ur_all is None else f32(ur_all[j])
                    if kr >= 0:
                        er = ur - kr
                        e2 = ex * ex + ey * ey + er * er
                        if f64(e2 * inv) > 7.8:
                            bump("reject_7_8"); continue
                        bump("pass_7_8")
                    else:
                        e2 = ex * ex + ey * ey
                        if f64(e2 * inv) > 5.99:
                            bump("reject_5_99"); continue
                        bump("pass_5_99")
                d = int(POPCOUNT[mps["desc"][i] ^ desc[j]].sum())
                if d < bd:
                    bd, bi = d, j
                elif d == bd:
                    bump("tie_kept_first")
            best_dist[i] = bd
            if bi >= 0 and bd <= min(th_low, 255):
                best_idx[i] = bi; exits[i] = EXIT_FUSED
            else:
                exits[i] = EXIT_ABOVE_TH_LOW
    return dict(best_idx=best_idx, best_dist=best_dist, exit=exits, n_fused=int((exits == EXIT_FUSED).sum()))


# ---------------------------------------------------------------- the map model ----------------------------------------------------------------
class Map:
    """MapPoints with an observation dict {keyframe: keypoint}, a bad flag and a descriptor (mDescriptor); keyframes with slots (mvpMapPoints) and
    descriptors (mDescriptors).  replace() is MapPoint::Replace (src/MapPoint.cc:249-301) INCLUDING the ComputeDistinctiveDescriptors() it ends
    with on the survivor (:298, :330-403): that call may rewrite the survivor's descriptor, which a later keyframe's search reads (:1517).
    Left out, because no Fuse reads them: IncreaseFound / IncreaseVisible (:296-297), mpReplaced, Map::EraseMapPoint (:300), and nObs counting a
    stereo observation twice (:162-165) - Observations() is the number of keyframes here.  No keyframe is bad.  std::map<KeyFrame*, ...> iterates
    in pointer order; the model iterates in keyframe-index order."""

    def __init__(self, point_desc, kf_desc):
        self.desc = [np.array(d, np.uint8) for d in point_desc]
        self.kf_desc = [np.asarray(d, np.uint8) for d in kf_desc]
        self.obs = [dict() for _ in self.desc]
        self.bad = [False] * len(self.desc)
        self.slots = [[-1] * len(d) for d in self.kf_desc]
        self.recomputed = set()                       # MapPoints that survived a Replace: ComputeDistinctiveDescriptors ran on them

    def copy(self):
        m = Map([], [])
        m.desc = [d.copy() for d in self.desc]; m.kf_desc = self.kf_desc
        m.obs = [dict(o) for o in self.obs]; m.bad = list(self.bad); m.slots = [list(s) for s in self.slots]; m.recomputed = set(self.recomputed)
        return m

    def add(self, mp, kf, idx):                       # AddObservation + AddMapPoint
        if kf not in self.obs[mp]:                    # MapPoint.cc:146-160 (NLeft == -1: one index per keyframe)
            self.obs[mp][kf] = idx
        self.slots[kf][idx] = mp

    def in_keyframe(self, mp, kf):
        return kf in self.obs[mp]

    def compute_distinctive_descriptors(self, mp):    # MapPoint.cc:330-403
        if self.bad[mp] or not self.obs[mp]:
            return
        ds = [self.kf_desc[kf][idx] for kf, idx in sorted(self.obs[mp].items())]
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
            idx = obs[kf]
            if not self.in_keyframe(new, kf):
                self.slots[kf][idx] = new              # ReplaceMapPointMatch + AddObservation
                self.obs[new][kf] = idx
            else:
                self.slots[kf][idx] = -1               # EraseMapPointMatch
        self.compute_distinctive_descriptors(new)
        self.recomputed.add(new)

    def state(self):
        return [list(s) for s in self.slots], [dict(o) for o in self.obs], list(self.bad), [d.tobytes() for d in self.desc]


def flags_of(mp_map, kf, mp_list):
    """bit 0 = pMP && !isBad() && !IsInKeyFrame(pKF) (:1435-1452); list entries < 0 are NULL"""
    return np.array([1 if mp >= 0 and not mp_map.bad[mp] and not mp_map.in_keyframe(mp, kf) else 0 for mp in mp_list], np.uint8)


def list_descriptors(mp_map, mp_list):
    """GetDescriptor() of every list entry as the map holds it now (zeros for NULL entries)"""
    return np.stack([mp_map.desc[mp] if mp >= 0 else np.zeros(32, np.uint8) for mp in mp_list])


def tail(mp_map, kf, mp, best_idx):
    """:1573-1592 for one MapPoint whose search ended with bestDist <= TH_LOW"""
    held = mp_map.slots[kf][best_idx]
    if held >= 0:
        if not mp_map.bad[held]:
            if len(mp_map.obs[held]) > len(mp_map.obs[mp]):
                mp_map.replace(mp, held)
            else:
                mp_map.replace(held, mp)
    else:
        mp_map.add(mp, kf, best_idx)


def fuse_sequential(mp_map, kf_index, kf, mp_list, mps, **kw):
    """the reference: one MapPoint after the other, every search on the map as the earlier tails left it - flags AND descriptor"""
    n = 0
    for i, mp in enumerate(mp_list):
        fl = flags_of(mp_map, kf_index, [mp])
        one = dict((k, v[i:i + 1]) for k, v in mps.items())
        if mp >= 0:
            one["desc"] = mp_map.desc[mp][None, :]
        r = search(kf, one, fl, **kw)
        if r["exit"][0] == EXIT_FUSED:
            tail(mp_map, kf_index, mp, int(r["best_idx"][0])); n += 1
    return n


def replay_tail(mp_map, kf_index, mp_list, result, uploaded_desc=None, search_again=None):
    """the batched form's host half for one keyframe.  The searches ran on the INITIAL flags and descriptors.
    1. (calls with several keyframes) the list entries that survived a Replace in an earlier keyframe and whose descriptor is no longer the
       uploaded one are searched again in this keyframe: search_again(flags, descriptors) -> a search() result, flags set for them alone;
    2. in list order, re-test isBad() / IsInKeyFrame and apply the tail.
    Returns (the count of tails applied, the list positions searched again)."""
    stale = []
    if search_again is not None:
        stale = [i for i, mp in enumerate(mp_list) if mp in mp_map.recomputed and not mp_map.bad[mp] and not mp_map.in_keyframe(mp, kf_index)
                 and not np.array_equal(mp_map.desc[mp], uploaded_desc[i])]
        if stale:
            fl = np.zeros(len(mp_list), np.uint8); fl[stale] = 1
            again = search_again(fl, list_descriptors(mp_map, mp_list))
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
