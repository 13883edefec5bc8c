"""The checker of orbx_update_map_points_device and orbx_update_map_points_two_eyes_device: a sequential statement of
MapPoint::ComputeDistinctiveDescriptors (reference src/MapPoint.cc:330-403) and MapPoint::UpdateNormalAndDepth (:427-494), one listed MapPoint
after the other, one observation after the other.  The normal and depth half is written ONCE over a number kind and exists in two kinds:
  Binary32  numpy binary32 scalars with the roundings of DESIGN.md section 2 where a cv::Mat / cv::MatExpr hides them (quoted below), built
            on fuse_walk.gemm_row and fuse_walk.camera_centre.  The library is held to this kind byte for byte;
  Float64   the same control flow in float64 on the same binary32 inputs: where the binary32 kind rounds, this kind does nothing.
The descriptor half is integers and has no kind.  Its Hamming rows are one numpy product per list (a 1024-long list is 1024 x 1024
distances), its median is the reference's own form, sorted(row)[int(0.5*(N-1))]; median_by_count() is the form the kernel uses.
A scene is the arrays of the C entries (tests/map_point_update_scenes.py).  OpenCV is not available to this project: parity unpinned."""
import math

import numpy as np

from fuse_walk import camera_centre, gemm_row

f32, f64 = np.float32, np.float64
OK, EMPTY, NO_DESCRIPTOR, BAD_INDEX, TOO_LONG = range(5)
STATUS_NAMES = ("ok", "empty", "no_descriptor", "bad_index", "too_long")
MAX_OBSERVATIONS = 1024
POISON_BYTE, POISON_FLOAT = 0xEE, -7.0


class Binary32:
    T = f32

    def centre(self, pose):
        return camera_centre(np.asarray(pose, f32))                 # Ow = -Rcw.t()*tcw, one cv::gemm row per element, alpha -1

    def gemm(self, a, b, c):
        return gemm_row(a, b, 1.0, c)                               # products and sums in double, the float addend, rounded to float once

    def from_double(self, x):
        return f32(x)                                               # (float)(1.0 / norm), (float)cv::norm


class Float64:
    T = f64

    def centre(self, pose):
        pose = np.asarray(pose, f64)
        return -pose[:, :3].T @ pose[:, 3]

    def gemm(self, a, b, c):
        return float(np.dot(np.asarray(a, f64), np.asarray(b, f64))) + float(c)

    def from_double(self, x):
        return f64(x)


def centres(N, s):
    """the camera centre of every device frame: GetCameraCenter, and for the right eye of a rig GetRightCameraCenter = Rwl*mTlr.t + Ow
    (KeyFrame.cc:1232-1240: one gemm row with the float Ow as addend; row r of Rwl is column r of Rcw)"""
    out = []
    for pose in s["poses"]:
        Ow = N.centre(pose)
        out.append(Ow)
        if s["two_eyes"]:
            pose_k, tlr = np.asarray(pose, N.T), np.asarray(s["tlr"], N.T)
            out.append(np.array([N.gemm(pose_k[:, r], tlr[:, 3], Ow[r]) for r in range(3)], N.T))
    return out


def norm64(d):
    """cv::norm: squares summed in element order and rooted in double"""
    return math.sqrt((float(d[0]) * float(d[0]) + float(d[1]) * float(d[1])) + float(d[2]) * float(d[2]))


def unit(N, pos, Ow):
    """normali/cv::norm(normali) as cv::scaleAdd sees it: normali * (float)(1.0/norm), the difference and each product rounded"""
    T = N.T
    d = [T(T(pos[c]) - T(Ow[c])) for c in range(3)]
    inv = N.from_double(1.0 / norm64(d))
    return [T(d[c] * inv) for c in range(3)]


def normal_and_depth(N, s, cen, frames, ref_frame, ref_octave, pos):
    """(mNormalVector, (0.8f*mfMinDistance, 1.2f*mfMaxDistance, mfMaxDistance)) of one point; frames: the device frame of every entry"""
    T = N.T
    normal = [T(0), T(0), T(0)]
    for f in frames:                                                # sequentially, in list order, one rounding per step (:457, :463)
        t = unit(N, pos, cen[f])
        normal = [T(t[c] + normal[c]) for c in range(3)]
    inv_n = N.from_double(1.0 / float(len(frames)))                 # normal/n
    normal = [T(normal[c] * inv_n) for c in range(3)]
    left = ref_frame & ~1 if s["two_eyes"] else ref_frame           # :468: GetCameraCenter() of pRefKF, the left centre
    d = [T(T(pos[c]) - T(cen[left][c])) for c in range(3)]
    dist = N.from_double(norm64(d))
    scale = s["scale"].astype(T)
    level = min(max(int(ref_octave), 0), s["nlevels"] - 1)          # (clamped, as everywhere in the library)
    max_d = T(dist * scale[level])
    min_d = T(max_d / scale[s["nlevels"] - 1])
    return normal, [T(T(f32(0.8)) * min_d), T(T(f32(1.2)) * max_d), max_d]      # 0.8f, 1.2f: the source's float constants in both kinds


def hamming_matrix(descs):
    """[P, P] int32 Hamming distances of P descriptors [P, 32] uint8"""
    bits = np.unpackbits(np.asarray(descs, np.uint8), axis=1).astype(np.int32)
    return bits @ (1 - bits).T + (1 - bits) @ bits.T


def median_sorted(row):
    return int(np.sort(row)[int(0.5 * (len(row) - 1))])             # :390-391


def median_by_count(row):
    """the smallest v with #{j : row[j] <= v} >= (N-1)/2 + 1, by nine bisection steps over 0 .. 256"""
    need = (len(row) - 1) // 2 + 1
    lo, hi = 0, 256
    for _ in range(9):
        mid = (lo + hi) >> 1
        if lo < hi:
            if int((row <= mid).sum()) >= need:
                hi = mid
            else:
                lo = mid + 1
    return lo


def distinctive(descs):
    """(BestIdx, BestMedian) of the descriptors that take part, in order: the first row with the smallest median (strict <, :393)"""
    D = hamming_matrix(descs)
    medians = np.sort(D, axis=1)[:, int(0.5 * (len(descs) - 1))]
    best = int(np.argmin(medians))                                  # (the first of equals)
    return best, int(medians[best])


def tables(s, T=f32):
    n = len(s["world"])
    return dict(mp_desc=np.full((n, 32), POISON_BYTE, np.uint8), mp_normal=np.full((n, 3), POISON_FLOAT, T), mp_dist=np.full((n, 3), POISON_FLOAT, T))


def update(N, s, what=3):
    """dict(mp_desc, mp_normal, mp_dist: the tables, poison where nothing was written; best, best_median, status per listed point)"""
    P = len(s["obs_off"]) - 1
    out = tables(s, N.T)
    best = np.full(P, -1, np.int32); best_median = np.full(P, -1, np.int32); status = np.zeros(P, np.uint8)
    cen = centres(N, s) if what & 2 else None
    B = len(s["n_out"])
    with np.errstate(all="ignore"):
        for m in range(P):
            off0 = int(s["obs_off"][m]); n = max(int(s["obs_off"][m + 1]) - off0, 0)
            if n == 0:
                status[m] = EMPTY; continue
            if n > MAX_OBSERVATIONS:
                status[m] = TOO_LONG; continue
            slot = m if s["slot"] is None else int(s["slot"][m])
            ref = int(s["ref"][m])
            ok = off0 >= 0 and slot >= 0 and 0 <= ref < n
            if ok:
                obs = s["obs"][off0:off0 + n]
                fr, rows = obs[:, 0], obs[:, 1]
                ok = bool(np.all((fr >= 0) & (fr < B)))
                ok = ok and bool(np.all((rows >= 0) & (rows < np.clip(s["n_out"][np.clip(fr, 0, B - 1)], 0, s["capacity"]))))
            if not ok:
                status[m] = BAD_INDEX; continue
            if what & 1:
                part = np.arange(n) if s["flags"] is None else np.flatnonzero((s["flags"][off0:off0 + n] & 1) == 0)      # :353
                if len(part) == 0:
                    status[m] = NO_DESCRIPTOR                        # :366
                else:
                    descs = s["desc"][fr[part], rows[part]]
                    b, med = distinctive(descs)
                    out["mp_desc"][slot] = descs[b]
                    best[m], best_median[m] = b, med
            if what & 2:
                rf, rr = int(fr[ref]), int(rows[ref])
                normal, dist = normal_and_depth(N, s, cen, [int(f) for f in fr], rf, s["octave"][rf, rr], s["world"][slot])
                out["mp_normal"][slot] = normal; out["mp_dist"][slot] = dist
    out.update(best=best, best_median=best_median, status=status)
    return out
