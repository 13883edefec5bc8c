"""The checker of orbx_search_by_projection_two_eyes_device: a fresh statement of ORBmatcher::SearchByProjection(F, vpMapPoints, th, ...)
for two-camera frames (reference src/ORBmatcher.cc:44-213, F.Nleft != -1) as a sequential walk over Python lists, with
Frame::GetFeaturesInArea (src/Frame.cc:655-724) over each eye's CSR grid and RAW keypoints, and a holder per keypoint (not a closed flag).

An eye is a dict: k = raw keypoints (oracle_lib.KEYPOINT_DTYPE), d = descriptors [N, 32], off = grid offsets [64*48 + 1], idx = grid indices.
queries: [NQ, 2] of oracle_lib.PROJ_QUERY_DTYPE (left, right request of MapPoint i); qdesc: [NQ, 32]."""
import numpy as np

GRID_COLS, GRID_ROWS = 64, 48
POPCOUNT = np.array([bin(b).count("1") for b in range(256)], np.int32)


def features_in_area(eye, bounds, x, y, r, min_level, max_level):
    """Frame::GetFeaturesInArea on one eye: keypoint indices in traversal order (cells by column, then row, push_back order inside)."""
    f32 = np.float32
    x, y, r = f32(x), f32(y), f32(r)
    w_inv = f32(GRID_COLS) / f32(f32(bounds[1]) - f32(bounds[0]))
    h_inv = f32(GRID_ROWS) / f32(f32(bounds[3]) - f32(bounds[2]))
    min_cx = max(0, int(np.floor(f32(f32(f32(x - f32(bounds[0])) - r) * w_inv))))
    if min_cx >= GRID_COLS:
        return []
    max_cx = min(GRID_COLS - 1, int(np.ceil(f32(f32(f32(x - f32(bounds[0])) + r) * w_inv))))
    if max_cx < 0:
        return []
    min_cy = max(0, int(np.floor(f32(f32(f32(y - f32(bounds[2])) - r) * h_inv))))
    if min_cy >= GRID_ROWS:
        return []
    max_cy = min(GRID_ROWS - 1, int(np.ceil(f32(f32(f32(y - f32(bounds[2])) + r) * h_inv))))
    if max_cy < 0:
        return []
    check_levels = min_level > 0 or max_level >= 0
    k, off, idx = eye["k"], eye["off"], eye["idx"]
    out = []
    for ix in range(min_cx, max_cx + 1):
        for iy in range(min_cy, max_cy + 1):
            c = ix * GRID_ROWS + iy
            for i in idx[off[c]:off[c + 1]]:
                i = int(i)
                if check_levels:
                    if k["octave"][i] < min_level or (max_level >= 0 and k["octave"][i] > max_level):
                        continue
                if abs(f32(k["x"][i] - x)) < r and abs(f32(k["y"][i] - y)) < r:
                    out.append(i)
    return out


def search_two_eyes(queries, qdesc, left, right, bounds, left_to_right=None, right_to_left=None, occupied=None, nnratio=0.8,
                    max_distance=100):
    """Returns dict(n = the return value, matches = [left list, right list] (MapPoint the keypoint holds afterwards if one was written,
    else -1), occupied = [left, right] (its holder has observations), reopens = writes of a MapPoint without observations onto a keypoint
    whose holder had observations (the corner the kernel settles by its walk))."""
    eyes = [left, right]
    n = [len(left["k"]), len(right["k"])]
    # holder per keypoint: (MapPoint written by this call or -1, holder has Observations() > 0); a caller's MapPoint holds it on entry
    holder = [[[-1, bool(occupied[e][i]) if occupied is not None else False] for i in range(n[e])] for e in (0, 1)]
    maps = [left_to_right, right_to_left]
    bits = [np.asarray(e["d"], np.uint8) for e in eyes]
    nm, reopens = 0, 0

    def partner(e, i):           # mvLeftToRightMatch / mvRightToLeftMatch; out of range = none
        m = maps[e]
        if m is None:
            return -1
        v = int(m[i])
        return v if 0 <= v < n[1 - e] else -1

    def write(e, i, mp, obs):
        nonlocal reopens
        if holder[e][i][1] and not obs:
            reopens += 1
        holder[e][i] = [mp, obs]

    def sub_search(e, q, qd):
        """None (nothing accepted, the next sub-search runs), "ratio" (rejected by the ratio test) or the keypoint index"""
        cands = features_in_area(eyes[e], bounds, q["u"], q["v"], q["radius"], int(q["min_level"]), int(q["max_level"]))
        if not cands:
            return None
        best, best2, lvl, lvl2, best_i = 256, 256, -1, -1, -1
        for i in cands:
            if holder[e][i][1]:                          # :89-91 / :158-160
                continue
            dist = int(POPCOUNT[np.bitwise_xor(qd, bits[e][i])].sum())
            if dist < best:
                best2, lvl2 = best, lvl
                best, lvl, best_i = dist, int(eyes[e]["k"]["octave"][i]), i
            elif dist < best2:
                best2, lvl2 = dist, int(eyes[e]["k"]["octave"][i])
        if best > max_distance:
            return None
        if lvl == lvl2 and np.float32(best) > np.float32(np.float32(nnratio) * np.float32(best2)):
            return "ratio"
        return best_i

    for mp in range(len(queries)):
        qL, qR = queries[mp][0], queries[mp][1]
        qd = np.asarray(qdesc[mp], np.uint8)
        if qL["flags"] & 1:
            got = sub_search(0, qL, qd)
            if got == "ratio":
                continue                                 # :127: the MapPoint's right sub-search is skipped too
            if got is not None:
                obs = bool(qL["flags"] & 2)
                write(0, got, mp, obs); nm += 1
                r = partner(0, got)
                if r >= 0:
                    write(1, r, mp, obs); nm += 1
        if qR["flags"] & 1:
            got = sub_search(1, qR, qd)
            if got is not None and got != "ratio":
                obs = bool(qR["flags"] & 2)
                lft = partner(1, got)
                if lft >= 0:
                    write(0, lft, mp, obs); nm += 1
                write(1, got, mp, obs); nm += 1
    return dict(n=nm, matches=[[h[0] for h in holder[e]] for e in (0, 1)], occupied=[[int(h[1]) for h in holder[e]] for e in (0, 1)],
                reopens=reopens)
