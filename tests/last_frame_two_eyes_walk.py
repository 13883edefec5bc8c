"""The checker of orbx_project_last_frame_two_eyes_device + orbx_search_last_frame_two_eyes_device: a fresh statement of
ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) for two-camera frames (reference src/ORBmatcher.cc:1961-2177 with
CurrentFrame.Nleft != -1) as a sequential walk in numpy binary32, with KannalaBrandt8::project (src/CameraModels/KannalaBrandt8.cpp:28-44),
Frame::GetFeaturesInArea (src/Frame.cc:655-724) over each eye's CSR grid and RAW keypoints, a holder per keypoint (not a closed flag),
rotHist as lists and ComputeThreeMaxima (:2303-2344).

The four libm functions the projection calls come from ONE table (`LIBM` below: ctypes on the host libm), so that a test can run the same
walk on the device header compiled for the host (tests/cpp/kb8_host_check.cpp: `header_math(lib)`).

An eye is a dict: k = raw keypoints (oracle_lib.KEYPOINT_DTYPE), d = descriptors [N, 32], off = grid offsets [64*48 + 1], idx = grid indices.
A last rig is two dicts (left, right): k = raw keypoints, mp = bool[N] (mvpMapPoints[i] != NULL), outlier = bool[N], obs = bool[N]
(Observations() > 0), world = float32[N, 3]."""
import ctypes as C
import ctypes.util
import math

import numpy as np

from fuse_walk import gemm_row

f32, f64 = np.float32, np.float64
GRID_COLS, GRID_ROWS, HISTO_LENGTH = 64, 48, 30
POPCOUNT = np.array([bin(b).count("1") for b in range(256)], np.int32)
PROJ_QUERY_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("radius", "<f4"), ("min_level", "<i4"), ("max_level", "<i4"),
                             ("flags", "<i4"), ("angle", "<f4")])
(EXIT_NO_MAPPOINT, EXIT_OUTLIER, EXIT_NEG_DEPTH, EXIT_LEFT_OF, EXIT_RIGHT_OF, EXIT_ABOVE, EXIT_BELOW, EXIT_REQUEST) = range(8)
INT_MIN = -2 ** 31


def _bind(lib, names):
    out = {}
    for key, name, nargs in names:
        fn = getattr(lib, name)
        fn.restype = C.c_float
        fn.argtypes = [C.c_float] * nargs
        out[key] = (lambda g: (lambda *a: f32(g(*[float(v) for v in a]))))(fn)
    return out


def libm_math():
    """sqrtf, atan2f, cosf, sinf of the host libm"""
    return _bind(C.CDLL(ctypes.util.find_library("m") or "libm.so.6"), [("sqrtf", "sqrtf", 1), ("atan2f", "atan2f", 2), ("cosf", "cosf", 1),
                                                                          ("sinf", "sinf", 1)])


def header_math(lib):
    """the same four from extractorb_amd/csrc/k_camera_kb8.hpp compiled for the host (tests/cpp/kb8_host_check.cpp)"""
    return _bind(lib, [("sqrtf", "kb8_sqrtf", 1), ("atan2f", "kb8_atan2f", 2), ("cosf", "kb8_cosf", 1), ("sinf", "kb8_sinf", 1)])


def kb8_project(m, k, x, y, z):
    """KannalaBrandt8::project(cv::Point3f): every operation rounded in binary32, in the reference's order; k = mvParameters[0..7]"""
    with np.errstate(all="ignore"):
        x, y, z = f32(x), f32(y), f32(z)
        k = [f32(v) for v in k]
        x2_plus_y2 = f32(f32(x * x) + f32(y * y))
        theta = m["atan2f"](m["sqrtf"](x2_plus_y2), z)
        psi = m["atan2f"](y, x)
        theta2 = f32(theta * theta)
        theta3 = f32(theta * theta2)
        theta5 = f32(theta3 * theta2)
        theta7 = f32(theta5 * theta2)
        theta9 = f32(theta7 * theta2)
        r = f32(f32(f32(f32(theta + f32(k[4] * theta3)) + f32(k[5] * theta5)) + f32(k[6] * theta7)) + f32(k[7] * theta9))
        u = f32(f32(f32(k[0] * r) * m["cosf"](psi)) + k[2])
        v = f32(f32(f32(k[1] * r) * m["sinf"](psi)) + k[3])
    return u, v


def project_last(m, last, Tcw, Tlw, trl, cam, bounds, scale_factors, mb, th, mono):
    """The front half (:1971-2023, :2084-2101).  Returns dict(queries = [N, 2] requests in the reference's order (left eye's keypoints, then
    the right eye's), eye / index = where each came from, exits = EXIT_* per MapPoint, form = 'forward' | 'backward' | 'neither')."""
    Tcw, Tlw, trl = np.asarray(Tcw, f32).reshape(3, 4), np.asarray(Tlw, f32).reshape(3, 4), np.asarray(trl, f32).reshape(3, 4)
    Rcw, tcw = Tcw[:, :3], Tcw[:, 3]
    twc = np.array([gemm_row(Rcw[:, r], tcw, -1.0) for r in range(3)], f32)                 # -Rcw.t()*tcw (:1974)
    tlc = np.array([gemm_row(Tlw[r, :3], twc, 1.0, Tlw[r, 3]) for r in range(3)], f32)     # Rlw*twc+tlw (:1979)
    forward = bool(tlc[2] > f32(mb)) and not mono
    backward = bool(-tlc[2] > f32(mb)) and not mono
    n = [len(last[0]["k"]), len(last[1]["k"])]
    q = np.zeros((n[0] + n[1], 2), PROJ_QUERY_DTYPE)
    exits = np.zeros(n[0] + n[1], np.int32)
    eye = np.array([0] * n[0] + [1] * n[1], np.int32)
    index = np.array(list(range(n[0])) + list(range(n[1])), np.int32)
    for a in range(n[0] + n[1]):
        E, i = last[eye[a]], int(index[a])
        if not E["mp"][i]:
            exits[a] = EXIT_NO_MAPPOINT
            continue
        if E["outlier"][i]:
            exits[a] = EXIT_OUTLIER
            continue
        xw = np.asarray(E["world"][i], f32)
        xc = np.array([gemm_row(Tcw[r, :3], xw, 1.0, Tcw[r, 3]) for r in range(3)], f32)    # Rcw*x3Dw+tcw (:1993)
        with np.errstate(all="ignore"):
            invzc = f32(f64(1.0) / f64(xc[2]))                                                # :1997
        if invzc < 0:
            exits[a] = EXIT_NEG_DEPTH
            continue
        u, v = kb8_project(m, cam, xc[0], xc[1], xc[2])                                       # :2002
        if u < f32(bounds[0]) or u > f32(bounds[1]):                                          # :2004
            exits[a] = EXIT_LEFT_OF if u < f32(bounds[0]) else EXIT_RIGHT_OF
            continue
        if v < f32(bounds[2]) or v > f32(bounds[3]):                                          # :2006
            exits[a] = EXIT_ABOVE if v < f32(bounds[2]) else EXIT_BELOW
            continue
        exits[a] = EXIT_REQUEST
        octave = int(E["k"]["octave"][i])                                                     # :2009-2010
        radius = f32(f32(th) * f32(scale_factors[octave]))                                    # :2013
        if forward:
            lv = (octave, -1)
        elif backward:
            lv = (0, octave)
        else:
            lv = (octave - 1, octave + 1)
        flags = 1 | (2 if E["obs"][i] else 0)
        xr = np.array([gemm_row(trl[r, :3], xc, 1.0, trl[r, 3]) for r in range(3)], f32)    # mTrl.R * x3Dc + mTrl.t (:2084)
        ur, vr = kb8_project(m, cam, xr[0], xr[1], xr[2])                                     # the LEFT camera's parameters (:2086)
        for e, (pu, pv) in enumerate(((u, v), (ur, vr))):
            r = q[a, e]
            r["u"], r["v"], r["radius"], r["min_level"], r["max_level"], r["flags"] = pu, pv, radius, lv[0], lv[1], flags
            r["angle"] = E["k"]["angle"][i]
    return dict(queries=q, eye=eye, index=index, exits=exits, form="forward" if forward else ("backward" if backward else "neither"))


def _to_int(x):
    """(int) of a float as the reference's x86-64 build converts it: out of range, infinite or NaN gives INT_MIN"""
    x = float(x)
    if not math.isfinite(x) or x >= 2.0 ** 31 or x < -2.0 ** 31:
        return INT_MIN
    return int(x)


def features_in_area(eye, bounds, x, y, r, min_level, max_level):
    """Frame::GetFeaturesInArea on one eye: keypoint indices in traversal order (cells by column, then row, push_back order inside)."""
    with np.errstate(all="ignore"):
        x, y, r = f32(x), f32(y), f32(r)
        w_inv = f32(GRID_COLS) / f32(f32(bounds[1]) - f32(bounds[0]))
        h_inv = f32(GRID_ROWS) / f32(f32(bounds[3]) - f32(bounds[2]))
        min_cx = max(0, _to_int(np.floor(f32(f32(f32(x - f32(bounds[0])) - r) * w_inv))))
        if min_cx >= GRID_COLS:
            return []
        max_cx = min(GRID_COLS - 1, _to_int(np.ceil(f32(f32(f32(x - f32(bounds[0])) + r) * w_inv))))
        if max_cx < 0:
            return []
        min_cy = max(0, _to_int(np.floor(f32(f32(f32(y - f32(bounds[2])) - r) * h_inv))))
        if min_cy >= GRID_ROWS:
            return []
        max_cy = min(GRID_ROWS - 1, _to_int(np.ceil(f32(f32(f32(y - f32(bounds[2])) + r) * h_inv))))
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


def rotation_bin(angle1, angle2):
    rot = f32(f32(angle1) - f32(angle2))                                                      # :2073-2078
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    v = float(f32(rot * f32(f32(1.0) / f32(HISTO_LENGTH))))
    b = int(math.floor(v + 0.5)) if v >= 0 else -int(math.floor(-v + 0.5))                    # round(): halves away from zero
    if b == HISTO_LENGTH:
        b = 0
    assert 0 <= b < HISTO_LENGTH
    return b


def three_maxima(sizes):
    """ORBmatcher::ComputeThreeMaxima (:2303-2344)"""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if f32(max2) < f32(f32(0.1) * f32(max1)):
        ind2 = ind3 = -1
    elif f32(max3) < f32(f32(0.1) * f32(max1)):
        ind3 = -1
    return ind1, ind2, ind3


def search(queries, qdesc, left, right, bounds, occupied=None, max_distance=100, check_orientation=True):
    """The search (:2013-2174) over requests [NQ, 2] (L, R) in order.  Returns dict(n = the return value, matches = [left list, right list]
    (request whose MapPoint the keypoint holds afterwards, -1 = none), occupied = [left, right] (its holder has observations),
    accepted = [NQ, 2] keypoint each sub-search took (-1 = none), suppressed = R sub-searches not run because L's area result was empty,
    closure_changed = sub-searches whose decision differs from the one taken against the occupancy on entry alone,
    bins = rotHist sizes, maxima = the three kept bins, dropped = entries cleared)."""
    eyes = [left, right]
    n = [len(left["k"]), len(right["k"])]
    holder = [[[-1, bool(occupied[e][i]) if occupied is not None else False] for i in range(n[e])] for e in (0, 1)]
    entry = [[h[1] for h in holder[e]] for e in (0, 1)]
    bits = [np.asarray(E["d"], np.uint8).reshape(-1, 32) for E in eyes]
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    accepted = np.full((len(queries), 2), -1, np.int32)
    nm = suppressed = closure_changed = 0

    def best_of(e, cands, qd, closed):
        best, best_i = 256, -1
        for i in cands:
            if closed(i):                                    # :2036-2038 / :2111-2113
                continue
            dist = int(POPCOUNT[np.bitwise_xor(qd, bits[e][i])].sum())
            if dist < best:
                best, best_i = dist, i
        return best_i if best <= max_distance else -1       # :2059 / :2126

    for j in range(len(queries)):
        qd = np.asarray(qdesc[j], np.uint8)
        for e in (0, 1):
            q = queries[j][e]
            if not q["flags"] & 1:
                continue
            cands = features_in_area(eyes[e], bounds, q["u"], q["v"], q["radius"], int(q["min_level"]), int(q["max_level"]))
            if e == 0 and not cands:                         # :2024: `continue` - the MapPoint's right sub-search is skipped too
                suppressed += int(queries[j][1]["flags"] & 1)
                break
            got = best_of(e, cands, qd, lambda i: holder[e][i][1])
            closure_changed += got != best_of(e, cands, qd, lambda i: entry[e][i])
            if got < 0:
                continue
            holder[e][got] = [j, bool(q["flags"] & 2)]
            accepted[j, e] = got
            nm += 1
            if check_orientation:
                rot_hist[rotation_bin(q["angle"], eyes[e]["k"]["angle"][got])].append((e, got))
    sizes = [len(b) for b in rot_hist]
    maxima, dropped = (-1, -1, -1), 0
    if check_orientation:                                    # :2155-2174
        maxima = three_maxima(sizes)
        for b in range(HISTO_LENGTH):
            if b not in maxima:
                for e, i in rot_hist[b]:
                    holder[e][i] = [-1, False]
                    nm -= 1
                    dropped += 1
    return dict(n=nm, matches=[[h[0] for h in holder[e]] for e in (0, 1)], occupied=[[int(h[1]) for h in holder[e]] for e in (0, 1)],
                accepted=accepted, suppressed=suppressed, closure_changed=closure_changed, bins=sizes, maxima=maxima, dropped=dropped)
