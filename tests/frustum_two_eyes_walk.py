"""The checker of orbx_frustum_requests_two_eyes_device: a sequential restatement, one MapPoint after the other, in numpy binary32 / binary64
scalars with the reference's roundings, of Frame::isInFrustum's Nleft != -1 branch (reference src/Frame.cc:571-581: Frame::isInFrustumChecks,
:1181-1254, once per eye), called from the loop of Tracking::SearchLocalPoints (src/Tracking.cc:2941-2959), followed by the prelude of
ORBmatcher::SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) for F.Nleft != -1 (src/ORBmatcher.cc:50-73, :145-151, :216-222).
cv::Mat products as cv::gemm (gemm_row of tests/fuse_walk.py), cv::norm (norm3 of tests/frustum_walk.py) and Mat::dot accumulated in double
in element order, MapPoint::PredictScale through the host libm's logf (predict_scale of tests/fuse_walk.py), KannalaBrandt8::project as
kb8_project of tests/last_frame_two_eyes_walk.py over a table of four libm functions: libm_math() of the host, or header_math(lib) of the
device header compiled for the host.  The slots are appended in list order, which is what the device entry's compaction must reproduce."""
import numpy as np

from extractorb_amd import PROJ_QUERY_DTYPE, TRACK_RECORD_DTYPE
from frustum_walk import (EXIT_DISTANCE, EXIT_FAR, EXIT_FLAG, EXIT_NAMES, EXIT_NEG_DEPTH, EXIT_NOT_IN_IMAGE, EXIT_REQUEST,  # noqa: F401
                          EXIT_VIEW_COS, norm3)
from fuse_walk import gemm_row, predict_scale, tables  # noqa: F401  (tables: re-exported for the tests)
from last_frame_two_eyes_walk import header_math, kb8_project, libm_math  # noqa: F401

f32, f64 = np.float32, np.float64
UNTOUCHED = (f32(-1.0), f32(-1.0), f32(0.0), f32(0.0), f32(0.0), -1)


def rig(pose, trl, tlr):
    """the invariants of a rig frame (:1186-1197): per eye (mR [3, 3], mt [3], twc [3]).  trl, tlr: mTrl and mTlr as the Frame holds them."""
    pose, trl, tlr = (np.asarray(a, f32).reshape(3, 4) for a in (pose, trl, tlr))
    Rcw, tcw = pose[:, :3], pose[:, 3]
    ow = np.array([gemm_row(Rcw[:, r], tcw, -1.0) for r in range(3)], f32)                                   # mOw = -mRcw.t()*mtcw
    Rrl = trl[:, :3]
    mR = np.array([[gemm_row(Rrl[r], Rcw[:, c], 1.0) for c in range(3)] for r in range(3)], f32)             # Rrl * mRcw
    mt = np.array([gemm_row(Rrl[r], tcw, 1.0, trl[r, 3]) for r in range(3)], f32)                            # Rrl * mtcw + trl, one gemm
    twc = np.array([gemm_row(Rcw[:, r], tlr[:, 3], 1.0, ow[r]) for r in range(3)], f32)                      # mRwc * mTlr.col(3) + mOw
    return (Rcw.copy(), tcw.copy(), ow), (mR, mt, twc)


def eye_check(m, eye, cam, pw, pn, dist3, bounds, tab, view_cos_limit, detail=None):
    """Frame::isInFrustumChecks for one eye: (exit, track tuple).  EXIT_REQUEST = it returned true.  A check that returns false assigns nothing.
    detail (a dict) receives Pc, uv, dist, view_cos and ratio as far as the check got."""
    mR, mt, twc = eye
    minx, maxx, miny, maxy = (f32(b) for b in bounds)
    pc = [gemm_row(mR[r], pw, 1.0, mt[r]) for r in range(3)]                                                 # :1200
    depth = norm3(pc)                                                                                        # :1201
    if detail is not None:
        detail["pc"] = pc
    if pc[2] < f32(0.0):                                                                                     # :1205
        return EXIT_NEG_DEPTH, UNTOUCHED
    u, v = kb8_project(m, cam, pc[0], pc[1], pc[2])                                                          # :1210-1211
    if detail is not None:
        detail["uv"] = (u, v)
    if u < minx or u > maxx:                                                                                 # :1213
        return EXIT_NOT_IN_IMAGE, UNTOUCHED
    if v < miny or v > maxy:                                                                                 # :1215
        return EXIT_NOT_IN_IMAGE, UNTOUCHED
    PO = [f32(pw[r] - twc[r]) for r in range(3)]                                                             # :1221
    dist = norm3(PO)
    if detail is not None:
        detail["dist"] = dist
    if dist < dist3[0] or dist > dist3[1]:                                                                   # :1224
        return EXIT_DISTANCE, UNTOUCHED
    dot = (f64(PO[0]) * f64(pn[0]) + f64(PO[1]) * f64(pn[1])) + f64(PO[2]) * f64(pn[2])
    view_cos = f32(dot / f64(dist))                                                                          # :1230
    if detail is not None:
        detail["view_cos"] = view_cos
    if view_cos < f32(view_cos_limit):                                                                       # :1232
        return EXIT_VIEW_COS, UNTOUCHED
    level = predict_scale(dist3[2], dist, tab["scale_factor"], tab["nlevels"])                               # :1236
    if detail is not None:
        detail["ratio"] = f32(dist3[2]) / dist
    return EXIT_REQUEST, (u, v, f32(0.0), depth, view_cos, level)


def request(track, exit_code, eye, flag, tab, th):
    """the request of one eye from its track record: all zero apart from bit 1 of the flag unless the eye is in view of a slot"""
    if exit_code != EXIT_REQUEST:
        return (0.0, 0.0, 0.0, 0.0, 0, 0, int(flag) & 2, 0.0)
    u, v, _, _, view_cos, level = track
    r = f32(2.5) if f64(view_cos) > 0.998 else f32(4.0)                                                      # RadiusByViewingCos
    if eye == 0 and f32(th) != f32(1.0):                                                                     # :69-70; :148 has no th
        r = f32(r * f32(th))
    return (u, v, 0.0, f32(r * tab["scale"][level]), level - 1, level, 1 | (int(flag) & 2), 0.0)


def point(m, eyes, cams, pw, pn, dist3, flag, prev_depth, bounds, tab, view_cos_limit, th, far_points, th_far_points):
    """one MapPoint: ((exit L, exit R), (track L, track R), (query L, query R) or None when it is no slot, in view)"""
    if not (int(flag) & 1):                                                                                  # Tracking.cc:2945-2948
        return (EXIT_FLAG, EXIT_FLAG), (UNTOUCHED, UNTOUCHED), None, False
    res = [eye_check(m, eyes[e], cams[e], pw, pn, dist3, bounds, tab, view_cos_limit) for e in (0, 1)]
    in_l, in_r = res[0][0] == EXIT_REQUEST, res[1][0] == EXIT_REQUEST
    if not (in_l or in_r):                                                                                   # ORBmatcher.cc:53
        return (res[0][0], res[1][0]), (res[0][1], res[1][1]), None, False
    track_depth = res[0][1][3] if in_l else f32(prev_depth)                                                  # mTrackDepth as the matcher finds it
    far = bool(far_points) and bool(track_depth > f32(th_far_points))                                        # :56
    exits = tuple((EXIT_FAR if far else EXIT_REQUEST) if res[e][0] == EXIT_REQUEST else res[e][0] for e in (0, 1))
    tracks = (res[0][1], res[1][1])
    if far:
        return exits, tracks, None, True
    return exits, tracks, tuple(request(tracks[e], exits[e], e, flag, tab, th) for e in (0, 1)), True


def walk(m, mps, flags, pose, trl, tlr, cams, bounds, tab, view_cos_limit=0.5, th=1.0, far_points=False, th_far_points=0.0, n_mp=None,
         prev_depth=None, query_capacity=None):
    """mps: dict(world [M, 3], normal [M, 3], dist [M, 3] (min invariance, max invariance, mfMaxDistance), desc [M, 32]); flags [M]; pose [3, 4];
    cams = (left, right) KannalaBrandt8 parameters; prev_depth [M] or None (= 0).
    Returns dict(queries [Q, 2] (Q = query_capacity or M; the first n_queries are the slots in list order, the rest all zero), desc [n_queries,
    32], src [Q] (-1 past n_queries), n_queries (written), n_wanted (produced), track [M, 2], n_in_view)."""
    M = len(mps["world"])
    n_mp = M if n_mp is None else max(0, min(int(n_mp), M))
    Q = M if query_capacity is None else int(query_capacity)
    eyes = rig(pose, trl, tlr)
    queries = np.zeros((Q, 2), PROJ_QUERY_DTYPE); src = np.full(Q, -1, np.int32); track = np.zeros((M, 2), TRACK_RECORD_DTYPE)
    desc = []
    n = wanted = n_in_view = 0
    with np.errstate(all="ignore"):
        for i in range(M):
            fl = flags[i] if i < n_mp else 0
            exits, tracks, q, in_view = point(m, eyes, cams, mps["world"][i].astype(f32), mps["normal"][i].astype(f32), mps["dist"][i].astype(f32), fl,
                                              0.0 if prev_depth is None else prev_depth[i], bounds, tab, view_cos_limit, th, far_points, th_far_points)
            for e in (0, 1):
                track[i, e] = tuple(tracks[e]) + (exits[e],)
            n_in_view += in_view
            if q is not None:
                if wanted < Q:
                    queries[n, 0] = q[0]; queries[n, 1] = q[1]; src[n] = i; desc.append(mps["desc"][i]); n += 1
                wanted += 1
    return dict(queries=queries, desc=np.array(desc, np.uint8).reshape(-1, 32), src=src, n_queries=n, n_wanted=wanted, track=track,
                n_in_view=int(n_in_view))


def is_slot(track):
    """[M] bool: the MapPoints of a track array [M, 2] that became slots"""
    return (track["exit"] == EXIT_REQUEST).any(1)


def truncate(full, n_mp, mps, query_capacity=None):
    """what walk(..., n_mp=n_mp, query_capacity=...) returns, derived from the walk over the whole list (with query_capacity = M): every
    MapPoint is a statement of its own, so a shorter list keeps the records and slots of its entries and the rest carry FLAG"""
    M = len(full["track"])
    Q = M if query_capacity is None else int(query_capacity)
    track = full["track"].copy()
    track[n_mp:] = (-1.0, -1.0, 0.0, 0.0, 0.0, -1, EXIT_FLAG)
    wanted = int((full["src"][:full["n_queries"]] < n_mp).sum())
    n = min(wanted, Q)
    queries = np.zeros((Q, 2), PROJ_QUERY_DTYPE); queries[:n] = full["queries"][:n]
    src = np.full(Q, -1, np.int32); src[:n] = full["src"][:n]
    return dict(queries=queries, desc=mps["desc"][src[:n]], src=src, n_queries=n, n_wanted=wanted, track=track,
                n_in_view=int((track["exit"] >= EXIT_FAR).any(1).sum()))
