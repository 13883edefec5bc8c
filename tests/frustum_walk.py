"""The checker of orbx_frustum_requests_device: a sequential restatement, one MapPoint after the other, in numpy binary32 / binary64 scalars with
the reference's roundings, of
  mode 0  Frame::isInFrustum, the Nleft == -1 branch (reference src/Frame.cc:493-570, called from src/Tracking.cc:2941-2959) followed by the
          prelude of ORBmatcher::SearchByProjection(F, vpMapPoints, th, bFarPoints, thFarPoints) (src/ORBmatcher.cc:50-73, :216-222);
  mode 1  the projection of pKF's MapPoints in ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (:2183-2230).
cv::Mat products as cv::gemm (gemm_row of tests/fuse_walk.py), cv::norm and Mat::dot accumulated in double in element order,
MapPoint::PredictScale through the host libm's logf (predict_scale of tests/fuse_walk.py).  The requests are appended in list order, which is
what the device entry's compaction must reproduce."""
import numpy as np

from extractorb_amd import PROJ_QUERY_DTYPE, TRACK_RECORD_DTYPE
from fuse_walk import gemm_row, predict_scale, tables  # noqa: F401  (tables: re-exported for the tests)

f32, f64 = np.float32, np.float64
LOCAL_MAP, RELOCALIZATION = 0, 1
EXIT_FLAG, EXIT_NEG_DEPTH, EXIT_NOT_IN_IMAGE, EXIT_DISTANCE, EXIT_VIEW_COS, EXIT_FAR, EXIT_REQUEST = range(7)
EXIT_NAMES = ("flag", "negdepth", "notinimage", "distance", "viewcos", "far", "request")


def norm3(v):
    """cv::norm of three CV_32F elements"""
    return f32(np.sqrt((f64(v[0]) * f64(v[0]) + f64(v[1]) * f64(v[1])) + f64(v[2]) * f64(v[2])))


def point(pw, pn, dist3, angle, flag, pose, cam, bounds, tab, mode, mbf, view_cos_limit, th, far_points, th_far_points):
    """one MapPoint: (exit, track tuple (proj_x, proj_y, proj_xr, depth, view_cos, level), query tuple or None)"""
    fx, fy, cx, cy = (f32(c) for c in cam[:4])
    minx, maxx, miny, maxy = (f32(b) for b in bounds)
    R, t = pose[:, :3], pose[:, 3]
    m1, zero = f32(-1.0), f32(0.0)
    if not (int(flag) & 1):
        return EXIT_FLAG, (m1, m1, zero, zero, zero, -1), None
    pc = [gemm_row(R[r], pw, 1.0, t[r]) for r in range(3)]                       # mRcw*P+mtcw
    depth = invz = zero
    if mode == LOCAL_MAP:
        depth = norm3(pc)                                                        # Frame.cc:508
        invz = f32(1.0) / pc[2]                                                  # :512
        if pc[2] < f32(0.0):
            return EXIT_NEG_DEPTH, (m1, m1, zero, zero, zero, -1), None
    u = fx * pc[0] / pc[2] + cx                                                  # Pinhole::project
    v = fy * pc[1] / pc[2] + cy
    if u < minx or u > maxx:
        return EXIT_NOT_IN_IMAGE, (m1, m1, zero, zero, zero, -1), None
    if v < miny or v > maxy:
        return EXIT_NOT_IN_IMAGE, (m1, m1, zero, zero, zero, -1), None
    Ow = [gemm_row(R[:, r], t, -1.0) for r in range(3)]                          # -mRcw.t()*mtcw
    PO = [pw[r] - Ow[r] for r in range(3)]
    dist = norm3(PO)
    if dist < dist3[0] or dist > dist3[1]:
        return EXIT_DISTANCE, (u, v, zero, zero, zero, -1), None
    view_cos = zero
    if mode == LOCAL_MAP:
        dot = (f64(PO[0]) * f64(pn[0]) + f64(PO[1]) * f64(pn[1])) + f64(PO[2]) * f64(pn[2])
        view_cos = f32(dot / f64(dist))                                          # :545
        if view_cos < f32(view_cos_limit):
            return EXIT_VIEW_COS, (u, v, zero, zero, zero, -1), None
    level = predict_scale(dist3[2], dist, tab["scale_factor"], tab["nlevels"])
    if mode == RELOCALIZATION:
        return EXIT_REQUEST, (u, v, zero, zero, zero, level), (u, v, zero, f32(th) * tab["scale"][level], level - 1, level + 1, 3, f32(angle))
    xr = u - f32(mbf) * invz
    track = (u, v, xr, depth, view_cos, level)
    if far_points and depth > f32(th_far_points):
        return EXIT_FAR, track, None
    r = f32(2.5) if f64(view_cos) > 0.998 else f32(4.0)                          # RadiusByViewingCos: a float against a double literal
    if f32(th) != f32(1.0):
        r = r * f32(th)
    return EXIT_REQUEST, track, (u, v, xr, r * tab["scale"][level], level - 1, level, 1 | (int(flag) & 2), zero)


def walk(mps, flags, pose, cam, bounds, tab, mode=LOCAL_MAP, mbf=40.0, view_cos_limit=0.5, th=1.0, far_points=False, th_far_points=0.0, n_mp=None,
         angle=None):
    """mps: dict(world [M, 3], normal [M, 3], dist [M, 3] (min invariance, max invariance, mfMaxDistance), desc [M, 32]); flags [M]; pose [3, 4].
    Returns dict(queries [M] (the first n_queries are the requests in list order, the rest all zero), desc [n_queries, 32], src [M] (-1 past
    n_queries), n_queries, track [M], n_in_view)."""
    M = len(mps["world"])
    n_mp = M if n_mp is None else max(0, min(int(n_mp), M))
    pose = np.asarray(pose, f32)
    queries = np.zeros(M, PROJ_QUERY_DTYPE); src = np.full(M, -1, np.int32); track = np.zeros(M, TRACK_RECORD_DTYPE)
    desc = []
    n = n_in_view = 0
    with np.errstate(all="ignore"):
        for i in range(M):
            fl = flags[i] if i < n_mp else 0
            ex, tr, q = point(mps["world"][i].astype(f32), mps["normal"][i].astype(f32), mps["dist"][i].astype(f32),
                              0.0 if angle is None else angle[i], fl, pose, cam, bounds, tab, mode, mbf, view_cos_limit, th, far_points, th_far_points)
            track[i] = tuple(tr) + (ex,)
            n_in_view += ex >= EXIT_FAR
            if q is not None:
                queries[n] = q; src[n] = i; desc.append(mps["desc"][i]); n += 1
    return dict(queries=queries, desc=np.array(desc, np.uint8).reshape(-1, 32), src=src, n_queries=n, track=track, n_in_view=int(n_in_view))


def truncate(full, n_mp, mps):
    """what walk(..., n_mp=n_mp) returns, derived from the walk over the whole list: every MapPoint is a statement of its own, so a shorter
    list keeps the records and requests of its entries and the rest carry FLAG (tests/test_frustum_requests.py holds this against the walk)"""
    M = len(full["track"])
    track = full["track"].copy()
    track[n_mp:] = (-1.0, -1.0, 0.0, 0.0, 0.0, -1, EXIT_FLAG)
    n = int((full["src"][:full["n_queries"]] < n_mp).sum())
    queries = np.zeros(M, PROJ_QUERY_DTYPE); queries[:n] = full["queries"][:n]
    src = np.full(M, -1, np.int32); src[:n] = full["src"][:n]
    return dict(queries=queries, desc=mps["desc"][src[:n]], src=src, n_queries=n, track=track, n_in_view=int((track["exit"] >= EXIT_FAR).sum()))
