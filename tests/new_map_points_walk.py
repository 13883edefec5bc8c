"""The checker of orbx_create_new_map_points_device and orbx_create_new_map_points_two_eyes_device: a sequential statement of the triangulation
loop of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:481-707), one match after the other, one function per group of
reference lines.  The statement is written ONCE over a number kind and exists in two kinds, side by side:
  Binary32  numpy binary32 scalars over the host libm (sqrtf, atan2f, cosf, sinf, tanf), every operation rounded on its own, with the
            roundings of DESIGN.md section 2 where a cv::Mat / cv::MatExpr hides them (quoted at each place below); vt.row(3) is the project's
            own Jacobi (tests/triangulation_two_eyes_walk.py: null_vector4).  The library is held to this kind byte for byte;
  Float64   the same control flow in float64 with np.linalg.svd and the math module: the independent statement the margin check compares the
            decisions with.  Where the binary32 kind rounds a double to float, this kind does nothing.
A one-camera keyframe is dict(pose [3, 4] f32, kps_un, kps (raw mvKeys), u_right [n] or None, depth [n] or None); a two-camera keyframe is
dict(pose, eyes = (left, right)), an eye dict(kps = the RAW keypoints).  cams: one camera (fx, fy, cx, cy, ...) or the pair of eight-float
KannalaBrandt8 parameter lists.  OpenCV is not available to this project: parity unpinned."""
import math

import numpy as np

import last_frame_two_eyes_walk as K
import triangulation_two_eyes_scenes as S2
import triangulation_two_eyes_walk as W
from fuse_two_eyes_walk import keyframe_rig
from fuse_walk import camera_centre, gemm_row

f32 = np.float32
(TRIANGULATED, STEREO_1, STEREO_2, ZERO_W, LOW_PARALLAX, EMPTY_STEREO, BEHIND_1, BEHIND_2, REPROJ_1, REPROJ_2, ZERO_DIST, FAR, SCALE,
 BAD_INDEX) = range(14)
EXIT_NAMES = ("triangulated", "stereo_1", "stereo_2", "zero_w", "low_parallax", "empty_stereo", "behind_1", "behind_2", "reproj_1", "reproj_2",
              "zero_dist", "far", "scale", "bad_index")


class Binary32:
    """numpy binary32 over the host libm; m = triangulation_two_eyes_walk.libm_math()"""
    T = f32

    def __init__(self, m=None):
        self.m = m or W.libm_math()

    def views(self, pose, tlr):
        """[(Rcw, tcw, Ow)] per eye: KeyFrame's getters (KeyFrame.cc:118, :1232-1262), each product one cv::gemm row"""
        pose = np.asarray(pose, f32)
        if tlr is None:
            return [(pose[:, :3].copy(), pose[:, 3].copy(), camera_centre(pose))]
        return list(keyframe_rig(pose, tlr))

    def gemm(self, a, b, c=None):
        return gemm_row(a, b, 1.0, c)                     # products and sums in double, the addend, rounded to float once

    def dot64(self, a, b):
        return float(a[0]) * float(b[0]) + float(a[1]) * float(b[1]) + float(a[2]) * float(b[2])      # Mat::dot / cv::norm accumulate in double

    def unproject(self, cam, u, v, two_eyes):
        if two_eyes:
            return W.unproject(self.m, cam, u, v)
        return f32(f32(f32(u) - f32(cam[2])) / f32(cam[0])), f32(f32(f32(v) - f32(cam[3])) / f32(cam[1]))      # Pinhole.cpp:59-62

    def project(self, cam, x, y, z, two_eyes):
        if two_eyes:
            return K.kb8_project(self.m, cam, x, y, z)
        return f32(f32(f32(f32(cam[0]) * x) / z) + f32(cam[2])), f32(f32(f32(f32(cam[1]) * y) / z) + f32(cam[3]))      # Pinhole.cpp:30-33

    def null_vector(self, A):
        return W.null_vector4(self.m, A)

    def stereo_cos(self, mb, depth):
        """cos(2*atan2(mb/2, depth)) with the float overloads (`using namespace std`, TemplatedVocabulary.h:36)"""
        return self.m["cosf"](f32(f32(2.0) * self.m["atan2f"](f32(f32(mb) / f32(2.0)), f32(depth))))


class Float64:
    T = np.float64

    def views(self, pose, tlr):
        pose = np.asarray(pose, np.float64)
        eyes = [(pose[:, :3], pose[:, 3])] if tlr is None else list(S2.eye_poses64(pose, tlr))
        return [(R, t, -R.T @ t) for R, t in eyes]

    def gemm(self, a, b, c=None):
        return float(np.dot(np.asarray(a, np.float64), np.asarray(b, np.float64))) + (0.0 if c is None else float(c))

    def dot64(self, a, b):
        return float(np.dot(np.asarray(a, np.float64), np.asarray(b, np.float64)))

    def unproject(self, cam, u, v, two_eyes):
        if two_eyes:
            return S2.unproject64(cam, u, v)
        return (float(u) - float(cam[2])) / float(cam[0]), (float(v) - float(cam[3])) / float(cam[1])

    def project(self, cam, x, y, z, two_eyes):
        if two_eyes:
            return S2.project64(cam, (x, y, z))
        return float(cam[0]) * x / z + float(cam[2]), float(cam[1]) * y / z + float(cam[3])

    def null_vector(self, A):
        return list(np.linalg.svd(np.asarray(A, np.float64))[2][3])

    def stereo_cos(self, mb, depth):
        return math.cos(2 * math.atan2(float(mb) / 2, float(depth)))


# ---- :483-501: the two observations of a match ----
def observation(N, kf, idx, two_eyes):
    """None for an index outside [0, N) (the reference would index out of bounds), else dict(eye = bRight, u, v, octave, ur = kp_ur,
    stereo = bStereo, depth = mvDepth, raw = mvKeys[idx].pt)"""
    T = N.T
    if two_eyes:
        n_left = len(kf["eyes"][0]["kps"])
        if not 0 <= idx < n_left + len(kf["eyes"][1]["kps"]):
            return None
        eye = 1 if idx >= n_left else 0                                              # :491, :500
        kp = kf["eyes"][eye]["kps"][idx - eye * n_left]                              # :486-488: mvKeys / mvKeysRight
        return dict(eye=eye, u=T(kp["x"]), v=T(kp["y"]), octave=int(kp["octave"]), ur=T(-1.0), stereo=False, depth=T(0), raw=None)      # :490: mpCamera2 is set
    if not 0 <= idx < len(kf["kps_un"]):
        return None
    kp = kf["kps_un"][idx]
    ur = T(-1.0) if kf.get("u_right") is None else T(kf["u_right"][idx])
    stereo = bool(ur >= 0)                                                           # :490, :499
    return dict(eye=0, u=T(kp["x"]), v=T(kp["y"]), octave=int(kp["octave"]), ur=ur, stereo=stereo,
                depth=T(kf["depth"][idx]) if stereo else T(0), raw=(T(kf["kps"]["x"][idx]), T(kf["kps"]["y"][idx])) if stereo else None)


# ---- :571-576 ----
def rays_and_parallax(N, view1, view2, cam1, cam2, o1, o2, two_eyes):
    T = N.T
    xn1 = [*N.unproject(cam1, o1["u"], o1["v"], two_eyes), T(1.0)]
    xn2 = [*N.unproject(cam2, o2["u"], o2["v"], two_eyes), T(1.0)]
    ray1 = [N.gemm(view1[0][:, r], xn1) for r in range(3)]                           # Rwc1*xn1, Rwc = Rcw.t()
    ray2 = [N.gemm(view2[0][:, r], xn2) for r in range(3)]
    with np.errstate(all="ignore"):
        cos_rays = T(np.float64(N.dot64(ray1, ray2)) / (np.sqrt(np.float64(N.dot64(ray1, ray1))) * np.sqrt(np.float64(N.dot64(ray2, ray2)))))      # rounded to float once
    return xn1, xn2, cos_rays


# ---- :578-587 ----
def stereo_parallax(N, cos_rays, o1, o2, mb):
    T = N.T
    cos1 = cos2 = T(cos_rays + T(1.0))
    if o1["stereo"]:
        cos1 = T(N.stereo_cos(mb, o1["depth"]))
    elif o2["stereo"]:                                                               # ELSE if: with both stereo only the first is replaced
        cos2 = T(N.stereo_cos(mb, o2["depth"]))
    return cos1, cos2, (cos2 if cos2 < cos1 else cos1)                               # std::min


# ---- :590-623 ----
def branch(cos_rays, cos1, cos2, cos_stereo, o1, o2):
    """'svd', 'stereo1', 'stereo2' or None (:622).  < cosParallaxStereo compares floats, > 0 an int, < 0.9998 in double; mbInertial changes nothing"""
    if cos_rays < cos_stereo and cos_rays > 0 and (o1["stereo"] or o2["stereo"] or float(cos_rays) < 0.9998):
        return "svd"
    if o1["stereo"] and cos1 < cos2:
        return "stereo1"
    if o2["stereo"] and cos2 < cos1:
        return "stereo2"
    return None


# ---- :594-609 ----
def triangulate(N, xn1, xn2, view1, view2):
    """(x3D or None for x3D[3] == 0, vt)"""
    T = N.T
    rows = []
    for xn, (R, t, _) in ((xn1, view1), (xn2, view2)):
        Tcw = [[T(R[r][0]), T(R[r][1]), T(R[r][2]), T(t[r])] for r in range(3)]
        for r in (0, 1):
            rows.append([T(T(xn[r] * Tcw[2][c]) - Tcw[r][c]) for c in range(4)])     # a scaled row difference, each rounded in float
    vt = N.null_vector(rows)
    if vt[3] == 0:
        return None, vt                                                              # :605
    with np.errstate(all="ignore"):
        return [T(vt[r] / vt[3]) for r in range(3)], vt                              # a division per element


# ---- KeyFrame::UnprojectStereo (KeyFrame.cc:821-834) ----
def unproject_stereo(N, view, cam, o):
    T = N.T
    z = o["depth"]
    if not z > 0:
        return None                                                                  # cv::Mat(): x3Dt.empty() at :627
    inv_fx, inv_fy = T(T(1.0) / T(cam[0])), T(T(1.0) / T(cam[1]))                    # KeyFrame's invfx, invfy
    x = T(T(T(o["raw"][0] - T(cam[2])) * z) * inv_fx)
    y = T(T(T(o["raw"][1] - T(cam[3])) * z) * inv_fy)
    return [N.gemm(view[0][:, r], [x, y, z], view[2][r]) for r in range(3)]          # Twc.R*x3Dc + Twc.t, Twc = [Rcw.t() | Ow]


# ---- :629-688, one keyframe ----
def depth_and_gate(N, view, cam, o, x3D, sigma2, mbf, two_eyes, margins=None, tag=""):
    """'behind', 'reproj' or None"""
    T = N.T
    R, t, _ = view
    with np.errstate(all="ignore"):
        z = T(N.dot64(R[2], x3D) + float(t[2]))                                      # products and sums in double, rounded once
        if margins is not None:
            margins.append(("z" + tag, float(z), 0.0))
        if z <= 0:
            return "behind"
        x = T(N.dot64(R[0], x3D) + float(t[0])); y = T(N.dot64(R[1], x3D) + float(t[1]))
        inv_z = T(1.0 / float(z))
        if not o["stereo"]:
            u, v = N.project(cam, x, y, z, two_eyes)
            ex, ey = T(T(u) - o["u"]), T(T(v) - o["v"])
            err, gate = float(T(T(ex * ex) + T(ey * ey))), 5.991 * float(sigma2)
        else:
            u = T(T(T(T(cam[0]) * x) * inv_z) + T(cam[2])); u_r = T(u - T(T(mbf) * inv_z)); v = T(T(T(T(cam[1]) * y) * inv_z) + T(cam[3]))
            ex, ey, er = T(u - o["u"]), T(v - o["v"]), T(u_r - o["ur"])
            err, gate = float(T(T(T(ex * ex) + T(ey * ey)) + T(er * er))), 7.8 * float(sigma2)
        if margins is not None:
            margins.append(("err" + tag, err, gate))
        return "reproj" if err > gate else None


# ---- :691-707 ----
def scale_consistency(N, x3D, view1, view2, scale1, scale2, ratio_factor, far_points, th_far, margins=None):
    """ZERO_DIST, FAR, SCALE or None"""
    T = N.T
    with np.errstate(all="ignore"):
        d = []
        for view in (view1, view2):
            n = [T(T(x3D[r]) - T(view[2][r])) for r in range(3)]
            d.append(T(np.sqrt(np.float64(N.dot64(n, n)))))                          # (float)cv::norm: the sum in double
        if d[0] == 0 or d[1] == 0:
            return ZERO_DIST
        if margins is not None and far_points:
            margins.append(("far", float(max(d)), float(th_far)))
        if far_points and (d[0] >= T(th_far) or d[1] >= T(th_far)):
            return FAR
        ratio_dist = T(d[1] / d[0]); ratio_octave = T(T(scale1) / T(scale2)); rf = T(ratio_factor)
        if margins is not None:
            margins.append(("scale_lo", float(ratio_octave), float(ratio_dist) * float(rf)))
            margins.append(("scale_hi", float(ratio_dist), float(ratio_octave) * float(rf)))
        if T(ratio_dist * rf) < ratio_octave or ratio_dist > T(ratio_octave * rf):
            return SCALE
    return None


def one_match(N, kf1, kf2, views1, views2, idx1, idx2, cams, tab, mb, mbf, far_points, th_far, two_eyes, margins=None):
    """(exit, x3D (zeros on a rejection), asked for the SVD, took an UnprojectStereo branch, eye1, eye2)"""
    T = N.T
    zero = [T(0.0)] * 3
    o1, o2 = observation(N, kf1, idx1, two_eyes), observation(N, kf2, idx2, two_eyes)
    if o1 is None or o2 is None:
        return BAD_INDEX, zero, False, False, 0, 0
    nl = tab["nlevels"]
    l1, l2 = min(max(o1["octave"], 0), nl - 1), min(max(o2["octave"], 0), nl - 1)   # (clamped: the reference would index past the tables)
    view1, view2 = views1[o1["eye"]], views2[o2["eye"]]                              # :503-568: re-picked per match, everything assigned
    cam1, cam2 = (cams[o1["eye"]], cams[o2["eye"]]) if two_eyes else (cams, cams)
    xn1, xn2, cos_rays = rays_and_parallax(N, view1, view2, cam1, cam2, o1, o2, two_eyes)
    cos1, cos2, cos_stereo = stereo_parallax(N, cos_rays, o1, o2, mb)
    if margins is not None:
        margins.append(("cos_stereo", float(cos_rays), float(cos_stereo)))
        margins.append(("cos_zero", float(cos_rays), 0.0))
        if not (o1["stereo"] or o2["stereo"]):
            margins.append(("cos", float(cos_rays), 0.9998))
    how = branch(cos_rays, cos1, cos2, cos_stereo, o1, o2)
    done = lambda e, x=zero: (e, x, how == "svd", how in ("stereo1", "stereo2"), o1["eye"], o2["eye"])
    if how == "svd":
        x3D, vt = triangulate(N, xn1, xn2, view1, view2)
        if margins is not None:
            margins.append(("w", float(vt[3]) / float(np.linalg.norm(np.asarray(vt, np.float64))), 0.0))
        if x3D is None:
            return done(ZERO_W)
    elif how is None:
        return done(LOW_PARALLAX)
    else:
        x3D = unproject_stereo(N, view1 if how == "stereo1" else view2, cam1, o1 if how == "stereo1" else o2)
        if x3D is None:
            return done(EMPTY_STEREO)
    for which, (view, cam, o, lv) in enumerate(((view1, cam1, o1, l1), (view2, cam2, o2, l2))):
        why = depth_and_gate(N, view, cam, o, x3D, tab["sigma2"][lv], mbf, two_eyes, margins, str(which + 1))
        if why:
            return done((BEHIND_1, BEHIND_2)[which] if why == "behind" else (REPROJ_1, REPROJ_2)[which])
    why = scale_consistency(N, x3D, view1, view2, tab["scale"][l1], tab["scale"][l2], tab["ratio_factor"], far_points, th_far, margins)
    if why is not None:
        return done(why)
    return done({"svd": TRIANGULATED, "stereo1": STEREO_1, "stereo2": STEREO_2}[how], [T(v) for v in x3D])


def tables(scale_factor=1.2, nlevels=8):
    """mvScaleFactors, mvLevelSigma2 as the handle holds them, ratioFactor = 1.5f * mfScaleFactor in binary32 (:424)"""
    from fuse_walk import tables as fuse_tables
    t = fuse_tables(scale_factor, nlevels)
    return dict(scale=t["scale"], sigma2=(t["scale"] * t["scale"]).astype(f32), nlevels=nlevels, ratio_factor=f32(f32(1.5) * f32(scale_factor)))


def create_new_map_points(N, kf1, kf2, pairs, cams, tab, mb=0.0, mbf=0.0, far_points=False, th_far=0.0, tlr=None, margins=None):
    """The loop over vMatchedIndices = pairs.  Returns dict(exit, x3d [n, 3], n_new, mark1 / mark2 (sets of (eye, local index) of the accepted
    matches' keypoints), svd, stereo (the debug counters)).  margins: a list that receives one list of (name, value, threshold) per match."""
    two_eyes = tlr is not None
    views1, views2 = N.views(kf1["pose"], tlr), N.views(kf2["pose"], tlr)
    out = dict(exit=[], x3d=[], n_new=0, mark1=set(), mark2=set(), svd=0, stereo=0)
    for idx1, idx2 in pairs:
        mg = [] if margins is not None else None
        e, x, svd, st, eye1, eye2 = one_match(N, kf1, kf2, views1, views2, int(idx1), int(idx2), cams, tab, mb, mbf, far_points, th_far, two_eyes, mg)
        if margins is not None:
            margins.append(mg)
        out["exit"].append(e); out["x3d"].append(x); out["svd"] += svd; out["stereo"] += st
        if e <= STEREO_2:
            out["n_new"] += 1
            n1 = len(kf1["eyes"][0]["kps"]) if two_eyes else 0; n2 = len(kf2["eyes"][0]["kps"]) if two_eyes else 0
            out["mark1"].add((eye1, int(idx1) - eye1 * n1)); out["mark2"].add((eye2, int(idx2) - eye2 * n2))
    out["x3d"] = np.array(out["x3d"], N.T).reshape(-1, 3)
    return out
