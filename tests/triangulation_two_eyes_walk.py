"""The checker of orbx_search_for_triangulation_two_eyes_device, orbx_kb8_unproject_device and orbx_kb8_triangulate_device: a fresh sequential
statement of ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, bCoarse) (reference src/ORBmatcher.cc:965-1206)
with the TWO-CAMERA branches (:994-1004, :1099-1129; mpCamera2 on both sides, a KannalaBrandt8 pair), in the reference's control flow: the
stacked FeatureVectors walked in step, the running bestDist, the camera and (R12, t12) switched per candidate, vbMatched2 created and tested
and never set, rotHist as lists of keyframe-1 indices.  With it KannalaBrandt8::unproject (src/CameraModels/KannalaBrandt8.cpp:103-130),
Triangulate (:424-437) and TriangulateMatches (:336-405) on numpy binary32 scalars over the host libm (tanf, sqrtf, atan2f, sinf, cosf).

cv::SVD is not one algorithm (OpenCV's Jacobi or LAPACK's sgesdd, by its build) and neither is available to this project: vt.row(3) is the
project's own definition, a one-sided Jacobi in binary32 with
    JACOBI_SWEEPS = 15, JACOBI_EPS = 2^-22, pair order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3),
the smallest squared column norm selecting the vector and of equal norms the highest index, and one correction step against the columns
whose squared norm exceeds JACOBI_POLISH_RATIO = 64 times the smallest.  The cv::Mat / cv::MatExpr roundings are the
project's restatement (parity unpinned), the same table.

A rig keyframe is dict(pose [3, 4] f32 (Rcw | tcw), eyes = (left, right)); an eye is dict(kps (the RAW keypoints: x, y, angle, octave),
desc [n, 32], fv = (nodes, idx) as ComputeBoW writes them for that eye, mp [n] bit 0: GetMapPoint != NULL)."""
import ctypes as C
import ctypes.util

import numpy as np

import last_frame_two_eyes_walk as K
from fuse_two_eyes_walk import keyframe_rig
from fuse_walk import gemm_row
from two_eyes_bow_walk import HISTO_LENGTH, POPCOUNT, three_maxima

f32 = np.float32
JACOBI_SWEEPS = 15
JACOBI_EPS = f32(2.0 ** -22)
JACOBI_POLISH_RATIO = f32(64.0)
JACOBI_PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
OK, PARALLAX, Z1, Z2, ERROR1, ERROR2 = range(6)          # why TriangulateMatches left


def libm_math():
    """sqrtf, atan2f, cosf, sinf and tanf of the host libm"""
    m = K.libm_math()
    lib = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    fn = lib.tanf
    fn.restype = C.c_float
    fn.argtypes = [C.c_float]
    m["tanf"] = lambda x: f32(fn(float(x)))
    return m


def _fmaxf(a, b):
    return b if a != a else a if b != b else (b if a < b else a)


def _fminf(a, b):
    return b if a != a else a if b != b else (b if b < a else a)


def unproject(m, k, u, v):
    """KannalaBrandt8::unproject (:103-130): (x, y) of the ray (x, y, 1).  The bounds of fminf / fmaxf are (float)(CV_PI / 2); theta_d > 1e-8
    is a compare in double; precision is the class's `const float precision` = 1e-6."""
    with np.errstate(all="ignore"):
        k = [f32(c) for c in k]
        pwx = f32(f32(f32(u) - k[2]) / k[0]); pwy = f32(f32(f32(v) - k[3]) / k[1])
        scale = f32(1.0)
        theta_d = m["sqrtf"](f32(f32(pwx * pwx) + f32(pwy * pwy)))
        pio2 = f32(np.pi / 2)
        theta_d = _fminf(_fmaxf(f32(-pio2), theta_d), pio2)
        if float(theta_d) > 1e-8:
            theta = theta_d
            for _ in range(10):
                theta2 = f32(theta * theta); theta4 = f32(theta2 * theta2); theta6 = f32(theta4 * theta2); theta8 = f32(theta4 * theta4)
                k0 = f32(k[4] * theta2); k1 = f32(k[5] * theta4); k2 = f32(k[6] * theta6); k3 = f32(k[7] * theta8)
                num = f32(f32(theta * f32(f32(f32(f32(f32(1) + k0) + k1) + k2) + k3)) - theta_d)
                den = f32(f32(f32(f32(f32(1) + f32(f32(3) * k0)) + f32(f32(5) * k1)) + f32(f32(7) * k2)) + f32(f32(9) * k3))
                fix = f32(num / den)
                theta = f32(theta - fix)
                if abs(fix) < f32(1e-6):
                    break
            scale = f32(m["tanf"](theta) / theta_d)
        return f32(pwx * scale), f32(pwy * scale)


def null_vector4(m, A):
    """vt.row(3) of cv::SVD::compute(A, ...) as the project defines it: the right singular vector of A's smallest singular value"""
    with np.errstate(all="ignore"):
        a = [[f32(A[r][c]) for r in range(4)] for c in range(4)]              # columns
        v = [[f32(1.0 if r == c else 0.0) for r in range(4)] for c in range(4)]
        for _ in range(JACOBI_SWEEPS):
            rotated = False
            for i, j in JACOBI_PAIRS:
                aa = bb = p = f32(0.0)
                for k in range(4):
                    aa = f32(aa + f32(a[i][k] * a[i][k])); bb = f32(bb + f32(a[j][k] * a[j][k])); p = f32(p + f32(a[i][k] * a[j][k]))
                if not (abs(p) > f32(JACOBI_EPS * m["sqrtf"](f32(aa * bb)))):
                    continue
                rotated = True
                p = f32(p * f32(2.0))
                beta = f32(aa - bb)
                gamma = m["sqrtf"](f32(f32(p * p) + f32(beta * beta)))
                if beta < 0:
                    delta = f32(f32(gamma - beta) * f32(0.5))
                    s = m["sqrtf"](f32(delta / gamma))
                    c = f32(p / f32(f32(gamma * s) * f32(2.0)))
                else:
                    c = m["sqrtf"](f32(f32(gamma + beta) / f32(gamma * f32(2.0))))
                    s = f32(p / f32(f32(gamma * c) * f32(2.0)))
                for k in range(4):
                    x0, x1, y0, y1 = a[i][k], a[j][k], v[i][k], v[j][k]
                    a[i][k] = f32(f32(c * x0) + f32(s * x1)); a[j][k] = f32(f32(c * x1) - f32(s * x0))
                    v[i][k] = f32(f32(c * y0) + f32(s * y1)); v[j][k] = f32(f32(c * y1) - f32(s * y0))
            if not rotated:
                break
        norms = []
        for c in range(4):
            n = f32(0.0)
            for k in range(4):
                n = f32(n + f32(a[c][k] * a[c][k]))
            norms.append(n)
        sel, best = 3, norms[3]
        for c in (2, 1, 0):
            if norms[c] < best:
                sel, best = c, norms[c]
        out = list(v[sel])
        # one correction step: A * out in binary64 from the original matrix; its component along every well-separated rotated column
        r = []
        for k in range(4):
            acc = float(A[k][0]) * float(out[0])
            for c in range(1, 4):
                acc = acc + float(A[k][c]) * float(out[c])
            r.append(acc)
        bound = f32(JACOBI_POLISH_RATIO * best)
        eps = []
        for c in range(4):
            if c != sel and norms[c] > bound:
                acc = float(a[c][0]) * r[0]
                for k in range(1, 4):
                    acc = acc + float(a[c][k]) * r[k]
                eps.append(f32(f32(acc) / norms[c]))
            else:
                eps.append(f32(0.0))
        for k in range(4):
            for c in range(4):
                out[k] = f32(out[k] - f32(eps[c] * v[c][k]))
        return out


def _dot3(a, b):
    return float(a[0]) * float(b[0]) + float(a[1]) * float(b[1]) + float(a[2]) * float(b[2])


def triangulate_matches(m, cam1, cam2, kp1, kp2, R12, t12, sigma1, sigma2, rays=None, debug=None):
    """KannalaBrandt8::TriangulateMatches (:336-405).  Returns (z1 or -1, x3D, why).  rays: ((r1x, r1y), (r2x, r2y)) if already unprojected;
    debug: a dict that receives vt = vt.row(3)."""
    with np.errstate(all="ignore"):
        R12 = np.asarray(R12, f32).reshape(3, 3); t12 = np.asarray(t12, f32).reshape(3)
        (r1x, r1y), (r2x, r2y) = rays if rays is not None else (unproject(m, cam1, *kp1), unproject(m, cam2, *kp2))
        r1 = [r1x, r1y, f32(1.0)]; r2 = [r2x, r2y, f32(1.0)]
        r21 = [gemm_row(R12[r], r2, 1.0) for r in range(3)]                                  # :341
        cos_parallax = f32(_dot3(r1, r21) / (np.sqrt(_dot3(r1, r1)) * np.sqrt(_dot3(r21, r21))))      # :343: dot and norm in double
        zero = [f32(0.0)] * 3
        if float(cos_parallax) > 0.9998:                                                     # :345
            return f32(-1.0), zero, PARALLAX
        R21 = R12.T                                                                          # :365
        t21 = [gemm_row(R21[r], t12, -1.0) for r in range(3)]                                # :366
        T1 = np.eye(3, 4, dtype=f32)
        T2 = np.array([[R21[r][0], R21[r][1], R21[r][2], t21[r]] for r in range(3)], f32)
        A = [[f32(f32(p * T[2][c]) - T[r][c]) for c in range(4)] for p, T, r in ((r1x, T1, 0), (r1y, T1, 1), (r2x, T2, 0), (r2y, T2, 1))]      # :428-431
        vt = null_vector4(m, A)
        if debug is not None:
            debug["vt"] = vt
        x3D = [f32(vt[r] / vt[3]) for r in range(3)]                                         # :436
        z1 = x3D[2]
        if z1 <= 0:                                                                          # :373
            return f32(-1.0), x3D, Z1
        z2 = f32(_dot3(R21[2], x3D) + float(t21[2]))                                         # :377
        if z2 <= 0:
            return f32(-1.0), x3D, Z2
        u, v = K.kb8_project(m, cam1, *x3D)                                                  # :383
        ex, ey = f32(u - f32(kp1[0])), f32(v - f32(kp1[1]))
        if float(f32(f32(ex * ex) + f32(ey * ey))) > 5.991 * float(f32(sigma1)):             # :388
            return f32(-1.0), x3D, ERROR1
        x2 = [gemm_row(R21[r], x3D, 1.0, t21[r]) for r in range(3)]                          # :392
        u, v = K.kb8_project(m, cam2, *x2)
        ex, ey = f32(u - f32(kp2[0])), f32(v - f32(kp2[1]))
        if float(f32(f32(ex * ex) + f32(ey * ey))) > 5.991 * float(f32(sigma2)):             # :398
            return f32(-1.0), x3D, ERROR2
        return z1, x3D, OK


def eye_relative(rig1, rig2, eye1, eye2):
    """(R12, t12) of :995-1003 for the eye combination: R1 * R2.t() and R1 * (-R2.t() * t2) + t1, each product one cv::gemm"""
    R1, t1, _ = rig1[eye1]
    R2, t2, _ = rig2[eye2]
    R12 = np.array([[gemm_row(R1[r], R2[c], 1.0) for c in range(3)] for r in range(3)], f32)
    inner = [gemm_row(R2[:, r], t2, -1.0) for r in range(3)]
    t12 = np.array([gemm_row(R1[r], inner, 1.0, t1[r]) for r in range(3)], f32)
    return R12, t12


def stacked_feature_vector(kf):
    """mFeatVec of the stacked descriptors as sorted (node, list): the left eye's list of a node followed by the right eye's (+ NLeft)"""
    n_left = len(kf["eyes"][0]["desc"])
    out = {}
    for e, eye in enumerate(kf["eyes"]):
        for node, i in zip(np.asarray(eye["fv"][0]).tolist(), np.asarray(eye["fv"][1]).tolist()):
            out.setdefault(node, []).append(i + e * n_left)
    return sorted(out.items())


def search_for_triangulation(m, kf1, kf2, tlr, cams, level_sigma2, only_stereo=False, coarse=False, th_low=50, check_orientation=True, trace=None):
    """Returns dict(n = the return value, matches12 = vMatches12 (stacked), pairs = vMatchedPairs, and the counters: mp (candidates dropped
    for a MapPoint), parallax / z1 / z2 / error1 / error2 (candidates TriangulateMatches rejected there), small_z (accepted by it with
    z <= 0.0001), equal (best replaced by an EQUAL distance), combos [4] (accepted per eye combination eye1 * 2 + eye2), tests
    (epipolarConstrain calls), within (candidates with dist <= th_low), removals (:1182-1191)).  trace: a list that receives (idx1, idx2,
    accepted, z) of every epipolarConstrain call, in order."""
    sig2 = np.asarray(level_sigma2, f32)
    cams = [[f32(c) for c in cam] for cam in cams]
    rig1, rig2 = keyframe_rig(kf1["pose"], tlr), keyframe_rig(kf2["pose"], tlr)
    rel = {(a, b): eye_relative(rig1, rig2, a, b) for a in (0, 1) for b in (0, 1)}       # Rll, Rlr, Rrl, Rrr and tll .. trr (:995-1003)
    n_left1, n_left2 = len(kf1["eyes"][0]["desc"]), len(kf2["eyes"][0]["desc"])
    N1, N2 = n_left1 + len(kf1["eyes"][1]["desc"]), n_left2 + len(kf2["eyes"][1]["desc"])
    desc1 = np.concatenate([np.asarray(e["desc"], np.uint8).reshape(-1, 32) for e in kf1["eyes"]])      # mDescriptors
    desc2 = np.concatenate([np.asarray(e["desc"], np.uint8).reshape(-1, 32) for e in kf2["eyes"]])
    mp1 = np.concatenate([np.asarray(e["mp"]) for e in kf1["eyes"]]); mp2 = np.concatenate([np.asarray(e["mp"]) for e in kf2["eyes"]])

    def key(kf, n_left, idx):                        # :1048-1050: mvKeys[idx] or mvKeysRight[idx - NLeft]
        right = idx >= n_left
        return kf["eyes"][1 if right else 0]["kps"][idx - (n_left if right else 0)], right

    rays2 = {}
    matched2 = [False] * N2                          # vbMatched2 (:1011): tested below, never set
    matches12 = [-1] * N1
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    c = dict(mp=0, parallax=0, z1=0, z2=0, error1=0, error2=0, small_z=0, equal=0, combos=[0, 0, 0, 0], tests=0, within=0, removals=0)
    names = {PARALLAX: "parallax", Z1: "z1", Z2: "z2", ERROR1: "error1", ERROR2: "error2"}
    nmatches = 0
    map2 = dict(stacked_feature_vector(kf2))
    for node, list1 in stacked_feature_vector(kf1):
        list2 = map2.get(node)
        if list2 is None:
            continue
        d12 = POPCOUNT[desc1[list1][:, None, :] ^ desc2[list2][None, :, :]].sum(2).tolist()
        for a1, idx1 in enumerate(list1):
            if int(mp1[idx1]) & 1:                   # :1033-1039
                continue
            stereo1 = False                          # :1041: !pKF1->mpCamera2 && ...
            if only_stereo and not stereo1:
                continue
            kp1, right1 = key(kf1, n_left1, idx1)
            ray1 = None
            best_dist, best_idx2, best_combo = th_low, -1, 0
            for a2, idx2 in enumerate(list2):
                if matched2[idx2] or int(mp2[idx2]) & 1:          # :1067
                    c["mp"] += 1
                    continue
                dist = d12[a1][a2]
                if dist <= th_low:
                    c["within"] += 1
                if dist > th_low or dist > best_dist:             # :1080
                    continue
                kp2, right2 = key(kf2, n_left2, idx2)
                combo = (1 if right1 else 0, 1 if right2 else 0)  # :1099-1129
                ok = coarse
                if not coarse:
                    R12, t12 = rel[combo]
                    cam1, cam2 = cams[combo[0]], cams[combo[1]]
                    if ray1 is None:
                        ray1 = unproject(m, cam1, kp1["x"], kp1["y"])
                    if idx2 not in rays2:
                        rays2[idx2] = unproject(m, cam2, kp2["x"], kp2["y"])
                    z, _, why = triangulate_matches(m, cam1, cam2, (kp1["x"], kp1["y"]), (kp2["x"], kp2["y"]), R12, t12,
                                                    sig2[int(kp1["octave"])], sig2[int(kp2["octave"])], rays=(ray1, rays2[idx2]))
                    c["tests"] += 1
                    ok = bool(z > f32(0.0001))       # epipolarConstrain (KannalaBrandt8.cpp:237-240)
                    if trace is not None:
                        trace.append((idx1, idx2, ok, z))
                    if not ok:
                        c[names.get(why, "small_z")] += 1
                if ok:                               # :1132
                    if best_idx2 >= 0 and dist == best_dist:
                        c["equal"] += 1
                    best_idx2, best_dist, best_combo = idx2, dist, combo[0] * 2 + combo[1]
            if best_idx2 >= 0:                       # :1139-1158
                matches12[idx1] = best_idx2
                nmatches += 1
                c["combos"][best_combo] += 1
                if check_orientation:
                    b = K.rotation_bin(kp1["angle"], key(kf2, n_left2, best_idx2)[0]["angle"])
                    rot_hist[b].append(idx1)
    if check_orientation:                            # :1174-1193
        keep = three_maxima([len(b) for b in rot_hist])
        for i in range(HISTO_LENGTH):
            if i in keep:
                continue
            for idx1 in rot_hist[i]:
                matches12[idx1] = -1
                nmatches -= 1
                c["removals"] += 1
    pairs = [(i, mm) for i, mm in enumerate(matches12) if mm >= 0]      # :1195-1203
    return dict(n=nmatches, matches12=matches12, pairs=pairs, **c)
