"""Scenes for the two-camera SearchForTriangulation (tests/test_search_triangulation_two_eyes.py, tests/
test_search_triangulation_two_eyes_gpu.py): 3-D points seen by fisheye-stereo rigs (a KannalaBrandt8 pair, mTlr with a 10 cm baseline), their
keypoints with at most 0.3 px of noise, descriptors far apart between points (or, families=True, in families per vocabulary node: every feature
of a node within TH_LOW of every other, so that wrong pairs reach the geometry), duplicates of equal descriptor (equal-distance replacements), decoys of equal descriptor displaced by 25 .. 60 px (and two per eye drawn until
the float64 statement rejects them by z2 and by the second reprojection error),
points near infinity (parallax), points only one eye sees (a node present in one eye only), MapPoint flags, outlier angles (removals).
With them a float64 statement of the geometric test (np.linalg.svd, math.tan, math.atan2), independent of the binary32 walk, which reports how
far each tested candidate is from every threshold.
DEVIATION from "decoys displaced at least 10 px off the epipolar curve": a decoy is displaced 25 .. 60 px from the true position in a random
direction (4 .. 150 px for the two drawn for the z2 and second-error exits) and REDRAWN until that float64 statement rejects it clear of
every threshold.  The same statement later serves the margin check of tests/test_search_triangulation_two_eyes.py, so for decoys the margin
condition holds by construction (for true observations and duplicates it holds by the 0.3 px noise); what that test still shows on them
is that the binary32 walk decides every tested candidate as the float64 statement does."""
import math

import numpy as np

import extractorb_amd as X

f32 = np.float32
CAMS = (np.array([190.97847715128717, 190.9733070521226, 254.93170605935475, 256.8974428996504, 0.0034823894022493434, 0.0007150348452162257,
                  -0.0020532361418706202, 0.00020293673591811182], f32),
        np.array([190.44236969414825, 190.4344384721956, 252.59949716835982, 254.91723064636983, 0.0034003170790442797, 0.001766278153469831,
                  -0.00266312569781606, 0.0003299517423931039], f32))
NODES = 9
def _level_sigma2(scale_factor, nlevels):
    """mvLevelSigma2 as ORBextractor builds it (reference src/ORBextractor.cc:417-425), in binary32; not taken from the library here: this
    module is imported while tests are collected, and the library is loaded only after torch has been asked for the GPU"""
    sf = [f32(1.0)]
    for _ in range(1, nlevels):
        sf.append(f32(sf[-1] * f32(scale_factor)))
    return np.array([f32(v * v) for v in sf], f32)


SIGMA2 = _level_sigma2(1.2, 8)


def rodrigues(w):
    w = np.asarray(w, np.float64); th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * Kx @ Kx


TLR = np.hstack([rodrigues([0.01, -0.02, 0.005]), np.array([[0.101], [0.002], [-0.001]])]).astype(f32)


# ---- float64 camera and geometry ----
def project64(cam, P):
    cam = [float(c) for c in cam]
    x, y, z = (float(v) for v in P)
    r = math.hypot(x, y); th = math.atan2(r, z); psi = math.atan2(y, x)
    rd = th + cam[4] * th ** 3 + cam[5] * th ** 5 + cam[6] * th ** 7 + cam[7] * th ** 9
    return cam[0] * rd * math.cos(psi) + cam[2], cam[1] * rd * math.sin(psi) + cam[3]


def unproject64(cam, u, v):
    cam = [float(c) for c in cam]
    x, y = (float(u) - cam[2]) / cam[0], (float(v) - cam[3]) / cam[1]
    td = min(max(-math.pi / 2, math.hypot(x, y)), math.pi / 2)
    if td <= 1e-8:
        return x, y
    th = td
    for _ in range(30):
        t2 = th * th
        th -= (th * (1 + cam[4] * t2 + cam[5] * t2 ** 2 + cam[6] * t2 ** 3 + cam[7] * t2 ** 4) - td) / \
              (1 + 3 * cam[4] * t2 + 5 * cam[5] * t2 ** 2 + 7 * cam[6] * t2 ** 3 + 9 * cam[7] * t2 ** 4)
    s = math.tan(th) / td
    return x * s, y * s


def eye_poses64(pose, tlr=TLR):
    """((R, t) of the left eye, (R, t) of the right eye), world -> eye"""
    pose = np.asarray(pose, np.float64); tlr = np.asarray(tlr, np.float64)
    Rl, tl = pose[:, :3], pose[:, 3]
    Rrl = tlr[:, :3].T
    trl = -Rrl @ tlr[:, 3]
    return (Rl, tl), (Rrl @ Rl, Rrl @ tl + trl)


def relative64(pose1, pose2, eye1, eye2, tlr=TLR):
    R1, t1 = eye_poses64(pose1, tlr)[eye1]
    R2, t2 = eye_poses64(pose2, tlr)[eye2]
    return R1 @ R2.T, -R1 @ R2.T @ t2 + t1


def triangulate64(cam1, cam2, kp1, kp2, R12, t12, sigma1, sigma2):
    """(accepted, margins): margins lists (name, value, threshold) of every test reached, in the reference's order"""
    r1 = np.array([*unproject64(cam1, *kp1), 1.0]); r2 = np.array([*unproject64(cam2, *kp2), 1.0])
    r21 = R12 @ r2
    cosp = float(r1 @ r21 / (np.linalg.norm(r1) * np.linalg.norm(r21)))
    m = [("cos", cosp, 0.9998)]
    if cosp > 0.9998:
        return False, m
    R21 = R12.T; t21 = -R21 @ t12
    T1 = np.eye(3, 4); T2 = np.hstack([R21, t21[:, None]])
    A = np.array([r1[0] * T1[2] - T1[0], r1[1] * T1[2] - T1[1], r2[0] * T2[2] - T2[0], r2[1] * T2[2] - T2[1]])
    vt = np.linalg.svd(A)[2]
    x = vt[3, :3] / vt[3, 3]
    m.append(("z1", float(x[2]), 0.0001))
    if not x[2] > 0.0001:
        return False, m
    z2 = float(R21[2] @ x + t21[2])
    m.append(("z2", z2, 0.0))
    if z2 <= 0:
        return False, m
    u, v = project64(cam1, x)
    e1 = (u - float(kp1[0])) ** 2 + (v - float(kp1[1])) ** 2
    m.append(("error1", e1, 5.991 * float(sigma1)))
    if e1 > 5.991 * float(sigma1):
        return False, m
    u, v = project64(cam2, R21 @ x + t21)
    e2 = (u - float(kp2[0])) ** 2 + (v - float(kp2[1])) ** 2
    m.append(("error2", e2, 5.991 * float(sigma2)))
    return e2 <= 5.991 * float(sigma2), m


def margins_hold(margins):
    """no candidate within a factor 2 of a gate, within 2e-5 of 0.9998 in cosParallaxRays, within a factor 10 of the z limits (0.0001 for z1
    through epipolarConstrain, and zero: |z| below 1e-3 counts as near)"""
    for name, value, thr in margins:
        if name == "cos" and abs(value - thr) < 2e-5:
            return False
        if name in ("z1", "z2") and abs(value) < 1e-3:
            return False
        if name in ("error1", "error2") and thr / 2 <= value <= thr * 2:
            return False
    return True


# ---- scenes ----
def _decoy(rng, p, u, v, pose, eye, ref_pose, want):
    """a position near (u, v) in eye `eye` of the rig at `pose` that, against keyframe 1's observations of the point (p["obs0"], the rig at
    ref_pose), is decided by the float64 statement clear of every threshold; want: None (any rejection), "z2" or "error2" (rejected there
    against keyframe 1's first observation).  None if the draws run out."""
    for _ in range(1500 if want else 200):
        a = rng.uniform(0, 2 * math.pi); d = rng.uniform(4, 150) if want else rng.uniform(25, 60)
        x, y, octave = u + d * math.cos(a), v + d * math.sin(a), int(rng.integers(0, 2))
        if not (5 < x < 507 and 5 < y < 507):
            continue
        fine = True
        for k, (eye0, (x0, y0, oct0)) in enumerate(sorted(p["obs0"].items())):
            R12, t12 = relative64(ref_pose, pose, eye0, eye)
            ok, mg = triangulate64(CAMS[eye0], CAMS[eye], (f32(x0), f32(y0)), (f32(x), f32(y)), R12, t12, SIGMA2[oct0], SIGMA2[octave])
            wide = [(n, val, thr) for n, val, thr in mg]
            fine = fine and not ok and margins_hold(wide) and all(not (thr / 3 <= val <= thr * 3) for n, val, thr in mg if n.startswith("error"))
            if k == 0 and want:
                fine = fine and mg[-1][0] == want
        if fine:
            return x, y, octave
    return None


def _features(rng, pts, pose, eye, cap, dup, decoys, ref_pose=None, empty=False):
    """the features of one eye: visible points (noise <= 0.3 px), duplicates, decoys, in a random order"""
    cam = CAMS[eye]
    R, t = eye_poses64(pose)[eye]
    feats = []
    if not empty:
        for p in pts:
            if p["only"] is not None and p["only"] != eye:
                continue
            Pc = R @ p["xyz"] + t
            if not np.isfinite(Pc).all() or Pc[2] < 0.2 or math.atan2(math.hypot(Pc[0], Pc[1]), Pc[2]) > 1.2:
                continue
            u, v = project64(cam, Pc)
            if not (15 < u < 497 and 15 < v < 497):
                continue
            feats.append(dict(p=p, u=u, v=v, decoy=False))
        rng.shuffle(feats)
        feats = feats[:cap - dup - decoys]
        base = list(feats)
        for k in range(min(dup, len(base))):
            feats.append(dict(base[k], dupe=True))
        seen = [f for f in reversed(base) if f["p"].get("obs0")]
        for k in range(min(decoys, len(seen))):
            b = seen[k]
            got = _decoy(rng, b["p"], b["u"], b["v"], pose, eye, ref_pose, ("z2", "error2")[k] if k < 2 else None)
            if got is not None:
                feats.append(dict(p=b["p"], u=got[0], v=got[1], octave=got[2], decoy=True))
        rng.shuffle(feats)
    n = len(feats)
    kps = np.zeros(n, X.KEYPOINT_DTYPE); desc = np.zeros((n, 32), np.uint8); mp = np.zeros(n, np.uint8); nodes = np.zeros(n, np.uint32)
    for i, f in enumerate(feats):
        a = rng.uniform(0, 2 * math.pi); r = 0.0 if f["decoy"] else rng.uniform(0, 0.3)
        kps["x"][i] = f["u"] + r * math.cos(a); kps["y"][i] = f["v"] + r * math.sin(a)
        kps["octave"][i] = f["octave"] if f["decoy"] else rng.integers(0, 4)
        ang = f["p"]["angle"] + rng.uniform(-2, 2) + (rng.uniform(60, 300) if rng.random() < 0.12 else 0)
        kps["angle"][i] = ang % 360.0
        kps["size"][i] = 31.0
        d = f["p"]["desc"].copy()
        if not f.get("dupe") and not f["decoy"]:
            for b in rng.integers(0, 256, rng.integers(0, 4)):
                d[b >> 3] ^= 1 << (b & 7)
        desc[i] = d
        mp[i] = 0 if f["decoy"] else rng.random() < 0.15
        nodes[i] = f["p"]["node"]
        if ref_pose is None:                                                                  # keyframe 1: what the decoys are judged against
            f["p"].setdefault("obs0", {})[eye] = (float(kps["x"][i]), float(kps["y"][i]), int(kps["octave"][i]))
    order = np.lexsort((np.arange(n), nodes))                                                 # ComputeBoW: by node, inside a node by feature index
    return dict(kps=kps, desc=desc, mp=mp, fv=(nodes[order].astype(np.uint32), order.astype(np.uint32)), feats=feats)


def make(seed, cap=32, n_points=30, rigs=4, nan_rig=3, skew=0.7, families=False, dup=3, decoys=6, nodes=NODES):
    """families: every point's descriptor is a few bits from its NODE's base, so all features of a node are within TH_LOW of each other and
    wrong pairs reach the geometric test (hundreds per search, some of them near a threshold by chance: equality tests only).  Without,
    descriptors of different points are far apart and the candidates within TH_LOW are a point's own observations, duplicates and decoys."""
    rng = np.random.default_rng(seed)
    bases = rng.integers(0, 256, (nodes, 32), dtype=np.uint8)
    pts = []
    for i in range(n_points):
        only = 1 if i in (0, 1) else 0 if i in (2, 3) else None
        node = nodes - 1 if only == 1 else nodes - 2 if only == 0 else (4 if rng.random() < skew else int(rng.integers(0, nodes - 2)))
        d = bases[node].copy() if families else rng.integers(0, 256, 32, dtype=np.uint8)
        for b in rng.integers(0, 256, 8):
            d[b >> 3] ^= 1 << (b & 7)
        far = i in (4, 5, 6)
        z = 300.0 if far else rng.uniform(1.5, 3.5)      # (cosParallaxRays of the 10 cm baseline stays clear of 0.9998)
        pts.append(dict(xyz=np.array([rng.uniform(-0.6, 0.6) * z, rng.uniform(-0.6, 0.6) * z, z]), node=node, desc=d, only=only,
                        angle=float(rng.uniform(0, 360))))
    poses, kfs = [], []
    for r in range(rigs):
        R = rodrigues(rng.uniform(-0.05, 0.05, 3)) if r else np.eye(3)
        t = rodrigues(rng.uniform(-1, 1, 3)) @ np.array([rng.uniform(0.3, 0.5), 0, 0]) * np.array([1, 1, 0.4]) + np.array([0, 0, -0.5 * (r == 2)]) if r else np.zeros(3)
        pose = np.hstack([R, t[:, None]]).astype(f32)
        good = pose.copy()
        if r == nan_rig:
            pose[1, 3] = np.nan
        poses.append(pose)
        kfs.append(dict(pose=pose, eyes=tuple(_features(rng, pts, good, e, cap, dup if r else 0, decoys if r else 0, ref_pose=poses[0] if r else None)
                                              for e in (0, 1))))
    return dict(cap=cap, tlr=TLR, cams=CAMS, sigma2=SIGMA2, kfs=kfs, seed=seed)


def variant(scene, name):
    """edge scenes (c) on top of a scene: an empty right eye in keyframe 1's neighbours, NLeft = 0 in keyframe 1, and zero_w: a ZERO FOURTH
    COMPONENT of the triangulated vector.  For the last, keyframe 2 = rig 1 gets the degenerate pose [diag(1, 1, 0) | (-0.5, 0, 0.3)], so
    that the left-left combination has R12 = diag(1, 1, 0), t12 = (0.5, 0, 0), and one point's left keypoints in both keyframes sit on the
    left camera's principal point with equal descriptors and no MapPoint: both rays are (0, 0, 1), R12*r2 is the zero vector,
    cosParallaxRays is 0 / 0 = NaN and passes `> 0.9998`, column 2 of A is zero, vt.row(3) = (0, 0, 1, 0), x3D = (NaN, NaN, inf), every
    later test is false on it and TriangulateMatches returns inf, which epipolarConstrain accepts.  s["zero_w"] = (idx1, idx2), stacked."""
    import copy
    s = copy.deepcopy(scene)
    empty = dict(kps=np.zeros(0, X.KEYPOINT_DTYPE), desc=np.zeros((0, 32), np.uint8), mp=np.zeros(0, np.uint8),
                 fv=(np.zeros(0, np.uint32), np.zeros(0, np.uint32)), feats=[])
    if name == "empty_right_eye":
        for kf in s["kfs"][1:]:
            kf["eyes"] = (kf["eyes"][0], empty)
    elif name == "nleft_zero":
        s["kfs"][0]["eyes"] = (empty, s["kfs"][0]["eyes"][1])
    elif name == "zero_w":
        s["kfs"][1]["pose"] = np.array([[1, 0, 0, -0.5], [0, 1, 0, 0], [0, 0, 0, 0.3]], f32)
        e1, e2 = s["kfs"][0]["eyes"][0], s["kfs"][1]["eyes"][0]
        by_point = {id(f["p"]): j for j, f in enumerate(e2["feats"]) if not f["decoy"]}
        a, b = next((i, by_point[id(f["p"])]) for i, f in enumerate(e1["feats"]) if id(f["p"]) in by_point)
        for eye, i in ((e1, a), (e2, b)):
            eye["kps"]["x"][i], eye["kps"]["y"][i] = CAMS[0][2], CAMS[0][3]
            eye["mp"][i] = 0
        e2["desc"][b] = e1["desc"][a]
        s["zero_w"] = (a, b)
    else:
        raise KeyError(name)
    return s


def pack(scene, pairs, cap=None):
    """the batch of the C entry: device frames 2X, 2X + 1 = the eyes of rig X; flags per pair (kf1, kf2)"""
    cap = cap or scene["cap"]
    R = len(scene["kfs"]); B = 2 * R
    kps = np.zeros((B, cap), X.KEYPOINT_DTYPE); desc = np.zeros((B, cap, 32), np.uint8)
    fn = np.zeros((B, cap), np.uint32); fi = np.zeros((B, cap), np.uint32)
    nout = np.zeros(B, np.int32); nfeat = np.zeros(B, np.int32)
    poses = np.stack([kf["pose"].reshape(12) for kf in scene["kfs"]]).astype(f32)
    for x, kf in enumerate(scene["kfs"]):
        for e, eye in enumerate(kf["eyes"]):
            n = len(eye["kps"]); f = 2 * x + e
            kps[f, :n] = eye["kps"]; desc[f, :n] = eye["desc"]; fn[f, :n] = eye["fv"][0]; fi[f, :n] = eye["fv"][1]
            nout[f] = nfeat[f] = n
    fl1 = np.zeros((len(pairs), 2, cap), np.uint8); fl2 = np.zeros((len(pairs), 2, cap), np.uint8)
    for p, (a, b) in enumerate(pairs):
        for e in (0, 1):
            m1, m2 = scene["kfs"][a]["eyes"][e]["mp"], scene["kfs"][b]["eyes"][e]["mp"]
            fl1[p, e, :len(m1)] = m1; fl2[p, e, :len(m2)] = m2
    return dict(kps=kps, desc=desc, fn=fn, fi=fi, nout=nout, nfeat=nfeat, poses=poses, fl1=fl1, fl2=fl2)
