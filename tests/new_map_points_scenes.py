"""Crafted scenes for the triangulation loop of CreateNewMapPoints (tests/test_new_map_points.py, tests/test_new_map_points_gpu.py), for both
rig kinds: known world points projected in float64 into a current keyframe (kf 0, the identity pose) and three neighbours, then disturbed so
that every `continue` of the loop and all three accepting branches are reached.  Capacity 32 (per eye).  One call of four pairs with
kf1_step = 0: (0, 0) - the keyframe against itself -, (0, 1), (0, 2), (0, 3).
  kf 1  a normal neighbour: 0.5 m sideways, 0.2 m FORWARD (a point 0.1 m in front of kf 0 lies behind it), a small rotation;
  kf 2  a neighbour 3 cm away: the rays' parallax is below the 10 cm stereo baseline's, so stereo features take UnprojectStereo and
        monocular ones leave by low parallax;
  kf 3  the degenerate pose [[0,0,0],[0,1,0],[0.1,0,1] | (-7,0,0.3)] for a ZERO FOURTH COMPONENT: with both keypoints on the principal point
        the rays are (0,0,1) and (0.1,0,1) (cosParallaxRays 0.995), and A = [(-1,0,0,0), (0,-1,0,0), (0,0,0,7), (0,-1,0,0)]: its third column is
        zero and orthogonal to all, so it is never rotated, its zero norm selects it, and vt.row(3) = (0,0,1,0) exactly.  (The zero_w case
        of tests/triangulation_two_eyes_scenes.py, imported below for the two-eye form's left camera, makes cosParallaxRays NaN, which
        this loop - unlike TriangulateMatches - rejects by parallax first: its pose is kept as kf 3 of the `nan_parallax` variant.)
Kinds of matches (the walk's exit each is built for is asserted by the tests, not assumed):
  tri            monocular observations, 0.3 px noise, equal octaves                     -> TRIANGULATED   (two eyes: all four eye combinations)
  tri_s1 / tri_s2 / tri_both   the same with stereo observations (large parallax: the SVD branch, the stereo gates)
  st1 / st2 / st_both          kf 2: stereo-1-only, stereo-2-only, both stereo (the `else if`: only cosParallaxStereo1 is replaced) -> STEREO_1 / _2 / _1
  empty          kf 2: mvuRight >= 0 with mvDepth = -1 and = 0                           -> EMPTY_STEREO
  low            kf 2, monocular                                                         -> LOW_PARALLAX
  behind1 / behind2   a point behind both keyframes / 0.1 m in front of kf 0 and behind kf 1
  reproj1        kp1 9 px off, octave 0;   reproj2: kp2 10 px off with kp1 at octave 7 (gate 8.8 px) and kp2 at octave 0 (2.4 px): REPROJ_2 alone
  far            a point 10 m away against mThFarPoints = 8;   scale: octaves 5 and 0
  oct            octaves (-3, -2) and (11, 9), clamped to (0, 0) and (7, 7);   bad: indices -1, N and 10^6
  zero_w         kf 3, above.
ZERO_DIST needs x3D == Ow EXACTLY with z > 0 and is its own scene (zero_dist_scene): one-camera only.
A float64 statement cannot mirror exits that hang on exact float identities (zero_w, zero_dist) or NaN: margin_ok leaves those kinds out."""
import math

import numpy as np

import extractorb_amd as X
import new_map_points_walk as NW
import triangulation_two_eyes_scenes as S2

f32 = np.float32
CAP = 32
CAM = X.camera(500.0, 500.0, 320.0, 240.0)
MB, MBF = 0.1, 50.0
TH_FAR = 8.0
RAW_SHIFT = (0.37, -0.21)                     # mvKeys - mvKeysUn of every feature: shows that UnprojectStereo reads mvKeys
TAB = NW.tables(1.2, 8)
POISON_PAIR = -1
# seeds on which margin_ok holds for both forms (drawn 1, 2, 3, ...; the ones that failed are not listed)
MARGIN_SEEDS = (1, 2, 3)
NO_MARGIN_KINDS = ("zero_w", "bad", "self", "nan")


def _poses():
    kf1 = np.hstack([S2.rodrigues([0.02, -0.03, 0.01]), np.zeros((3, 1))])
    kf1[:, 3] = -kf1[:, :3] @ np.array([0.5, 0.05, 0.2])                              # the centre is (0.5, 0.05, 0.2)
    kf2 = np.hstack([S2.rodrigues([0.001, 0.002, -0.001]), np.zeros((3, 1))])
    kf2[:, 3] = -kf2[:, :3] @ np.array([0.03, 0.0, 0.0])
    kf3 = np.array([[0, 0, 0, -7.0], [0, 1, 0, 0], [0.1, 0, 1, 0.3]])
    return [np.eye(3, 4), kf1, kf2, kf3]


class _Builder:
    def __init__(self, two_eyes, seed):
        self.two, self.rng = two_eyes, np.random.default_rng(seed)
        self.poses = _poses()
        self.feats = [[[], []] for _ in self.poses]          # [kf][eye] -> list of dict
        self.matches = {0: [], 1: [], 2: [], 3: []}         # pair (0, k) -> [(kind, (eye1, i1) or raw int, (eye2, i2) or raw int)]

    def eye_pose(self, k, eye):
        return S2.eye_poses64(self.poses[k])[eye] if self.two else (self.poses[k][:, :3], self.poses[k][:, 3])

    def pixel(self, k, eye, P):
        """the pixel of the LINE through the eye's centre and P (also for a point behind the eye), and P's depth in the eye"""
        R, t = self.eye_pose(k, eye)
        x, y, z = R @ np.asarray(P, np.float64) + t
        if self.two:
            return (*S2.project64(S2.CAMS[eye], (x / z, y / z, 1.0)), z)
        return float(CAM[0]) * x / z + float(CAM[2]), float(CAM[1]) * y / z + float(CAM[3]), z

    def add(self, k, eye, P, octave, shift=(0.0, 0.0), stereo=False, depth=None, noise=0.3, at=None):
        u, v, z = self.pixel(k, eye, P) if at is None else (*at, 1.0)
        a, r = self.rng.uniform(0, 2 * math.pi), self.rng.uniform(0, noise)
        u, v = u + r * math.cos(a) + shift[0], v + r * math.sin(a) + shift[1]
        ur = u - MBF / z + self.rng.uniform(-0.3, 0.3) if stereo else -1.0
        self.feats[k][eye].append(dict(u=u, v=v, octave=octave, ur=ur, depth=(z if depth is None else depth) if stereo else -1.0))
        assert len(self.feats[k][eye]) <= CAP
        return (eye, len(self.feats[k][eye]) - 1)

    def point(self, lo=3.0, hi=6.0):
        z = self.rng.uniform(lo, hi)
        return np.array([self.rng.uniform(-0.35, 0.35) * z, self.rng.uniform(-0.25, 0.25) * z, z])

    def match(self, k, kind, P, eyes=(0, 0), octaves=(0, 0), s1=False, s2=False, shift1=(0, 0), shift2=(0, 0), depth1=None, depth2=None):
        a = self.add(0, eyes[0], P, octaves[0], shift1, s1, depth1)
        b = self.add(k, eyes[1], P, octaves[1], shift2, s2, depth2)
        self.matches[k].append((kind, a, b))

    def build(self):
        rng, two = self.rng, self.two
        combos = [(0, 0), (0, 1), (1, 0), (1, 1)] if two else [(0, 0)]
        for n in range(8 if two else 6):                                             # kf 1: the SVD branch
            o = int(rng.integers(0, 4))
            self.match(1, "tri", self.point(), combos[n % len(combos)], (o, o))
        if not two:
            self.match(1, "tri_s1", self.point(), s1=True); self.match(1, "tri_s2", self.point(), s2=True)
            self.match(1, "tri_both", self.point(), s1=True, s2=True); self.match(1, "tri_both", self.point(), octaves=(2, 2), s1=True, s2=True)
        e = combos[-1]
        self.match(1, "behind1", [0.1, 0.1, -2.0], e)
        self.match(1, "behind2", [0.02, 0.01, 0.1])
        self.match(1, "reproj1", self.point(), e, shift1=(0.0, 9.0))
        self.match(1, "reproj2", self.point(), octaves=(7, 0), shift2=(0.0, 10.0))
        self.match(1, "far", [1.0, -0.5, 10.0], e)
        self.match(1, "scale", self.point(), octaves=(5, 0))
        self.match(1, "oct", self.point(), e, octaves=(-3, -2)); self.match(1, "oct", self.point(), octaves=(11, 9))
        n1 = sum(len(f) for f in self.feats[1])
        self.matches[1] += [("bad", -1, 0), ("bad", 0, n1), ("bad", 10 ** 6, 3)]
        for n in range(3):                                                           # kf 2: below the stereo parallax
            self.match(2, "low", self.point(), (n % 2, n % 2) if two else (0, 0))    # (the same eye on both sides: across the eyes the 10 cm count)
        if not two:
            self.match(2, "st1", self.point(2.0, 4.0), s1=True); self.match(2, "st2", self.point(2.0, 4.0), s2=True)
            self.match(2, "st_both", self.point(2.0, 4.0), s1=True, s2=True)
            self.match(2, "st1", self.point(2.0, 4.0), octaves=(1, 1), s1=True)
            self.match(2, "empty", self.point(), s1=True, depth1=-1.0); self.match(2, "empty", self.point(), s2=True, depth2=0.0)
        pp = (float(S2.CAMS[0][2]), float(S2.CAMS[0][3])) if two else (float(CAM[2]), float(CAM[3]))      # kf 3: the principal points
        a = self.add(0, 0, None, 0, noise=0.0, at=pp); b = self.add(3, 0, None, 0, noise=0.0, at=pp)
        self.matches[3].append(("zero_w", a, b))
        self.match(3, "self", self.point())                                          # (whatever the degenerate pose makes of a real point)
        feats0 = [(e, i) for e in (0, 1) for i in range(len(self.feats[0][e]))]      # kf 0 against itself: a feature with itself, with another
        for j in range(0, len(feats0), 3):
            self.matches[0].append(("self", feats0[j], feats0[j]))
        self.matches[0].append(("self", feats0[0], feats0[1]))
        return self.finish()

    def finish(self):
        kfs = []
        for k, pose in enumerate(self.poses):
            eyes = []
            for feats in self.feats[k]:
                kp = np.zeros(len(feats), X.KEYPOINT_DTYPE)
                kp["x"] = [f["u"] for f in feats]; kp["y"] = [f["v"] for f in feats]; kp["octave"] = [f["octave"] for f in feats]
                kp["size"] = 31.0
                eyes.append(dict(kps=kp, u_right=np.array([f["ur"] for f in feats], f32), depth=np.array([f["depth"] for f in feats], f32)))
            if self.two:
                kfs.append(dict(pose=pose.astype(f32), eyes=tuple(dict(kps=e["kps"]) for e in eyes)))
            else:
                raw = eyes[0]["kps"].copy(); raw["x"] += f32(RAW_SHIFT[0]); raw["y"] += f32(RAW_SHIFT[1])
                kfs.append(dict(pose=pose.astype(f32), kps_un=eyes[0]["kps"], kps=raw, u_right=eyes[0]["u_right"], depth=eyes[0]["depth"]))
        stacked = lambda k, m: m if isinstance(m, int) else m[1] + m[0] * len(self.feats[k][0])
        pairs = [[(stacked(0, a), stacked(k, b)) for _, a, b in self.matches[k]] for k in range(4)]
        kinds = [[kind for kind, _, _ in self.matches[k]] for k in range(4)]
        return dict(two_eyes=self.two, cap=CAP, kfs=kfs, pairs=pairs, kinds=kinds, kf1=(0, 0), kf2=(0, 1), tlr=S2.TLR if self.two else None,
                    cams=S2.CAMS if self.two else CAM, mb=MB, mbf=MBF, far_points=True, th_far=TH_FAR)


def make(two_eyes, seed):
    return _Builder(two_eyes, seed).build()


def variant(scene, name):
    """edge scenes on top of a crafted one: nan_pose (kf 1's rotation holds a NaN: its rays are NaN, every test is false and every match of the
    pair leaves by LOW_PARALLAX, stereo or not), nan_parallax (kf 3 gets the zero_w pose of
    tests/triangulation_two_eyes_scenes.py: cosParallaxRays is 0 / 0), mono (one camera: d_u_right / d_kps / d_depth NULL), nleft_zero (two eyes:
    kf 1 has no left keypoint, its matches name right keypoints only)"""
    import copy
    s = copy.deepcopy(scene)
    if name == "nan_pose":
        s["kfs"][1]["pose"][1, 1] = np.nan
    elif name == "nan_parallax":
        s["kfs"][3]["pose"] = S2.variant(S2.make(1), "zero_w")["kfs"][1]["pose"].copy()
    elif name == "mono":
        for kf in s["kfs"]:
            kf["u_right"] = kf["depth"] = None
    elif name == "nleft_zero":
        kf = s["kfs"][1]
        n_left = len(kf["eyes"][0]["kps"])
        kept = [(a, b - n_left) for (a, b), kind in zip(s["pairs"][1], s["kinds"][1]) if b >= n_left and kind != "bad"]
        s["kinds"][1] = [kind for (a, b), kind in zip(s["pairs"][1], s["kinds"][1]) if b >= n_left and kind != "bad"]
        s["pairs"][1] = kept
        kf["eyes"] = (dict(kps=np.zeros(0, X.KEYPOINT_DTYPE)), kf["eyes"][1])
    else:
        raise KeyError(name)
    return s


def zero_dist_scene(max_tries=50000):
    """ZERO_DIST (:697) needs dist == 0, which is x3D == Ow bit for bit, behind a z > 0: only rounding residue can do that.  Two one-camera
    keyframes share their CENTRE (different rotations); the keyframe-2 feature is stereo with mvDepth = 1e-30, so that pKF2->UnprojectStereo
    gives Ow2 + (something that vanishes in the sum) = Ow exactly, while z1 and z2 are the residue of Rcw.row(2).dot(Ow) + tcw[2], about 1e-8
    of either sign.  Rotations are drawn until both residues are positive; the keypoints are then PLACED on the projections of the residue
    (mbf = 0 in this call, so that the stereo gate's third error is the first again) - found by the binary32 walk itself, which is
    legitimate for a scene: the test then holds the library to the same walk."""
    N = NW.Binary32()
    rng = np.random.default_rng(7)
    for _ in range(max_tries):
        C = rng.uniform(-2, 2, 3)
        poses = []
        for _k in range(2):
            R = S2.rodrigues(rng.uniform(-0.6, 0.6, 3))
            poses.append(np.hstack([R, (-R @ C)[:, None]]).astype(f32))
        Ow = [NW.camera_centre(p) for p in poses]
        if not (Ow[0] == Ow[1]).all():                                               # the centres must agree bit for bit
            continue
        res = []
        for p, o in zip(poses, Ow):
            x, y, z = (f32(N.dot64(p[r, :3], o) + float(p[r, 3])) for r in range(3))
            res.append((x, y, z))
        if not all(z > 0 for _, _, z in res):
            continue
        uv = [N.project(CAM, x, y, z, False) for x, y, z in res]
        inv_z2 = f32(1.0 / float(res[1][2]))
        u2 = f32(f32(f32(CAM[0] * res[1][0]) * inv_z2) + CAM[2]); v2 = f32(f32(f32(CAM[1] * res[1][1]) * inv_z2) + CAM[3])
        if not (all(np.isfinite(c) and abs(c) < 1e6 for p in uv for c in p) and np.isfinite(u2) and 0 <= u2 < 1e6 and abs(v2) < 1e6):
            continue
        kfs = []
        for k, (p, (u, v)) in enumerate(zip(poses, ((uv[0]), (u2, v2)))):
            kp = np.zeros(1, X.KEYPOINT_DTYPE); kp["x"], kp["y"] = u, v
            kfs.append(dict(pose=p, kps_un=kp, kps=kp.copy(), u_right=np.array([u2 if k else -1.0], f32), depth=np.array([1e-30 if k else -1.0], f32)))
        return dict(two_eyes=False, cap=CAP, kfs=kfs, pairs=[[(0, 0)]], kinds=[["zero_dist"]], kf1=(0, 0), kf2=(1, 0), tlr=None, cams=CAM, mb=MB,
                    mbf=0.0, far_points=False, th_far=0.0)
    raise AssertionError("no draw gave two positive residues")


def pair_frames(scene, n_pairs=None):
    n_pairs = len(scene["pairs"]) if n_pairs is None else n_pairs
    return [(scene["kf1"][0] + p * scene["kf1"][1], scene["kf2"][0] + p * scene["kf2"][1]) for p in range(n_pairs)]


def walk(scene, N=None, margins=None, far_points=None):
    """the walk of every pair of the call: a list of new_map_points_walk.create_new_map_points results"""
    N = N or NW.Binary32()
    out = []
    for p, (a, b) in enumerate(pair_frames(scene)):
        mg = [] if margins is not None else None
        out.append(NW.create_new_map_points(N, scene["kfs"][a], scene["kfs"][b], scene["pairs"][p], scene["cams"], TAB, scene["mb"], scene["mbf"],
                                            scene["far_points"] if far_points is None else far_points, scene["th_far"], scene["tlr"], mg))
        if margins is not None:
            margins.append(mg)
    return out


def pack(scene, cap=None, n_matches=None):
    """the arrays of the C entries: batch frame k (one camera) or 2k, 2k + 1 (two eyes) of keyframe k; the pair lists, poison behind their ends"""
    cap = cap or scene["cap"]
    two = scene["two_eyes"]
    K = len(scene["kfs"]); B = 2 * K if two else K; L = 2 * cap if two else cap; P = len(scene["pairs"])
    kps_un = np.zeros((B, cap), X.KEYPOINT_DTYPE); kps = np.zeros((B, cap), X.KEYPOINT_DTYPE)
    u_right = np.full((B, cap), -1.0, f32); depth = np.full((B, cap), -1.0, f32); n_out = np.zeros(B, np.int32)
    mono = False
    for k, kf in enumerate(scene["kfs"]):
        if two:
            for e, eye in enumerate(kf["eyes"]):
                n = len(eye["kps"]); kps_un[2 * k + e, :n] = eye["kps"]; n_out[2 * k + e] = n
        else:
            n = len(kf["kps_un"]); kps_un[k, :n] = kf["kps_un"]; kps[k, :n] = kf["kps"]; n_out[k] = n
            if kf["u_right"] is None:
                mono = True
            else:
                u_right[k, :n] = kf["u_right"]; depth[k, :n] = kf["depth"]
    pairs = np.full((P, L, 2), POISON_PAIR, np.int32); n = np.zeros(P, np.int32)
    for p, lst in enumerate(scene["pairs"]):
        n[p] = len(lst)
        if lst:
            pairs[p, :len(lst)] = np.array(lst, np.int64).clip(-2 ** 31, 2 ** 31 - 1)
    if n_matches is not None:
        n[:] = n_matches
    poses = np.stack([kf["pose"].reshape(12) for kf in scene["kfs"]]).astype(f32)
    return dict(kps_un=kps_un, kps=None if mono or two else kps, u_right=None if mono or two else u_right, depth=None if mono or two else depth,
                n_out=n_out, pairs=pairs, n_matches=n, poses=poses, L=L, cap=cap, P=P)


def margin_ok(margins):
    """no compared quantity of a match near its threshold in float64: cosParallaxRays 2e-5 from 0.9998, 1e-5 from cosParallaxStereo and 1e-3
    from 0, |z| and the normalised fourth component above 1e-3, a squared error not within a factor 2 of its gate, the distances 1 % from
    mThFarPoints and the two scale ratios 1 % from their bounds"""
    for name, value, thr in margins:
        if not np.isfinite(value):
            return False
        if name == "cos" and abs(value - thr) < 2e-5:
            return False
        if name == "cos_stereo" and abs(value - thr) < 1e-5:
            return False
        if name in ("cos_zero", "z1", "z2", "w") and abs(value) < 1e-3:
            return False
        if name in ("err1", "err2") and thr / 2 <= value <= thr * 2:
            return False
        if name in ("far", "scale_lo", "scale_hi") and abs(value - thr) < 0.01 * abs(thr):
            return False
    return True
