"""Scenes for orbx_frustum_requests_two_eyes_device, shared by the CPU tests (tests/test_frustum_requests_two_eyes.py) and the GPU tests
(tests/test_frustum_requests_two_eyes_gpu.py): two fisheye rigs, seeded uniform scenes for the float64 cross-check, and the CRAFTED points -
one pair of MapPoints per comparison of the statement and eye, the points of adjacent floats of one number on the two sides of the comparison
(found by bisection with the walk itself under the host libm, as tests/last_frame_two_eyes_scenes.py does) or the threshold itself and the float
beside it where the threshold is the MapPoint's own, each with what it was built to reach."""
import functools

import numpy as np

import frustum_two_eyes_walk as W
import last_frame_two_eyes_scenes as L2

f32, f64 = np.float32, np.float64
BOUNDS = np.array([0, 512, 0, 512], f32)
CAM_LEFT = L2.CAM
CAM_RIGHT = np.array([190.44236969414825, 190.4344384721956, 252.59949716835982, 254.91723064636983,
                      0.0034003170790442797, 0.001766278153469831, -0.00266312569781606, 0.0003299517423931039], f32)
CAMS = (CAM_LEFT, CAM_RIGHT)
SETTING = (1.2, 8)
TH_FAR = 3.0
POSE = L2.CUR
POSES = [L2.CUR, L2.pose(-0.01, 0.04, 0.02, (-0.2, 0.05, 0.3)), L2.pose(0.03, 0.3, -0.02, (0.6, 0.0, -0.2))]


def _inverse(T):
    T = np.asarray(T, f64)
    R = T[:, :3].T
    return np.concatenate([R, (-R @ T[:, 3]).reshape(3, 1)], 1).astype(f32)


def _rig(name, trl):
    return dict(name=name, trl=np.asarray(trl, f32), tlr=_inverse(trl))


# narrow: a 10 cm baseline and a hundredth of a radian between the eyes; wide: 30 cm and the right eye yawed 0.7 rad, so that many points are
# in one eye only.  mTlr is the inverse of mTrl rounded to float, as a calibration file would hold it: the entry takes both as they are.
RIGS = dict(narrow=_rig("narrow", L2.TRL), wide=_rig("wide", L2.pose(0.0, 0.7, 0.0, (-0.3, 0.004, 0.02))))


def eye_pose64(rig, e, pose=POSE):
    """float64 [R | t] of eye e under `pose` (for building points, not for checking them)"""
    T = np.asarray(pose, f64)
    if e == 0:
        return T
    A = rig["trl"].astype(f64)
    return np.concatenate([A[:, :3] @ T[:, :3], (A[:, :3] @ T[:, 3] + A[:, 3]).reshape(3, 1)], 1)


def world_of(rig, e, xc, pose=POSE):
    """a world point with (about) the coordinates xc in eye e's camera frame"""
    T = eye_pose64(rig, e, pose)
    return (T[:, :3].T @ (np.asarray(xc, f64) - T[:, 3])).astype(f32)


def uniform_scene(seed, n, box=((-6, 6), (-4, 4), (-1, 12)), noise=0.6, pose=POSE):
    """P uniform in `box`, mfMaxDistance in [2, 20], normals along the left eye's viewing ray plus noise, earlier depths in [0, 6]"""
    rng = np.random.default_rng(seed)
    world = np.stack([rng.uniform(lo, hi, n) for lo, hi in box], 1).astype(f32)
    T = np.asarray(pose, f64)
    PO = world.astype(f64) - (-T[:, :3].T @ T[:, 3])
    nrm = PO / np.linalg.norm(PO, axis=1, keepdims=True) + noise * rng.standard_normal((n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    mf_max = rng.uniform(2, 20, n).astype(f32)
    mf_min = (mf_max / f32(1.2 ** 7)).astype(f32)
    dist = np.stack([f32(0.8) * mf_min, f32(1.2) * mf_max, mf_max], 1).astype(f32)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    flags = ((rng.random(n) < 0.93).astype(np.uint8) | ((rng.random(n) < 0.8).astype(np.uint8) << 1)).astype(np.uint8)
    prev = rng.uniform(0, 6, n).astype(f32)
    return dict(world=world, normal=nrm.astype(f32), dist=dist, desc=desc), flags, prev


def _pred(x):
    return np.nextafter(f32(x), f32(-np.inf))


def _succ(x):
    return np.nextafter(f32(x), f32(np.inf))


WIDE_DIST = (0.01, 100.0, 2.0)


def check_eye(m, rig, e, world, normal, dist=WIDE_DIST, detail=None):
    eyes = W.rig(POSE, rig["trl"], rig["tlr"])
    with np.errstate(all="ignore"):
        return W.eye_check(m, eyes[e], CAMS[e], np.asarray(world, f32), np.asarray(normal, f32), np.asarray(dist, f32), BOUNDS, W.tables(*SETTING), 0.5,
                           detail)


def _along(rig, e, inside, outside):
    """c in [0, 1] -> the world point at inside + c * (outside - inside) of eye e's camera frame.  The crafted pairs are the points of two
    ADJACENT FLOATS of c on the two sides of a comparison."""
    a, b = np.asarray(inside, f64), np.asarray(outside, f64)
    return lambda c: world_of(rig, e, a + f64(c) * (b - a))


def _toward(rig, e, world):
    """the unit normal that looks at eye e's centre from `world`: viewCos about 1"""
    T = eye_pose64(rig, e)
    PO = np.asarray(world, f64) - (-T[:, :3].T @ T[:, 3])
    return (PO / np.linalg.norm(PO)).astype(f32)


@functools.lru_cache(None)
def crafted(rig_name):
    """list of dict(name, world, normal, dist, flag, prev, eye, want, check): `want` is the exit of eye `eye` under POSE with far_points and
    TH_FAR, th = 1 and d_mp_prev_depth given; check: fields of that eye's record / request that must hold.  eye = None: want = (exit L, exit R)."""
    m = W.libm_math()
    rig = RIGS[rig_name]
    E = W
    pts = []

    def add(name, world, eye, want, normal=None, dist=WIDE_DIST, flag=3, prev=0.0, **check):
        world = np.array(world, f32)
        if normal is None:
            normal = _toward(rig, eye or 0, world)
        pts.append(dict(name=name, world=world, normal=np.array(normal, f32), dist=np.array(dist, f32), flag=flag, prev=f32(prev), eye=eye, want=want,
                        check=check))

    def exit_at(e, world, normal=None, dist=WIDE_DIST):
        return check_eye(m, rig, e, world, _toward(rig, e, world) if normal is None else normal, dist)[0]

    add("flag clear", world_of(rig, 0, (0.1, 0.1, 2.0)), None, (E.EXIT_FLAG, E.EXIT_FLAG), flag=2)
    for e in (0, 1):
        tag = "LR"[e]
        # ---- a point moved along a segment of the eye's camera frame, from in view (and near: not far) to where it leaves by the test: the
        #      depth test at the sign change of z (x = y: the projection of z = 0 lies on the image diagonal, inside), the four bounds
        for name, inside, outside, axis, code in (("z", (0.4, 0.4, 0.5), (0.4, 0.4, -0.5), 2, E.EXIT_NEG_DEPTH),
                                                  ("mnMinX", (0.0, 0.03, 0.3), (-3.0, 0.03, 0.3), 0, E.EXIT_NOT_IN_IMAGE),
                                                  ("mnMaxX", (0.0, 0.03, 0.3), (3.0, 0.03, 0.3), 0, E.EXIT_NOT_IN_IMAGE),
                                                  ("mnMinY", (0.03, 0.0, 0.3), (0.03, -3.0, 0.3), 1, E.EXIT_NOT_IN_IMAGE),
                                                  ("mnMaxY", (0.03, 0.0, 0.3), (0.03, 3.0, 0.3), 1, E.EXIT_NOT_IN_IMAGE)):
            at = _along(rig, e, inside, outside)
            c0, c1 = L2.crossing(lambda c: exit_at(e, at(c)) == code, 0.0, 1.0)
            add("%s: %s, the last float that stays" % (tag, name), at(c0), e, E.EXIT_REQUEST)
            add("%s: %s, the first float that leaves" % (tag, name), at(c1), e, code)
        # ---- the MapPoint's own thresholds: the value itself and the float beside it
        p0 = world_of(rig, e, (0.2, -0.1, 1.5))
        det = {}
        check_eye(m, rig, e, p0, _toward(rig, e, p0), detail=det)
        d = det["dist"]
        add("%s: dist == min" % tag, p0, e, E.EXIT_REQUEST, dist=(d, 5.0, 3.0))
        add("%s: dist one float below min" % tag, p0, e, E.EXIT_DISTANCE, dist=(_succ(d), 5.0, 3.0))
        add("%s: dist == max" % tag, p0, e, E.EXIT_REQUEST, dist=(0.5, d, 1.5))
        add("%s: dist one float above max" % tag, p0, e, E.EXIT_DISTANCE, dist=(0.5, _pred(d), 1.5))
        # ---- viewCos against 0.5 and against 0.998f: the normal along PO, scaled
        n0 = _toward(rig, e, p0).astype(f64)

        def view_cos(s):
            det = {}
            check_eye(m, rig, e, p0, (n0 * f64(s)).astype(f32), detail=det)
            return det["view_cos"]
        s0, s1 = L2.crossing(lambda s: view_cos(s) < f32(0.5), 0.6, 0.4)
        add("%s: viewCos at 0.5, the last that stays" % tag, p0, e, E.EXIT_REQUEST, normal=(n0 * f64(s0)).astype(f32), radius_base=4.0)
        add("%s: viewCos below 0.5" % tag, p0, e, E.EXIT_VIEW_COS, normal=(n0 * f64(s1)).astype(f32))
        s0, s1 = L2.crossing(lambda s: f64(view_cos(s)) > 0.998, 0.9, 1.0)
        add("%s: viewCos below 0.998f: radius 4.0" % tag, p0, e, E.EXIT_REQUEST, normal=(n0 * f64(s0)).astype(f32), radius_base=4.0)
        add("%s: viewCos at 0.998f: radius 2.5" % tag, p0, e, E.EXIT_REQUEST, normal=(n0 * f64(s1)).astype(f32), radius_base=2.5)
        # ---- a level breakpoint: mfMaxDistance moved across the step from level 2 to level 3

        def level(mf):
            return check_eye(m, rig, e, p0, n0.astype(f32), (0.01, 100.0, mf))[1][5]
        m0, m1 = L2.crossing(lambda mf: level(mf) >= 3, f32(d) * f32(1.2 ** 1.5), f32(d) * f32(1.2 ** 2.5))
        add("%s: ratio below the breakpoint of level 3" % tag, p0, e, E.EXIT_REQUEST, dist=(0.01, 100.0, m0), level=2)
        add("%s: ratio on the breakpoint of level 3" % tag, p0, e, E.EXIT_REQUEST, dist=(0.01, 100.0, m1), level=3)
    # ---- th_far_points against mTrackDepth, the LEFT eye's Pc_dist: the left camera's z moved across it

    at = _along(rig, 0, (0.2, 0.1, 2.0), (0.2, 0.1, 4.0))
    c0, c1 = L2.crossing(lambda c: check_eye(m, rig, 0, at(c), _toward(rig, 0, at(c)))[1][3] > f32(TH_FAR), 0.0, 1.0)
    add("mTrackDepth at th_far_points: kept", at(c0), 0, E.EXIT_REQUEST)
    add("mTrackDepth above th_far_points", at(c1), 0, E.EXIT_FAR)
    # ---- which eye sees it
    both_far = world_of(rig, 0, (0.05, 0.0, 5.0))
    add("far with both eyes in view", both_far, None, (E.EXIT_FAR, E.EXIT_FAR))
    add("both eyes, near", world_of(rig, 0, (0.05, 0.0, 1.2)), None, (E.EXIT_REQUEST, E.EXIT_REQUEST))
    if rig_name == "wide":
        l_only = world_of(rig, 0, (1.26, 0.1, 0.81))         # 1.0 rad off the left axis, 1.7 rad off the yawed right one: outside its image
        r_only = world_of(rig, 0, (-1.496, 0.1, 0.106))      # 1.5 rad off the left axis (outside), 0.8 rad off the right one
    else:                                                    # the narrow rig's eyes see the same: a MapPoint whose normal one eye alone passes
        l_only = r_only = None
    if l_only is not None:
        assert exit_at(0, l_only) == E.EXIT_REQUEST and exit_at(1, l_only, _toward(rig, 0, l_only)) != E.EXIT_REQUEST
        add("left eye only", l_only, None, (E.EXIT_REQUEST, exit_at(1, l_only, _toward(rig, 0, l_only))))
        nr = _toward(rig, 1, r_only)
        not_l = exit_at(0, r_only, nr)
        assert exit_at(1, r_only, nr) == E.EXIT_REQUEST and not_l != E.EXIT_REQUEST
        add("right eye only, no earlier depth", r_only, None, (not_l, E.EXIT_REQUEST), normal=nr)
        add("right eye only, earlier depth below th_far_points", r_only, None, (not_l, E.EXIT_REQUEST), normal=nr, prev=_pred(TH_FAR))
        add("right eye only, earlier depth at th_far_points", r_only, None, (not_l, E.EXIT_REQUEST), normal=nr, prev=TH_FAR)
        add("right eye only, earlier depth above th_far_points: far unless d_mp_prev_depth is NULL", r_only, None, (not_l, E.EXIT_FAR), normal=nr,
            prev=_succ(TH_FAR))
    return pts


def crafted_arrays(rig_name):
    pts = crafted(rig_name)
    n = len(pts)
    rng = np.random.default_rng(11)
    mps = dict(world=np.stack([p["world"] for p in pts]), normal=np.stack([p["normal"] for p in pts]), dist=np.stack([p["dist"] for p in pts]),
               desc=rng.integers(0, 256, (n, 32), dtype=np.uint8))
    return mps, np.array([p["flag"] for p in pts], np.uint8), np.array([p["prev"] for p in pts], f32)
