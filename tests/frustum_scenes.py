"""Scenes for orbx_frustum_requests_device, shared by the CPU tests (tests/test_frustum_requests.py) and the GPU tests
(tests/test_frustum_requests_gpu.py): the seeded uniform scene of the float64 cross-check, three poses, and the CRAFTED points - one MapPoint
per comparison of the statement, placed exactly on it or one float beside it, each with what it was built to reach."""
import numpy as np

import extractorb_amd as X
import frustum_walk as W

f32, f64 = np.float32, np.float64
CAM = (520.0, 520.0, 320.0, 240.0)
BOUNDS = np.array([0.0, 640.0, 0.0, 480.0], f32)
CAM_CRAFTED = (512.0, 512.0, 320.0, 240.0)
MBF = 40.0
SETTING = (1.2, 8)
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], f32)
TH_FAR = 3.0


def pose(tx=0.0, ty=0.0, tz=0.0, yaw=0.0, pitch=0.0):
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]); Rx = np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
    T = np.zeros((3, 4), f32)
    T[:, :3] = (Rx @ Ry).astype(f32); T[:, 3] = (tx, ty, tz)
    return T


POSES = [pose(0.07, -0.03, 0.1, 0.02, -0.01), pose(-0.4, 0.1, 0.5, -0.15, 0.05), pose(1.0, 0.0, -0.3, 0.3, 0.0)]


def uniform_scene(seed, n, pose_index=0, box=((-6, 6), (-4, 4), (-1, 12)), noise=0.6):
    """P uniform in [-6, 6] x [-4, 4] x [-1, 12] (or `box`), mfMaxDistance in [2, 20], normals along the viewing ray plus noise"""
    rng = np.random.default_rng(seed)
    world = np.stack([rng.uniform(lo, hi, n) for lo, hi in box], 1).astype(f32)
    T = POSES[pose_index].astype(f64)
    Ow = -T[:, :3].T @ T[:, 3]
    PO = world.astype(f64) - Ow
    nrm = PO / np.linalg.norm(PO, axis=1, keepdims=True) + noise * rng.standard_normal((n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    mf_max = rng.uniform(2, 20, n).astype(f32)
    mf_min = (mf_max / f32(1.2 ** 7)).astype(f32)
    dist = np.stack([f32(0.8) * mf_min, f32(1.2) * mf_max, mf_max], 1).astype(f32)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    flags = ((rng.random(n) < 0.93).astype(np.uint8) | ((rng.random(n) < 0.8).astype(np.uint8) << 1)).astype(np.uint8)
    angle = rng.uniform(0, 360, n).astype(f32)
    return dict(world=world, normal=nrm.astype(f32), dist=dist, desc=desc), flags, angle


def _pred(x):
    return np.nextafter(f32(x), f32(-np.inf))


def _succ(x):
    return np.nextafter(f32(x), f32(np.inf))


def find_disagreement(seed=5):
    """A float triple PO = (a, 0, c), Pn = (0, 0, n) where isInFrustum's (float)(dot / dist) < 0.5f is FALSE while Fuse's dot < 0.5 * dist is
    TRUE: the double quotient lies below 0.5 by less than half a float step and rounds to 0.5f."""
    rng = np.random.default_rng(seed)
    for _ in range(10000):
        a, c = f32(rng.uniform(0.2, 0.45)), f32(rng.uniform(0.8, 2.0))      # a / c < 0.6: inside the image
        dist = W.norm3((a, f32(0), c))
        n0 = f32(0.5) * dist / c
        for n in (_pred(_pred(n0)), _pred(n0), n0, _succ(n0), _succ(_succ(n0))):
            dot = f64(c) * f64(n)
            if dot < 0.5 * f64(dist) and not f32(dot / f64(dist)) < f32(0.5):
                return (a, f32(0), c), (f32(0), f32(0), f32(n))
    return None


def crafted():
    """list of dict(name, world, normal, dist, flag, want0, want1, check) for the IDENTITY pose, CAM_CRAFTED, BOUNDS, far_points with TH_FAR;
    want0 / want1: the exit in mode 0 / 1; check: fields of the mode-0 result that must hold (radius for th = 1)."""
    E = W
    b = X.predict_scale_breakpoints(*SETTING)
    wide = (0.1, 100.0, 2.0)
    pts = []

    def add(name, world, want0, want1, normal=None, dist=wide, flag=3, **check):
        world = np.array(world, f32)
        if normal is None:
            normal = world / max(float(np.linalg.norm(world.astype(f64))), 1e-9)
        pts.append(dict(name=name, world=world, normal=np.array(normal, f32), dist=np.array(dist, f32), flag=flag, want0=want0, want1=want1,
                        check=check))

    add("flag clear", (0, 0, 2), E.EXIT_FLAG, E.EXIT_FLAG, flag=2)
    add("plain, seen head on", (0, 0, 2), E.EXIT_REQUEST, E.EXIT_REQUEST, radius=2.5, level=0, proj_x=320.0, proj_y=240.0, depth=2.0, proj_xr=300.0)
    add("no observations", (0, 0, 2), E.EXIT_REQUEST, E.EXIT_REQUEST, flag=1, flags=1)
    add("behind the camera: a request in mode 1", (0, 0, -2), E.EXIT_NEG_DEPTH, E.EXIT_REQUEST)
    add("outside the image", (10, 0, 2), E.EXIT_NOT_IN_IMAGE, E.EXIT_NOT_IN_IMAGE)
    add("z = +0 with x != 0: infinity leaves by the bounds", (1, 0, 0), E.EXIT_NOT_IN_IMAGE, E.EXIT_NOT_IN_IMAGE)
    add("z = +0 with x < 0", (-1, 0.5, 0), E.EXIT_NOT_IN_IMAGE, E.EXIT_NOT_IN_IMAGE)
    add("u == mnMinX", (-1.25, 0, 2), E.EXIT_REQUEST, E.EXIT_REQUEST, proj_x=0.0)
    add("u == mnMaxX", (1.25, 0, 2), E.EXIT_REQUEST, E.EXIT_REQUEST, proj_x=640.0)
    add("u 2^-13 below mnMinX", (-(1.25 + 2.0 ** -21), 0, 2), E.EXIT_NOT_IN_IMAGE, E.EXIT_NOT_IN_IMAGE)
    add("u 2^-13 above mnMaxX", (1.25 + 2.0 ** -21, 0, 2), E.EXIT_NOT_IN_IMAGE, E.EXIT_NOT_IN_IMAGE)
    add("v == mnMinY", (0, -0.9375, 2), E.EXIT_REQUEST, E.EXIT_REQUEST, proj_y=0.0)
    add("v == mnMaxY", (0, 0.9375, 2), E.EXIT_REQUEST, E.EXIT_REQUEST, proj_y=480.0)
    add("v 2^-13 above mnMaxY", (0, 0.9375 + 2.0 ** -21, 2), E.EXIT_NOT_IN_IMAGE, E.EXIT_NOT_IN_IMAGE)
    add("dist == min", (0, 0, 2), E.EXIT_REQUEST, E.EXIT_REQUEST, dist=(2.0, 5.0, 3.0))
    add("dist == max", (0, 0, 2), E.EXIT_REQUEST, E.EXIT_REQUEST, dist=(0.5, 2.0, 1.5))
    add("dist one float below min", (0, 0, 2), E.EXIT_DISTANCE, E.EXIT_DISTANCE, dist=(_succ(2.0), 5.0, 3.0), proj_x=320.0, proj_y=240.0, level=-1)
    add("dist one float above max", (0, 0, 2), E.EXIT_DISTANCE, E.EXIT_DISTANCE, dist=(0.5, _pred(2.0), 1.5))
    add("viewCos == 0.5", (0, 0, 2), E.EXIT_REQUEST, E.EXIT_REQUEST, normal=(0.8, 0, 0.5), view_cos=0.5, radius=4.0)
    add("viewCos one float below 0.5", (0, 0, 2), E.EXIT_VIEW_COS, E.EXIT_REQUEST, normal=(0.8, 0, _pred(0.5)), view_cos=0.0, level=-1, proj_x=320.0)
    add("seen from behind", (0, 0, 2), E.EXIT_VIEW_COS, E.EXIT_REQUEST, normal=(0, 0, -1))
    add("viewCos == 0.998f: radius 2.5", (0, 0, 1), E.EXIT_REQUEST, E.EXIT_REQUEST, normal=(0, 0, f32(0.998)), dist=(0.1, 100.0, 1.0),
        view_cos=f32(0.998), radius=2.5, level=0)
    add("viewCos one float below 0.998f: radius 4.0", (0, 0, 1), E.EXIT_REQUEST, E.EXIT_REQUEST, normal=(0, 0, _pred(0.998)), dist=(0.1, 100.0, 1.0),
        view_cos=_pred(0.998), radius=4.0, level=0)
    sc = W.tables(*SETTING)["scale"]
    for k, bk in enumerate(b, 1):
        add("ratio == breakpoint %d" % k, (0, 0, 1), E.EXIT_REQUEST, E.EXIT_REQUEST, dist=(0.1, 100.0, bk), level=k, radius=f32(2.5) * sc[k])
        add("ratio one float below breakpoint %d" % k, (0, 0, 1), E.EXIT_REQUEST, E.EXIT_REQUEST, dist=(0.1, 100.0, _pred(bk)), level=k - 1,
            radius=f32(2.5) * sc[k - 1])
    add("mTrackDepth == th_far_points: kept", (0, 0, TH_FAR), E.EXIT_REQUEST, E.EXIT_REQUEST, depth=TH_FAR)
    add("mTrackDepth one float above th_far_points", (0, 0, _succ(TH_FAR)), E.EXIT_FAR, E.EXIT_REQUEST, depth=_succ(TH_FAR), level=0)
    dis = find_disagreement()
    if dis is not None:
        add("isInFrustum keeps what Fuse's normal test rejects", dis[0], E.EXIT_REQUEST, E.EXIT_REQUEST, normal=dis[1], view_cos=0.5)
    return pts


def crafted_arrays(pts=None):
    pts = crafted() if pts is None else pts
    n = len(pts)
    rng = np.random.default_rng(11)
    mps = dict(world=np.stack([p["world"] for p in pts]), normal=np.stack([p["normal"] for p in pts]), dist=np.stack([p["dist"] for p in pts]),
               desc=rng.integers(0, 256, (n, 32), dtype=np.uint8))
    return mps, np.array([p["flag"] for p in pts], np.uint8), rng.uniform(0, 360, n).astype(f32)


def map_for_frame(rng, frame, T, n, cam=(500.0, 500.0, 320.0, 240.0), behind=0.15):
    """a local map aimed at the keypoints of a synthetic frame (un, d of tests/test_search_projection.random_scene) seen under pose T: MapPoint
    i sits on the ray of a keypoint, a few pixels off, with a descriptor a few bits away and an mfMaxDistance that predicts its octave; a share
    lies behind the camera, outside the image or is seen from the side"""
    un, d = frame["un"], frame["d"]
    R, t = T[:, :3].astype(f64), T[:, 3].astype(f64)
    Ow = -R.T @ t
    world = np.zeros((n, 3), f32); nrm = np.zeros((n, 3), f32); dist = np.zeros((n, 3), f32); desc = np.zeros((n, 32), np.uint8)
    for i in range(n):
        k = int(rng.integers(0, len(un)))
        z = rng.uniform(1.5, 9.0) * (-1 if rng.random() < behind else 1)
        u, v = un["x"][k] + rng.uniform(-4, 4), un["y"][k] + rng.uniform(-4, 4)
        if rng.random() < 0.2:
            u += rng.choice([-900, 900])
        pc = np.array([(u - cam[2]) / cam[0] * z, (v - cam[3]) / cam[1] * z, z])
        pw = R.T @ (pc - t)
        PO = pw - Ow
        dd = np.linalg.norm(PO)
        nv = PO / dd + rng.standard_normal(3) * (0.9 if rng.random() < 0.25 else 0.05)
        lvl = int(np.clip(un["octave"][k], 0, 7))
        mf = dd * 1.2 ** (lvl - 0.5 + (1 if rng.random() < 0.3 else 0))
        world[i] = pw; nrm[i] = nv / np.linalg.norm(nv); dist[i] = (0.8 * mf / 1.2 ** 7, 1.2 * mf, mf)
        desc[i] = d[k]
        for bit in rng.integers(0, 256, int(rng.integers(0, 40))):
            desc[i, bit >> 3] ^= np.uint8(1 << (bit & 7))
    flags = ((rng.random(n) < 0.93).astype(np.uint8) | ((rng.random(n) < 0.85).astype(np.uint8) << 1)).astype(np.uint8)
    return dict(world=world, normal=nrm, dist=dist, desc=desc), flags
