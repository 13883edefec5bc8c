"""ORBmatcher::Fuse on two-camera keyframes (NLeft != -1, a KannalaBrandt8 pair; reference src/ORBmatcher.cc:1399-1609 with bRight false and
true, the loop-closing overload :1611-1733; orbx_fuse_two_eyes_device) - the CPU side.
(a) the sequential walk (tests/fuse_two_eyes_walk.py) against a separately written vectorised statement: its own rig getters, the projection by
    a C statement of KannalaBrandt8::project, masks for the exits, brute force over the in-grid keypoints, argmin of (distance, CSR
    position), the level from the LIBRARY's breakpoint table - on every scene the GPU tests use, both modes, th 3 and 4;
(b) the scenes reach every exit and every candidate filter in EACH eye, and MapPoints fused in the left eye only, the right only and both;
(c) the edge scene's planted probes end where they were planted;
(d) the right eye's own camera and KeyFrame's own right pose decide;
(e) the batching licence on a map model with (left, right) observations: one batched search with eyes = 3 plus the replay (left tail, then
    right tail, changed survivors searched again) equals the sequential reference order; without searching again it does not;
(f) k_fuse_two_eyes.hip's own source compiled for the host against the walk on every scene, and under ASan + UBSan as a stand-alone program;
(g) the surface.
The GPU tests are in tests/test_fuse_two_eyes_gpu.py and use the scenes and walks of this module."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import extractorb_amd as X
import fuse_two_eyes_walk as FW
import fuse_walk as W
import test_kb8_math as KB
from fuse_walk import f32, f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS = np.array([0, 640, 0, 480], f32)
FRAC_BOUNDS = np.array([-3.75, 643.5, -2.25, 482.5], f32)      # KeyFrame truncates them to -3, 643, -2, 482
CAM_L = np.array([284.1, 285.3, 318.2, 242.9, -0.0035, 0.0392, -0.0374, 0.0062], f32)
CAM_R = np.array([286.8, 283.9, 322.6, 236.1, -0.0012, 0.0351, -0.0331, 0.0048], f32)
CAM_EXACT = np.array([256, 256, 256, 192, 0, 0, 0, 0], f32)      # k1..k4 = 0 and power-of-two focal lengths: projections can be planted


def rot(ax, ay):
    cx, sx, cy, sy = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
    return (np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]))


TLR = np.concatenate([rot(0.011, -0.023), np.array([[0.101], [0.0019], [0.0012]])], axis=1).astype(f32)      # mTlr: a rotation and a baseline


def make_eye(kps, desc, bounds):
    off, idx, _ = W.build_grid(kps, bounds)                     # AssignFeaturesToGrid's Nleft != -1 branch: the cells of the RAW keypoints
    return dict(kps=kps, desc=desc, grid_off=off, grid_idx=idx)


def random_scene(seed, n_kp, n_mp, n_rigs, setting=(1.2, 8), lists=1, cams=(CAM_L, CAM_R), bounds=BOUNDS, tlr=TLR, right_extra=9):
    """n_rigs two-camera keyframes around one place; `lists` MapPoint lists, each built on the rigs in turn.  Six in ten MapPoints are seen by
    the rig they are built on, and in every rig a keypoint is planted under their projection in the left eye, the right eye or both (noise, flipped
    descriptor bits, an octave of its own); the others are anywhere - in front, behind, beside, too far, turned away.  The right eye holds
    more keypoints than the left (NRight > NLeft)."""
    rng = np.random.default_rng(seed)
    tab = W.tables(*setting); sc = tab["scale"]; L = tab["nlevels"]
    rigs = []
    for k in range(n_rigs):
        pose = np.concatenate([rot(rng.normal(0, 0.03), rng.normal(0, 0.03)), rng.normal(0, 0.15, (3, 1))], axis=1).astype(f32)
        rigs.append(dict(pose=pose, n=(n_kp - right_extra - 7 * k, n_kp - 3 * k), planted=([], []), geo=FW.keyframe_rig(pose, tlr)))

    def points_for(rig, m):
        world = np.zeros((m, 3), f32); normal = np.zeros((m, 3), f32); dist = np.zeros((m, 3), f32); desc = rng.integers(0, 256, (m, 32), dtype=np.uint8)
        R = rig["pose"][:, :3].astype(f64); t = rig["pose"][:, 3].astype(f64)
        Ow = rig["geo"][0][2].astype(f64)
        for i in range(m):
            kind = rng.random()
            if kind < 0.6:
                u = rng.uniform(bounds[0] + 4, bounds[1] - 8); v = rng.uniform(bounds[2] + 4, bounds[3] - 8); d = rng.uniform(2, 9)
                a, b = (u - cams[0][2]) / cams[0][0], (v - cams[0][3]) / cams[0][1]
                theta, psi = np.hypot(a, b), np.arctan2(b, a)
                xc = d * np.array([np.sin(theta) * np.cos(psi), np.sin(theta) * np.sin(psi), np.cos(theta)])
                lv = min(int(rng.geometric(0.35)) - 1, L - 1)
            else:
                z = rng.uniform(-3, 12) if kind < 0.8 else rng.uniform(1, 9)
                xc = np.array([rng.uniform(-2.5, 2.5) * abs(z), rng.uniform(-2.0, 2.0) * abs(z), z]); lv = int(rng.integers(L))
            p = (R.T @ (xc - t)).astype(f32)
            world[i] = p
            dl = np.linalg.norm(p.astype(f64) - Ow)
            mf_max = dl * sc[lv] * rng.uniform(0.93, 0.999)
            dist[i] = (0.8 * mf_max / sc[-1], 1.2 * mf_max, mf_max)
            if rng.random() < 0.08:
                dist[i, :2] = (dist[i, 1] * 1.05, dist[i, 1] * 1.3) if rng.random() < 0.5 else (dist[i, 0] * 0.2, dist[i, 0] * 0.9)
            nv = (p.astype(f64) - Ow) / max(dl, 1e-9)
            normal[i] = rot(rng.normal(0, 0.25), rng.normal(0, 0.25)) @ nv if rng.random() < 0.8 else rot(rng.uniform(1.0, 2.0), 0.3) @ nv
            if kind < 0.6:
                for other, e in [(g, e) for g in rigs for e in ((0, 1), (0,), (1,))[rng.choice(3, p=[0.4, 0.3, 0.3])]]:      # both eyes, the left only, the right only
                    if len(other["planted"][e]) >= int(0.7 * other["n"][e]):
                        continue
                    _, pu, pv = FW.project(other["geo"][e], cams[e], p)
                    o = int(min(max(lv + rng.choice([0, 0, 0, 0, -1, 1, -2, 2]), 0), L - 1))
                    s = rng.choice([0.5, 0.9, 1.6, 1.6]) * sc[o]
                    x = float(np.clip(pu + rng.normal(0, s), bounds[0] + 1, bounds[1] - 1)); y = float(np.clip(pv + rng.normal(0, s), bounds[2] + 1, bounds[3] - 1))
                    dk = desc[i].copy()
                    for bit in rng.integers(0, 256, rng.choice([0, 3, 20, 45, 50, 51, 70])):
                        dk[bit >> 3] ^= 1 << (bit & 7)
                    other["planted"][e].append((x, y, o, dk))
        return dict(world=world, normal=normal, dist=dist, desc=desc)

    mp_lists = []
    for l in range(lists):
        parts = [points_for(rigs[(l + q) % n_rigs], n_mp // n_rigs + (q < n_mp % n_rigs)) for q in range(n_rigs)]
        mps = dict((key, np.concatenate([p[key] for p in parts])) for key in parts[0])
        perm = rng.permutation(n_mp)
        mp_lists.append(dict((key, v[perm]) for key, v in mps.items()))
    kfs = []
    for rig in rigs:
        eyes = []
        for e in (0, 1):
            n = rig["n"][e]; pl = rig["planted"][e]
            kps = np.zeros(n, X.KEYPOINT_DTYPE); desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
            kps["x"] = rng.uniform(bounds[0] + 2, bounds[1] - 2, n).astype(f32); kps["y"] = rng.uniform(bounds[2] + 2, bounds[3] - 2, n).astype(f32)
            kps["octave"] = np.minimum(rng.geometric(0.35, n) - 1, L - 1)
            where = rng.permutation(n)[:len(pl)]                               # planted keypoints at any index: right winners above NLeft occur
            for j, (x, y, o, dk) in zip(where, pl):
                kps["x"][j] = x; kps["y"][j] = y; kps["octave"][j] = o; desc[j] = dk
            eyes.append(make_eye(kps, desc, bounds))
        kfs.append(dict(pose=rig["pose"], eyes=tuple(eyes)))
    return dict(tab=tab, setting=setting, cams=(np.asarray(cams[0], f32), np.asarray(cams[1], f32)), bounds=bounds, tlr=np.asarray(tlr, f32), kfs=kfs,
                lists=mp_lists, seed=seed)


def flags_for(scene, pair, n):
    """bit 0 per (pair, MapPoint), one flag for both eyes; the edge scene searches every probe"""
    return (np.random.default_rng(scene["seed"] * 131 + pair).random(n) < scene.get("flag_density", 0.85)).astype(np.uint8)


# ---------------------------------------------------------------- the edge scene ----------------------------------------------------------------
# numerically the identity and a baseline of 1/8 along x, with NEGATIVE zeros where a camera-frame z of -0.0f needs them: a sum of products is
# -0 only if every term is (cv::gemm adds the addend last), so row 2 of the pose, its t_z and column 2 of mTlr's rotation carry the sign
EDGE_POSE = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [-0.0, -0.0, 1, -0.0]], f32)
EDGE_TLR = np.array([[1, 0, -0.0, 0.125], [0, 1, -0.0, 0], [0, 0, 1, 0]], f32)
RETURNS = dict(th=-300.0)          # the option set under which the early returns are reached (a negative radius)


def edge_scene(setting=(1.2, 8)):
    """one rig keyframe, both eyes with CAM_EXACT, FRAC_BOUNDS; every MapPoint is a named probe "L_..." / "R_..." meant for one eye (the
    other eye sees it too, a baseline away: nothing is asserted there).  Returns the scene and {name: MapPoint index}."""
    tab = W.tables(*setting); L = tab["nlevels"]
    rng = np.random.default_rng(5)
    geo = FW.keyframe_rig(EDGE_POSE, EDGE_TLR)
    kp = ([], []); mp = []; names = {}
    rnd = lambda: rng.integers(0, 256, 32, dtype=np.uint8)      # noqa: E731
    for _ in range(10):                                          # NRight > NLeft: ten right keypoints more, in a corner no probe looks at
        kp[1].append((f32(rng.uniform(600, 630)), f32(rng.uniform(5, 30)), 0, rnd()))

    def uv(e, p):
        return FW.project(geo[e], CAM_EXACT, p)[1:]

    def cam_to_world(e, c):
        return np.array([c[0] + (0.125 if e else 0.0), c[1], c[2]], f32)

    def near(e, u, v, z=4.0):
        """a world point whose projection in eye e is close to (u, v)"""
        a, b = (u - 256.0) / 256.0, (v - 192.0) / 256.0
        theta, psi = np.hypot(a, b), np.arctan2(b, a)
        return cam_to_world(e, z * np.array([np.tan(theta) * np.cos(psi), np.tan(theta) * np.sin(psi), 1.0]))

    def on_axis(e, axis, target):
        """a world point whose projection in eye e is EXACTLY target along `axis` (0: u, with v on the principal row; 1: v), found by
        bisection over the float bit patterns of the camera-frame coordinate through the walk's own projection"""
        c0 = 256.0 if axis == 0 else 192.0
        sign = 1.0 if target >= c0 else -1.0
        for z in (4.0, 2.0, 1.0, 8.0, 3.0, 5.0, 6.0, 7.0):
            def value(bits):
                m = np.array([bits], np.int32).view(f32)[0]
                c = [0.0, 0.0, z]; c[axis] = sign * float(m)
                p = cam_to_world(e, c)
                return uv(e, p)[axis], p
            lo, hi = np.array([1e-6], f32).view(np.int32)[0], np.array([1e5], f32).view(np.int32)[0]
            while hi - lo > 1:
                mid = (int(lo) + int(hi)) // 2
                if sign * (float(value(mid)[0]) - target) < 0:
                    lo = mid
                else:
                    hi = mid
            for bits in range(int(lo) - 4, int(lo) + 6):
                got, p = value(bits)
                if got == f32(target):
                    return p
        raise AssertionError("no exact projection for %r" % ((e, axis, target),))

    def add_kp(e, x, y, octave=0, desc=None):
        kp[e].append((f32(x), f32(y), int(octave), rnd() if desc is None else desc))
        return len(kp[e]) - 1

    def add_mp(name, e, p, desc, ratio=1.0, normal=None, dist=None, mf_max=None):
        p = np.asarray(p, f32); po = p - geo[e][2]
        d = f32(np.sqrt((f64(po[0]) * f64(po[0]) + f64(po[1]) * f64(po[1])) + f64(po[2]) * f64(po[2])))
        mf = f32(ratio) * d if mf_max is None else f32(mf_max)
        lo, hi = (f32(0.0), f32(1e9)) if dist is None else dist
        nv = po / max(float(d), 1e-9) if normal is None else normal
        names["LR"[e] + "_" + name] = len(mp); mp.append((p, np.asarray(nv, f32), (lo, hi, mf), desc))

    def under(name, e, p, octave=0, desc_mp=None, dx=0.0, dy=0.0, **kw):
        """a probe and a keypoint with its descriptor under its projection (moved by dx, dy)"""
        d0 = rnd(); u, v = uv(e, p)
        j = add_kp(e, u + f32(dx), v + f32(dy), octave, d0)
        add_mp(name, e, p, d0 if desc_mp is None else desc_mp(d0), **kw)
        return j

    def flipped(bits):
        def f(d0):
            dm = d0.copy()
            for b in range(bits):
                dm[b >> 3] ^= 1 << (b & 7)
            return dm
        return f

    for e in (0, 1):
        # KeyFrame::IsInImage on the truncated bounds: the lower bound itself passes, the upper bound itself fails (strict); between a float
        # bound and its truncation is outside although Frame's own bounds hold it
        under("u_is_truncated_min", e, on_axis(e, 0, -3.0)); under("u_between_float_and_truncated_min", e, on_axis(e, 0, -3.5))
        under("v_is_truncated_min", e, on_axis(e, 1, -2.0)); under("v_between_float_and_truncated_min", e, on_axis(e, 1, -2.125))
        add_mp("u_is_truncated_max", e, on_axis(e, 0, 643.0), rnd()); add_mp("u_below_truncated_max", e, on_axis(e, 0, 642.75), rnd())
        add_mp("v_is_truncated_max", e, on_axis(e, 1, 482.0), rnd()); add_mp("v_below_truncated_max", e, on_axis(e, 1, 481.75), rnd())
        # z == 0 and z == -0.0f do not leave by themselves: theta = atan2f(r, +-0) = pi / 2, on the diagonal that is inside this image
        under("z_is_zero", e, cam_to_world(e, (1.0, 1.0, 0.0))); under("z_is_negative_zero", e, cam_to_world(e, (1.5, 1.5, -0.0)), dx=0.25)
        # on the axis r = 0: atan2f(0, +0) = 0 projects on the principal point, at distance 0 from the centre (ratio = inf: the top level);
        # atan2f(0, -0) = pi projects far outside
        under("z_is_zero_on_axis", e, cam_to_world(e, (0.0, 0.0, 0.0)), octave=L - 1, mf_max=1.0)
        add_mp("z_is_negative_zero_on_axis", e, cam_to_world(e, (0.0, 0.0, -0.0)), rnd(), mf_max=1.0)
        add_mp("z_negative", e, near(e, 300.0, 250.0, -4.0), rnd())
        # the four early returns of GetFeaturesInArea need a negative radius: see RETURNS
        for name, (u, v) in dict(min_x=(500.0, 240.0), max_x=(100.0, 240.0), min_y=(300.0, 200.0), max_y=(300.0, 100.0)).items():
            add_mp("return_" + name, e, near(e, u, v + 60.0 * e), rnd())
        # candidates: the box test, the level filter on both sides, level - 1 = -1, the 5.99 gate, a tie decided by visit order, th_low
        base = 40.0 + 200.0 * e                                             # the two eyes' probes on rows of their own
        p = near(e, 60.0, base); under("box_rejects", e, p, dx=3.5)           # in the window's cells, |dx| >= r = 3
        under("level_too_high", e, near(e, 100.0, base), octave=2); under("level_too_low", e, near(e, 140.0, base), octave=0, ratio=float(tab["scale"][2]) * 0.97)
        under("level_minus_one", e, near(e, 180.0, base), octave=-1)
        under("gate_rejects", e, near(e, 220.0, base), dx=2.5); under("gate_passes", e, near(e, 260.0, base), dx=2.0)      # 6.25 > 5.99 >= 4
        h_inv = f32(48) / (FRAC_BOUNDS[3] - FRAC_BOUNDS[2])
        row = np.round((base + 2.25) * h_inv)
        p = near(e, 304.0, (row + 0.5) / h_inv - 2.25); u, v = uv(e, p); d0 = rnd()      # on the border between two rows of cells
        first = add_kp(e, u, v + 1.0, 0, d0)             # the cell below: visited second
        second = add_kp(e, u, v - 1.0, 0, d0)            # the cell above: visited first, although its index is larger
        add_mp("tie_by_visit_order", e, p, d0)
        d1 = d0.copy(); d1[0] ^= 1
        add_kp(e, u + 2.0, v, 0, d1)                                        # a worse distance changes nothing
        names["LR"[e] + "_twins"] = (first, second)
        under("dist_50", e, near(e, 350.0, base), desc_mp=flipped(50)); under("dist_51", e, near(e, 400.0, base), desc_mp=flipped(51))
        under("last", e, near(e, 450.0, base))                              # the last keypoint of its eye: in the right eye an index >= NLeft
    eyes = []
    for e in (0, 1):
        kps = np.zeros(len(kp[e]), X.KEYPOINT_DTYPE)
        kps["x"] = [k[0] for k in kp[e]]; kps["y"] = [k[1] for k in kp[e]]; kps["octave"] = [k[2] for k in kp[e]]
        eyes.append(make_eye(kps, np.stack([k[3] for k in kp[e]]), FRAC_BOUNDS))
    mps = dict(world=np.stack([m[0] for m in mp]), normal=np.stack([m[1] for m in mp]), dist=np.array([m[2] for m in mp], f32), desc=np.stack([m[3] for m in mp]))
    scene = dict(tab=tab, setting=setting, cams=(CAM_EXACT, CAM_EXACT), bounds=FRAC_BOUNDS, tlr=EDGE_TLR, kfs=[dict(pose=EDGE_POSE, eyes=tuple(eyes))],
                 lists=[mps], seed=5, flag_density=1.0)
    return scene, names


_scenes = {}


def get(name):
    """the scenes of the CPU and the GPU tests, built once"""
    if name not in _scenes:
        _scenes[name] = dict(
            small=lambda: random_scene(1, 96, 150, 3),                            # capacity 96 per eye x 150 MapPoints x 3 rigs, one list
            small_lists=lambda: random_scene(2, 96, 150, 3, lists=3),             # one list per rig
            small_12=lambda: random_scene(4, 96, 150, 3, setting=(1.1, 12)),
            small_frac=lambda: random_scene(8, 96, 150, 3, bounds=FRAC_BOUNDS),  # non-integer image bounds
            real=lambda: random_scene(6, 1200, 1000, 4),                          # capacity 1302, 1000 MapPoints x 4 rigs
            long=lambda: random_scene(7, 1200, 5000, 1),                          # one long list into one rig
            edge=lambda: edge_scene()[0],
            edge_12=lambda: edge_scene((1.1, 12))[0],
        )[name]()
    return _scenes[name]


SCENES = ("small", "small_lists", "small_12", "small_frac", "real", "long", "edge", "edge_12")
_walks = {}


def walk(name, kf, lst, right, reproj_check=True, th=3.0, th_low=50, n_mp=None):
    """the walk of list `lst` into eye `right` of rig `kf` of a scene under the flags flags_for(scene, kf) - shared by all tests, never changed"""
    key = (name, kf, lst, bool(right), reproj_check, th, th_low, n_mp)
    if key not in _walks:
        s = get(name)
        stats = {}
        mps = s["lists"][lst]
        r = FW.search(s["kfs"][kf], right, mps, flags_for(s, kf, len(mps["world"])), s["tlr"], s["cams"], s["bounds"], s["tab"], th=th, th_low=th_low,
                      reproj_check=reproj_check, n_mp=n_mp, stats=stats)
        r["stats"] = stats
        _walks[key] = r
    return _walks[key]


def cases(name):
    """(rig, list) pairs a scene is searched as"""
    s = get(name)
    return [(k, k % len(s["lists"])) for k in range(len(s["kfs"]))]


@pytest.fixture(scope="module")
def kb8_host(tmp_path_factory):
    return KB.build_kb8_host(tmp_path_factory.mktemp("kb8_for_fuse"))


# ---------------------------------------------------------------- (a) the independent statement ----------------------------------------------------------------
def mat_vec(A, b, alpha=1.0, c=None):
    """cv::gemm of a 3x3 on a 3-vector, all rows at once: products and sums in double in element order, scaled, the addend, one rounding"""
    A = np.asarray(A, f32).astype(f64); b = np.asarray(b, f32).astype(f64)
    s = ((A[:, 0] * b[0] + A[:, 1] * b[1]) + A[:, 2] * b[2]) * alpha
    return (s if c is None else s + np.asarray(c, f32).astype(f64)).astype(f32)


def statement_rig(pose, tlr, right):
    P = np.asarray(pose, f32); T = np.asarray(tlr, f32)
    Rlw, tlw = P[:, :3], P[:, 3]
    Ow = mat_vec(Rlw.T, tlw, -1.0)
    if not right:
        return Rlw, tlw, Ow
    Rrl = T[:, :3].T
    Rrw = np.stack([mat_vec(Rrl, Rlw[:, c]) for c in range(3)], axis=1)
    trl = mat_vec(Rrl, T[:, 3], -1.0)
    return Rrw, mat_vec(Rrl, tlw, 1.0, trl), mat_vec(Rlw.T, T[:, 3], 1.0, Ow)


def statement(host, s, kf, right, mps, flags, reproj_check=True, th=3.0, th_low=50):
    """per MapPoint, no walk: vector arithmetic for the front end, the projection by the C statement of KannalaBrandt8::project, masks for the
    exits, brute force over the in-grid keypoints, the level from the library's breakpoint table (the walk uses the expression)"""
    tab = s["tab"]; cam = np.ascontiguousarray(s["cams"][1 if right else 0], f32)
    fb = np.asarray(s["bounds"], f32)
    w_inv = f32(64) / (fb[1] - fb[0]); h_inv = f32(48) / (fb[3] - fb[2])
    minx, maxx, miny, maxy = (f32(int(b)) for b in fb)
    bp = X.predict_scale_breakpoints(*s["setting"])
    R, t, O = statement_rig(kf["pose"], s["tlr"], right)
    eye = kf["eyes"][1 if right else 0]; n_left = len(kf["eyes"][0]["kps"])
    M = len(mps["world"]); w = mps["world"].astype(f32)
    with np.errstate(all="ignore"):
        w64 = w.astype(f64); R64 = R.astype(f64)
        pc = np.stack([(((R64[r, 0] * w64[:, 0] + R64[r, 1] * w64[:, 1]) + R64[r, 2] * w64[:, 2]) * 1.0 + f64(t[r])).astype(f32) for r in range(3)], axis=1)
        pc = np.ascontiguousarray(pc); uv = np.zeros((M, 2), f32)
        host.kb8_project_libm(cam.ctypes.data_as(C.c_void_p), M, pc.ctypes.data_as(C.c_void_p), uv.ctypes.data_as(C.c_void_p))
        u, v = uv[:, 0], uv[:, 1]
        PO64 = (w - O[None, :]).astype(f64)
        d3 = np.sqrt((PO64[:, 0] ** 2 + PO64[:, 1] ** 2) + PO64[:, 2] ** 2).astype(f32)
        nv = mps["normal"].astype(f32).astype(f64)
        dot = (PO64[:, 0] * nv[:, 0] + PO64[:, 1] * nv[:, 1]) + PO64[:, 2] * nv[:, 2]
        ratio = mps["dist"][:, 2].astype(f32) / d3
        level = np.searchsorted(bp, np.where(np.isnan(ratio), f32(0), ratio), side="right")
        radius = f32(th) * tab["scale"][level]
        code = np.full(M, -1, np.int32)

        def leave(mask, c):
            code[(code < 0) & mask] = c
        leave((flags & 1) == 0, W.EXIT_FLAG)
        leave(pc[:, 2] < 0, W.EXIT_NEG_DEPTH)
        leave(~((u >= minx) & (u < maxx) & (v >= miny) & (v < maxy)), W.EXIT_NOT_IN_IMAGE)
        leave((d3 < mps["dist"][:, 0]) | (d3 > mps["dist"][:, 1]), W.EXIT_DISTANCE)
        leave(dot < 0.5 * d3.astype(f64), W.EXIT_NORMAL)
        kps = eye["kps"]
        _, order, cell = W.build_grid(kps, s["bounds"])
        pos = np.full(len(kps), 1 << 30, np.int64); pos[order] = np.arange(len(order))
        kx, ky, ko = kps["x"].astype(f32), kps["y"].astype(f32), kps["octave"].astype(np.int64)
        best_idx = np.full(M, -1, np.int32); best_dist = np.full(M, 256, np.int32)
        for i in np.nonzero(code < 0)[0]:
            r = radius[i]
            lo_x = np.floor((u[i] - minx - r) * w_inv); hi_x = np.ceil((u[i] - minx + r) * w_inv)
            lo_y = np.floor((v[i] - miny - r) * h_inv); hi_y = np.ceil((v[i] - miny + r) * h_inv)
            seen = (cell >= 0) & (lo_x < 64) & (hi_x >= 0) & (lo_y < 48) & (hi_y >= 0)
            seen &= (cell // 48 >= lo_x) & (cell // 48 <= hi_x) & (cell % 48 >= lo_y) & (cell % 48 <= hi_y)
            seen &= (np.abs(kx - u[i]) < r) & (np.abs(ky - v[i]) < r)
            if not seen.any():
                code[i] = W.EXIT_EMPTY_WINDOW; continue
            ok = seen & (ko >= level[i] - 1) & (ko <= level[i])
            if reproj_check:
                inv = tab["inv_sigma2"][np.clip(ko, 0, tab["nlevels"] - 1)]
                ex = u[i] - kx; ey = v[i] - ky
                ok &= ~(((ex * ex + ey * ey) * inv).astype(f64) > 5.99)
            if ok.any():
                j = np.nonzero(ok)[0]
                dist = W.POPCOUNT[eye["desc"][j] ^ mps["desc"][i][None, :]].sum(axis=1)
                b = j[np.lexsort((pos[j], dist))[0]]
                best_dist[i] = int(W.POPCOUNT[eye["desc"][b] ^ mps["desc"][i]].sum())
                if best_dist[i] <= th_low:
                    best_idx[i] = b + (n_left if right else 0)
            code[i] = W.EXIT_FUSED if best_idx[i] >= 0 else W.EXIT_ABOVE_TH_LOW
    return dict(best_idx=best_idx, best_dist=best_dist, exit=code.astype(np.uint8), n_fused=int((code == W.EXIT_FUSED).sum()))


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("best_idx", "best_dist", "exit")) and a["n_fused"] == b["n_fused"]


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("reproj_check", [True, False])
def test_walk_equals_the_independent_statement(kb8_host, name, reproj_check):
    s = get(name)
    for kf, lst in cases(name):
        mps = s["lists"][lst]
        for right in (False, True):
            want = statement(kb8_host, s, s["kfs"][kf], right, mps, flags_for(s, kf, len(mps["world"])), reproj_check)
            got = walk(name, kf, lst, right, reproj_check)
            bad = np.nonzero((want["best_idx"] != got["best_idx"]) | (want["best_dist"] != got["best_dist"]) | (want["exit"] != got["exit"]))[0]
            assert same(want, got), (name, kf, right, bad[:5], want["exit"][bad[:5]], got["exit"][bad[:5]])


@pytest.mark.parametrize("name", ["small", "small_frac", "edge"])
def test_walk_equals_the_statement_with_the_wider_window_and_under_the_early_returns(kb8_host, name):
    s = get(name)
    for opt in [dict(th=4.0), dict(th=4.0, reproj_check=False)] + ([RETURNS] if name == "edge" else []):
        for kf, lst in cases(name):
            mps = s["lists"][lst]
            for right in (False, True):
                assert same(statement(kb8_host, s, s["kfs"][kf], right, mps, flags_for(s, kf, len(mps["world"])), **opt), walk(name, kf, lst, right, **opt)), (opt, kf, right)


def test_statement_rig_equals_the_walks_getters():
    for seed in range(5):
        rng = np.random.default_rng(seed)
        pose = np.concatenate([rot(rng.normal(0, 0.5), rng.normal(0, 0.5)), rng.normal(0, 1.0, (3, 1))], axis=1).astype(f32)
        tlr = np.concatenate([rot(rng.normal(0, 0.2), rng.normal(0, 0.2)), rng.normal(0, 0.2, (3, 1))], axis=1).astype(f32)
        for e in (0, 1):
            for a, b in zip(FW.keyframe_rig(pose, tlr)[e], statement_rig(pose, tlr, bool(e))):
                assert np.array_equal(a, b)
        # and they are the rig: the right pose maps a world point where the left pose followed by the inverse of mTlr does
        (Rl, tl, Ol), (Rr, tr, Or) = FW.keyframe_rig(pose, tlr)
        p = rng.normal(0, 3, 3)
        x_l = Rl.astype(f64) @ p + tl; x_r = tlr[:, :3].astype(f64).T @ (x_l - tlr[:, 3])
        assert np.allclose(Rr.astype(f64) @ p + tr, x_r, atol=1e-5) and np.allclose(Rr.astype(f64) @ Or + tr, 0, atol=1e-5)


# ---------------------------------------------------------------- (b) reach ----------------------------------------------------------------
def test_scenes_reach_every_exit_and_every_candidate_filter_in_each_eye():
    for name in ("small", "small_lists", "small_12", "small_frac", "real", "long"):
        for right in (False, True):
            for rc in (True, False):
                seen = set(); stats = {}
                for kf, lst in cases(name):
                    r = walk(name, kf, lst, right, rc)
                    seen |= set(r["exit"].tolist())
                    for k, v in r["stats"].items():
                        stats[k] = stats.get(k, 0) + v
                assert seen == set(range(8)), (name, right, rc, seen)
                need = ["box_test", "level_too_low", "level_too_high"] + (["reject_5_99", "pass_5_99"] if rc else [])
                if name in ("real", "long"):
                    need += ["window_past_left", "window_past_right", "window_past_top", "window_past_bottom"]
                assert not [k for k in need if not stats.get(k, 0)], (name, right, rc, stats)
        # fused in the left eye only, in the right eye only, in both
        left = np.concatenate([walk(name, kf, lst, False)["exit"] for kf, lst in cases(name)]) == W.EXIT_FUSED
        right = np.concatenate([walk(name, kf, lst, True)["exit"] for kf, lst in cases(name)]) == W.EXIT_FUSED
        assert (left & ~right).sum() > 0 and (~left & right).sum() > 0 and (left & right).sum() > 0, name
    assert walk("real", 0, 0, False)["n_fused"] > 50 and walk("real", 0, 0, True)["n_fused"] > 50
    assert walk("long", 0, 0, False)["n_fused"] > 200 and walk("long", 0, 0, True)["n_fused"] > 200
    # NRight > NLeft, and right winners at or above NLeft
    s = get("small")
    assert all(len(k["eyes"][1]["kps"]) > len(k["eyes"][0]["kps"]) for k in s["kfs"])
    assert sum(walk("small", kf, lst, True)["stats"].get("right_winner_at_or_above_nleft", 0) for kf, lst in cases("small")) > 0


# ---------------------------------------------------------------- (c) the planted probes ----------------------------------------------------------------
@pytest.mark.parametrize("setting", [(1.2, 8), (1.1, 12)])
def test_edge_scene_probes_end_where_they_were_planted(setting):
    s, at_ = edge_scene(setting)
    kf = s["kfs"][0]; mps = s["lists"][0]
    n = len(mps["world"]); ones = np.ones(n, np.uint8)
    kw = dict(tlr=s["tlr"], cams=s["cams"], bounds=s["bounds"], tab=s["tab"])
    geo = FW.keyframe_rig(kf["pose"], s["tlr"])
    n_left, n_right = len(kf["eyes"][0]["kps"]), len(kf["eyes"][1]["kps"])
    assert n_right > n_left
    for e, tag in ((0, "L_"), (1, "R_")):
        stats = {}
        r = FW.search(kf, bool(e), mps, ones, stats=stats, **kw)
        ex = lambda k: int(r["exit"][at_[tag + k]])      # noqa: E731
        proj = lambda k: FW.project(geo[e], CAM_EXACT, mps["world"][at_[tag + k]])      # noqa: E731
        # the bounds: exact projections on the truncated bounds and between them and the float bounds
        assert proj("u_is_truncated_min")[1] == -3.0 and ex("u_is_truncated_min") == W.EXIT_FUSED
        assert proj("u_between_float_and_truncated_min")[1] == -3.5 and ex("u_between_float_and_truncated_min") == W.EXIT_NOT_IN_IMAGE
        assert proj("v_is_truncated_min")[2] == -2.0 and ex("v_is_truncated_min") == W.EXIT_FUSED
        assert proj("v_between_float_and_truncated_min")[2] == -2.125 and ex("v_between_float_and_truncated_min") == W.EXIT_NOT_IN_IMAGE
        assert proj("u_is_truncated_max")[1] == 643.0 and ex("u_is_truncated_max") == W.EXIT_NOT_IN_IMAGE
        assert proj("u_below_truncated_max")[1] == 642.75 and ex("u_below_truncated_max") > W.EXIT_NOT_IN_IMAGE
        assert proj("v_is_truncated_max")[2] == 482.0 and ex("v_is_truncated_max") == W.EXIT_NOT_IN_IMAGE
        assert proj("v_below_truncated_max")[2] == 481.75 and ex("v_below_truncated_max") > W.EXIT_NOT_IN_IMAGE
        # under the float bounds the "between" probes would have fused: a keypoint with their descriptor lies under them, in a grid cell
        for k in ("u_between_float_and_truncated_min", "v_between_float_and_truncated_min"):
            _, u, v = proj(k)
            eye = kf["eyes"][e]
            cand = [j for j in eye["grid_idx"] if abs(eye["kps"]["x"][j] - u) < 3 and abs(eye["kps"]["y"][j] - v) < 3]
            assert any(np.array_equal(eye["desc"][j], mps["desc"][at_[tag + k]]) for j in cand)
        # z = +0 and z = -0.0f: not negative, a finite projection; off the axis inside the image and fused
        for k in ("z_is_zero", "z_is_negative_zero"):
            pc, u, v = proj(k)
            assert pc[2] == 0 and bool(np.signbit(pc[2])) == (k == "z_is_negative_zero") and np.isfinite(u) and np.isfinite(v) and ex(k) == W.EXIT_FUSED, k
        pc, u, v = proj("z_is_zero_on_axis")
        assert pc[0] == 0 and pc[1] == 0 and pc[2] == 0 and not np.signbit(pc[2]) and (u, v) == (256.0, 192.0) and ex("z_is_zero_on_axis") == W.EXIT_FUSED
        pc, u, v = proj("z_is_negative_zero_on_axis")
        assert pc[2] == 0 and np.signbit(pc[2]) and u > 643 and ex("z_is_negative_zero_on_axis") == W.EXIT_NOT_IN_IMAGE
        assert stats["z_is_zero"] >= 4 and ex("z_negative") == W.EXIT_NEG_DEPTH
        # the candidates
        assert ex("box_rejects") == W.EXIT_EMPTY_WINDOW and stats["box_test"] >= 1
        assert ex("level_too_high") == W.EXIT_ABOVE_TH_LOW and r["best_dist"][at_[tag + "level_too_high"]] == 256 and stats["level_too_high"] >= 1
        assert ex("level_too_low") == W.EXIT_ABOVE_TH_LOW and r["best_dist"][at_[tag + "level_too_low"]] == 256 and stats["level_too_low"] >= 1
        assert ex("level_minus_one") == W.EXIT_FUSED and stats["level_minus_one"] >= 1
        assert ex("gate_rejects") == W.EXIT_ABOVE_TH_LOW and ex("gate_passes") == W.EXIT_FUSED and stats["reject_5_99"] >= 1
        first, second = at_[tag + "twins"]
        eye = kf["eyes"][e]
        pos = dict((int(j), q) for q, j in enumerate(eye["grid_idx"]))
        cell = lambda j: int(np.searchsorted(eye["grid_off"], pos[j], side="right")) - 1      # noqa: E731
        assert second > first and cell(second) < cell(first)                  # the later index sits in the earlier cell: visited first
        i = at_[tag + "tie_by_visit_order"]
        assert r["best_idx"][i] == second + (n_left if e else 0) and r["best_dist"][i] == 0 and stats["tie_kept_first"] >= 1
        assert ex("dist_50") == W.EXIT_FUSED and r["best_dist"][at_[tag + "dist_50"]] == 50
        assert ex("dist_51") == W.EXIT_ABOVE_TH_LOW and r["best_dist"][at_[tag + "dist_51"]] == 51 and r["best_idx"][at_[tag + "dist_51"]] == -1
        # the keyframe's numbering: the right eye's last keypoint has an index of its own >= NLeft and comes back as NLeft + it
        last = len(eye["kps"]) - 1
        assert ex("last") == W.EXIT_FUSED and r["best_idx"][at_[tag + "last"]] == last + (n_left if e else 0)
        if e:
            assert last >= n_left and stats["right_winner_at_or_above_nleft"] >= 1
        # the Sim3 mode has no gate
        r0 = FW.search(kf, bool(e), mps, ones, reproj_check=False, **kw)
        assert r0["exit"][at_[tag + "gate_rejects"]] == W.EXIT_FUSED
        # the early returns (a negative radius): each of the four is taken, and everything that reaches the window leaves as "empty window"
        stats = {}
        rr = FW.search(kf, bool(e), mps, ones, stats=stats, **dict(kw, **RETURNS))
        for k in ("min_x", "max_x", "min_y", "max_y"):
            assert stats.get("return_%s_cell_%s" % tuple(k.split("_")), 0) >= 1, (k, stats)
            assert rr["exit"][at_[tag + "return_" + k]] == W.EXIT_EMPTY_WINDOW
        assert not (rr["exit"] > W.EXIT_EMPTY_WINDOW).any()


# ---------------------------------------------------------------- (d) the eye's own parameters ----------------------------------------------------------------
def test_the_right_eye_projects_with_its_own_camera():
    s = get("small")
    mps = s["lists"][0]; fl = flags_for(s, 0, 150)
    kw = dict(tlr=s["tlr"], bounds=s["bounds"], tab=s["tab"])
    own = walk("small", 0, 0, True)
    swapped = FW.search(s["kfs"][0], True, mps, fl, cams=(s["cams"][1], s["cams"][0]), **kw)
    assert not same(own, swapped)
    assert same(walk("small", 0, 0, False), FW.search(s["kfs"][0], False, mps, fl, cams=(s["cams"][0], s["cams"][0]), **kw))      # the left eye never reads mpCamera2


def test_the_right_pose_is_the_keyframes_not_one_built_from_a_separate_trl():
    """The frustum entry takes mTrl and mTlr side by side, as the Frame holds them.  KeyFrame's getters take mTlr alone: trl = -Rrl*mTlr.t is
    ONE cv::gemm (sums in double, one rounding).  A Trl that reaches the caller another way - here the same inverse in binary32 arithmetic, as a
    calibration tool would write it - differs from that in the last bit once mTlr has a rotation, and with it the right translation"""
    differing = 0
    for seed in range(8):
        rng = np.random.default_rng(seed)
        tlr = np.concatenate([rot(rng.normal(0, 0.05), rng.normal(0, 0.05)), rng.normal(0, 0.1, (3, 1))], axis=1).astype(f32)
        pose = np.concatenate([rot(rng.normal(0, 0.3), rng.normal(0, 0.3)), rng.normal(0, 1.0, (3, 1))], axis=1).astype(f32)
        Rrl = tlr[:, :3].T
        t_apart = np.array([-f32(f32(f32(Rrl[r, 0] * tlr[0, 3]) + f32(Rrl[r, 1] * tlr[1, 3])) + f32(Rrl[r, 2] * tlr[2, 3])) for r in range(3)], f32)
        (_, _, _), (Rrw, trw, twr) = FW.keyframe_rig(pose, tlr)
        t_frame = np.array([W.gemm_row(Rrl[r], pose[:, 3], 1.0, t_apart[r]) for r in range(3)], f32)      # Frame.cc:1190 with that Trl
        assert np.allclose(t_frame, trw, atol=1e-6)
        differing += int(not np.array_equal(t_frame, trw))
    assert differing > 0


# ---------------------------------------------------------------- (e) the batching licence ----------------------------------------------------------------
def licence_scene(seed):
    """three rig keyframes with the same view but descriptors of their own in both eyes (bits flipped), one list of MapPoints; many keypoints
    already hold MapPoints (some of them in the list, some with more observations than the list's, some with fewer).  As
    tests/test_fuse.py's, for keyframes whose slots run over the left and then the right keypoints."""
    s = random_scene(seed, 96, 150, 1)
    rng = np.random.default_rng(seed + 1000)
    base = s["kfs"][0]
    kfs = [base]
    for k in (1, 2):
        eyes = []
        for eye in base["eyes"]:
            d = eye["desc"].copy()
            for j in range(len(d)):
                for b in rng.integers(0, 256, rng.choice([0, 8, 16, 28])):
                    d[j, b >> 3] ^= 1 << (b & 7)
            eyes.append(dict(eye, desc=d))
        kfs.append(dict(base, eyes=tuple(eyes)))
    s["kfs"] = kfs
    n_list = 150
    n_points = n_list + 200
    mp_list = [int(v) if rng.random() < 0.95 else -1 for v in rng.permutation(n_list)]
    point_desc = rng.integers(0, 256, (n_points, 32), dtype=np.uint8)
    for i, mp in enumerate(mp_list):
        if mp >= 0:
            point_desc[mp] = s["lists"][0]["desc"][i]
    elsewhere = [rng.integers(0, 256, (1, 32), dtype=np.uint8) for _ in range(4)]      # four more keyframes, one (left) keypoint each
    n_left = [len(k["eyes"][0]["kps"]) for k in kfs] + [1] * 4
    m = FW.Map(point_desc, [np.concatenate([k["eyes"][0]["desc"], k["eyes"][1]["desc"]]) for k in kfs] + elsewhere, n_left)
    for k, kf in enumerate(kfs):
        for idx in rng.permutation(len(m.kf_desc[k]))[:130]:
            mp = int(rng.integers(n_points))
            if not m.in_keyframe(mp, k):
                m.add(mp, k, int(idx))
        for _ in range(25):                                      # MapPoints both eyes of the keyframe see (the Frame's own stereo matches)
            mp = int(rng.integers(n_points))
            free_l = [i for i in range(n_left[k]) if m.slots[k][i] < 0]; free_r = [i for i in range(n_left[k], len(m.kf_desc[k])) if m.slots[k][i] < 0]
            if not m.in_keyframe(mp, k):
                m.add(mp, k, int(rng.choice(free_l))); m.add(mp, k, int(rng.choice(free_r)))
    for mp in rng.integers(n_list, n_points, 60):
        m.obs[int(mp)][3 + int(rng.integers(4))] = (0, -1)
    return s, m, mp_list


def sequential(s, m0, mp_list, keyframes):
    """the reference order: per keyframe, the left Fuse with its tail, then the right Fuse with its tail (LocalMapping.cc:787-788)"""
    kw = dict(tlr=s["tlr"], cams=s["cams"], bounds=s["bounds"], tab=s["tab"])
    seq = m0.copy(); counts = []
    for k in keyframes:
        for right in (False, True):
            counts.append(FW.fuse_sequential(seq, k, s["kfs"][k], right, mp_list, s["lists"][0], **kw))
    return seq, counts


def batched(s, m0, mp_list, keyframes, search_again):
    """one search of every (keyframe, eye) on the initial map (a call with eyes = 3), then the replay of INTEGRATION.md: per keyframe the left
    tail, then the right tail; before each, the changed survivors are searched again in that keyframe and eye (search_again)"""
    mps = s["lists"][0]
    kw = dict(tlr=s["tlr"], cams=s["cams"], bounds=s["bounds"], tab=s["tab"])
    uploaded = W.list_descriptors(m0, mp_list)
    results = dict(((k, right), FW.search(s["kfs"][k], right, mps, W.flags_of(m0, k, mp_list), **kw)) for k in keyframes for right in (False, True))
    bat = m0.copy(); counts = []; stale_all = []
    for k in keyframes:
        for right in (False, True):
            again = (lambda fl, descs, k=k, right=right: FW.search(s["kfs"][k], right, dict(mps, desc=descs), fl, **kw)) if search_again else None
            n, stale = FW.replay_tail(bat, k, mp_list, results[(k, right)], uploaded, again)
            counts.append(n); stale_all.append(stale)
    return bat, counts, stale_all, results


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_batched_searches_plus_replay_equal_the_sequential_fuse(seed):
    s, m0, mp_list = licence_scene(seed)
    seq, n_seq = sequential(s, m0, mp_list, [0, 1, 2])
    bat, n_bat, stale, results = batched(s, m0, mp_list, [0, 1, 2], search_again=True)
    assert seq.state() == bat.state() and n_seq == n_bat
    assert sum(n_seq) > 20 and sum(seq.bad) > 5 and min(sum(n_seq[0::2]), sum(n_seq[1::2])) > 5      # both eyes fuse
    assert sum(a != b for a, b in zip(m0.state()[3], seq.state()[3])) > 3 and sum(len(x) for x in stale) > 0
    # observations with both halves exist (Observations() counts them twice) and Replace has moved some of them to their survivor
    both = lambda mm: set((mp, kf) for mp, o in enumerate(mm.obs) for kf, (l, r) in o.items() if l != -1 and r != -1)      # noqa: E731
    assert both(m0) and both(seq) - both(m0)
    # the re-test matters: what the left tail added or replaced is skipped in the right eye, as the reference's second call does
    skipped = 0
    chk = m0.copy()
    kw = dict(tlr=s["tlr"], cams=s["cams"], bounds=s["bounds"], tab=s["tab"])
    for k in range(3):
        for right in (False, True):
            for i, mp in enumerate(mp_list):
                if right and results[(k, right)]["exit"][i] == W.EXIT_FUSED and mp >= 0 and (chk.bad[mp] or chk.in_keyframe(mp, k)):
                    skipped += 1
            FW.replay_tail(chk, k, mp_list, results[(k, right)], W.list_descriptors(m0, mp_list),
                           lambda fl, descs, k=k, right=right: FW.search(s["kfs"][k], right, dict(s["lists"][0], desc=descs), fl, **kw))
    assert skipped > 0 and chk.state() == seq.state()


def test_replay_without_searching_the_changed_survivors_again_is_not_the_reference():
    departed = 0
    for seed in (11, 12, 13):
        s, m0, mp_list = licence_scene(seed)
        seq, _ = sequential(s, m0, mp_list, [0, 1, 2])
        naive = batched(s, m0, mp_list, [0, 1, 2], search_again=False)[0]
        departed += naive.state() != seq.state()
    assert departed == 3


@pytest.mark.parametrize("k", [0, 1, 2])
def test_one_keyframe_call_plus_replay_is_the_reference_without_searching_again(k):
    """n_pairs = 1 with eyes = 3: both survivors of a Replace in the left eye are in the keyframe afterwards, so the right search reads no
    descriptor the left tail rewrote"""
    s, m0, mp_list = licence_scene(14)
    seq, n_seq = sequential(s, m0, mp_list, [k])
    bat, n_bat, _, _ = batched(s, m0, mp_list, [k], search_again=False)
    assert bat.state() == seq.state() and n_seq == n_bat and sum(n_seq) > 5 and len(seq.recomputed) > 0


# ---------------------------------------------------------------- (f) the kernel's own source, on the host ----------------------------------------------------------------
HOST_FLAGS = ["-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"), "-I" + os.path.join(ROOT, "extractorb_amd", "csrc"),
              "-I" + os.path.join(ROOT, "include")]
HOST_SOURCES = [os.path.join(ROOT, "tests", "cpp", "fuse_two_eyes_host_check.cpp"), os.path.join(ROOT, "extractorb_amd", "csrc", "orbx_predict_scale.cpp")]


class HostParams(C.Structure):      # == FuseTwoEyesParams of extractorb_amd/csrc/orbx_params.hpp
    _fields_ = ([("cam", C.c_float * 16)] + [(n, C.c_float) for n in "minX maxX minY maxY wInv hInv".split()] +
                [("scale", C.c_float * 16), ("invSigma2", C.c_float * 16), ("breaks", C.c_float * 16), ("tlr", C.c_float * 12), ("th", C.c_float)] +
                [(n, C.c_int) for n in "nlevels thLow reprojCheck eyes capacity mpCapacity kfFirst kfStep mpFirst mpStep".split()])


def pack(scene, cap, mp_cap):
    """the batch as the entry takes it: device frame 2r = the left eye of rig r, 2r + 1 its right eye; list l = MapPoint list l"""
    kfs, lists = scene["kfs"], scene["lists"]
    B, NL = 2 * len(kfs), len(lists)
    kps = np.zeros((B, cap), X.KEYPOINT_DTYPE); desc = np.zeros((B, cap, 32), np.uint8)
    nout = np.zeros(B, np.int32); off = np.zeros((B, 64 * 48 + 1), np.int32); idx = np.zeros((B, cap), np.int32); poses = np.zeros((len(kfs), 12), f32)
    for r, k in enumerate(kfs):
        poses[r] = k["pose"].reshape(12)
        for e, eye in enumerate(k["eyes"]):
            f = 2 * r + e; n = len(eye["kps"])
            kps[f, :n] = eye["kps"]; desc[f, :n] = eye["desc"]; nout[f] = n; off[f] = eye["grid_off"]; idx[f, :len(eye["grid_idx"])] = eye["grid_idx"]
    world = np.zeros((NL, mp_cap, 3), f32); normal = np.zeros((NL, mp_cap, 3), f32); dist = np.zeros((NL, mp_cap, 3), f32)
    mdesc = np.zeros((NL, mp_cap, 32), np.uint8)
    for l, m in enumerate(lists):
        n = len(m["world"])
        world[l, :n] = m["world"]; normal[l, :n] = m["normal"]; dist[l, :n] = m["dist"]; mdesc[l, :n] = m["desc"]
    return dict(kps=kps, desc=desc, nout=nout, off=off, idx=idx, poses=poses, world=world, normal=normal, dist=dist, mdesc=mdesc)


@pytest.fixture(scope="module")
def host_kernel(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("fuse_two_eyes") / "libfuse_two_eyes_host.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", *HOST_FLAGS, *HOST_SOURCES, "-o", so])
    L = C.CDLL(so)
    assert L.fuse_two_eyes_host_params_size() == C.sizeof(HostParams)
    return L


def test_kernel_source_compiled_for_the_host_equals_the_walk(host_kernel):
    """k_fuse_two_eyes.hip itself (not a restatement), built with g++ behind tests/cpp/host_shim and run one thread at a time, on every scene
    of the GPU tests: eyes = 3 in both modes... the loop-closing mode with eyes = 1, eyes = 2 alone, the edge scenes under the early returns"""
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    compared = 0
    for name in SCENES:
        s = get(name); tab = s["tab"]; kfs, lists = s["kfs"], s["lists"]
        cap = max(len(e["kps"]) for k in kfs for e in k["eyes"]) + 3; mp_cap = len(lists[0]["world"])
        a = pack(s, cap, mp_cap)
        pairs = cases(name)
        fl = np.stack([flags_for(s, k, mp_cap) for k, _ in pairs])
        runs = [(dict(), 3), (dict(reproj_check=False), 1), (dict(), 2)] + ([(RETURNS, 3)] if name.startswith("edge") else [])
        runs += [(dict(th=4.0), 1)] if name in ("small", "small_frac", "edge") else []
        for opt, eyes in runs:
            p = HostParams()
            for e in (0, 1):
                for c in range(8):
                    p.cam[8 * e + c] = float(s["cams"][e][c])
            p.minX, p.maxX, p.minY, p.maxY = (float(int(b)) for b in s["bounds"])      # as the entry fills them: truncated
            p.wInv = f32(64) / (s["bounds"][1] - s["bounds"][0]); p.hInv = f32(48) / (s["bounds"][3] - s["bounds"][2])
            for i in range(tab["nlevels"]):
                p.scale[i] = tab["scale"][i]; p.invSigma2[i] = tab["inv_sigma2"][i]
            for i, b in enumerate(X.predict_scale_breakpoints(*s["setting"])):
                p.breaks[i] = b
            for i, v in enumerate(np.asarray(s["tlr"], f32).reshape(12)):
                p.tlr[i] = v                                                               # (negative zeros travel as they are)
            p.th = opt.get("th", 3.0); p.nlevels = tab["nlevels"]; p.thLow = 50; p.reprojCheck = int(opt.get("reproj_check", True)); p.eyes = eyes
            p.capacity = cap; p.mpCapacity = mp_cap; p.kfFirst = 0; p.kfStep = 1; p.mpFirst = 0; p.mpStep = 1 if len(lists) > 1 else 0
            n = len(pairs)
            bi = np.full((n, 2, mp_cap), -7, np.int32); bd = bi.copy(); ex = np.full((n, 2, mp_cap), 99, np.uint8); nf = np.zeros((n, 2), np.int32)
            host_kernel.fuse_two_eyes_host(ptr(a["world"]), ptr(a["normal"]), ptr(a["dist"]), ptr(a["mdesc"]), None, ptr(fl), ptr(a["poses"]), ptr(a["kps"]),
                                           ptr(a["desc"]), ptr(a["nout"]), ptr(a["off"]), ptr(a["idx"]), C.byref(p), ptr(bi), ptr(bd), ptr(ex), ptr(nf), n)
            for q, (k, l) in enumerate(pairs):
                for e in (0, 1):
                    if not (eyes >> e) & 1:
                        assert (bi[q, e] == -7).all() and (bd[q, e] == -7).all() and (ex[q, e] == 99).all()      # an eye not asked for is untouched
                        continue
                    want = walk(name, k, l, bool(e), **opt)
                    assert np.array_equal(bi[q, e], want["best_idx"]) and np.array_equal(bd[q, e], want["best_dist"]) and np.array_equal(ex[q, e], want["exit"]), (name, opt, eyes, q, e)
                    compared += len(want["exit"])
    assert compared > 40000


def test_rig_invariants_of_the_kernel_equal_the_walks_getters(host_kernel):
    """the thirty floats the kernel's thirty lanes compute, bit for bit - negative zeros included"""
    cases_ = [(EDGE_POSE, EDGE_TLR)] + [(k["pose"], get("real")["tlr"]) for k in get("real")["kfs"]]
    for pose, tlr in cases_:
        out = np.zeros(30, f32)
        pose = np.ascontiguousarray(pose, f32); tlr = np.ascontiguousarray(tlr, f32)
        host_kernel.fuse_two_eyes_rig(pose.ctypes.data_as(C.c_void_p), tlr.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        want = np.concatenate([np.concatenate([R.reshape(9), t, O]) for R, t, O in FW.keyframe_rig(pose, tlr)]).astype(f32)
        assert out.tobytes() == want.tobytes()


def test_the_entrys_predicate_on_eyes(host_kernel):
    for eyes in range(-2, 7):
        for rc in (0, 1):
            assert host_kernel.fuse_two_eyes_bad_eyes(eyes, rc) == int(eyes not in (1, 2, 3) or (rc == 0 and eyes != 1)), (eyes, rc)


def test_kernel_source_stays_inside_its_arrays_as_a_sanitized_host_program(tmp_path):
    """the same source as a stand-alone program under AddressSanitizer + UBSan: exact-size buffers, valid and corrupt grids, every `eyes`"""
    exe = str(tmp_path / "fuse_two_eyes_host_check")
    subprocess.check_call(["g++", "-O1", "-g", "-DFUSE_TWO_EYES_HOST_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *HOST_FLAGS, *HOST_SOURCES,
                           "-o", exe])
    out = subprocess.check_output([exe], text=True)
    assert out.count("trial") == 8 and out.strip().endswith("clean")


# ---------------------------------------------------------------- (g) the surface ----------------------------------------------------------------
def test_entry_is_declared_documented_and_exported():
    assert "orbx_fuse_two_eyes_device" in X.header_symbols() and hasattr(X.load_library(), "orbx_fuse_two_eyes_device")
    text = open(X.orbextractor._HEADER).read()
    pos = text.index("int orbx_fuse_two_eyes_device(")
    doc = text[text.rindex("/*", 0, pos):pos]
    for word in ("1399-1609", "1611-1733", "1232-1262", "mTlr ALONE", "2r + 1", "NLeft + i", "RAW", "5.99", "eyes", "left untouched", "Nright > Nleft",
                 "atan2f(r, 0)", "no capacity bound"):
        assert word in doc, word
    older = text[text.rindex("/*", 0, text.index("int orbx_fuse_device(")):text.index("int orbx_fuse_device(")]
    assert "orbx_fuse_two_eyes_device" in older and "NOT covered" in older
    z = C.c_void_p(16)      # never dereferenced: the handle is checked first
    assert X.load_library().orbx_fuse_two_eyes_device(None, 1, 0, 1, 0, 0, z, z, z, z, z, 16, z, z, z, z, z, z, z, z, 16, z, z, z, 8, 3.0, 50, 1, 3, z, z, z, z) == -2
    assert callable(getattr(X.ORBextractor, "fuse_two_eyes_device", None))
    assert X.load_library().orbx_abi_version() == 1
