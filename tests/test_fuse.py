"""ORBmatcher::Fuse, the search half (reference src/ORBmatcher.cc:1399-1609 and the Sim3 overload :1611-1733; orbx_fuse_device) - the CPU side.
(a) the sequential walk (tests/fuse_walk.py) against an independent per-MapPoint numpy statement: masks for the exits, brute force over all
    in-grid keypoints, argmin of (distance, CSR position), the level from the LIBRARY's breakpoint table - on every scene the GPU tests use;
(b) the batching licence: the reference's sequence (Fuse keyframe after keyframe, every tail changing the map, Replace recomputing the survivor's
    descriptor) against all searches on the initial state + the replay with re-tests and with the changed survivors searched again, on a tiny
    map model with descriptors; the replay WITHOUT searching again is shown to end elsewhere;
(c) the scenes reach every exit, every candidate filter, a tie and the planted edge cases;
(d) orbx_predict_scale_breakpoints against orbx_predict_scale, and the stand-alone sweep over every float (tests/cpp/predict_scale_sweep.cpp);
(e) k_fuse.hip's own source compiled for the host (tests/cpp/host_shim) against the walk on every scene, and under ASan + UBSan on corrupt grids.
The GPU tests are in tests/test_fuse_gpu.py and use the scenes and walks of this module."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import extractorb_amd as X
import fuse_walk as W
from fuse_walk import f32, f64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = [(1.2, 8), (1.1, 12), (2.0, 4)]
BOUNDS = np.array([0, 640, 0, 480], f32)
FRAC_BOUNDS = np.array([-3.75, 643.5, -2.25, 482.5], f32)      # a distorted camera's: KeyFrame truncates them to -3, 643, -2, 482
CAM = np.array([512, 512, 256, 192], f32)          # powers of two: the edge scenes plant exact projections
CAM_REAL = np.array([458.654, 457.296, 317.215, 238.375], f32)
MBF = f32(47.9)


def rot(ax, ay):
    cx, sx, cy, sy = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
    return (np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]))


def keyframe(rng, n, tab, cam, pose, stereo=True, bounds=BOUNDS):
    kps = np.zeros(n, X.KEYPOINT_DTYPE)
    kps["x"] = rng.uniform(bounds[0] + 2, bounds[1] - 2, n).astype(f32); kps["y"] = rng.uniform(bounds[2] + 2, bounds[3] - 2, n).astype(f32)
    kps["octave"] = np.minimum(rng.geometric(0.35, n) - 1, tab["nlevels"] - 1)
    depth = rng.uniform(2, 9, n).astype(f32)
    ur = np.where(rng.random(n) < 0.65, kps["x"] - MBF / depth, -1).astype(f32) if stereo else None
    off, idx, _ = W.build_grid(kps, bounds)
    return dict(pose=pose.astype(f32), kps=kps, ur=ur, desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), grid_off=off, grid_idx=idx, depth=depth)


def points_for(rng, kf, m, tab, cam):
    """MapPoints for one keyframe: half of them sit on its keypoints (noise, flipped descriptor bits, a level of their own), the others are
    anywhere - in front, behind, beside, too far, turned away"""
    n = len(kf["kps"]); sc = tab["scale"]
    R = kf["pose"][:, :3].astype(f64); t = kf["pose"][:, 3].astype(f64)
    Ow = -R.T @ t
    world = np.zeros((m, 3), f32); normal = np.zeros((m, 3), f32); dist = np.zeros((m, 3), f32); desc = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    for i in range(m):
        kind = rng.random()
        if kind < 0.55:
            j = rng.integers(n); o = int(kf["kps"]["octave"][j]); z = float(kf["depth"][j])
            px = kf["kps"]["x"][j] + rng.normal(0, 0.9) * sc[o]; py = kf["kps"]["y"][j] + rng.normal(0, 0.9) * sc[o]
            xc = np.array([(px - cam[2]) / cam[0] * z, (py - cam[3]) / cam[1] * z, z])
            desc[i] = kf["desc"][j]
            for b in rng.integers(0, 256, rng.choice([0, 3, 20, 45, 50, 51, 70])):
                desc[i, b >> 3] ^= 1 << (b & 7)
            lv = min(max(o + rng.choice([0, 0, 0, 1, -1]), 0), tab["nlevels"] - 1)
        else:
            z = rng.uniform(-3, 12) if kind < 0.75 else rng.uniform(1, 9)
            xc = np.array([rng.uniform(-0.9, 0.9) * abs(z), rng.uniform(-0.7, 0.7) * abs(z), z]); lv = rng.integers(tab["nlevels"])
        p = R.T @ (xc - t)
        world[i] = p
        d = np.linalg.norm(p - Ow)
        mf_max = d * sc[lv] * rng.uniform(0.93, 0.999)
        dist[i] = (0.8 * mf_max / sc[-1], 1.2 * mf_max, mf_max)
        if rng.random() < 0.08:
            dist[i, :2] = (dist[i, 1] * 1.05, dist[i, 1] * 1.3) if rng.random() < 0.5 else (dist[i, 0] * 0.2, dist[i, 0] * 0.9)
        nv = (p - Ow) / max(d, 1e-9)
        nv = rot(rng.normal(0, 0.25), rng.normal(0, 0.25)) @ nv if rng.random() < 0.8 else rot(rng.uniform(1.0, 2.0), 0.3) @ nv
        normal[i] = nv
    return dict(world=world, normal=normal, dist=dist, desc=desc)


def random_scene(seed, n_kp, n_mp, n_kf, setting=(1.2, 8), stereo=True, lists=1, cam=CAM_REAL, bounds=BOUNDS):
    """n_kf keyframes around one place; `lists` MapPoint lists, each built on the keyframes in turn so that every keyframe finds some"""
    rng = np.random.default_rng(seed)
    tab = W.tables(*setting)
    kfs = []
    for k in range(n_kf):
        pose = np.concatenate([rot(rng.normal(0, 0.03), rng.normal(0, 0.03)), rng.normal(0, 0.15, (3, 1))], axis=1)
        kfs.append(keyframe(rng, n_kp - 7 * k, tab, cam, pose, stereo, bounds))
    mp_lists = []
    for l in range(lists):
        parts = [points_for(rng, kfs[(l + q) % n_kf], n_mp // n_kf + (q < n_mp % n_kf), tab, cam) for q in range(n_kf)]
        mps = dict((key, np.concatenate([p[key] for p in parts])) for key in parts[0])
        perm = rng.permutation(n_mp)
        mp_lists.append(dict((key, v[perm]) for key, v in mps.items()))
    return dict(tab=tab, setting=setting, cam=cam, bounds=bounds, mbf=MBF, kfs=kfs, lists=mp_lists, seed=seed)


def flags_for(scene, pair, n):
    """bit 0 per (pair, MapPoint); the edge scenes search every probe"""
    return (np.random.default_rng(scene["seed"] * 131 + pair).random(n) < scene.get("flag_density", 0.85)).astype(np.uint8)


# ---------------------------------------------------------------- the edge scene ----------------------------------------------------------------
def at(u, v, z=4.0):
    """a world point (identity pose) whose projection under CAM is exactly (u, v) for u, v with few fraction bits"""
    return np.array([(u - 256.0) / 512.0 * z, (v - 192.0) / 512.0 * z, z], f32)


def projection(p):
    return CAM[0] * p[0] / p[2] + CAM[2], CAM[1] * p[1] / p[2] + CAM[3]


def dist3d_of(p):
    return f32(np.sqrt((f64(p[0]) * f64(p[0]) + f64(p[1]) * f64(p[1])) + f64(p[2]) * f64(p[2])))


def plant_ratio(d, target):
    """mfMaxDistance with fl(mfMaxDistance / d) == target exactly, or None (the caller then moves the probe)"""
    lo = hi = f32(f32(target) * d)
    for _ in range(8):
        for c in (lo, hi):
            if f32(c) / d == f32(target):
                return f32(c)
        lo = np.nextafter(lo, f32(-np.inf)); hi = np.nextafter(hi, f32(np.inf))
    return None


def edge_scene(setting=(1.2, 8)):
    """identity pose, one keyframe; every MapPoint is a named probe.  Returns the scene and {name: MapPoint index}"""
    tab = W.tables(*setting); sc = tab["scale"]; L = tab["nlevels"]
    bp = X.predict_scale_breakpoints(*setting)
    rng = np.random.default_rng(5)
    kp, mp, names = [], [], {}

    def add_kp(x, y, octave, ur=-1.0, desc=None):
        kp.append((f32(x), f32(y), int(octave), f32(ur), rng.integers(0, 256, 32, dtype=np.uint8) if desc is None else desc))
        return len(kp) - 1

    def add_mp(name, p, desc, ratio=1.0, normal=None, dist=None, mf_max=None):
        p = np.asarray(p, f32); d = dist3d_of(p)
        mf = f32(ratio) * d if mf_max is None else mf_max
        lo, hi = (f32(0.0), f32(1e9)) if dist is None else dist
        nv = p / max(float(d), 1e-9) if normal is None else normal
        names[name] = len(mp); mp.append((p, np.asarray(nv, f32), (lo, hi, mf), desc))

    rnd = lambda: rng.integers(0, 256, 32, dtype=np.uint8)      # noqa: E731
    # image bounds: u exactly mnMinX is kept, exactly mnMaxX is dropped (strict); the same for v
    d0 = rnd(); add_kp(0.0, 100.0, 0, desc=d0); add_mp("u_is_min_x", at(0.0, 100.0), d0)
    add_mp("u_is_max_x", at(640.0, 100.0), rnd())
    d0 = rnd(); add_kp(100.0, 0.0, 0, desc=d0); add_mp("v_is_min_y", at(100.0, 0.0), d0)
    add_mp("v_is_max_y", at(100.0, 480.0), rnd())
    add_mp("z_is_zero", np.array([0.5, 0.5, 0.0], f32), rnd())
    add_mp("z_is_zero_on_axis", np.array([0.0, 0.0, 0.0], f32), rnd())
    add_mp("z_negative", at(300.0, 200.0, -4.0), rnd())
    # windows leaving the grid on each side (cells are 10 x 10 px; radius 3 at level 0)
    for name, (u, v) in dict(left=(1.0, 240.0), right=(636.0, 240.0), top=(320.0, 1.0), bottom=(320.0, 476.0)).items():
        # (a keypoint right of x = 635 or below y = 475 rounds to cell 64 / 48 and is in no cell: PosInGrid, src/Frame.cc:726-736)
        d0 = rnd(); add_kp(u + (0.5 if u < 320 else -1.5), v + (0.5 if v < 240 else -1.5), 0, desc=d0); add_mp("window_" + name, at(u, v), d0)
    # the four early returns of GetFeaturesInArea need a negative radius (th = -300 at level 0): see RETURNS
    for name, (u, v) in dict(min_x=(500.0, 240.0), max_x=(100.0, 240.0), min_y=(300.0, 200.0), max_y=(300.0, 100.0)).items():
        add_mp("return_" + name, at(u, v), rnd())
    # dist3D equal to each bound (kept) and one ulp inside it (dropped)
    p = at(200.0, 300.0); d = dist3d_of(p); up, dn = np.nextafter(d, f32(np.inf)), np.nextafter(d, f32(0))
    d0 = rnd(); add_kp(200.0, 300.0, 0, desc=d0)
    add_mp("dist_is_min", p, d0, dist=(d, f32(1e9))); add_mp("dist_is_max", p, d0, dist=(f32(0), d))
    add_mp("dist_below_min", p, d0, dist=(up, f32(1e9))); add_mp("dist_above_max", p, d0, dist=(f32(0), dn))
    # the normal: exactly 60 degrees is kept (dot == 0.5 * dist3D is not <), more is dropped
    p = np.array([0.0, 0.0, 4.0], f32)
    d0 = rnd(); add_kp(256.0, 192.0, 0, desc=d0)
    add_mp("normal_at_half", p, d0, normal=(0.0, np.sqrt(0.75), 0.5)); add_mp("normal_below_half", p, d0, normal=(0.0, 0.9, np.nextafter(f32(0.5), f32(0))))
    # every breakpoint and the float just below it: a keypoint of octave k under the probe is inside [level - 1, level] only at level >= k
    u, v = 30.0, 330.0
    for k in range(1, L):
        for below in (False, True):
            target = np.nextafter(bp[k - 1], f32(0)) if below else bp[k - 1]
            while True:
                p = at(u, v); mf = plant_ratio(dist3d_of(p), target)
                if mf is not None:
                    break
                u += 0.5
            d0 = rnd(); add_kp(u, v, k, desc=d0)
            add_mp("ratio_%s_break_%d" % ("below" if below else "on", k), p, d0, mf_max=mf)
            u += 28.0                                # farther apart than two radii of the top level
            if u > 600.0:
                u, v = 30.0, v + 28.0
    # ratios where the reference is undefined: +inf (dist3D = 0 is not reachable in front of a camera at the origin: mfMaxDistance = inf) and NaN
    d0 = rnd(); add_kp(400.0, 60.0, L - 1, desc=d0); add_mp("ratio_inf", at(400.0, 60.0), d0, mf_max=f32(np.inf))
    d0 = rnd(); add_kp(500.0, 60.0, 0, desc=d0); add_mp("ratio_nan", at(500.0, 60.0), d0, mf_max=f32(np.nan))
    # candidates: the level filter, the two chi-square gates, a tie decided by visit order (the later INDEX sits in the earlier CELL)
    d0 = rnd(); add_kp(60.0, 60.0, 3, desc=d0); add_mp("level_filtered", at(60.0, 60.0), d0)
    d0 = rnd(); add_kp(122.5, 60.0, 0, desc=d0); add_mp("mono_gate_rejects", at(120.0, 60.0), d0)           # 2.5^2 = 6.25 > 5.99
    d0 = rnd(); add_kp(182.0, 60.0, 0, desc=d0); add_mp("mono_gate_passes", at(180.0, 60.0), d0)            # 4 <= 5.99
    z = 4.0; ur_true = 240.0 - float(MBF) / z
    d0 = rnd(); add_kp(242.0, 60.0, 0, ur=ur_true + 2.0, desc=d0); add_mp("stereo_gate_rejects", at(240.0, 60.0), d0)      # 4 + 0 + ~4 > 7.8
    d0 = rnd(); add_kp(301.5, 60.0, 0, ur=300.0 - float(MBF) / z + 1.5, desc=d0); add_mp("stereo_gate_passes", at(300.0, 60.0), d0)
    d0 = rnd()
    first = add_kp(64.0, 145.5, 0, desc=d0)          # cell (6, 15): visited second
    second = add_kp(64.0, 143.5, 0, desc=d0)         # cell (6, 14): visited first, although its index is larger
    add_mp("tie_by_visit_order", at(64.0, 144.5), d0)
    d1 = d0.copy(); d1[0] ^= 1
    add_kp(66.0, 144.5, 0, desc=d1)                  # cell (7, 14): a worse distance later changes nothing
    # th_low: distance 50 fuses, 51 does not
    for name, bits in (("dist_50", 50), ("dist_51", 51)):
        d0 = rnd(); dm = d0.copy()
        for b in range(bits):
            dm[b >> 3] ^= 1 << (b & 7)
        x = 450.0 if bits == 50 else 520.0
        add_kp(x, 200.0, 0, desc=d0); add_mp(name, at(x, 200.0), dm)
    kps = np.zeros(len(kp), X.KEYPOINT_DTYPE)
    kps["x"] = [k[0] for k in kp]; kps["y"] = [k[1] for k in kp]; kps["octave"] = [k[2] for k in kp]
    off, idx, _ = W.build_grid(kps, BOUNDS)
    kf = dict(pose=np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(f32), kps=kps, ur=np.array([k[3] for k in kp], f32),
              desc=np.stack([k[4] for k in kp]), grid_off=off, grid_idx=idx)
    mps = dict(world=np.stack([m[0] for m in mp]), normal=np.stack([m[1] for m in mp]), dist=np.array([m[2] for m in mp], f32),
               desc=np.stack([m[3] for m in mp]))
    scene = dict(tab=tab, setting=setting, cam=CAM, bounds=BOUNDS, mbf=MBF, kfs=[kf], lists=[mps], seed=5, twins=(first, second), flag_density=1.0)
    return scene, names


def frac_edge_scene():
    """non-integer image bounds (FRAC_BOUNDS): KeyFrame::IsInImage compares with the TRUNCATED bounds (-3, 643, -2, 482), so a projection between
    a float bound and its truncation is outside although Frame's own bounds hold it.  Every "between" probe has a keypoint with its descriptor
    under it: with the float bounds it would fuse.  (Near the right and lower edge no keypoint is in a grid cell - PosInGrid rounds it to cell
    64 / 48 - so the probes kept there end as empty windows.)"""
    tab = W.tables(); rng = np.random.default_rng(15)
    kp, mp, names = [], [], {}

    def probe(name, u, v, with_kp=True):
        d0 = rng.integers(0, 256, 32, dtype=np.uint8)
        if with_kp:
            kp.append((f32(u), f32(v), d0))
        p = at(u, v); d = dist3d_of(p)
        names[name] = len(mp); mp.append((p, p / d, (f32(0), f32(1e9), d), d0))

    probe("u_is_truncated_min", -3.0, 100.0); probe("u_between_float_and_truncated_min", -3.5, 130.0); probe("u_is_float_min", -3.75, 160.0)
    probe("v_is_truncated_min", 100.0, -2.0); probe("v_between_float_and_truncated_min", 130.0, -2.125); probe("v_is_float_min", 160.0, -2.25)
    probe("u_below_truncated_max", 642.75, 100.0, False); probe("u_is_truncated_max", 643.0, 130.0, False)
    probe("u_between_truncated_and_float_max", 643.25, 160.0, False)
    probe("v_below_truncated_max", 100.0, 481.75, False); probe("v_is_truncated_max", 130.0, 482.0, False)
    probe("v_between_truncated_and_float_max", 160.0, 482.25, False)
    probe("inside", 300.0, 200.0)
    kps = np.zeros(len(kp), X.KEYPOINT_DTYPE)
    kps["x"] = [k[0] for k in kp]; kps["y"] = [k[1] for k in kp]
    off, idx, cell = W.build_grid(kps, FRAC_BOUNDS)
    assert (cell >= 0).all()
    kf = dict(pose=np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(f32), kps=kps, ur=np.full(len(kp), -1, f32),
              desc=np.stack([k[2] for k in kp]), grid_off=off, grid_idx=idx)
    mps = dict(world=np.stack([m[0] for m in mp]), normal=np.stack([m[1] for m in mp]).astype(f32), dist=np.array([m[2] for m in mp], f32),
               desc=np.stack([m[3] for m in mp]))
    return dict(tab=tab, setting=(1.2, 8), cam=CAM, bounds=FRAC_BOUNDS, mbf=MBF, kfs=[kf], lists=[mps], seed=15, flag_density=1.0), names


RETURNS = dict(th=-300.0)          # the option set under which the early returns are reached

_scenes = {}


def get(name):
    """the scenes of the CPU and the GPU tests, built once"""
    if name not in _scenes:
        _scenes[name] = dict(
            small=lambda: random_scene(1, 96, 150, 3),                            # capacity 96 x 150 MapPoints x 3 keyframes, one list
            small_lists=lambda: random_scene(2, 96, 150, 3, lists=3),             # one list per keyframe
            small_mono=lambda: random_scene(3, 96, 150, 3, stereo=False),
            small_12=lambda: random_scene(4, 96, 150, 3, setting=(1.1, 12)),
            real=lambda: random_scene(6, 1200, 1000, 4),                          # capacity 1302, 1000 MapPoints x 4 keyframes
            long=lambda: random_scene(7, 1200, 5000, 1),                          # one long list into one keyframe
            edge=lambda: edge_scene()[0],
            edge_12=lambda: edge_scene((1.1, 12))[0],
            small_frac=lambda: random_scene(8, 96, 150, 3, bounds=FRAC_BOUNDS),  # non-integer image bounds
            edge_frac=lambda: frac_edge_scene()[0],
        )[name]()
    return _scenes[name]


SCENES = ("small", "small_lists", "small_mono", "small_12", "real", "long", "edge", "edge_12", "small_frac", "edge_frac")
_walks = {}


def walk(name, kf, lst, reproj_check=True, th=3.0, th_low=50, n_mp=None, use_u_right=True):
    """the walk of list `lst` into keyframe `kf` of a scene under the flags flags_for(scene, kf) - shared by all tests, never changed"""
    key = (name, kf, lst, reproj_check, th, th_low, n_mp, use_u_right)
    if key not in _walks:
        s = get(name)
        stats = {}
        k = s["kfs"][kf] if use_u_right else dict(s["kfs"][kf], ur=None)
        mps = s["lists"][lst]
        r = W.search(k, mps, flags_for(s, kf, len(mps["world"])), s["cam"], s["bounds"], s["mbf"], s["tab"], th=th, th_low=th_low,
                     reproj_check=reproj_check, n_mp=n_mp, stats=stats)
        r["stats"] = stats
        _walks[key] = r
    return _walks[key]


def cases(name):
    """(keyframe, list) pairs a scene is searched as"""
    s = get(name)
    return [(k, k % len(s["lists"])) for k in range(len(s["kfs"]))]


# ---------------------------------------------------------------- (a) the independent statement ----------------------------------------------------------------
def statement(s, kf, mps, flags, reproj_check=True, th=3.0, th_low=50):
    """per MapPoint, no walk: vector arithmetic for the front end, masks for the exits, brute force over the in-grid keypoints, the level
    from the library's breakpoint table (the walk uses the expression)"""
    tab, cam = s["tab"], s["cam"]
    fb = np.asarray(s["bounds"], f32)
    w_inv = f32(64) / (fb[1] - fb[0]); h_inv = f32(48) / (fb[3] - fb[2])      # Frame's inverses, from the float bounds
    minx, maxx, miny, maxy = (f32(int(b)) for b in fb)                        # KeyFrame's const int bounds
    bp = X.predict_scale_breakpoints(*s["setting"])
    P = kf["pose"].astype(f32); M = len(mps["world"])
    w = mps["world"].astype(f32)
    with np.errstate(all="ignore"):
        pc = [(((P[r, 0].astype(f64) * w[:, 0].astype(f64) + P[r, 1].astype(f64) * w[:, 1].astype(f64)) + P[r, 2].astype(f64) * w[:, 2].astype(f64)) * 1.0 +
               P[r, 3].astype(f64)).astype(f32) for r in range(3)]
        Ow = np.array([f32(((f64(P[0, r]) * f64(P[0, 3]) + f64(P[1, r]) * f64(P[1, 3])) + f64(P[2, r]) * f64(P[2, 3])) * -1.0) for r in range(3)], f32)
        invz = f32(1) / pc[2]
        u = cam[0] * pc[0] / pc[2] + cam[2]; v = cam[1] * pc[1] / pc[2] + cam[3]
        ur = u - f32(s["mbf"]) * invz
        PO = w - Ow[None, :]
        PO64 = PO.astype(f64)
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
        leave(pc[2] < 0, W.EXIT_NEG_DEPTH)
        leave(~((u >= minx) & (u < maxx) & (v >= miny) & (v < maxy)), W.EXIT_NOT_IN_IMAGE)
        leave((d3 < mps["dist"][:, 0]) | (d3 > mps["dist"][:, 1]), W.EXIT_DISTANCE)
        leave(dot < 0.5 * d3.astype(f64), W.EXIT_NORMAL)
        kps = kf["kps"]
        _, order, cell = W.build_grid(kps, s["bounds"])
        pos = np.full(len(kps), 1 << 30, np.int64); pos[order] = np.arange(len(order))
        kx, ky, ko = kps["x"].astype(f32), kps["y"].astype(f32), kps["octave"].astype(np.int64)
        kr = np.full(len(kps), -1, f32) if kf["ur"] is None else kf["ur"].astype(f32)
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
                ex = u[i] - kx; ey = v[i] - ky; er = ur[i] - kr
                stereo = kr >= 0
                e2 = np.where(stereo, ex * ex + ey * ey + er * er, ex * ex + ey * ey)
                ok &= ~((e2 * inv).astype(f64) > np.where(stereo, 7.8, 5.99))
            if ok.any():
                j = np.nonzero(ok)[0]
                dist = W.POPCOUNT[kf["desc"][j] ^ mps["desc"][i][None, :]].sum(axis=1)
                b = j[np.lexsort((pos[j], dist))[0]]
                best_dist[i] = int(W.POPCOUNT[kf["desc"][b] ^ mps["desc"][i]].sum())
                if best_dist[i] <= th_low:
                    best_idx[i] = b
            code[i] = W.EXIT_FUSED if best_idx[i] >= 0 else W.EXIT_ABOVE_TH_LOW
    return dict(best_idx=best_idx, best_dist=best_dist, exit=code.astype(np.uint8), n_fused=int((code == W.EXIT_FUSED).sum()))


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("best_idx", "best_dist", "exit")) and a["n_fused"] == b["n_fused"]


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("reproj_check", [True, False])
def test_walk_equals_the_independent_statement(name, reproj_check):
    s = get(name)
    for kf, lst in cases(name):
        mps = s["lists"][lst]
        want = statement(s, s["kfs"][kf], mps, flags_for(s, kf, len(mps["world"])), reproj_check)
        got = walk(name, kf, lst, reproj_check)
        bad = np.nonzero((want["best_idx"] != got["best_idx"]) | (want["best_dist"] != got["best_dist"]) | (want["exit"] != got["exit"]))[0]
        assert same(want, got), (name, kf, bad[:5], want["exit"][bad[:5]], got["exit"][bad[:5]])


def test_walk_equals_the_statement_without_u_right_and_under_the_early_returns():
    s = get("small")
    mps = s["lists"][0]
    assert same(statement(s, dict(s["kfs"][1], ur=None), mps, flags_for(s, 1, 150)), walk("small", 1, 0, use_u_right=False))
    s = get("edge")
    mps = s["lists"][0]
    assert same(statement(s, s["kfs"][0], mps, flags_for(s, 0, len(mps["world"])), th=RETURNS["th"]), walk("edge", 0, 0, **RETURNS))


def test_walk_tables_are_the_librarys():
    for sf, nl in SETTINGS:
        t = X.compute_tables(1000, sf, nl); w = W.tables(sf, nl)
        assert np.array_equal(t["scale_factors"], w["scale"]) and np.array_equal(t["inv_level_sigma2"], w["inv_sigma2"])


# ---------------------------------------------------------------- (c) reach ----------------------------------------------------------------
def test_scenes_reach_every_exit_and_every_candidate_filter():
    for name in ("small", "small_lists", "small_12", "real", "long"):
        for rc in (True, False):
            seen = set()
            stats = {}
            for kf, lst in cases(name):
                r = walk(name, kf, lst, rc)
                seen |= set(r["exit"].tolist())
                for k, v in r["stats"].items():
                    stats[k] = stats.get(k, 0) + v
            assert seen == set(range(8)), (name, rc, seen)
            need = ["level_filter", "pass_7_8", "pass_5_99"] if rc else ["level_filter"]      # (the small scenes' gates REJECT in the edge scenes' probes)
            if name in ("real", "long"):
                need += ["window_past_left", "window_past_right", "window_past_top", "window_past_bottom"]
                need += ["reject_7_8", "reject_5_99"] if rc else []
            assert not [k for k in need if not stats.get(k, 0)], (name, rc, stats)
    r = walk("small_mono", 0, 0)
    assert r["stats"].get("reject_5_99", 0) > 0 and "reject_7_8" not in r["stats"] and "pass_7_8" not in r["stats"]
    assert walk("real", 0, 0)["n_fused"] > 50 and walk("long", 0, 0)["n_fused"] > 200


@pytest.mark.parametrize("name", ["edge", "edge_12"])
def test_edge_scene_probes_end_where_they_were_planted(name):
    setting = get(name)["setting"]
    s, at_ = edge_scene(setting)
    L = setting[1]
    n = len(s["lists"][0]["world"])
    ones = np.ones(n, np.uint8)
    stats = {}
    r = W.search(s["kfs"][0], s["lists"][0], ones, s["cam"], s["bounds"], s["mbf"], s["tab"], stats=stats)
    e = lambda k: int(r["exit"][at_[k]])      # noqa: E731
    assert e("u_is_min_x") == W.EXIT_FUSED and e("u_is_max_x") == W.EXIT_NOT_IN_IMAGE
    assert e("v_is_min_y") == W.EXIT_FUSED and e("v_is_max_y") == W.EXIT_NOT_IN_IMAGE
    assert e("z_is_zero") == W.EXIT_NOT_IN_IMAGE and e("z_is_zero_on_axis") == W.EXIT_NOT_IN_IMAGE and e("z_negative") == W.EXIT_NEG_DEPTH
    for side in ("left", "right", "top", "bottom"):
        assert e("window_" + side) == W.EXIT_FUSED and stats["window_past_" + side] >= 1
    assert e("dist_is_min") == W.EXIT_FUSED and e("dist_is_max") == W.EXIT_FUSED
    assert e("dist_below_min") == W.EXIT_DISTANCE and e("dist_above_max") == W.EXIT_DISTANCE
    assert e("normal_at_half") == W.EXIT_FUSED and e("normal_below_half") == W.EXIT_NORMAL
    bp = X.predict_scale_breakpoints(*setting)
    for k in range(1, L):
        for where, code in (("on", W.EXIT_FUSED), ("below", W.EXIT_ABOVE_TH_LOW)):
            i = at_["ratio_%s_break_%d" % (where, k)]
            ratio = f32(s["lists"][0]["dist"][i, 2]) / dist3d_of(s["lists"][0]["world"][i])
            assert ratio == (bp[k - 1] if where == "on" else np.nextafter(bp[k - 1], f32(0)))
            assert int(r["exit"][i]) == code, (k, where)
    assert e("ratio_inf") == W.EXIT_FUSED and e("ratio_nan") == W.EXIT_FUSED
    assert e("level_filtered") == W.EXIT_ABOVE_TH_LOW and r["best_dist"][at_["level_filtered"]] == 256 and stats["level_filter"] >= L
    assert e("mono_gate_rejects") == W.EXIT_ABOVE_TH_LOW and e("mono_gate_passes") == W.EXIT_FUSED
    assert e("stereo_gate_rejects") == W.EXIT_ABOVE_TH_LOW and e("stereo_gate_passes") == W.EXIT_FUSED
    assert stats["reject_7_8"] >= 1 and stats["reject_5_99"] >= 1
    first, second = s["twins"]
    assert second > first and r["best_idx"][at_["tie_by_visit_order"]] == second and r["best_dist"][at_["tie_by_visit_order"]] == 0
    assert stats["tie_kept_first"] >= 1
    assert e("dist_50") == W.EXIT_FUSED and r["best_dist"][at_["dist_50"]] == 50
    assert e("dist_51") == W.EXIT_ABOVE_TH_LOW and r["best_dist"][at_["dist_51"]] == 51 and r["best_idx"][at_["dist_51"]] == -1
    # the Sim3 mode has no gates: the two rejected probes fuse
    r0 = W.search(s["kfs"][0], s["lists"][0], ones, s["cam"], s["bounds"], s["mbf"], s["tab"], reproj_check=False)
    assert r0["exit"][at_["mono_gate_rejects"]] == W.EXIT_FUSED and r0["exit"][at_["stereo_gate_rejects"]] == W.EXIT_FUSED
    # the early returns (a negative radius): each of the four is taken, and everything that reaches the window leaves as "empty window"
    stats = {}
    rr = W.search(s["kfs"][0], s["lists"][0], ones, s["cam"], s["bounds"], s["mbf"], s["tab"], stats=stats, **RETURNS)
    for k in ("min_x", "max_x", "min_y", "max_y"):
        assert stats.get("return_%s_cell_%s" % tuple(k.split("_")), 0) >= 1, (k, stats)
        assert rr["exit"][at_["return_" + k]] == W.EXIT_EMPTY_WINDOW
    assert not (rr["exit"] > W.EXIT_EMPTY_WINDOW).any()


def test_non_integer_bounds_are_truncated_for_is_in_image_and_kept_for_the_grid():
    s, at_ = frac_edge_scene()
    n = len(s["lists"][0]["world"])
    r = W.search(s["kfs"][0], s["lists"][0], np.ones(n, np.uint8), s["cam"], s["bounds"], s["mbf"], s["tab"])
    e = lambda k: int(r["exit"][at_[k]])      # noqa: E731
    fb = FRAC_BOUNDS
    for axis, c, lo, hi in (("u", 0, fb[0], fb[1]), ("v", 1, fb[2], fb[3])):
        uv = lambda k: projection(s["lists"][0]["world"][at_[k]])[c]      # noqa: E731
        k = axis + "_between_float_and_truncated_min"
        assert lo <= uv(k) < f32(int(lo)) and e(k) == W.EXIT_NOT_IN_IMAGE            # Frame's bounds hold it, KeyFrame's do not
        assert uv(axis + "_is_float_min") == lo and e(axis + "_is_float_min") == W.EXIT_NOT_IN_IMAGE
        assert uv(axis + "_is_truncated_min") == f32(int(lo)) and e(axis + "_is_truncated_min") == W.EXIT_FUSED
        k = axis + "_between_truncated_and_float_max"
        assert f32(int(hi)) <= uv(k) < hi and e(k) == W.EXIT_NOT_IN_IMAGE
        assert uv(axis + "_is_truncated_max") == f32(int(hi)) and e(axis + "_is_truncated_max") == W.EXIT_NOT_IN_IMAGE
        assert uv(axis + "_below_truncated_max") < f32(int(hi)) and e(axis + "_below_truncated_max") == W.EXIT_EMPTY_WINDOW
    assert e("inside") == W.EXIT_FUSED
    # under Frame's float bounds (what the grid was built with) the "between" probes at the lower bounds would have fused
    for k in ("u_between_float_and_truncated_min", "v_between_float_and_truncated_min"):
        u, v = projection(s["lists"][0]["world"][at_[k]])
        cand = [j for j in range(len(s["kfs"][0]["kps"])) if abs(s["kfs"][0]["kps"]["x"][j] - u) < 3 and abs(s["kfs"][0]["kps"]["y"][j] - v) < 3]
        assert len(cand) == 1 and np.array_equal(s["kfs"][0]["desc"][cand[0]], s["lists"][0]["desc"][at_[k]])


# ---------------------------------------------------------------- (b) the batching licence ----------------------------------------------------------------
def licence_scene(seed):
    """three keyframes with the same view but each with descriptors of its own (bits flipped), one list of MapPoints; many keypoints already
    hold MapPoints (some of them in the list, some with more observations than the list's, some with fewer).  So a Replace in one keyframe
    makes list entries bad for the later ones, and the survivor's ComputeDistinctiveDescriptors picks a descriptor that the later keyframes
    match differently."""
    s = random_scene(seed, 96, 150, 1)
    rng = np.random.default_rng(seed + 1000)
    base = s["kfs"][0]
    kfs = [base]
    for k in (1, 2):
        d = base["desc"].copy()
        for j in range(len(d)):
            for b in rng.integers(0, 256, rng.choice([0, 8, 16, 28])):
                d[j, b >> 3] ^= 1 << (b & 7)
        kfs.append(dict(base, desc=d))
    s["kfs"] = kfs
    n_list = 150
    n_points = n_list + 200                                   # the list's MapPoints first, then MapPoints only keyframes hold
    mp_list = [int(v) if rng.random() < 0.95 else -1 for v in rng.permutation(n_list)]
    point_desc = rng.integers(0, 256, (n_points, 32), dtype=np.uint8)
    for i, mp in enumerate(mp_list):
        if mp >= 0:
            point_desc[mp] = s["lists"][0]["desc"][i]
    elsewhere = [rng.integers(0, 256, (1, 32), dtype=np.uint8) for _ in range(4)]      # four more keyframes, one keypoint each
    m = W.Map(point_desc, [k["desc"] for k in kfs] + elsewhere)
    for k, kf in enumerate(kfs):
        for idx in rng.permutation(len(kf["kps"]))[:70]:
            mp = int(rng.integers(n_points))
            if not m.in_keyframe(mp, k):
                m.add(mp, k, int(idx))
    for mp in rng.integers(n_list, n_points, 60):               # extra observations elsewhere: both Replace directions occur
        m.obs[int(mp)][3 + int(rng.integers(4))] = 0
    return s, m, mp_list


def batched(s, m0, mp_list, keyframes, search_again):
    """all searches of `keyframes` on the initial map, then the replay keyframe after keyframe; returns the map, the counts, the list positions
    searched again per keyframe and the batched results"""
    mps = s["lists"][0]
    kw = dict(cam=s["cam"], bounds=s["bounds"], mbf=s["mbf"], tab=s["tab"])
    uploaded = W.list_descriptors(m0, mp_list)
    assert all(np.array_equal(uploaded[i], mps["desc"][i]) for i, mp in enumerate(mp_list) if mp >= 0)
    results = dict((k, W.search(s["kfs"][k], mps, W.flags_of(m0, k, mp_list), **kw)) for k in keyframes)      # all searches on the INITIAL state
    bat = m0.copy()
    counts, stale_all = [], []
    for k in keyframes:
        again = (lambda fl, descs, k=k: W.search(s["kfs"][k], dict(mps, desc=descs), fl, **kw)) if search_again else None
        n, stale = W.replay_tail(bat, k, mp_list, results[k], uploaded, again)
        counts.append(n); stale_all.append(stale)
    return bat, counts, stale_all, results


@pytest.mark.parametrize("seed", [11, 12, 13])
def test_batched_searches_plus_replay_equal_the_sequential_fuse(seed):
    s, m0, mp_list = licence_scene(seed)
    mps = s["lists"][0]
    kw = dict(cam=s["cam"], bounds=s["bounds"], mbf=s["mbf"], tab=s["tab"])
    seq = m0.copy()
    n_seq = [W.fuse_sequential(seq, k, kf, mp_list, mps, **kw) for k, kf in enumerate(s["kfs"])]
    bat, n_bat, stale, results = batched(s, m0, mp_list, [0, 1, 2], search_again=True)
    assert seq.state() == bat.state() and n_seq == n_bat
    assert sum(n_seq) > 20 and sum(seq.bad) > 5
    # descriptors did change, and list entries were searched again because of it
    assert sum(a != b for a, b in zip(m0.state()[3], seq.state()[3])) > 3 and not stale[0] and len(stale[1]) + len(stale[2]) > 0
    # the re-test matters: list entries the initial flags admitted were bad (or already in the keyframe) when their turn came
    skipped = 0
    chk = m0.copy()
    for k in range(3):
        for i, mp in enumerate(mp_list):
            if results[k]["exit"][i] == W.EXIT_FUSED and (chk.bad[mp] or chk.in_keyframe(mp, k)):
                skipped += 1
        W.replay_tail(chk, k, mp_list, results[k], W.list_descriptors(m0, mp_list),
                      lambda fl, descs, k=k: W.search(s["kfs"][k], dict(mps, desc=descs), fl, **kw))
    assert skipped > 0 and chk.state() == seq.state()


def test_replay_without_searching_the_changed_survivors_again_is_not_the_reference():
    """what the licence test is able to catch: on each of its seeds, the replay that keeps the batched results of entries whose descriptor
    has changed ends in another map than the sequential Fuse"""
    departed = 0
    for seed in (11, 12, 13):
        s, m0, mp_list = licence_scene(seed)
        kw = dict(cam=s["cam"], bounds=s["bounds"], mbf=s["mbf"], tab=s["tab"])
        seq = m0.copy()
        for k, kf in enumerate(s["kfs"]):
            W.fuse_sequential(seq, k, kf, mp_list, s["lists"][0], **kw)
        naive = batched(s, m0, mp_list, [0, 1, 2], search_again=False)[0]
        departed += naive.state() != seq.state()
    assert departed == 3


@pytest.mark.parametrize("k", [0, 1, 2])
def test_one_keyframe_call_plus_replay_is_the_reference_without_searching_again(k):
    """n_pairs = 1 (SearchInNeighbors' second half, LoopClosing): the survivor of a Replace is in the keyframe and is not searched there again"""
    s, m0, mp_list = licence_scene(14)
    kw = dict(cam=s["cam"], bounds=s["bounds"], mbf=s["mbf"], tab=s["tab"])
    seq = m0.copy()
    n_seq = W.fuse_sequential(seq, k, s["kfs"][k], mp_list, s["lists"][0], **kw)
    bat, n_bat, _, _ = batched(s, m0, mp_list, [k], search_again=False)
    assert bat.state() == seq.state() and [n_seq] == n_bat and n_seq > 5 and len(seq.recomputed) > 0


# ---------------------------------------------------------------- (d) PredictScale ----------------------------------------------------------------
def level_by_table(bp, ratios):
    return (ratios[:, None] >= bp[None, :]).sum(axis=1)


def level_by_expression(ratios, sf, nl):
    L = X.load_library()
    return np.array([L.orbx_predict_scale(C.c_float(r), C.c_float(1.0), C.c_float(sf), nl) for r in ratios.tolist()])


@pytest.mark.parametrize("sf,nl", SETTINGS)
def test_breakpoints_equal_the_expression(sf, nl):
    bp = X.predict_scale_breakpoints(sf, nl)
    assert len(bp) == nl - 1 and (np.diff(bp) > 0).all() and bp[0] == np.nextafter(f32(1), f32(2))
    around = np.concatenate([(b.view(np.int32) + np.arange(-64, 65)).astype(np.int32).view(f32) for b in bp.reshape(-1, 1)])
    assert np.array_equal(level_by_table(bp, around), level_by_expression(around, sf, nl))
    for k, b in enumerate(bp):                           # the definition: the smallest float at level >= k + 1
        assert X.predict_scale(float(b), 1.0, sf, nl) == k + 1 and X.predict_scale(float(np.nextafter(b, f32(0))), 1.0, sf, nl) == k
    rng = np.random.default_rng(9)
    ratios = np.exp(rng.uniform(np.log(1e-6), np.log(1e6), 1000000)).astype(f32)
    assert np.array_equal(level_by_table(bp, ratios), level_by_expression(ratios, sf, nl))
    special = np.array([0.0, 1e-45, 1e-40, 1.1754942e-38, np.inf, np.nan], f32)
    with np.errstate(all="ignore"):
        assert level_by_table(bp, special).tolist() == [0, 0, 0, 0, nl - 1, 0] == level_by_expression(special, sf, nl).tolist()
    # the walk's ctypes logf statement is the same function
    some = np.concatenate([around[::7], ratios[:2000], special])
    with np.errstate(all="ignore"):
        assert [W.predict_scale(r, 1.0, sf, nl) for r in some] == level_by_expression(some, sf, nl).tolist()


def test_breakpoints_are_not_the_powers():
    bp = X.predict_scale_breakpoints(1.2, 8)
    assert abs(float(bp[1]) - 1.20000017) < 1e-8 and abs(float(bp[2]) - 1.44000018) < 1e-8
    assert bp[1] > f32(1.2) and bp[2] > f32(1.44) and bp[1] > f32(1.2) * f32(1.0) and bp[2] > f32(1.2) * f32(1.2)


def test_predict_scale_rejects_bad_arguments():
    L = X.load_library()
    b = np.zeros(16, f32)
    for sf, nl in ((1.0, 8), (0.9, 8), (float("nan"), 8), (float("inf"), 8), (1.2, 0)):
        assert L.orbx_predict_scale(1.0, 1.0, sf, nl) == -2
        assert L.orbx_predict_scale_breakpoints(sf, nl, b.ctypes.data_as(C.c_void_p)) == -2
    assert L.orbx_predict_scale_breakpoints(1.2, 8, None) == -2 and L.orbx_predict_scale_breakpoints(1.2, 1, None) == 0


SWEEP_SOURCES = [os.path.join(ROOT, "tests", "cpp", "predict_scale_sweep.cpp"), os.path.join(ROOT, "extractorb_amd", "csrc", "orbx_predict_scale.cpp")]


def build_sweep(tmp_path, *flags):
    exe = str(tmp_path / "predict_scale_sweep")
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-I" + os.path.join(ROOT, "include"), *flags, *SWEEP_SOURCES, "-o", exe])
    return exe


def test_sweep_over_every_float_between_a_half_and_twice_the_last_breakpoint(tmp_path):
    out = subprocess.check_output([build_sweep(tmp_path, "-O2")], text=True)
    print(out)
    lines = [l for l in out.splitlines() if l.startswith("scale")]
    assert len(lines) == 3 and all("mismatches 0" in l and "non-monotone 0" in l for l in lines)
    assert sum(int(l.split("floats ")[1].split()[0]) for l in lines) > 2.5e7


def test_sweep_is_clean_as_a_sanitized_host_program(tmp_path):
    """the stand-alone program under AddressSanitizer + UBSan, on a narrower range (+-4096 floats around every breakpoint)"""
    exe = build_sweep(tmp_path, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    out = subprocess.check_output([exe, "4096"], text=True)
    assert out.count("mismatches 0") == 3


# ---------------------------------------------------------------- the kernel's own source, on the host ----------------------------------------------------------------
HOST_FLAGS = ["-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"), "-I" + os.path.join(ROOT, "extractorb_amd", "csrc"),
              "-I" + os.path.join(ROOT, "include")]
HOST_SOURCES = [os.path.join(ROOT, "tests", "cpp", "fuse_host_check.cpp"), os.path.join(ROOT, "extractorb_amd", "csrc", "orbx_predict_scale.cpp")]


class HostParams(C.Structure):      # == FuseParams of extractorb_amd/csrc/orbx_params.hpp
    _fields_ = ([(n, C.c_float) for n in "fx fy cx cy minX maxX minY maxY wInv hInv".split()] +
                [("scale", C.c_float * 16), ("invSigma2", C.c_float * 16), ("breaks", C.c_float * 16), ("mbf", C.c_float), ("th", C.c_float)] +
                [(n, C.c_int) for n in "nlevels thLow reprojCheck capacity mpCapacity kfFirst kfStep mpFirst mpStep".split()])


def test_kernel_source_compiled_for_the_host_equals_the_walk(tmp_path):
    """k_fuse.hip itself (not a restatement), built with g++ behind tests/cpp/host_shim and run one thread at a time, on every scene of the GPU
    tests, both modes, and the edge scenes under the early returns: best index, best distance and exit code of every MapPoint"""
    so = str(tmp_path / "libfuse_host.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", *HOST_FLAGS, *HOST_SOURCES, "-o", so])
    L = C.CDLL(so)
    assert L.fuse_host_params_size() == C.sizeof(HostParams)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)      # noqa: E731
    compared = 0
    for name in SCENES:
        s = get(name); tab = s["tab"]; kfs, lists = s["kfs"], s["lists"]
        cap = max(len(k["kps"]) for k in kfs) + 3; mp_cap = len(lists[0]["world"]); B = len(kfs)
        kps = np.zeros((B, cap), X.KEYPOINT_DTYPE); desc = np.zeros((B, cap, 32), np.uint8); ur = np.full((B, cap), -1, f32)
        nout = np.zeros(B, np.int32); off = np.zeros((B, 64 * 48 + 1), np.int32); idx = np.zeros((B, cap), np.int32); poses = np.zeros((B, 12), f32)
        for f, k in enumerate(kfs):
            n = len(k["kps"])
            kps[f, :n] = k["kps"]; desc[f, :n] = k["desc"]; nout[f] = n; off[f] = k["grid_off"]; idx[f, :len(k["grid_idx"])] = k["grid_idx"]
            poses[f] = k["pose"].reshape(12)
            if k["ur"] is not None:
                ur[f, :n] = k["ur"]
        w = np.stack([m["world"] for m in lists]); nv = np.stack([m["normal"] for m in lists]); dist = np.stack([m["dist"] for m in lists])
        md = np.stack([m["desc"] for m in lists])
        pairs = cases(name)
        fl = np.stack([flags_for(s, k, mp_cap) for k, _ in pairs])
        for opt in [dict(), dict(reproj_check=False)] + ([RETURNS] if name.startswith("edge") else []):
            p = HostParams()
            p.fx, p.fy, p.cx, p.cy = (float(c) for c in s["cam"][:4])
            p.minX, p.maxX, p.minY, p.maxY = (float(int(b)) for b in s["bounds"])      # as orbx_fuse_device fills them: truncated
            p.wInv = f32(64) / (s["bounds"][1] - s["bounds"][0]); p.hInv = f32(48) / (s["bounds"][3] - s["bounds"][2])
            for i in range(tab["nlevels"]):
                p.scale[i] = tab["scale"][i]; p.invSigma2[i] = tab["inv_sigma2"][i]
            for i, b in enumerate(X.predict_scale_breakpoints(*s["setting"])):
                p.breaks[i] = b
            p.mbf = float(s["mbf"]); p.th = opt.get("th", 3.0); p.nlevels = tab["nlevels"]; p.thLow = 50; p.reprojCheck = int(opt.get("reproj_check", True))
            p.capacity = cap; p.mpCapacity = mp_cap; p.kfFirst = 0; p.kfStep = 1; p.mpFirst = 0; p.mpStep = 1 if len(lists) > 1 else 0
            n = len(pairs)
            bi = np.full((n, mp_cap), -7, np.int32); bd = bi.copy(); ex = np.full((n, mp_cap), 99, np.uint8); nf = np.zeros(n, np.int32)
            L.fuse_host(ptr(w), ptr(nv), ptr(dist), ptr(md), None, ptr(fl), ptr(poses), ptr(kps), ptr(ur), ptr(desc), ptr(nout), ptr(off), ptr(idx),
                        C.byref(p), ptr(bi), ptr(bd), ptr(ex), ptr(nf), n)
            for q, (k, l) in enumerate(pairs):
                want = walk(name, k, l, **opt)
                assert np.array_equal(bi[q], want["best_idx"]) and np.array_equal(bd[q], want["best_dist"]) and np.array_equal(ex[q], want["exit"]), (name, opt, q)
                compared += len(want["exit"])
    assert compared > 20000


def test_kernel_source_stays_inside_its_arrays_as_a_sanitized_host_program(tmp_path):
    """the same source as a stand-alone program under AddressSanitizer + UBSan: exact-size buffers, valid and corrupt grids"""
    exe = str(tmp_path / "fuse_host_check")
    subprocess.check_call(["g++", "-O1", "-g", "-DFUSE_HOST_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *HOST_FLAGS, *HOST_SOURCES,
                           "-o", exe])
    out = subprocess.check_output([exe], text=True)
    assert out.count("trial") == 6 and out.strip().endswith("clean")


# ---------------------------------------------------------------- the surface ----------------------------------------------------------------
def test_entries_are_declared_documented_and_exported():
    for n in ("orbx_fuse_device", "orbx_predict_scale", "orbx_predict_scale_breakpoints"):
        assert n in X.header_symbols() and hasattr(X.load_library(), n)
    text = open(X.orbextractor._HEADER).read()
    pos = text.index("int orbx_fuse_device(")
    doc = text[text.rindex("/*", 0, pos):pos]
    for word in ("1399-1609", "1611-1733", "1404-1410", "1524-1526", "1573-1592", "bRight", "FIRST", "CLAMPED", "no capacity bound", "mfMaxDistance"):
        assert word in doc, word
    z = C.c_void_p(16)      # never dereferenced: the handle is checked first
    assert X.load_library().orbx_fuse_device(None, 1, 0, 1, 0, 0, z, z, z, z, z, 16, z, z, z, z, z, z, 16, z, z, z, z, 8, 40.0, 3.0, 50, 1, z, z, z, z) == -2
    for m in ("fuse_device",):
        assert callable(getattr(X.ORBextractor, m, None))
    assert callable(X.predict_scale) and callable(X.predict_scale_breakpoints)
