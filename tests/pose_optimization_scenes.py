"""Scenes of orbx_optimize_pose_device for tests/test_pose_optimization.py (CPU) and tests/test_pose_optimization_gpu.py: a synthetic camera,
points in front of it, keypoints that are their projections plus noise, a planted share of gross outliers, an initial pose a little off the
true one (what a motion model hands the optimiser).  A scene is a dict in the ENTRY'S layouts: problems (POSE_PROBLEM_DTYPE), kps
(KEYPOINT_DTYPE [frames*cap]), n_out [frames], u_right [frames*cap] or None, matches [rows*cap], world [M, 3], poses [pose frames*12],
eyes, cap, nlevels, first, step, n_problems; `planted` [rows*cap] marks the gross outliers.  expected() runs the walk
(tests/pose_optimization_walk.py) on every problem ONCE per scene and the tests share it."""
import functools

import numpy as np

import pose_optimization_walk as PW

f32, f64 = np.float32, np.float64
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])
PROBLEM_DTYPE = np.dtype([("model", "<i4"), ("model2", "<i4"), ("cam", "<f4", 8), ("cam2", "<f4", 8), ("mbf", "<f4"), ("Trl", "<f4", 12),
                          ("inv_level_sigma2", "<f4", 16)])
RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_initial", "<i4"), ("n_bad", "<i4"), ("n_inliers", "<i4"), ("rounds", "<i4"),
                         ("empty_rounds", "<i4"), ("its", "<i4", 4), ("trials", "<i4", 4), ("lambda", "<f8", 4), ("chi2", "<f8", 4)])
NLEVELS = 8
PINHOLE = [458.654, 457.296, 367.215, 248.375, 0, 0, 0, 0]
KB8_L = [190.978, 190.973, 254.931, 256.897, 0.0034823, 0.0007150, -0.0020532, 0.0002029]
KB8_R = [190.442, 190.434, 252.597, 254.917, 0.0034003, 0.0017669, -0.0026630, 0.0003299]
MBF = 47.9
TRL = [0.9999, 0.0023, 0.0141, -0.1011, -0.0023, 1.0, -0.0007, 0.0019, -0.0141, 0.0007, 0.9999, 0.0011]
POISON_FLAG = 0xEE


def inv_sigma2():
    out = np.zeros(16, f32)
    s = f32(1.0)
    for l in range(NLEVELS):
        out[l] = f32(1.0) / f32(s * s)
        s = f32(s * f32(1.2))
    return out


def rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def pose12(R, t):
    return np.concatenate([np.asarray(R, f64), np.asarray(t, f64).reshape(3, 1)], axis=1).astype(f32).reshape(12)


def project64(model, cam, Xc):
    """float64, libm: the scene's own camera (not the statement under test)"""
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    if not model:
        return np.stack([cam[0] * x / z + cam[2], cam[1] * y / z + cam[3]], 1)
    theta = np.arctan2(np.sqrt(x * x + y * y), z)
    psi = np.arctan2(y, x)
    r = theta + cam[4] * theta ** 3 + cam[5] * theta ** 5 + cam[6] * theta ** 7 + cam[7] * theta ** 9
    return np.stack([cam[0] * r * np.cos(psi) + cam[2], cam[1] * r * np.sin(psi) + cam[3]], 1)


def make(counts, model=0, eyes=1, stereo=False, outliers=0.3, seed=1, first=0, step=1, spare=3, off=(0.01, 0.05), noise=0.6):
    """counts: per problem the correspondences (eyes = 2: a pair (left, right) per problem).  outliers: a share, or one per problem."""
    rng = np.random.default_rng(seed)
    P = len(counts)
    counts = [c if isinstance(c, tuple) else (c,) for c in counts]
    shares = outliers if isinstance(outliers, (list, tuple)) else [outliers] * P
    n_kp = [[c + (c // 5) + 1 for c in cs] for cs in counts]            # every problem has keypoints without a MapPoint
    cap = max(max(n) for n in n_kp) + spare
    frames = first + (P - 1) * step + 1 if step >= 0 else first + 1
    rows = P * eyes
    s = dict(eyes=eyes, cap=cap, nlevels=NLEVELS, first=first, step=step, n_problems=P,
             problems=np.zeros(P, PROBLEM_DTYPE), kps=np.zeros(frames * eyes * cap, KEYPOINT_DTYPE), n_out=np.zeros(frames * eyes, np.int32),
             u_right=(np.full(frames * cap, -1, f32) if stereo else None), matches=np.full(rows * cap, -1, np.int32),
             poses=np.zeros(frames * 12, f32), planted=np.zeros(rows * cap, bool), true_pose=np.zeros((P, 12), f32))
    s["kps"]["octave"] = 0
    for f in range(frames):
        s["poses"][f * 12:(f + 1) * 12] = pose12(np.eye(3), [0, 0, 0])
    world = []
    sig = inv_sigma2()
    for p in range(P):
        f = first + p * step
        pb = s["problems"][p]
        pb["model"], pb["model2"] = model, (1 if eyes == 2 else 0)
        pb["cam"] = KB8_L if model else PINHOLE
        pb["cam2"] = KB8_R if eyes == 2 else np.zeros(8)
        pb["mbf"] = MBF
        pb["Trl"] = TRL if eyes == 2 else [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]
        pb["inv_level_sigma2"] = sig
        R = rotation(*(rng.uniform(-0.1, 0.1, 3)))
        t = rng.uniform(-0.5, 0.5, 3)
        s["true_pose"][p] = pose12(R, t)
        dR = rotation(*(rng.uniform(-off[0], off[0], 3)))
        s["poses"][f * 12:(f + 1) * 12] = pose12(dR @ R, t + rng.uniform(-off[1], off[1], 3))
        Rrl, trl = np.asarray(TRL, f64).reshape(3, 4)[:, :3], np.asarray(TRL, f64).reshape(3, 4)[:, 3]
        for eye in range(eyes):
            n, c = n_kp[p][eye], counts[p][eye]
            row, frame = p * eyes + eye, f * eyes + eye
            s["n_out"][frame] = n
            holders = np.sort(rng.choice(n, c, replace=False))
            cam = np.asarray((KB8_R if eye else (KB8_L if model else PINHOLE)), f64)
            mdl = 1 if eye else model
            # points in front of the camera, spread over the image
            Xc = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(4, 12, n)], 1)
            Xl = Xc if not eye else (Xc - trl) @ Rrl                      # the right eye sees Rrl * Xl + trl
            Xw = (Xl - t) @ R                                             # R^T (Xl - t)
            uv = project64(mdl, cam, Xc)
            octave = rng.integers(0, NLEVELS, n)
            jitter = rng.normal(0, noise, (n, 2)) * (1.2 ** octave)[:, None]
            bad = np.zeros(n, bool)
            k_bad = int(round(shares[p] * c))
            bad[rng.choice(holders, k_bad, replace=False)] = True
            gross = rng.uniform(25, 70, (n, 2)) * rng.choice([-1, 1], (n, 2))
            uv = uv + jitter + np.where(bad[:, None], gross, 0)
            at = frame * cap
            s["kps"]["x"][at:at + n], s["kps"]["y"][at:at + n], s["kps"]["octave"][at:at + n] = uv[:, 0], uv[:, 1], octave
            if stereo:
                has = rng.random(n) < 0.5
                ur = uv[:, 0] - MBF / Xc[:, 2] + rng.normal(0, 0.6, n) * (1.2 ** octave)
                s["u_right"][f * cap:f * cap + n] = np.where(has, ur, -1)
            base = len(world)
            world.extend(Xw[holders].astype(f32))
            s["matches"][row * cap + holders] = base + np.arange(c)
            s["planted"][row * cap + holders] = bad[holders]
    s["world"] = np.asarray(world, f32).reshape(-1, 3) if world else np.zeros((1, 3), f32)
    return s


def problem(s, p, poses=None, outlier=None):
    """problem p of scene s as the walk takes it; flags are views into `outlier` (rows*cap uint8), updated in place"""
    eyes, cap = s["eyes"], s["cap"]
    f = s["first"] + p * s["step"]
    pb = s["problems"][p]
    outlier = outlier if outlier is not None else np.full(s["n_problems"] * eyes * cap, POISON_FLAG, np.uint8)
    poses = poses if poses is not None else s["poses"]
    return dict(eyes=eyes, cap=cap, nlevels=s["nlevels"], model=int(pb["model"]), model2=int(pb["model2"]), cam=pb["cam"], cam2=pb["cam2"],
                mbf=pb["mbf"], Trl=pb["Trl"], inv_sigma2=pb["inv_level_sigma2"], n=[int(s["n_out"][f * eyes + e]) for e in range(eyes)],
                kps=[s["kps"][(f * eyes + e) * cap:(f * eyes + e + 1) * cap] for e in range(eyes)],
                u_right=None if s["u_right"] is None else s["u_right"][f * cap:(f + 1) * cap],
                matches=[s["matches"][(p * eyes + e) * cap:(p * eyes + e + 1) * cap] for e in range(eyes)], world=s["world"],
                pose=poses[f * 12:(f + 1) * 12].copy(), flags=[outlier[(p * eyes + e) * cap:(p * eyes + e + 1) * cap] for e in range(eyes)])


def poisoned_outputs(s):
    return dict(poses=s["poses"].copy(), outlier=np.full(s["n_problems"] * s["eyes"] * s["cap"], POISON_FLAG, np.uint8),
                result=np.frombuffer(bytes([0xAB]) * (RESULT_DTYPE.itemsize * s["n_problems"]), RESULT_DTYPE).copy())


def expected(s, **walk_args):
    """(walked, outputs): the walk on every problem and the arrays the entry must leave"""
    o = poisoned_outputs(s)
    walked = []
    for p in range(s["n_problems"]):
        w = PW.solve(problem(s, p, outlier=o["outlier"]), **walk_args)
        walked.append(w)
        r = o["result"][p]
        for k in ("status", "n_initial", "n_bad", "n_inliers", "rounds", "empty_rounds", "its", "trials", "chi2"):
            r[k] = w[k]
        r["lambda"] = w["lam"]
        if w["pose"] is not None:
            f = s["first"] + p * s["step"]
            o["poses"][f * 12:(f + 1) * 12] = w["pose"]
    return walked, o


def differences(got, want):
    return [k for k in ("poses", "outlier", "result") if got[k].tobytes() != want[k].tobytes()]


CASES = {"mono_n%d" % n: dict(counts=[n], seed=10 + n) for n in (2, 3, 9, 10, 11, 63, 64, 65, 257, 300)}
CASES.update({
    "mono_n64_clean": dict(counts=[64], outliers=0.0, seed=31),
    "mono_n64_all_outliers": dict(counts=[64], outliers=1.0, seed=32),
    "mixed_stereo_batch3": dict(counts=[40, 64, 130], stereo=True, seed=33),
    "mono_batch17": dict(counts=[5, 9, 10, 12, 20, 33, 47, 63, 64, 65, 80, 96, 101, 120, 7, 3, 2], outliers=[0.0, 0.3, 1.0] * 5 + [0.0, 0.3], seed=34),
    "kb8_mono_batch3": dict(counts=[30, 65, 100], model=1, outliers=[0.0, 0.3, 1.0], seed=35),
    "kb8_rig_batch3": dict(counts=[(30, 25), (65, 40), (12, 70)], model=1, eyes=2, outliers=[0.3, 0.0, 1.0], seed=36),
    "mixed_stereo_first2_step3": dict(counts=[20, 35, 64], stereo=True, first=2, step=3, seed=37),
})


# ---- crafted scenes: each reaches one exit or event (tests/test_pose_optimization.py (b) asserts that it does) -------------------------
def _edges(s, p=0):
    """(rows of kps / matches of problem p's frame) for a one-camera scene"""
    f = s["first"] + p * s["step"]
    return f * s["cap"], p * s["cap"]


def crafted_non_finite_trial():
    """Twelve observations 1e12 px off: Huber's weights shrink H, the first trial's rotation is beyond 2^20 rad, its sin / cos and so the trial
    pose are NaN, the trial is rejected with a NaN rho (which ends the trials without terminating) - and the errors the classification reads
    are that trial's: NaN, NOT > 5.991f.  Every edge stays an inlier, where a fresh computeError at the final pose flags them all."""
    s = make(counts=[12], outliers=0.0, seed=51)
    at, row = _edges(s)
    hold = np.nonzero(s["matches"][row:row + s["cap"]] >= 0)[0]
    s["kps"]["x"][at + hold] += f32(1e12)
    return s


def crafted_behind_the_camera():
    """three MapPoints behind the camera (z < 0 at every pose of the optimisation): there is no depth test, they contribute"""
    s = make(counts=[40], seed=52)
    at, row = _edges(s)
    hold = np.nonzero(s["matches"][row:row + s["cap"]] >= 0)[0][:3]
    T = s["true_pose"][0].reshape(3, 4).astype(f64)
    for i in hold:
        Xc = np.array([0.5, -0.3, -6.0])
        s["world"][s["matches"][row + i]] = ((Xc - T[:, 3]) @ T[:, :3]).astype(f32)
    return s


def crafted_z_zero():
    """the identity pose, exactly, and one MapPoint with z == 0: its error is non-finite at the initial pose, chi2 and H are NaN, every solve
    fails, every trial is rejected by a NaN rho, the pose stays the initial one through ten iterations of four rounds; its own chi2 is NaN
    (0 * inf), which is not > 5.991f"""
    s = make(counts=[30], outliers=0.2, seed=53)
    s["poses"][:12] = pose12(np.eye(3), [0, 0, 0])
    at, row = _edges(s)
    T = s["true_pose"][0].reshape(3, 4).astype(f64)
    s["world"][:] = ((s["world"].astype(f64) @ T[:, :3].T) + T[:, 3]).astype(f32)      # the true pose becomes the identity
    i = np.nonzero(s["matches"][row:row + s["cap"]] >= 0)[0][4]
    s["world"][s["matches"][row + i]] = [1.0, 0.5, 0.0]
    return s


def crafted_thresholds():
    """chi2 a hair on each side of 5.991f and of 7.815f.  Every observation is a gross outlier, so round 0 flags them all and round 1 finds
    no active edge: it classifies every edge at the INITIAL pose with a fresh computeError - a pose the scene controls.  Two mono and two
    stereo edges get observations whose error at that pose is sqrt(threshold / invSigma2) * (1 -+ 2e-4) along x: chi2 of about 5.9886,
    5.9934, 7.8119 and 7.8181"""
    s = make(counts=[100], outliers=1.0, seed=55, stereo=True)
    pb = problem(s, 0)
    ed = PW.Edges(pb)
    e, chi2, _ = PW.errors(pb, ed, PW.se3_from_float(pb["pose"]), PW.HEADER_MATH)
    mono, stereo = np.nonzero(ed.kind == 1)[0][:2], np.nonzero(ed.kind == 2)[0][:2]
    s["planted_thresholds"] = []
    for k, thr, sign in ((mono[0], 5.991, -1), (mono[1], 5.991, 1), (stereo[0], 7.815, -1), (stereo[1], 7.815, 1)):
        d = np.sqrt(thr / ed.w[k]) * (1 + sign * 2e-4)
        s["kps"]["x"][k] = f32(ed.obs[k, 0] - e[k, 0] + d)          # the projection at the initial pose, plus d
        s["kps"]["y"][k] = f32(ed.obs[k, 1] - e[k, 1])
        if ed.kind[k] == 2:
            s["u_right"][k] = f32(ed.obs[k, 2] - e[k, 2])
        s["planted_thresholds"].append((int(k), thr, sign))
    return s


CRAFTED = {"non_finite_trial": crafted_non_finite_trial, "behind_the_camera": crafted_behind_the_camera, "z_zero": crafted_z_zero,
           "thresholds": crafted_thresholds,
           "huber_keeps_round3_flags": lambda: make(counts=[40], seed=104, noise=1.4, outliers=0.2),
           "no_active_edge_n100": lambda: make(counts=[100], outliers=1.0, seed=55)}


@functools.lru_cache(maxsize=None)
def case(name):
    return CRAFTED[name]() if name in CRAFTED else make(**CASES[name])


@functools.lru_cache(maxsize=None)
def case_expected(name):
    return expected(case(name))
