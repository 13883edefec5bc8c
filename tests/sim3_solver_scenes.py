"""Scenes for Sim3Solver (tests/test_sim3_solver.py, tests/test_sim3_solver_gpu.py), small on purpose.  A problem: points in front of
keyframe 2's camera (x +-2, y +-1.5, z 4 .. 8 m), carried into keyframe 1's camera by a true Sim3 of scale 1.7 (a rotation of 0.12 rad
about a skew axis, t = (0.3, -0.2, 0.4)), both taken back to world coordinates through the keyframes' poses; 5 mm noise on pMP1's position,
about half of the correspondences gross outliers; N present slots among n1 ~ 1.3 N, so that the compaction and mvnIndices1 differ from the
identity.  Octaves 0 .. 3 of a 1.2 pyramid (thresholds 9, 13, 19, 27).
A scene is a dict of the arrays orbx_sim3_solve_device takes, on the host: problems [P] (SIM3_PROBLEM_DTYPE), x1w / x2w [P, cap, 3],
oct1 / oct2 [P, cap], rand [P, max_iterations, 3], and cap, probability, min_inliers, max_iterations, nlevels."""
import functools

import numpy as np

import sim3_solver_walk as SW

f32 = np.float32
NLEVELS = 8
PINHOLE = (458.0, 457.0, 367.0, 248.0, 0.0, 0.0, 0.0, 0.0)
KB8 = (190.97847, 190.97330, 254.93170, 256.89744, 0.0034823894, 0.0007150348, -0.0020532361, 0.00020293673)
SIGMA2 = np.zeros(16, f32)
SIGMA2[:NLEVELS] = (f32(1.2) ** np.arange(NLEVELS, dtype=f32)) ** 2
PROBLEM_DTYPE = np.dtype([("n1", "<i4"), ("fix_scale", "<i4"), ("model1", "<i4"), ("model2", "<i4"), ("cam1", "<f4", 8), ("cam2", "<f4", 8),
                          ("Tcw1", "<f4", 12), ("Tcw2", "<f4", 12), ("level_sigma2", "<f4", 16)])
RESULT_DTYPE = np.dtype([("status", "<i4"), ("n", "<i4"), ("max_its", "<i4"), ("iterations", "<i4"), ("best_it", "<i4"), ("n_inliers", "<i4"),
                         ("best_inliers", "<i4"), ("scale", "<f4"), ("R", "<f4", 9), ("t", "<f4", 3), ("T12", "<f4", 16)])
POISON_B = 0xEE
TRUE_SCALE = 1.7


def rot(axis, angle):
    axis = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


def pose(axis, angle, t):
    return np.hstack([rot(axis, angle), np.asarray(t, float).reshape(3, 1)])


def problem(rng, N, cap, fix_scale=0, model=0, outliers=0.5, n1=None, noise=0.005, scale=TRUE_SCALE):
    """one problem dict (sim3_solver_walk's) with N present slots among n1"""
    n1 = min(cap, int(round(1.3 * N)) + 1) if n1 is None else n1
    T1, T2 = pose((0.2, 1.0, 0.1), 0.3, (0.5, -0.1, 0.2)), pose((1.0, -0.3, 0.2), -0.2, (-0.4, 0.3, 0.1))
    R12, t12 = rot((0.3, 1.0, -0.2), 0.12), np.array([0.3, -0.2, 0.4])
    X2c = np.stack([rng.uniform(-2, 2, n1), rng.uniform(-1.5, 1.5, n1), rng.uniform(4, 8, n1)], axis=1)
    X1c = scale * X2c @ R12.T + t12
    gross = rng.random(n1) < outliers
    X1c[gross] = np.stack([rng.uniform(-4, 4, gross.sum()), rng.uniform(-3, 3, gross.sum()), rng.uniform(6, 14, gross.sum())], axis=1)
    x1w = (X1c - T1[:, 3]) @ T1[:, :3] + rng.normal(0, noise, (n1, 3))
    x2w = (X2c - T2[:, 3]) @ T2[:, :3]
    present = np.zeros(n1, bool)
    present[rng.permutation(n1)[:N]] = True
    oct1, oct2 = rng.integers(0, 4, n1).astype(np.int32), rng.integers(0, 4, n1).astype(np.int32)
    gone = np.nonzero(~present)[0]
    oct1[gone[0::2]] = -1                                   # absent by either octave, or by both
    oct2[gone[1::2]] = -1
    oct2[gone[0::4]] = -1
    full = lambda a, fill: np.concatenate([a, np.full((cap - n1,) + a.shape[1:], fill, a.dtype)])
    cam = KB8 if model else PINHOLE
    return dict(n1=n1, fix_scale=int(fix_scale), model1=model, model2=model, cam1=np.array(cam, f32), cam2=np.array(cam, f32),
                Tcw1=T1.astype(f32).reshape(-1), Tcw2=T2.astype(f32).reshape(-1), sigma2=SIGMA2.copy(), x1w=full(x1w.astype(f32), 1e6),
                x2w=full(x2w.astype(f32), -1e6), oct1=full(oct1, 2), oct2=full(oct2, 2))      # beyond n1: present-looking slots, never read


def scene(problems, rng, max_iterations=300, min_inliers=15, probability=0.99):
    cap = len(problems[0]["oct1"])
    rows = np.zeros(len(problems), PROBLEM_DTYPE)
    for r, pb in zip(rows, problems):
        for k in ("n1", "fix_scale", "model1", "model2", "cam1", "cam2", "Tcw1", "Tcw2"):
            r[k] = pb[k]
        r["level_sigma2"] = pb["sigma2"]
    return dict(list=problems, problems=rows, x1w=np.stack([p["x1w"] for p in problems]), x2w=np.stack([p["x2w"] for p in problems]),
                oct1=np.stack([p["oct1"] for p in problems]), oct2=np.stack([p["oct2"] for p in problems]),
                rand=rng.integers(0, 2 ** 31, (len(problems), max_iterations, 3)).astype(np.int32), cap=cap, probability=probability,
                min_inliers=min_inliers, max_iterations=max_iterations, nlevels=NLEVELS)


def make(Ns, seed, cap=None, max_iterations=300, min_inliers=15, **kw):
    """a batch with one problem per entry of Ns; kw: per-problem keywords, a list gives one value per problem"""
    rng = np.random.default_rng(2400 + seed)
    cap = cap or int(round(1.3 * max(Ns))) + 8
    each = lambda i: dict((k, v[i % len(v)] if isinstance(v, (list, tuple)) else v) for k, v in kw.items())
    return scene([problem(rng, N, cap, **each(i)) for i, N in enumerate(Ns)], rng, max_iterations, min_inliers)


def rand_for(triples, N):
    """raw rand() values that make ssDraw3 / draw3 return the given index triples"""
    out = np.zeros((len(triples), 3), np.int32)
    for it, tr in enumerate(triples):
        avail = list(range(N))
        for j, want in enumerate(tr):
            pos, size = avail.index(want), len(avail)
            out[it, j] = int((pos + 0.5) * 2147483648.0 / size)
            avail[pos] = avail[-1]
            avail.pop()
        assert SW.draw3(out[it], N) == list(tr)
    return out


CASES = {
    "n3_min3_one_iteration": lambda: make([3], 1, min_inliers=3, outliers=0.0),
    "n14_too_few": lambda: make([14], 2),
    "n15_equals_min_inliers": lambda: make([15], 3, outliers=0.0),
    "n16_it20": lambda: make([16], 4, max_iterations=20, outliers=0.2),
    "n20_it21": lambda: make([20], 5, max_iterations=21),
    "n63_it20_kb8": lambda: make([63], 6, max_iterations=20, model=1),
    "n64_it300": lambda: make([64], 7),
    "n65_it21_fix_scale": lambda: make([65], 8, max_iterations=21, fix_scale=1),
    "n65_it300_fix_scale_true_scale_1": lambda: make([65], 9, fix_scale=1, scale=1.0),
    "n130_it20_kb8": lambda: make([130], 10, max_iterations=20, model=1),
    "n300_it300": lambda: make([300], 11),
    "n64_it1": lambda: make([64], 12, max_iterations=1),
    "n64_pure_outliers_it300": lambda: make([64], 13, outliers=1.0),
    "batch3": lambda: make([20, 64, 14], 14, max_iterations=21),
    "batch17": lambda: make([3, 14, 15, 16, 20, 63, 64, 65, 130, 40, 33, 17, 100, 64, 15, 28, 90], 15, max_iterations=20,
                            model=[0, 0, 1, 0, 0], fix_scale=[0, 0, 0, 1], outliers=[0.5, 0.3, 0.5, 1.0, 0.5, 0.0, 0.5]),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


def walk(s, form=SW.solve, m=SW.HEADER_MATH):
    return [form(pb, s["rand"][p], s["probability"], s["min_inliers"], s["max_iterations"], s["nlevels"], m) for p, pb in enumerate(s["list"])]


def canon(a):
    a = np.array(a, f32)
    a.view(np.uint32)[np.isnan(a)] = 0x7fc00000
    return a


def poisoned_outputs(s):
    P = len(s["list"])
    return dict(result=np.full(P * RESULT_DTYPE.itemsize, POISON_B, np.uint8).view(RESULT_DTYPE), inliers=np.full((P, s["cap"]), POISON_B, np.uint8))


def expected(s, walked=None):
    """the outputs a call on poisoned arrays must leave"""
    walked = walked or walk(s)
    o = poisoned_outputs(s)
    for p, w in enumerate(walked):
        r = o["result"][p]
        for k in ("status", "n", "max_its", "iterations", "best_it", "n_inliers", "best_inliers"):
            r[k] = w[k]
        r["scale"], r["R"], r["t"], r["T12"] = canon(w["scale"]), canon(w["R"]), canon(w["t"]), canon(w["T12"])
        if w["flags"] is not None:
            o["inliers"][p, :len(w["flags"])] = w["flags"]
    return o


@functools.lru_cache(maxsize=None)
def case_expected(name):
    walked = walk(case(name))
    return walked, expected(case(name), walked)


def differences(got, want):
    out = []
    for f in RESULT_DTYPE.names:
        a, b = got["result"][f], want["result"][f]
        bad = [p for p in range(len(a)) if a[p].tobytes() != b[p].tobytes()]
        if bad:
            out.append((f, bad[:4], a[bad[0]], b[bad[0]]))
    if not np.array_equal(got["inliers"], want["inliers"]):
        out.append(("inliers", np.argwhere(got["inliers"] != want["inliers"])[:4].tolist()))
    return out
