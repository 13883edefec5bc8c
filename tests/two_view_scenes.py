"""Scenes for TwoViewReconstruction::Reconstruct (tests/test_two_view.py, tests/test_two_view_gpu.py): small synthetic frame pairs at
capacity 128 whose frames hold about 120 keypoints, matched and unmatched ones, so that Normalize over all keypoints differs from over the
matched ones.  A scene is a dict of the arrays orbx_reconstruct_two_views_device takes, on the host:
  kps [frames, cap] (KEYPOINT_DTYPE), n_out [frames], matches [pairs, cap], n_matches [pairs], rand [pairs, iterations, 8], cam (fx, fy, cx,
  cy), frames1 / frames2 = (first, step), and the parameters.
K = (458, 457, 367, 248); the second camera is a yaw of 0.05 rad with t = (-0.6, 0.05, 0.1); 0.3 px noise, 10 % gross outliers; points
in x +-2.5, y +-1.5 at a depth of 4 .. 8 m ("general"), on z = 4 + 0.8x - 0.2y ("plane") or z = 5 + 0.3x - 0.2y ("frontal");
"zero_t" has no translation."""
import numpy as np

import two_view_walk as TW

CAP = 128
CAM = (458.0, 457.0, 367.0, 248.0)
f32 = np.float32
KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


def _project(X):
    return np.stack([CAM[0] * X[:, 0] / X[:, 2] + CAM[2], CAM[1] * X[:, 1] / X[:, 2] + CAM[3]], axis=1)


def frame_pair(rng, kind, N, n_keys=120, noise=0.3, outliers=0.1, yaw=0.05, t=(-0.6, 0.05, 0.1), far=0, far_z=300.0):
    """(pts1 [n1, 2], pts2 [n2, 2], matches12 [n1]) of one pair: N matches among n_keys keypoints per frame, in shuffled order"""
    n_keys = max(n_keys, N)
    x, y = rng.uniform(-2.5, 2.5, N), rng.uniform(-1.5, 1.5, N)
    z = dict(general=rng.uniform(4.0, 8.0, N), plane=4.0 + 0.8 * x - 0.2 * y, frontal=5.0 + 0.3 * x - 0.2 * y, zero_t=rng.uniform(4.0, 8.0, N))[kind]
    z[:far] = far_z                                     # `far` points, far away: counted by CheckRT, cosParallax >= 0.99998
    X = np.stack([x * (z / np.where(z > 100, 6.0, z)), y * (z / np.where(z > 100, 6.0, z)), z], axis=1) if far else np.stack([x, y, z], axis=1)
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    tt = np.zeros(3) if kind == "zero_t" else np.array(t)
    a = _project(X) + rng.normal(0, noise, (N, 2))
    b = _project(X @ R.T + tt) + rng.normal(0, noise, (N, 2))
    gross = rng.random(N) < outliers
    b[gross] = np.stack([rng.uniform(20, 730, gross.sum()), rng.uniform(20, 460, gross.sum())], axis=1)
    pts1 = np.vstack([a, np.stack([rng.uniform(20, 730, n_keys - N), rng.uniform(20, 460, n_keys - N)], axis=1)])
    pts2 = np.vstack([b, np.stack([rng.uniform(20, 730, n_keys - N), rng.uniform(20, 460, n_keys - N)], axis=1)])
    o1, o2 = rng.permutation(n_keys), rng.permutation(n_keys)      # new position -> old index
    inv2 = np.argsort(o2)
    m = np.full(n_keys, -1, np.int32)
    for new1, old in enumerate(o1):
        if old < N:
            m[new1] = inv2[old]
    return pts1[o1].astype(f32), pts2[o2].astype(f32), m


def make(kind="general", N=96, seed=1, iterations=12, rh_threshold=0.5, pairs=1, shape="stream", cap=CAP, min_triangulated=50, min_parallax=1.0, **kw):
    """shape "stream": pair p = frames (2p, 2p + 1); "twice": every pair names frames (0, 1), each with its own draws; "fan": frame 0
    against frames 1 .. pairs (the matches of every pair index frame 0's keypoints)"""
    rng = np.random.default_rng(1000 * seed + N)
    if shape == "stream":
        built = [frame_pair(rng, kind, N, **kw) for _ in range(pairs)]
        frames = [f for b in built for f in (b[0], b[1])]
        tables = [b[2] for b in built]
        frames1, frames2 = (0, 2), (1, 2)
    elif shape == "twice":
        b = frame_pair(rng, kind, N, **kw)
        frames, tables, frames1, frames2 = [b[0], b[1]], [b[2]] * pairs, (0, 0), (1, 0)
    else:
        b = frame_pair(rng, kind, N, **kw)
        frames, tables = [b[0], b[1]], [b[2]]
        for p in range(1, pairs):                            # further views of the same frame 0: jitter the second frame
            frames.append((b[1] + rng.normal(0, 0.2, b[1].shape)).astype(f32))
            tables.append(b[2])
        frames1, frames2 = (0, 0), (1, 1)
    kps = np.zeros((len(frames), cap), KP)
    kps["x"], kps["y"] = -1e6, -1e6
    n_out = np.zeros(len(frames), np.int32)
    for f, pts in enumerate(frames):
        n_out[f] = len(pts)
        kps["x"][f, :len(pts)], kps["y"][f, :len(pts)] = pts[:, 0], pts[:, 1]
    matches = np.full((pairs, cap), -1, np.int32)
    for p, m in enumerate(tables):
        matches[p, :len(m)] = m
    return dict(kind=kind, kps=kps, n_out=n_out, matches=matches, n_matches=(matches >= 0).sum(axis=1).astype(np.int32),
                rand=rng.integers(0, 2 ** 31, (pairs, iterations, 8)).astype(np.int32), cam=CAM, frames1=frames1, frames2=frames2, pairs=pairs,
                cap=cap, sigma=1.0, iterations=iterations, min_parallax=min_parallax, min_triangulated=min_triangulated, rh_threshold=rh_threshold, prune=1)


def pair_frames(s, p):
    return s["frames1"][0] + p * s["frames1"][1], s["frames2"][0] + p * s["frames2"][1]


def pair_inputs(s, p):
    """what two_view_walk.reconstruct takes for pair p"""
    f1, f2 = pair_frames(s, p)
    n1, n2 = (max(0, min(int(s["n_out"][f]), s["cap"])) for f in (f1, f2))
    pts = lambda f, n: np.stack([s["kps"]["x"][f, :n], s["kps"]["y"][f, :n]], axis=1)
    return pts(f1, n1), pts(f2, n2), s["matches"][p][:n1]


def walk(s, K=None, traces=None, zero_f=False):
    """the walk of every pair of a scene"""
    K = K or TW.Binary32()
    out = []
    for p in range(s["pairs"]):
        k1, k2, m = pair_inputs(s, p)
        tr = {} if traces is not None else None
        out.append(TW.reconstruct(K, k1, k2, m, s["cam"], s["rand"][p], s["sigma"], s["iterations"], s["min_parallax"], s["min_triangulated"],
                                  s["rh_threshold"], trace=tr, zero_f=zero_f))
        if traces is not None:
            traces.append(tr)
    return out


RESULT_DTYPE = np.dtype([("status", "<i4"), ("model", "<i4"), ("n_matches", "<i4"), ("best_it_h", "<i4"), ("best_it_f", "<i4"), ("n_inliers", "<i4"),
                         ("chosen", "<i4"), ("SH", "<f4"), ("SF", "<f4"), ("RH", "<f4"), ("H21", "<f4", 9), ("F21", "<f4", 9), ("R21", "<f4", 9),
                         ("t21", "<f4", 3), ("n_good", "<i4", 8), ("parallax", "<f4", 8)])
POISON_F, POISON_B, POISON_I = -7.0, 0xEE, -559038737


def expected(s, walked=None):
    """the arrays the entry must leave, from the binary32 walk: result rows, p3d, triangulated, matches and n_matches (prune as the scene
    says), on poisoned outputs: entries from n of frame 1 on stay poison"""
    walked = walked or walk(s)
    P, cap = s["pairs"], s["cap"]
    res = np.zeros(P, RESULT_DTYPE)
    p3d = np.full((P, cap, 3), POISON_F, f32)
    tri = np.full((P, cap), POISON_B, np.uint8)
    matches, n_matches = s["matches"].copy(), s["n_matches"].copy()
    for p, w in enumerate(walked):
        for name in RESULT_DTYPE.names:
            res[name][p] = w[name]
        n1 = len(w["triangulated"])
        p3d[p, :n1], tri[p, :n1] = w["p3d"], w["triangulated"]
        if s["prune"] and w["status"] <= TW.ACCEPTED_F:
            matches[p, :n1] = w["pruned"]
            n_matches[p] -= w["n_pruned"]
    return dict(result=res, p3d=p3d, tri=tri, matches=matches, n_matches=n_matches)


def poisoned_outputs(s):
    P, cap = s["pairs"], s["cap"]
    res = np.zeros(P, RESULT_DTYPE)
    res.view(np.int32)[:] = POISON_I
    return dict(result=res, p3d=np.full((P, cap, 3), POISON_F, f32), tri=np.full((P, cap), POISON_B, np.uint8), matches=s["matches"].copy(),
                n_matches=s["n_matches"].copy())


def differences(got, want):
    """the names of the arrays that differ byte for byte"""
    return [k for k in want if np.asarray(got[k]).tobytes() != np.asarray(want[k]).tobytes()]


# The scenes of the CPU and the GPU tests: name -> arguments of make().  N in {7, 8, 63, 64, 65, 96} and one of 300 (capacity 384);
# iterations in {1, 3, 65, 200}; several pairs per call: one pair named twice, one initial frame against many, a stream of pairs.
CASES = {
    "n7_too_few": dict(N=7, iterations=3),
    "n8_sets_are_permutations": dict(N=8, iterations=3, outliers=0.0, min_triangulated=4),
    "n63": dict(N=63, iterations=3, seed=2),
    "plane_n64_it65": dict(kind="plane", N=64, iterations=65, rh_threshold=0.40),
    "n65_it1": dict(N=65, iterations=1, seed=3),
    "general_n96_it200": dict(N=96, iterations=200),
    "plane_n96": dict(kind="plane", N=96, rh_threshold=0.40),
    "plane_n96_seed2": dict(kind="plane", N=96, rh_threshold=0.40, seed=2, iterations=65),
    "frontal_n96": dict(kind="frontal", N=96, rh_threshold=0.40),
    "zero_translation": dict(kind="zero_t", N=96, rh_threshold=0.40),
    "plane_n48_few_points": dict(kind="plane", N=48, rh_threshold=0.40, iterations=65, seed=2),
    "small_baseline_ambiguous": dict(N=96, iterations=200, t=(-0.03, 0.0025, 0.005), yaw=0.002),
    "f_low_parallax": dict(N=96, iterations=65, noise=0.1, seed=3, min_parallax=1e3),
    "h_low_parallax": dict(kind="plane", N=96, rh_threshold=0.40, min_parallax=1e3),
    "h_degenerate_exact_rotation": dict(kind="zero_t", N=96, rh_threshold=0.40, noise=0.0, outliers=0.0),
    "nan_parallax_all_far": dict(N=40, iterations=65, far=40, far_z=3000.0, noise=0.05, min_triangulated=10, outliers=0.0, n_keys=60),
    "far_points": dict(N=96, iterations=65, far=3, far_z=3000.0, noise=0.1, seed=3),
    "n300": dict(N=300, iterations=12, cap=384, n_keys=330),
    "named_twice": dict(N=96, iterations=65, pairs=2, shape="twice"),
    "one_against_many": dict(N=96, iterations=65, pairs=3, shape="fan", seed=2),
    "stream_of_pairs": dict(kind="plane", N=64, iterations=12, pairs=3, rh_threshold=0.40, seed=4),
}
_MADE, _WALKED = {}, {}


def case(name):
    """the scene of CASES[name], made once and left unchanged"""
    if name not in _MADE:
        _MADE[name] = make(**CASES[name])
    return _MADE[name]


def case_expected(name):
    """expected() of a case from the binary32 walk, computed once per process"""
    if name not in _WALKED:
        w = walk(case(name))
        _WALKED[name] = (w, expected(case(name), w))
    return _WALKED[name]


def parallax_pair(seed, rows=240, cols=320, tile=80, shifts=(6, 34)):
    """Two views of a layered scene: the second shows every tile x tile block of the first moved left by the block's own disparity -
    fronto-parallel patches at different depths under a sideways camera step, so no single homography explains the pair."""
    from extractorb_amd import synth
    rng = np.random.default_rng(seed)
    big = synth.textured_frame(seed, rows + 128, cols + 128)
    a = np.ascontiguousarray(big[64:64 + rows, 64:64 + cols])
    b = np.zeros_like(a)
    for y in range(0, rows, tile):
        for x in range(0, cols, tile):
            d = int(rng.integers(shifts[0], shifts[1]))
            b[y:y + tile, x:x + tile] = big[64 + y:64 + y + tile, 64 + x + d:64 + x + d + tile]
    return a, b
