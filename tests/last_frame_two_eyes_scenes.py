"""Scenes of the two-camera frame-to-frame projection search (tests/test_last_frame_two_eyes.py, CPU and GPU): synthesized keypoints and
descriptors, as tests/test_search_projection_two_eyes.py has them.  A 512 x 512 fisheye rig (the TUM-VI shape): KannalaBrandt8 parameters,
a small rotation and a 10 cm baseline in mTrl."""
import functools

import numpy as np

import extractorb_amd as X
import last_frame_two_eyes_walk as W
import oracle_lib as O

f32 = np.float32
ROWS = COLS = 512
BOUNDS = np.array([0, COLS, 0, ROWS], f32)
CAM = np.array([190.97847715128717, 190.9733070521226, 254.93170605935475, 256.8974428996504,
                0.0034823894022493434, 0.0007150348452162257, -0.0020532361418706202, 0.00020293673591811182], f32)
TH, MB = 7.0, 0.1


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
            np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def pose(rx, ry, rz, t):
    return np.concatenate([rot(rx, ry, rz), np.asarray(t, np.float64).reshape(3, 1)], 1).astype(f32)


TRL = pose(0.004, -0.017, 0.01, (-0.1009, 0.0012, 0.0021))       # a non-trivial mTrl
CUR = pose(0.02, -0.03, 0.01, (0.05, -0.02, 0.1))
# last poses against CUR: tlc.z = the current camera centre's depth in the last frame: beyond +mb, beyond -mb, inside
LAST = dict(forward=pose(0.02, -0.03, 0.01, (0.05, -0.02, 0.6)), backward=pose(0.02, -0.03, 0.01, (0.05, -0.02, -0.4)),
            neither=pose(0.025, -0.02, 0.0, (0.07, -0.02, 0.13)))


@functools.lru_cache(None)
def scales():
    return np.asarray(X.compute_tables(1200, 1.2, 8)["scale_factors"], f32)


def keypoints(x, y, octave, angle=0.0):
    k = np.zeros(len(x), O.KEYPOINT_DTYPE)
    k["x"], k["y"], k["octave"], k["angle"] = np.asarray(x, f32), np.asarray(y, f32), octave, angle
    k["size"], k["class_id"] = 31, -1
    return k


def flip(d, rng, n):
    d = d.copy()
    for bit in rng.integers(0, 256, n):
        d[bit >> 3] ^= np.uint8(1 << (bit & 7))
    return d


def eye(k, d, grid):
    return dict(k=k, d=np.asarray(d, np.uint8).reshape(-1, 32), off=grid[0], idx=grid[1])


def make_eyes(kl, dl, kr, dr, bounds=BOUNDS):
    gl, gr = O.assign_features_two_eyes(kl, kr, bounds)
    return eye(kl, dl, gl), eye(kr, dr, gr)


# ---------------------------------------------------------------- front half ----------------------------------------------------------------
def ordered_bits(v):
    """a float's position among the floats: adjacent floats differ by one (+0 and -0 by none)"""
    b = int(np.asarray(v, f32).view(np.int32))
    return b if b >= 0 else -(b & 0x7fffffff)


def _unordered(o):
    return np.array(o if o >= 0 else ((-o) | 0x80000000), np.uint32).view(f32)[()]


def crossing(fn, a, b):
    """adjacent floats (x0, x1) between a and b with fn(x0) != fn(x1), x0 on a's side"""
    lo, hi = ordered_bits(f32(a)), ordered_bits(f32(b))
    want = fn(_unordered(lo))
    assert fn(_unordered(hi)) != want
    while abs(hi - lo) > 1:
        mid = (lo + hi) // 2
        if fn(_unordered(mid)) == want:
            lo = mid
        else:
            hi = mid
    return _unordered(lo), _unordered(hi)


def exit_of(m, world, Tcw=CUR):
    one = dict(k=keypoints([10.0], [10.0], 1), mp=[True], outlier=[False], obs=[True], world=np.asarray([world], f32))
    none = dict(k=keypoints([], [], 0), mp=[], outlier=[], obs=[], world=np.zeros((0, 3), f32))
    return int(W.project_last(m, (one, none), Tcw, LAST["neither"], TRL, CAM, BOUNDS, scales(), MB, TH, False)["exits"][0])


@functools.lru_cache(None)
def crafted_points():
    """(world point, has MapPoint, outlier): every exit, each threshold on the value and one float beside it (adjacent floats of a world
    coordinate on the two sides of the comparison, found with the walk itself under the host libm)"""
    m = W.libm_math()
    Rt = CUR[:, :3].astype(np.float64).T
    centre = -Rt @ CUR[:, 3].astype(np.float64)

    def world_of(xc):                                        # a point with (about) these camera coordinates
        return (Rt @ np.asarray(xc, np.float64) + centre).astype(f32)

    pts = [(world_of((0.3, -0.2, 3.0)), False, False), (world_of((0.3, -0.2, 3.0)), True, True), (world_of((0.1, 0.1, -2.0)), True, False)]
    # the depth test at the sign change of z, and the four bounds: one world coordinate moved between a point inside and one outside, the other two kept
    for inside, outside, axis in (((0.1, 0.1, 1.0), (0.1, 0.1, -1.0), 2), ((0.0, 0.1, 1.0), (-9.0, 0.1, 1.0), 0), ((0.0, 0.1, 1.0), (9.0, 0.1, 1.0), 0),
                                  ((0.1, 0.0, 1.0), (0.1, -9.0, 1.0), 1), ((0.1, 0.0, 1.0), (0.1, 9.0, 1.0), 1)):
        a, b = world_of(inside), world_of(outside)

        def at(c, a=a, axis=axis):
            w = a.copy()
            w[axis] = c
            return w
        c0, c1 = crossing(lambda c: exit_of(m, at(c)) == W.EXIT_REQUEST, a[axis], b[axis])
        pts += [(at(c0), True, False), (at(c1), True, False)]
    pts += [(world_of((0.5, 0.4, 2.0)), True, False), (world_of((-1.5, 0.8, 1.0)), True, False), (world_of((0.0, 0.0, 4.0)), True, False)]
    return pts


def rig_of_points(pts, rng, obs_share=0.7):
    """one eye half of a last rig holding `pts`"""
    n = len(pts)
    return dict(k=keypoints(rng.uniform(20, 490, n), rng.uniform(20, 490, n), rng.integers(0, 8, n), rng.uniform(0, 360, n).astype(f32)),
                mp=[p[1] for p in pts], outlier=[p[2] for p in pts], obs=(rng.random(n) < obs_share).tolist(),
                world=np.array([p[0] for p in pts], f32).reshape(n, 3))


def crafted_front_half(capacity=5):
    """Rig 0 is the current rig; the crafted points, in chunks of `capacity` per eye half, form last rigs under each of the three last poses.
    Returns (rigs = [(left, right)], poses [R, 3, 4], pairs = [(last rig, form)])."""
    rng = np.random.default_rng(5)
    pts = crafted_points()
    order_r = list(reversed(range(len(pts))))                # the right eye half holds the same points in another order
    empty = dict(k=keypoints([], [], 0), mp=[], outlier=[], obs=[], world=np.zeros((0, 3), f32))
    rigs, poses, pairs = [(empty, empty)], [CUR], []
    for form in ("forward", "backward", "neither"):
        for c in range(0, len(pts), capacity):
            left = rig_of_points(pts[c:c + capacity], rng)
            right = rig_of_points([pts[i] for i in order_r[c:c + capacity]], rng)
            pairs.append((len(rigs), form))
            rigs.append((left, right)); poses.append(LAST[form])
    return rigs, np.array(poses, f32), pairs


def full_front_half(capacity=600):
    """one last rig with both eye halves full of random MapPoints around the rig (a third behind it or far off axis)"""
    rng = np.random.default_rng(6)
    def half():
        n = capacity
        w = np.stack([rng.uniform(-8, 8, n), rng.uniform(-8, 8, n), rng.uniform(-2, 8, n)], 1).astype(f32)
        return dict(k=keypoints(rng.uniform(0, 512, n), rng.uniform(0, 512, n), rng.integers(0, 8, n), rng.uniform(0, 360, n).astype(f32)),
                    mp=(rng.random(n) < 0.9).tolist(), outlier=(rng.random(n) < 0.1).tolist(), obs=(rng.random(n) < 0.7).tolist(), world=w)
    empty = dict(k=keypoints([], [], 0), mp=[], outlier=[], obs=[], world=np.zeros((0, 3), f32))
    return [(empty, empty), (half(), half())], np.array([CUR, LAST["neither"]], f32), [(1, "neither")]


def front_half_arrays(rigs, capacity):
    """the per-device-frame arrays of orbx_project_last_frame_two_eyes_device: keypoints, counts, flags, world"""
    F = 2 * len(rigs)
    k = np.zeros((F, capacity), O.KEYPOINT_DTYPE); n = np.zeros(F, np.int32); fl = np.zeros((F, capacity), np.uint8)
    w = np.zeros((F, capacity, 3), f32)
    for r, rig in enumerate(rigs):
        for e, E in enumerate(rig):
            f, m = 2 * r + e, len(E["k"])
            k[f, :m], n[f], w[f, :m] = E["k"], m, E["world"]
            fl[f, :m] = (np.asarray(E["mp"], bool) & ~np.asarray(E["outlier"], bool)).astype(np.uint8) | (np.asarray(E["obs"], bool).astype(np.uint8) << 1)
    return k, n, fl, w


def walk_front_half(m, rigs, poses, last, cur, capacity, mono=False, th=TH, mb=MB):
    """the walk's requests in the device layout [2 * capacity, 2] (request j = eye * capacity + i), and its exits in the same layout (-1: no keypoint)"""
    got = W.project_last(m, rigs[last], poses[cur], poses[last], TRL, CAM, BOUNDS, scales(), mb, th, mono)
    q = np.zeros((2 * capacity, 2), O.PROJ_QUERY_DTYPE); ex = np.full(2 * capacity, -1, np.int32)
    j = got["eye"] * capacity + got["index"]
    q[j] = got["queries"]; ex[j] = got["exits"]
    return q, ex, got["form"]


# ---------------------------------------------------------------- search ----------------------------------------------------------------
def bits(n):
    d = np.zeros(32, np.uint8)
    for b in range(n):
        d[b >> 3] |= np.uint8(1 << (b & 7))
    return d


def request(q, u, v, octave, on=True, obs=True, angle=0.0, th=TH):
    q["u"], q["v"], q["min_level"], q["max_level"], q["angle"] = u, v, octave - 1, octave + 1, angle
    q["radius"] = f32(f32(th) * scales()[octave])
    q["flags"] = (1 if on else 0) | (2 if obs else 0)


def crafted(kl, kr, reqs, occ=None):
    """kl / kr: (x, y, octave, angle, descriptor bits set) per keypoint; reqs: per request ((u, v, octave, obs, angle) or None for L, the same
    for R); request descriptors are all zero, so a keypoint's distance is its number of set bits"""
    def half(ks):
        k = keypoints([a[0] for a in ks], [a[1] for a in ks], [a[2] for a in ks], np.array([a[3] for a in ks], f32))
        return k, np.array([bits(a[4]) for a in ks], np.uint8).reshape(-1, 32)
    (a, da), (b, db) = half(kl), half(kr)
    L, R = make_eyes(a, da, b, db)
    q = np.zeros((len(reqs), 2), O.PROJ_QUERY_DTYPE)
    for j, pair in enumerate(reqs):
        for e, r in enumerate(pair):
            if r is not None:
                request(q[j, e], r[0], r[1], r[2], True, r[3], r[4])
    o = None if occ is None else [np.asarray(occ[0], np.uint8), np.asarray(occ[1], np.uint8)]
    return dict(left=L, right=R, q=q, qd=np.zeros((len(reqs), 32), np.uint8), occ=o, bounds=BOUNDS)


def both(u, v, obs=True, angle=0.0, du=-20.0):
    """a MapPoint seen at (u, v) on the left and 20 px further left on the right, level 1"""
    return ((u, v, 1, obs, angle), (u + du, v, 1, obs, angle))


def crafted_scenes():
    """name -> scene, one per consequence (the tests assert on the walk that each really occurs)"""
    S = {}
    # three requests at one place in the left eye, three keypoints at distances 0, 5, 10: each takes the best one still open; the same in the right eye
    S["closure_chain"] = crafted([(100, 100, 1, 0, 0), (102, 101, 1, 0, 5), (98, 99, 1, 0, 10)],
                                 [(300, 300, 1, 0, 10), (302, 301, 1, 0, 0), (298, 299, 1, 0, 5), (303, 299, 1, 0, 20)],
                                 [((100, 100, 1, True, 0), (300, 300, 1, True, 0))] * 4)
    # a MapPoint without observations does not close: the later one takes the same keypoint, both count
    S["overwritten"] = crafted([(100, 100, 1, 0, 0)], [(80, 100, 1, 0, 0)], [both(100, 100, obs=False), both(100, 100, obs=True), both(100, 100, obs=True)])
    # equal distances: the keypoint met first in the traversal (lower cell column, then row) wins, whatever its index
    S["ties"] = crafted([(108, 100, 1, 0, 3), (99, 112, 1, 0, 3), (99, 100, 1, 0, 3)], [(300, 100, 1, 0, 4), (299, 90, 1, 0, 4)],
                        [((103, 104, 1, True, 0), (300, 96, 1, True, 0))])
    # L's area result is empty (the only left keypoint near is on level 5), R would have matched: nothing is matched
    S["empty_left_suppresses_right"] = crafted([(100, 100, 5, 0, 0), (400, 400, 1, 0, 0)], [(80, 100, 1, 0, 0), (380, 400, 1, 0, 0)],
                                               [both(100, 100), both(400, 400)])
    # L's best is above TH_HIGH: R still runs and matches; so does the R of an L whose only candidate is closed on entry
    S["left_above_th_high"] = crafted([(100, 100, 1, 0, 120), (400, 400, 1, 0, 0)], [(80, 100, 1, 0, 0), (380, 400, 1, 0, 7)],
                                      [both(100, 100), both(400, 400)], occ=([0, 1], [0, 0]))
    # the right window lies wholly off the grid
    S["right_off_grid"] = crafted([(100, 100, 1, 0, 0)], [(80, 100, 1, 0, 0)], [((100, 100, 1, True, 0), (5000, 100, 1, True, 0)),
                                                                                 ((100, 100, 1, True, 0), (80, -900, 1, True, 0))])
    # twenty-six matches in bin 0; left keypoint 0 is pushed to bin 0 by a MapPoint without observations, then to bin 5 (a lone entry, dropped) by
    # the next one: the keypoint is cleared although its bin-0 entry stays
    kl = [(40 + 36 * i, 200, 1, 0, 0) for i in range(13)]
    kr = [(20 + 36 * i, 200, 1, 0, 0) for i in range(13)]
    reqs = [both(40 + 36 * i, 200, obs=(i != 0)) for i in range(13)] + [((40, 200, 1, True, 150.0), None)]
    S["two_bins_one_dropped"] = crafted(kl, kr, reqs)
    # joint maxima {3, 0, 1}; the left eye alone keeps {0, 1, 2}, the right eye alone {3, 4}
    kl, kr, reqs = [], [], []
    for count, b, e in ((10, 0, 0), (5, 1, 0), (4, 2, 0), (3, 3, 0), (8, 3, 1), (2, 4, 1)):
        for _ in range(count):
            i = len(reqs)
            x, y = 30 + 40 * (i % 12), 30 + 40 * (i // 12)
            (kl if e == 0 else kr).append((x, y, 1, 0, 0))
            (kr if e == 0 else kl).append((x, y, 6, 0, 0))      # the other eye has a keypoint there too, on a level the request does not take
            reqs.append(((x, y, 1, True, 30.0 * b), (x, y, 1, True, 30.0 * b)) if e == 0 else (None, (x, y, 1, True, 30.0 * b)))
    S["joint_histogram"] = crafted(kl, kr, reqs)
    return S


def random_requests(rng, nl=300, nr=280, nq=400, occ_share=0.1, obs_share=0.8, clusters=0, bounds=BOUNDS):
    """two eyes of random raw keypoints (some outside the grid) and requests aimed near them, with angles that fill a few rotation bins; clusters > 0: crowded windows"""
    proto = rng.integers(0, 256, (max(clusters, 1), 32), dtype=np.uint8)      # clusters: both eyes draw their descriptors from these

    def half(n):
        if clusters:
            c = np.stack([rng.uniform(60, 450, clusters), rng.uniform(60, 450, clusters)], 1)
            w = rng.integers(0, clusters, n)
            x, y = c[w, 0] + rng.uniform(-9, 9, n), c[w, 1] + rng.uniform(-9, 9, n)
            d = np.stack([flip(proto[a], rng, int(rng.integers(0, 4))) for a in w]) if n else np.zeros((0, 32), np.uint8)
            octv = rng.integers(1, 3, n)
        else:
            x, y = rng.uniform(-6, 518, n), rng.uniform(-6, 518, n)
            d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
            octv = rng.integers(0, 8, n)
        return keypoints(x, y, octv, (rng.integers(0, 4, n) * 30 + rng.uniform(0, 8, n)).astype(f32)), d
    (kl, dl), (kr, dr) = half(nl), half(nr)
    partner = np.full(nl, -1, np.int64)                      # a right keypoint that looks like the left one (any place, any level)
    m = min(nl, nr) * 2 // 3
    if m and not clusters:
        partner[rng.permutation(nl)[:m]] = rng.permutation(nr)[:m]
        for a in np.nonzero(partner >= 0)[0]:
            dr[partner[a]] = flip(dl[a], rng, int(rng.integers(0, 8)))
    L, R = make_eyes(kl, dl, kr, dr, bounds)
    q = np.zeros((nq, 2), O.PROJ_QUERY_DTYPE); qd = np.zeros((nq, 32), np.uint8)
    for j in range(nq):
        obs = rng.random() < obs_share
        src, tl = None, -1
        for e, (k, d, n) in enumerate(((kl, dl, nl), (kr, dr, nr))):
            if n == 0:
                request(q[j, e], rng.uniform(0, 512), rng.uniform(0, 512), 1, rng.random() < 0.9, obs, 0.0)
                continue
            t = int(rng.integers(0, n))
            if e == 1 and nl and tl >= 0 and partner[tl] >= 0:
                t = int(partner[tl])
            if e == 0:
                tl = t
            request(q[j, e], k["x"][t] + rng.uniform(-4, 4), k["y"][t] + rng.uniform(-4, 4), int(k["octave"][t]), rng.random() < 0.9, obs,
                    f32((k["angle"][t] + rng.uniform(0, 8) + rng.choice([0, 30, 60, 90, 150, 240], p=[.6, .15, .1, .08, .04, .03])) % 360))
            if src is None:
                src = d[t]
        qd[j] = flip(src, rng, int(rng.integers(0, 30))) if src is not None else rng.integers(0, 256, 32, dtype=np.uint8)
    if nq > 12:
        qd[5] = qd[4]; q[5] = q[4]                           # exact ties
        q[7, 0]["u"] = -400.0; q[8, 1]["v"] = 5000.0; q[9, 0]["min_level"], q[9, 0]["max_level"] = 3, -1; q[10, 1]["min_level"], q[10, 1]["max_level"] = 0, 2
    occ = [(rng.random(nl) < occ_share).astype(np.uint8), (rng.random(nr) < occ_share).astype(np.uint8)]
    return dict(left=L, right=R, q=q, qd=qd, occ=occ, bounds=bounds)


def walk_search(s, check_orientation=True, occ=True):
    return W.search(s["q"], s["qd"], s["left"], s["right"], s["bounds"], s["occ"] if occ else None, 100, check_orientation)


# ---------------------------------------------------------------- front half + search ----------------------------------------------------------------
def moving_rigs(seed, n_rigs=2, n_points=260, shared=0.5, extra=40):
    """A map of points seen by a rig that moves a little between frames.  Every rig's left eye sees each point, its right eye `shared` of
    them (those MapPoints sit in both eye halves of the last frame) plus points of its own; keypoints = the projections (host libm) plus
    jitter, descriptors = the MapPoint's with a few bits flipped, `extra` unrelated keypoints per eye.  Returns rigs (as the front half takes
    them, with d / mpd = keypoint / MapPoint descriptors) and poses."""
    rng = np.random.default_rng(seed)
    m = W.libm_math()
    th, ps, dp = rng.uniform(0.05, 1.0, n_points), rng.uniform(-np.pi, np.pi, n_points), rng.uniform(2.0, 8.0, n_points)
    world = np.stack([np.sin(th) * np.cos(ps) * dp, np.sin(th) * np.sin(ps) * dp, np.cos(th) * dp], 1).astype(f32)
    mpd = rng.integers(0, 256, (n_points, 32), dtype=np.uint8)
    octv = rng.integers(0, 4, n_points)
    ang = rng.uniform(0, 360, n_points)
    in_right = rng.random(n_points) < shared
    poses = [pose(0.01 * r, -0.008 * r, 0.004 * r, (0.02 * r, -0.01 * r, 0.03 * r)) for r in range(n_rigs)]
    rigs = []
    for r in range(n_rigs):
        halves = []
        for e in (0, 1):
            ids = [i for i in range(n_points) if e == 0 or in_right[i]]
            xs, ys = [], []
            for i in ids:
                xc = poses[r][:, :3].astype(np.float64) @ world[i].astype(np.float64) + poses[r][:, 3]
                if e:
                    xc = TRL[:, :3].astype(np.float64) @ xc + TRL[:, 3]
                u, v = W.kb8_project(m, CAM, xc[0], xc[1], xc[2])
                xs.append(float(u) + rng.uniform(-2, 2)); ys.append(float(v) + rng.uniform(-2, 2))
            n = len(ids) + extra
            k = keypoints(xs + rng.uniform(0, 512, extra).tolist(), ys + rng.uniform(0, 512, extra).tolist(),
                          octv[ids].tolist() + rng.integers(0, 4, extra).tolist(),
                          np.array([(ang[i] + rng.uniform(-6, 6)) % 360 for i in ids] + rng.uniform(0, 360, extra).tolist(), f32))
            d = np.array([flip(mpd[i], rng, int(rng.integers(0, 25))) for i in ids] + [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(extra)], np.uint8)
            has = np.array([rng.random() < 0.92 for _ in ids] + [False] * extra)
            w = np.zeros((n, 3), f32); w[:len(ids)] = world[ids]
            md = np.zeros((n, 32), np.uint8); md[:len(ids)] = mpd[ids]
            halves.append(dict(k=k, d=d, mp=has.tolist(), outlier=(rng.random(n) < 0.05).tolist(), obs=(rng.random(n) < 0.8).tolist(), world=w, mpd=md))
        rigs.append(tuple(halves))
    return rigs, np.array(poses, f32)


def chained_scene(m, rigs, poses, last, cur, capacity):
    """requests of rig `last` under rig `cur`'s pose (the walk's front half, device layout) and rig `cur` as the search scene"""
    q, ex, _ = walk_front_half(m, rigs, poses, last, cur, capacity)
    qd = np.zeros((2 * capacity, 32), np.uint8)
    for e in (0, 1):
        n = len(rigs[last][e]["k"])
        qd[e * capacity:e * capacity + n] = rigs[last][e]["mpd"]
    L, R = make_eyes(rigs[cur][0]["k"], rigs[cur][0]["d"], rigs[cur][1]["k"], rigs[cur][1]["d"])
    return dict(left=L, right=R, q=q, qd=qd, occ=None, bounds=BOUNDS), ex
