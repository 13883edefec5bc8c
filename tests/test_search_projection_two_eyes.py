"""ORBmatcher::SearchByProjection(F, vpMapPoints, th, ...) for two-camera frames (reference src/ORBmatcher.cc:44-213, F.Nleft != -1; caller
Tracking::SearchLocalPoints).  CPU: the checker (tests/two_eyes_walk.py) against the one-eye oracle on its degenerate halves and on crafted
chains, one per consequence of the two-eye form; the C entry's existence and argument checks.  GPU: orbx_search_by_projection_two_eyes_device
against the walk, bit-exact (matches, occupancy, match count)."""
import ctypes as C
import functools

import numpy as np
import pytest

import helpers
import oracle_lib as O
import extractorb_amd as X
import two_eyes_walk as W
from extractorb_amd import synth

ROWS, COLS = 480, 640
BOUNDS = np.array([0, COLS, 0, ROWS], np.float32)
CAP_1200 = 1302                # orbx_max_keypoints() of a 1200-feature extractor (asserted on the GPU)


@functools.lru_cache(None)
def scales():
    """mvScaleFactors of a 1200-feature, 1.2, 8-level extractor (computed on first use: nothing calls the library at import)"""
    return np.asarray(X.compute_tables(1200, 1.2, 8)["scale_factors"], np.float32)


def radius_by_viewing_cos(c):
    return np.float32(2.5) if c > 0.998 else np.float32(4.0)


def lds_bytes(capacity, query_capacity):
    """the bound the header documents: 100 * ((capacity + 3) & ~3) + 8 * query_capacity + 12 392 <= 163 328"""
    return 100 * ((capacity + 3) & ~3) + 8 * query_capacity + 12392


def flip(d, rng, n):
    d = d.copy()
    for bit in rng.integers(0, 256, n):
        d[bit >> 3] ^= np.uint8(1 << (bit & 7))
    return d


def eye(k, d, grid):
    return dict(k=k, d=d, off=grid[0], idx=grid[1])


def keypoints(x, y, octave):
    k = np.zeros(len(x), O.KEYPOINT_DTYPE)
    k["x"], k["y"], k["octave"] = np.asarray(x, np.float32), np.asarray(y, np.float32), octave
    k["size"], k["class_id"], k["angle"] = 31, -1, 0
    return k


def requests(nq):
    return np.zeros((nq, 2), O.PROJ_QUERY_DTYPE)


def set_request(q, u, v, level, radius, on=True, obs=True):
    q["u"], q["v"], q["min_level"], q["max_level"] = u, v, level - 1, level
    q["radius"] = np.float32(radius) * scales()[level]
    q["flags"] = (1 if on else 0) | (2 if obs else 0)


def random_scene(rng, nl=600, nr=560, nq=700, paired=0.6, maps=True, obs=0.85, occ=0.1, th=5.0, crowd=0, bounds=BOUNDS):
    """Two eyes of random raw keypoints (some outside the grid), ~`paired` of the left keypoints with a right partner 5..40 px to the
    left on the same level and consistent pairing maps, MapPoints aimed at a keypoint and its partner.  crowd > 0: that many clusters of
    near-identical keypoints that many MapPoints aim at (long chains)."""
    if crowd:
        centres = np.stack([rng.uniform(60, COLS - 60, crowd), rng.uniform(60, ROWS - 60, crowd)], 1)
        which = rng.integers(0, crowd, nl)
        xl, yl = centres[which, 0] + rng.uniform(-9, 9, nl), centres[which, 1] + rng.uniform(-9, 9, nl)
        oct_l = rng.integers(1, 3, nl)
        proto = rng.integers(0, 256, (crowd, 32), dtype=np.uint8)
        dl = np.stack([flip(proto[w], rng, int(rng.integers(0, 4))) for w in which])
    else:
        xl, yl = rng.uniform(-5, COLS + 5, nl), rng.uniform(-5, ROWS + 5, nl)
        oct_l = rng.integers(0, 8, nl)
        dl = rng.integers(0, 256, (nl, 32), dtype=np.uint8)
    kl = keypoints(xl, yl, oct_l)
    npair = min(int(paired * nl), nr)
    left_of = rng.permutation(nl)[:npair]
    slots = rng.permutation(nr)
    xr, yr = rng.uniform(-5, COLS + 5, nr), rng.uniform(-5, ROWS + 5, nr)
    oct_r = rng.integers(0, 8, nr)
    dr = rng.integers(0, 256, (nr, 32), dtype=np.uint8)
    l2r, r2l = np.full(nl, -1, np.int32), np.full(nr, -1, np.int32)
    for a, li in enumerate(left_of):
        j = int(slots[a])
        xr[j], yr[j] = kl["x"][li] - rng.uniform(5, 40), kl["y"][li] + rng.uniform(-0.5, 0.5)
        oct_r[j] = kl["octave"][li]
        dr[j] = flip(dl[li], rng, int(rng.integers(0, 6)))
        l2r[li], r2l[j] = j, li
    kr = keypoints(xr, yr, oct_r)
    gl, gr = O.assign_features_two_eyes(kl, kr, bounds)
    q = requests(nq)
    qd = np.zeros((nq, 32), np.uint8)
    for i in range(nq):
        t = int(rng.integers(0, nl))
        lvl = int(kl["octave"][t])
        o = rng.random() < obs
        set_request(q[i, 0], kl["x"][t] + rng.uniform(-3, 3), kl["y"][t] + rng.uniform(-3, 3), lvl,
                    radius_by_viewing_cos(rng.uniform(0.99, 1.0)) * np.float32(th), rng.random() < 0.85, o)      # th != 1: r *= th (:69-70)
        j = int(l2r[t]) if l2r[t] >= 0 else int(rng.integers(0, nr))
        lvr = int(kr["octave"][j])
        set_request(q[i, 1], kr["x"][j] + rng.uniform(-3, 3), kr["y"][j] + rng.uniform(-3, 3), lvr,
                    radius_by_viewing_cos(rng.uniform(0.99, 1.0)), rng.random() < 0.7, o)           # no th on the right (:148)
        qd[i] = flip(dl[t], rng, int(rng.integers(0, 40)))
    if nq > 10:                                               # exact ties and requests outside the image
        qd[5] = qd[4]; q[5] = q[4]
        q[7, 0]["u"] = -400.0; q[8, 1]["v"] = 5000.0
    occ = [(rng.random(nl) < occ).astype(np.uint8), (rng.random(nr) < occ).astype(np.uint8)]
    return dict(left=eye(kl, dl, gl), right=eye(kr, dr, gr), q=q, qd=qd, l2r=l2r if maps else None, r2l=r2l if maps else None, occ=occ,
                bounds=bounds)


def walk(s, nnratio=0.8):
    return W.search_two_eyes(s["q"], s["qd"], s["left"], s["right"], s["bounds"], s["l2r"], s["r2l"], s["occ"], nnratio)


# ---------------------------------------------------------------- CPU: the checker ----------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_walk_left_half_equals_the_one_eye_oracle(seed):
    rng = np.random.default_rng(seed)
    s = random_scene(rng, maps=False)
    s["q"][:, 1]["flags"] = 0
    got = walk(s)
    L = s["left"]
    nm, m, o = O.search_by_projection(s["q"][:, 0], s["qd"], L["k"], L["d"], L["off"], L["idx"], s["bounds"], None, s["occ"][0], True, 0.8, False, 100)
    assert got["n"] == nm and got["matches"][0] == m.tolist() and got["occupied"][0] == o.tolist()
    assert got["matches"][1] == [-1] * len(s["right"]["k"]) and got["occupied"][1] == s["occ"][1].tolist()
    assert nm > 100


@pytest.mark.parametrize("seed", [4, 5, 6])
def test_walk_right_half_equals_the_one_eye_oracle(seed):
    rng = np.random.default_rng(seed)
    s = random_scene(rng, maps=False)
    s["q"][:, 0]["flags"] = 0
    got = walk(s)
    R = s["right"]
    nm, m, o = O.search_by_projection(s["q"][:, 1], s["qd"], R["k"], R["d"], R["off"], R["idx"], s["bounds"], None, s["occ"][1], True, 0.8, False, 100)
    assert got["n"] == nm and got["matches"][1] == m.tolist() and got["occupied"][1] == o.tolist()
    assert got["matches"][0] == [-1] * len(s["left"]["k"])
    assert nm > 50


def crafted(kl_xyo, kr_xyo, reqs, l2r=None, r2l=None, occ=None):
    """A hand-built frame pair: keypoints (x, y, octave) per eye, descriptors = base with `dist` bits flipped where the request list asks
    for a distance; reqs: per MapPoint ((u, v, level, on, obs) or None for L, the same for R, descriptor bits flipped per keypoint)."""
    base = np.zeros(32, np.uint8)
    kl = keypoints(*zip(*kl_xyo)) if kl_xyo else keypoints([], [], [])
    kr = keypoints(*zip(*kr_xyo)) if kr_xyo else keypoints([], [], [])
    gl, gr = O.assign_features_two_eyes(kl, kr, BOUNDS)
    dl = np.zeros((len(kl), 32), np.uint8); dr = np.zeros((len(kr), 32), np.uint8)
    for (e, i), nbits in reqs["desc"].items():
        d = base.copy()
        for b in range(nbits):
            d[b >> 3] |= np.uint8(1 << (b & 7))
        (dl if e == 0 else dr)[i] = d
    q = requests(len(reqs["mp"]))
    for i, (a, b) in enumerate(reqs["mp"]):
        for e, r in ((0, a), (1, b)):
            if r is not None:
                u, v, lvl, on, obs = r
                set_request(q[i, e], u, v, lvl, 2.5, on, obs)
    qd = np.zeros((len(q), 32), np.uint8)
    o = None if occ is None else [np.asarray(occ[0], np.uint8), np.asarray(occ[1], np.uint8)]
    return dict(left=eye(kl, dl, gl), right=eye(kr, dr, gr), q=q, qd=qd, bounds=BOUNDS, occ=o,
                l2r=None if l2r is None else np.asarray(l2r, np.int32), r2l=None if r2l is None else np.asarray(r2l, np.int32))


def crafted_scenes():
    """(name, scene, expected n, expected left holders, right holders, left occupancy, right occupancy, reopen writes)"""
    out = []
    # 1. closure crosses eyes: MapPoint 0's L takes L0, its pairing write closes R0, so its own R settles for R1 (distance 10)
    s = crafted([(100, 100, 0)], [(90, 100, 0), (92, 100, 0)],
                dict(desc={(0, 0): 0, (1, 0): 0, (1, 1): 10}, mp=[((100, 100, 0, True, True), (91, 100, 0, True, True))]),
                l2r=[0], r2l=[-1, -1])
    out.append(("pairing_write_closes_own_right", s, 3, [0], [0, 0], [1], [1, 1], 0))
    # 2. reopen: R0 is closed on entry; MapPoint 0 (no observations) takes L0 and its pairing write reopens R0, which MapPoint 1 takes;
    #    the same through a closure by an earlier MapPoint (2 takes R2 and closes it, 3 without observations reopens it, 4 takes it)
    s = crafted([(100, 100, 0), (300, 200, 0)], [(90, 100, 0), (500, 400, 0), (290, 200, 0)],
                dict(desc={(0, 0): 0, (1, 0): 0, (1, 1): 50, (0, 1): 0, (1, 2): 0},
                     mp=[((100, 100, 0, True, False), None), (None, (90, 100, 0, True, True)),
                         (None, (290, 200, 0, True, True)), ((300, 200, 0, True, False), None), (None, (290, 200, 0, True, True))]),
                l2r=[0, 2], r2l=[-1, -1, -1], occ=([0, 0], [1, 0, 0]))
    out.append(("reopen_by_mappoint_without_observations", s, 1 + 1 + 1 + 1 + 1 + 1 + 1, [0, 3], [1, -1, 4], [0, 0], [1, 0, 1], 2))
    # 3. a ratio-rejected L skips its R; an L without candidates or above TH_HIGH does not
    s = crafted([(100, 100, 0), (101, 100, 0), (300, 300, 0)], [(80, 100, 0), (400, 300, 0), (200, 200, 0)],
                dict(desc={(0, 0): 10, (0, 1): 11, (1, 0): 0, (1, 1): 0, (0, 2): 120, (1, 2): 0},
                     mp=[((100, 100, 0, True, True), (80, 100, 0, True, True)),          # 10 > 0.8 * 11: rejected, R0 stays free
                         ((600, 50, 0, True, True), (400, 300, 0, True, True)),          # no candidate on the left: R1 matched
                         ((300, 300, 0, True, True), (200, 200, 0, True, True))]),       # left best 120 > 100: R2 matched
                l2r=[0, 0, -1], r2l=[0, -1, -1])
    out.append(("ratio_rejection_suppresses_right", s, 2, [-1, -1, -1], [-1, 1, 2], [0, 0, 0], [0, 1, 1], 0))
    # 4. a pairing write lands on a right keypoint outside the grid (x = -50): written, never a candidate
    s = crafted([(100, 100, 0)], [(-50, 100, 0), (90, 100, 0)],
                dict(desc={(0, 0): 0, (1, 0): 0, (1, 1): 30}, mp=[((100, 100, 0, True, True), None), (None, (-50, 100, 0, True, True))]),
                l2r=[0], r2l=[-1, -1])
    out.append(("pairing_write_outside_the_grid", s, 2, [0], [0, -1], [1], [1, 0], 0))
    # 5. maps out of range (5, -7, 99) and not inverse of each other; a keypoint written twice holds the LAST writer, both writes count
    s = crafted([(100, 100, 0), (200, 100, 0), (300, 100, 0), (400, 100, 0)], [(290, 100, 0), (190, 100, 0), (90, 100, 0), (390, 100, 0)],
                dict(desc={(0, 0): 0, (0, 1): 0, (0, 2): 0, (0, 3): 0, (1, 0): 0, (1, 1): 0, (1, 2): 0, (1, 3): 0},
                     mp=[((100, 100, 0, True, True), None),                 # L0: l2r = 5 (out of range): one write
                         ((300, 100, 0, True, True), None),                 # L2 and, by l2r, R0 (whose r2l says L1)
                         (None, (190, 100, 0, True, True)),                 # R1: r2l = 99: one write
                         (None, (90, 100, 0, True, True)),                  # R2 and, by r2l, L1 (whose l2r is -7)
                         ((400, 100, 0, True, False), None),                # L3 (no observations) and R3
                         (None, (390, 100, 0, True, True))]),               # R3 is open: taken again, and by r2l L3 again
                l2r=[5, -7, 0, 3], r2l=[1, 99, 1, 3])
    out.append(("maps_out_of_range_and_inconsistent_last_writer", s, 1 + 2 + 1 + 2 + 2 + 2, [0, 3, 1, 5], [1, 2, 3, 5], [1, 1, 1, 1],
                [1, 1, 1, 1], 0))
    return out


@pytest.mark.parametrize("case", range(5))
def test_walk_on_crafted_chains(case):
    name, s, n, ml, mr, ol, orr, reopens = crafted_scenes()[case]
    got = walk(s)
    assert (got["n"], got["matches"][0], got["matches"][1], got["occupied"][0], got["occupied"][1], got["reopens"]) == (n, ml, mr, ol, orr, reopens), name


def test_entry_is_declared_exported_and_rejects_a_null_handle():
    assert "orbx_search_by_projection_two_eyes_device" in X.header_symbols()
    assert "orbx_debug_two_eyes_search_stats" in X.header_symbols()
    L = X.load_library()
    assert hasattr(L, "orbx_search_by_projection_two_eyes_device") and hasattr(L, "orbx_debug_two_eyes_search_stats")
    b = np.array([0, 640, 0, 480], np.float32)
    z = C.c_void_p(16)      # never dereferenced: the handle is checked first
    rc = L.orbx_search_by_projection_two_eyes_device(None, 1, 0, 1, z, z, 0, 1, None, 16, z, z, z, 16, z, z,
                                                     b.ctypes.data_as(C.c_void_p), None, None, None, C.c_float(0.8), 100, z, z)
    assert rc == -2
    assert L.orbx_debug_two_eyes_search_stats(None) == -2
    text = open(X.orbextractor._HEADER).read()
    pos = text.index("int orbx_search_by_projection_two_eyes_device(")
    doc = text[text.rindex("/*", 0, pos):pos]
    assert "ORBX_ERR_UNSUPPORTED" in doc and "WITHOUT th" in doc


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def stats():
    out = (C.c_int * 4)()
    assert X.load_library().orbx_debug_two_eyes_search_stats(out) == 0
    return list(out)


def to_device(scenes, cap, qcap):
    """scenes -> the frame-major arrays of the C entry: frame 2p = left eye of pair p, 2p + 1 = right eye"""
    P = len(scenes)
    k = np.zeros((2 * P, cap), O.KEYPOINT_DTYPE); d = np.zeros((2 * P, cap, 32), np.uint8); n = np.zeros(2 * P, np.int32)
    off = np.zeros((2 * P, 64 * 48 + 1), np.int32); idx = np.zeros((2 * P, cap), np.int32)
    l2r = np.full((2 * P, cap), -1, np.int32); r2l = np.full((2 * P, cap), -1, np.int32)
    q = np.zeros((P, qcap, 2), O.PROJ_QUERY_DTYPE); qd = np.zeros((P, qcap, 32), np.uint8); nq = np.zeros(P, np.int32)
    occ = np.zeros((P, 2, cap), np.uint8)
    for p, s in enumerate(scenes):
        for e, E in enumerate((s["left"], s["right"])):
            f = 2 * p + e
            m = len(E["k"])
            k[f, :m], d[f, :m], n[f], off[f] = E["k"], E["d"], m, E["off"]
            idx[f, :len(E["idx"])] = E["idx"]
            if s["occ"] is not None:
                occ[p, e, :m] = s["occ"][e]
        if s["l2r"] is not None:
            l2r[2 * p, :len(s["l2r"])] = s["l2r"]
        if s["r2l"] is not None:
            r2l[2 * p + 1, :len(s["r2l"])] = s["r2l"]
        q[p, :len(s["q"])] = s["q"]; qd[p, :len(s["q"])] = s["qd"]; nq[p] = len(s["q"])
    maps = scenes[0]["l2r"] is not None
    return dict(k=_dev(k.view(np.uint8)), d=_dev(d), n=_dev(n), off=_dev(off), idx=_dev(idx), l2r=_dev(l2r) if maps else None,
                r2l=_dev(r2l) if maps else None, q=_dev(q.view(np.uint8)), qd=_dev(qd), nq=_dev(nq), occ=_dev(occ))


def run_two_eyes(ex, scenes, cap, qcap, nnratio=0.8):
    import torch
    P = len(scenes)
    dv = to_device(scenes, cap, qcap)
    d_m = torch.full((P, 2, cap), -7, dtype=torch.int32, device="cuda"); d_nm = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                            # torch's copies and fills have landed before the handle's stream runs
    stats()                                             # resets the walk counter
    ex.search_by_projection_two_eyes_device(P, (0, 1), dv["q"], dv["qd"], (0, 1), dv["nq"], qcap, dv["k"], dv["d"], dv["n"], cap, dv["off"],
                                            dv["idx"], scenes[0]["bounds"], dv["l2r"], dv["r2l"], dv["occ"], nnratio, d_m, d_nm)
    ex.synchronize()
    return d_m.cpu().numpy(), dv["occ"].cpu().numpy(), d_nm.cpu().numpy(), stats()


def assert_equal_to_walk(scenes, m, occ, nm, cap):
    walked = 0
    for p, s in enumerate(scenes):
        want = walk(s)
        walked += want["reopens"] > 0
        assert int(nm[p]) == want["n"], "pair %d" % p
        for e, E in enumerate((s["left"], s["right"])):
            n = len(E["k"])
            assert m[p, e, :n].tolist() == want["matches"][e], "pair %d eye %d" % (p, e)
            assert occ[p, e, :n].tolist() == want["occupied"][e], "pair %d eye %d" % (p, e)
            assert (m[p, e, n:] == -1).all()
    return walked


@pytest.mark.gpu
@pytest.mark.parametrize("seed,maps,th", [(11, True, 5.0), (12, False, 10.0), (13, True, 15.0)])
def test_gpu_random_two_eye_scenes_equal_the_walk(seed, maps, th):
    rng = np.random.default_rng(seed)
    ex = X.ORBextractor(1200)
    cap, qcap = ex.capacity, 2048
    assert cap == CAP_1200
    scenes = [random_scene(rng, nl=int(rng.integers(1000, cap + 1)), nr=int(rng.integers(1000, cap + 1)), nq=int(rng.integers(1500, qcap + 1)),
                           maps=maps, th=th) for _ in range(3)]
    m, occ, nm, st = run_two_eyes(ex, scenes, cap, qcap)
    walked = assert_equal_to_walk(scenes, m, occ, nm, cap)
    assert st[2] == walked and st[1] == int(walk(scenes[0])["reopens"] > 0)     # the walk settles exactly the pairs with a reopen
    if not maps:
        assert walked == 0                              # no pairing write, no reopen: the fixed point settles every pair
    assert min(nm) > 300


@pytest.mark.gpu
def test_gpu_reopen_corner_takes_the_walk_and_crowds_take_many_rounds():
    rng = np.random.default_rng(21)
    ex = X.ORBextractor(1200)
    cap, qcap = ex.capacity, 2048
    # pair 0: crowded windows, every MapPoint with observations: long chains, no reopen, settled by the fixed point
    crowd = random_scene(rng, nl=500, nr=480, nq=900, obs=1.0, occ=0.05, crowd=5)
    # pair 1: many MapPoints without observations, much occupancy on entry: pairing writes reopen keypoints
    reopen = random_scene(rng, nl=700, nr=650, nq=1200, obs=0.3, occ=0.3)
    plain = random_scene(rng, nl=900, nr=900, nq=1400, obs=1.0)
    assert walk(crowd)["reopens"] == 0 and walk(reopen)["reopens"] > 0 and walk(plain)["reopens"] == 0
    scenes = [crowd, reopen, plain]
    m, occ, nm, st = run_two_eyes(ex, scenes, cap, qcap)
    assert assert_equal_to_walk(scenes, m, occ, nm, cap) == 1
    assert st[0] > 8 and st[1] == 0 and st[2] == 1
    # the reopen pair alone at pair 0: the readout names the walk for it
    m, occ, nm, st = run_two_eyes(ex, [reopen], cap, qcap)
    assert_equal_to_walk([reopen], m, occ, nm, cap)
    assert st[1] == 1 and st[2] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(5))
def test_gpu_crafted_chains(case):
    name, s, n, ml, mr, ol, orr, reopens = crafted_scenes()[case]
    if s["occ"] is None:
        s["occ"] = [np.zeros(len(s["left"]["k"]), np.uint8), np.zeros(len(s["right"]["k"]), np.uint8)]
    for key, size in (("l2r", len(s["left"]["k"])), ("r2l", len(s["right"]["k"]))):
        if s[key] is None:
            s[key] = np.full(size, -1, np.int32)
    m, occ, nm, st = run_two_eyes(X.ORBextractor(1000), [s], 64, 16)
    assert int(nm[0]) == n, name
    assert m[0, 0, :len(ml)].tolist() == ml and m[0, 1, :len(mr)].tolist() == mr, name
    assert occ[0, 0, :len(ol)].tolist() == ol and occ[0, 1, :len(orr)].tolist() == orr, name
    assert st[1] == int(reopens > 0), name


def _left_half_run(ex, scenes, cap, qcap):
    """the two-eye entry with right requests off and no pairing maps"""
    import torch
    P = len(scenes)
    dv = to_device(scenes, cap, qcap)
    d_m = torch.full((P, 2, cap), -7, dtype=torch.int32, device="cuda"); d_nm = torch.zeros(P, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                            # torch's copies and fills have landed before the handle's stream reads / writes them
    ex.search_by_projection_two_eyes_device(P, (0, 1), dv["q"], dv["qd"], (0, 1), dv["nq"], qcap, dv["k"], dv["d"], dv["n"], cap, dv["off"],
                                            dv["idx"], BOUNDS, None, None, dv["occ"], 0.8, d_m, d_nm)
    ex.synchronize()
    return d_m.cpu().numpy(), dv["occ"].cpu().numpy(), d_nm.cpu().numpy()


def _assert_left_half_is_the_one_eye_oracle(scenes, m, occ, nm):
    for p, s in enumerate(scenes):
        L = s["left"]
        n = len(L["k"])
        onm, om, oo = O.search_by_projection(s["q"][:, 0], s["qd"], L["k"], L["d"], L["off"], L["idx"], s["bounds"], None, s["occ"][0], True, 0.8,
                                             False, 100)
        assert int(nm[p]) == onm and m[p, 0, :n].tolist() == om.tolist() and occ[p, 0, :n].tolist() == oo.tolist(), "pair %d" % p
        assert (m[p, 1] == -1).all() and (m[p, 0, n:] == -1).all()


@pytest.mark.gpu
def test_gpu_left_half_equals_the_one_eye_oracle():
    """Right requests off, no pairing maps: the left half of the two-eye entry is SearchByProjection's one-eye form in ratio mode without
    mvuRight (oracle_lib.search_by_projection, the statement the one-eye entry is checked against) on the raw keypoints and mGrid, output
    for output, in the envelope of the one-eye entry's own tests (capacity 1024, query_capacity 768, up to 768 MapPoints, th = 1 windows)."""
    rng = np.random.default_rng(31)
    ex = X.ORBextractor(1000)
    cap, qcap, P = 1024, 768, 3
    scenes = [random_scene(rng, nl=int(rng.integers(700, 1000)), nr=800, nq=int(rng.integers(500, 769)), maps=False, th=1.0) for _ in range(P)]
    for s in scenes:
        s["q"][:, 1]["flags"] = 0
    m, occ, nm = _left_half_run(ex, scenes, cap, qcap)
    _assert_left_half_is_the_one_eye_oracle(scenes, m, occ, nm)
    assert int(nm.min()) > 200


@pytest.mark.gpu
def test_gpu_left_half_equals_the_one_eye_oracle_on_large_windows():
    """1800 MapPoints with th = 5 windows over 1100 keypoints at the 1200-feature capacity: the same check."""
    rng = np.random.default_rng(31)
    ex = X.ORBextractor(1200)
    cap, qcap, P = ex.capacity, 2048, 3
    scenes = [random_scene(rng, nl=1100, nr=1000, nq=1800, maps=False) for _ in range(P)]
    for s in scenes:
        s["q"][:, 1]["flags"] = 0
    m, occ, nm = _left_half_run(ex, scenes, cap, qcap)
    _assert_left_half_is_the_one_eye_oracle(scenes, m, occ, nm)


@pytest.mark.gpu
def test_gpu_forced_walk_equals_the_fixed_point_and_the_walk():
    rng = np.random.default_rng(41)
    scenes = [random_scene(rng, nl=900, nr=850, nq=1200, th=10.0) for _ in range(2)] + \
             [random_scene(rng, nl=400, nr=380, nq=700, obs=0.5, occ=0.3, crowd=4)]
    cap, qcap = CAP_1200, 2048
    m0, occ0, nm0, st0 = run_two_eyes(X.ORBextractor(1000), scenes, cap, qcap)
    X.debug_set_option("two_eyes_walk", 1)
    ex = X.ORBextractor(1000)
    m1, occ1, nm1, st1 = run_two_eyes(ex, scenes, cap, qcap)
    X.debug_set_option("two_eyes_walk", 0)
    assert st1[1] == 1 and st1[2] == len(scenes)
    assert np.array_equal(m0, m1) and np.array_equal(occ0, occ1) and np.array_equal(nm0, nm1)
    assert_equal_to_walk(scenes, m1, occ1, nm1, cap)


@pytest.mark.gpu
def test_gpu_size_bound_both_sides():
    import torch
    limit = 160 * 1024 - 512
    assert limit == helpers.entry_lds_budget()
    rng = np.random.default_rng(51)
    ex = X.ORBextractor(1000)
    s = random_scene(rng, nl=500, nr=450, nq=600)
    for qcap in (2048, 600):
        cap = max(c for c in range(1, 4000) if lds_bytes(c, qcap) <= limit)
        assert lds_bytes(cap + 1, qcap) > limit
        m, occ, nm, _ = run_two_eyes(ex, [s], cap, qcap)             # the largest accepted size runs
        assert_equal_to_walk([s], m, occ, nm, cap)
        dv = to_device([s], cap + 1, qcap)
        d_m = torch.zeros((1, 2, cap + 1), dtype=torch.int32, device="cuda"); d_nm = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        with pytest.raises(X.OrbxError) as e:                           # the first refused one
            ex.search_by_projection_two_eyes_device(1, (0, 1), dv["q"], dv["qd"], (0, 1), dv["nq"], qcap, dv["k"], dv["d"], dv["n"], cap + 1,
                                                    dv["off"], dv["idx"], BOUNDS, None, None, dv["occ"], 0.8, d_m, d_nm)
        assert e.value.code == -8
    assert max(c for c in range(1, 4000) if lds_bytes(c, 2048) <= limit) >= CAP_1200     # the required envelope
    qmax = max(q for q in range(1, 5000) if lds_bytes(CAP_1200, q) <= limit)
    assert qmax >= 2048
    m, occ, nm, _ = run_two_eyes(ex, [s], CAP_1200, qmax)
    assert_equal_to_walk([s], m, occ, nm, CAP_1200)
    dv = to_device([s], CAP_1200, qmax + 1)
    d_m = torch.zeros((1, 2, CAP_1200), dtype=torch.int32, device="cuda"); d_nm = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    with pytest.raises(X.OrbxError) as e:
        ex.search_by_projection_two_eyes_device(1, (0, 1), dv["q"], dv["qd"], (0, 1), dv["nq"], qmax + 1, dv["k"], dv["d"], dv["n"], CAP_1200,
                                                dv["off"], dv["idx"], BOUNDS, None, None, dv["occ"], 0.8, d_m, d_nm)
    assert e.value.code == -8


@pytest.mark.gpu
def test_gpu_argument_errors_are_rejected_before_any_launch():
    import torch
    ex = X.ORBextractor(1000)
    z = torch.zeros(4096, dtype=torch.int32, device="cuda")
    nm = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    good = dict(n_pairs=1, pairs=(0, 1), d_queries=z, d_query_desc=z, desc_blocks=(0, 1), d_n_queries=None, query_capacity=16, d_kps=z,
                d_desc=z, d_n=z, capacity=16, d_grid_off=z, d_grid_idx=z, bounds=BOUNDS, d_left_to_right=None, d_right_to_left=None,
                d_occupied=None, nnratio=0.8, d_matches=z, d_n_matches=nm, max_distance=100)
    bad = [dict(n_pairs=0), dict(pairs=(-1, 1)), dict(pairs=(0, -1)), dict(desc_blocks=(-1, 1)), dict(desc_blocks=(0, -2)),
           dict(capacity=0), dict(query_capacity=0), dict(max_distance=-1), dict(bounds=np.array([10, 10, 0, 480], np.float32)),
           dict(bounds=np.array([0, 640, 5, 1], np.float32)), dict(d_queries=None), dict(d_query_desc=None), dict(d_kps=None), dict(d_desc=None),
           dict(d_n=None), dict(d_grid_off=None), dict(d_grid_idx=None), dict(d_matches=None), dict(d_n_matches=None)]
    for change in bad:
        with pytest.raises(X.OrbxError) as e:
            ex.search_by_projection_two_eyes_device(**dict(good, **change))
        assert e.value.code == -2, change
    with pytest.raises(X.OrbxError) as e:
        ex.search_by_projection_two_eyes_device(**dict(good, capacity=40000))
    assert e.value.code == -8
    ex.synchronize()
    assert (nm == -7).all()                             # nothing ran


@pytest.mark.gpu
def test_gpu_pipeline_on_synthetic_stereo_pairs():
    """extract_batch_device -> frame_finish_two_eyes_device (bounds that leave keypoints outside the grid) -> requests from a synthetic map
    (each MapPoint seen by the left keypoint it comes from and, 12 px to the left, by the right eye) -> the two-eye search, against the walk."""
    import torch
    P, nf, disp = 2, 1200, 12
    big = synth.textured_frame(7, ROWS + 64, COLS + 64)
    fr = np.zeros((2 * P, ROWS, COLS), np.uint8)
    for p in range(P):
        fr[2 * p] = big[32 + 3 * p:32 + 3 * p + ROWS, 32:32 + COLS]
        fr[2 * p + 1] = big[32 + 3 * p:32 + 3 * p + ROWS, 32 + disp:32 + disp + COLS]      # right eye: content 12 px further left
    ex = X.ORBextractor(nf, max_batch=2 * P)
    cap = ex.capacity
    ex.set_stream(torch.cuda.current_stream().cuda_stream)
    B = 2 * P
    d_k = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda"); d_d = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda"); d_mo = torch.zeros(B, dtype=torch.int32, device="cuda")
    ex.extract_batch_device(_dev(fr), B, ROWS, COLS, d_k, d_d, d_n, d_mo, cap, lapping=(0, 0))
    cam = X.camera(fx=500.0, fy=500.0, cx=320.0, cy=240.0)
    bounds = np.array([40, 600, 30, 450], np.float32)
    d_un = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda")
    d_off = torch.zeros((B, 64 * 48 + 1), dtype=torch.int32, device="cuda"); d_idx = torch.zeros((B, cap), dtype=torch.int32, device="cuda")
    d_nin = torch.zeros(B, dtype=torch.int32, device="cuda")
    ex.frame_finish_two_eyes_device(P, d_k, d_n, cap, cam, bounds, d_un, d_off, d_idx, d_nin)
    ex.synchronize()
    K = d_k.cpu().numpy().view(O.KEYPOINT_DTYPE).reshape(B, cap); D = d_d.cpu().numpy(); N = d_n.cpu().numpy()
    OFF = d_off.cpu().numpy(); IDX = d_idx.cpu().numpy(); NIN = d_nin.cpu().numpy()
    rng = np.random.default_rng(61)
    scenes = []
    for p in range(P):
        kl, kr = K[2 * p, :N[2 * p]].copy(), K[2 * p + 1, :N[2 * p + 1]].copy()
        gl, gr = O.assign_features_two_eyes(kl, kr, bounds)
        assert np.array_equal(OFF[2 * p], gl[0]) and np.array_equal(IDX[2 * p, :NIN[2 * p]], gl[1])
        assert np.array_equal(OFF[2 * p + 1], gr[0]) and np.array_equal(IDX[2 * p + 1, :NIN[2 * p + 1]], gr[1])
        assert NIN[2 * p] < N[2 * p] and NIN[2 * p + 1] < N[2 * p + 1]        # keypoints outside the grid in both eyes
        # the pairing maps (ComputeStereoFishEyeMatches' role): the nearest right keypoint on the same level 12 px to the left, mutual
        l2r, r2l = np.full(len(kl), -1, np.int32), np.full(len(kr), -1, np.int32)
        for i in range(len(kl)):
            dx = np.abs(kr["x"] - (kl["x"][i] - disp)) + np.abs(kr["y"] - kl["y"][i])
            dx[kr["octave"] != kl["octave"][i]] = 1e9
            j = int(np.argmin(dx)) if len(kr) else -1
            if j >= 0 and dx[j] < 2.0 and r2l[j] < 0:
                l2r[i], r2l[j] = j, i
        assert (l2r >= 0).mean() > 0.3
        nq = min(2048, len(kl))
        mps = rng.permutation(len(kl))[:nq]
        q = requests(nq); qd = np.zeros((nq, 32), np.uint8)
        for a, i in enumerate(mps):
            lvl = int(kl["octave"][i]); obs = rng.random() < 0.9
            set_request(q[a, 0], kl["x"][i] + rng.uniform(-2, 2), kl["y"][i] + rng.uniform(-2, 2), lvl,
                        radius_by_viewing_cos(rng.uniform(0.99, 1.0)) * np.float32(5.0), True, obs)
            set_request(q[a, 1], kl["x"][i] - disp + rng.uniform(-2, 2), kl["y"][i] + rng.uniform(-2, 2), lvl,
                        radius_by_viewing_cos(rng.uniform(0.99, 1.0)), rng.random() < 0.8, obs)
            qd[a] = flip(D[2 * p, i], rng, int(rng.integers(0, 20)))
        scenes.append(dict(left=eye(kl, D[2 * p, :len(kl)], gl), right=eye(kr, D[2 * p + 1, :len(kr)], gr), q=q, qd=qd, l2r=l2r, r2l=r2l,
                           occ=[np.zeros(len(kl), np.uint8), np.zeros(len(kr), np.uint8)], bounds=bounds))
    qcap = 2048
    qa = np.zeros((P, qcap, 2), O.PROJ_QUERY_DTYPE); qda = np.zeros((P, qcap, 32), np.uint8); nqa = np.zeros(P, np.int32)
    l2ra = np.full((B, cap), -1, np.int32); r2la = np.full((B, cap), -1, np.int32)
    for p, s in enumerate(scenes):
        qa[p, :len(s["q"])] = s["q"]; qda[p, :len(s["q"])] = s["qd"]; nqa[p] = len(s["q"])
        l2ra[2 * p, :len(s["l2r"])] = s["l2r"]; r2la[2 * p + 1, :len(s["r2l"])] = s["r2l"]
    d_occ = torch.zeros((P, 2, cap), dtype=torch.uint8, device="cuda")
    d_m = torch.full((P, 2, cap), -7, dtype=torch.int32, device="cuda"); d_nm = torch.zeros(P, dtype=torch.int32, device="cuda")
    ex.search_by_projection_two_eyes_device(P, (0, 1), _dev(qa.view(np.uint8)), _dev(qda), (0, 1), _dev(nqa), qcap, d_k, d_d, d_n, cap, d_off,
                                            d_idx, bounds, _dev(l2ra), _dev(r2la), d_occ, 0.8, d_m, d_nm)
    ex.synchronize()
    assert_equal_to_walk(scenes, d_m.cpu().numpy(), d_occ.cpu().numpy(), d_nm.cpu().numpy(), cap)
    assert int(d_nm.cpu().min()) > 300
