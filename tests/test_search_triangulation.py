"""The mapping thread's matcher: ORBmatcher::SearchForTriangulation(pKF1, pKF2, F12, vMatchedPairs, bOnlyStereo, bCoarse) (reference
src/ORBmatcher.cc:965-1206; LocalMapping::CreateNewMapPoints, src/LocalMapping.cc:456-463) for one-camera keyframes with the Pinhole model.
CPU: the sequential walk (tests/triangulation_walk.py) against an independent per-feature numpy statement (masks, last argmin) on every
scene and option set the GPU tests use: vbMatched2 is never set in this function, so every keyframe-1 feature is a search of its own, and
that equality is what licenses the kernel's parallel form.  The scenes carry real geometry and are asserted to reach every filter.
GPU: orbx_search_for_triangulation_device against the walk, exact: vMatches12 in all its capacity entries, vMatchedPairs, the count."""
import ctypes as C

import numpy as np
import pytest

import helpers
import extractorb_amd as X
from extractorb_amd import synth
from test_bow import make_vocab
from triangulation_walk import POPCOUNT, epipolar_constrain, search_for_triangulation, three_maxima

f32 = np.float32
TABLES = X.compute_tables(1200, 1.2, 8)
SF, SIG2 = TABLES["scale_factors"], TABLES["level_sigma2"]
CAP_1200 = 1302                # orbx_max_keypoints() of a 1200-feature extractor (asserted on the GPU)
LDS_LIMIT = 160 * 1024 - 512
K = np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1]])
POISON = -7


def lds_bytes(capacity, staged=False):
    """the bound the header documents: 28 * ((capacity + 15) & ~15) + 64 <= 163 328 (60 per slot with keyframe 2's descriptors staged)"""
    return (60 if staged else 28) * ((capacity + 15) & ~15) + 64


# ---------------------------------------------------------------- scenes ----------------------------------------------------------------
def rot_y(a):
    return np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])


def world(seed, n=1200, n_nodes=100):
    """n 3-D points in front of the cameras, each with a descriptor, a vocabulary node, an orientation and a pyramid level"""
    rng = np.random.default_rng(seed)
    return dict(rng=rng, n=n, n_nodes=n_nodes, X=np.c_[rng.uniform(-4, 4, n), rng.uniform(-3, 3, n), rng.uniform(4, 12, n)],
                desc=rng.integers(0, 256, (n, 32), dtype=np.uint8), node=rng.integers(1, n_nodes + 1, n).astype(np.uint32) * 7,
                angle=rng.uniform(0, 360, n), octave=rng.integers(0, 8, n))


def fundamental(pose1, pose2):
    """F12 = K1^-T [t12]x R12 K2^-1 with R12 = R1w R2w^T, t12 = -R1w R2w^T t2w + t1w (the one-camera branch, :990-993, and Pinhole.cpp:124-127)
    and the epipole = keyframe 1's centre projected into keyframe 2 (:972-977), in float64, cast to binary32"""
    (R1, t1), (R2, t2) = pose1, pose2
    R12 = R1 @ R2.T
    t12 = -R1 @ R2.T @ t2 + t1
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    F12 = np.linalg.inv(K.T) @ tx @ R12 @ np.linalg.inv(K)
    C2 = R2 @ (-R1.T @ t1) + t2
    ep = np.array([K[0, 0] * C2[0] / C2[2] + K[0, 2], K[1, 1] * C2[1] / C2[2] + K[1, 2]])
    return F12.astype(np.float32), ep.astype(np.float32)


def view(w, pose, noise_px, turn, off_line=0.0, around=None, flips=20, n_seen=None):
    """One keyframe: the world's points through `pose` with pixel noise scaled by the octave, in an order of its own, descriptors with up
    to `flips` flipped bits, 15 % of the features in other nodes, 5 % in no node, 40 % holding MapPoints, 30 % with mvuRight >= 0;
    off_line: share pushed off its place (and so off its epipolar line); around: an epipole some features are planted around."""
    rng, n = w["rng"], w["n"]
    R, t = pose
    Xc = w["X"] @ R.T + t
    pt = np.c_[K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2], K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2]]
    octave = np.clip(w["octave"] + rng.integers(-1, 2, n), 0, 7)
    pt = pt + rng.normal(0, noise_px, (n, 2)) * SF[octave][:, None]
    off = rng.random(n) < off_line
    pt[off] += rng.normal(0, 12, (int(off.sum()), 2))
    if around is not None:
        near = rng.random(n) < 0.05
        pt[near] = around + rng.normal(0, 4, (int(near.sum()), 2))
    desc = w["desc"].copy()
    for i in range(n):
        for b in rng.integers(0, 256, rng.integers(0, flips + 1)):
            desc[i, b >> 3] ^= np.uint8(1 << (b & 7))
    node = w["node"].copy()
    wrong = rng.random(n) < 0.15
    node[wrong] = rng.integers(1, w["n_nodes"] + 40, int(wrong.sum())).astype(np.uint32) * 7
    angle = np.where(rng.random(n) < 0.8, np.mod(w["angle"] + turn + rng.normal(0, 3, n), 360), rng.uniform(0, 360, n)).astype(np.float32)
    angle[angle >= 360] = 0
    order = rng.permutation(n)[:n if n_seen is None else n_seen]
    m = len(order)
    kps = np.zeros(m, X.KEYPOINT_DTYPE)
    kps["x"], kps["y"], kps["angle"], kps["octave"] = pt[order, 0], pt[order, 1], angle[order], octave[order]
    kps["size"], kps["class_id"] = 31, -1
    node = node[order]
    idx = np.nonzero(rng.random(m) > 0.05)[0]
    o = np.lexsort((idx, node[idx]))
    mp = (rng.random(m) < 0.4).astype(np.uint8) | (rng.integers(0, 2, m).astype(np.uint8) << 1)      # bit 1 is noise
    ur = np.where(rng.random(m) < 0.3, rng.uniform(0, 600, m), -1.0).astype(np.float32)
    return dict(kps=kps, desc=np.ascontiguousarray(desc[order]), fv=(node[idx][o].astype(np.uint32), idx[o].astype(np.uint32)), mp=mp, ur=ur)


SIDE = ((rot_y(0.0), np.zeros(3)), (rot_y(0.03), np.array([-0.5, 0.03, 0.02])))
FORWARD = ((rot_y(0.0), np.zeros(3)), (rot_y(0.01), np.array([0.05, 0.02, -0.6])))


def pair_of(kf1, kf2, F12, ep):
    return dict(kf1=kf1, kf2=kf2, F=F12, ep=ep)


def scene(kind, seed=7, n=1200, n_nodes=100):
    """side: sideways motion; forward: forward motion, the epipole inside the image and features planted around it; twins: the side scene
    with, inside common nodes, pairs of keyframe-1 features and pairs of keyframe-2 features made identical in descriptor AND place"""
    w = world(seed, n, n_nodes)
    poses = FORWARD if kind == "forward" else SIDE
    F12, ep = fundamental(*poses)
    kf1 = view(w, poses[0], 0.3, 0.0)
    kf2 = view(w, poses[1], 0.5, -12.0, off_line=0.25, around=ep if kind == "forward" else None)
    if kind == "twins":
        rng = np.random.default_rng(seed + 1000)
        l1, l2 = as_map(kf1["fv"]), as_map(kf2["fv"])
        for node in sorted(set(l1) & set(l2)):
            for kf, lst in ((kf1, l1[node]), (kf2, l2[node])):
                if len(lst) >= 2 and rng.random() < 0.5:
                    for key in ("kps", "desc", "ur"):
                        kf[key][lst[-1]] = kf[key][lst[0]]
                    kf["mp"][lst[-1]] = kf["mp"][lst[0]] = 0
    return pair_of(kf1, kf2, F12, ep)


def empty_keyframe():
    z = np.zeros(0, np.uint32)
    return dict(kps=np.zeros(0, X.KEYPOINT_DTYPE), desc=np.zeros((0, 32), np.uint8), fv=(z, z), mp=np.zeros(0, np.uint8), ur=np.zeros(0, np.float32))


def degenerate(kind):
    s = scene("side", 11, 300, 20)
    if kind == "empty_kf1":
        s["kf1"] = empty_keyframe()
    elif kind == "empty_kf2":
        s["kf2"] = empty_keyframe()
    elif kind == "no_common_node":
        s["kf2"]["fv"] = (s["kf2"]["fv"][0] + np.uint32(3), s["kf2"]["fv"][1])      # node ids are multiples of 7
    return s


def as_map(fv):
    out = {}
    for node, i in zip(fv[0].tolist(), fv[1].tolist()):
        out.setdefault(node, []).append(i)
    return out


STANDARD = ("side", "forward", "twins")
DEGENERATE = ("empty_kf1", "empty_kf2", "no_common_node")
OPTIONS = [dict(), dict(only_stereo=True), dict(coarse=True), dict(check_orientation=False), dict(th_low=0), dict(th_low=256),
           dict(only_stereo=True, coarse=True, check_orientation=False)]
_scenes = {}


def get(kind):
    if kind not in _scenes:
        _scenes[kind] = degenerate(kind) if kind in DEGENERATE else scene(kind)
    return _scenes[kind]


_walks = {}


def walk(s, use_u_right=True, **opt):
    key = (id(s), use_u_right, tuple(sorted(opt.items())))
    if key not in _walks:
        a, b = s["kf1"], s["kf2"]
        _walks[key] = (s, search_for_triangulation(a["fv"], b["fv"], a["mp"], b["mp"], a["kps"], b["kps"], a["ur"] if use_u_right else None,
                                                   b["ur"] if use_u_right else None, a["desc"], b["desc"], s["F"], s["ep"], SF, SIG2, **opt))
    return _walks[key][1]


def brute(s, only_stereo=False, coarse=False, th_low=50, check_orientation=True):
    """Independent statement: per keyframe-1 feature, masks over its node's candidates and the LAST smallest distance"""
    a, b = s["kf1"], s["kf2"]
    l1, l2 = as_map(a["fv"]), as_map(b["fv"])
    m12 = np.full(len(a["desc"]), -1)
    p2 = np.c_[b["kps"]["x"], b["kps"]["y"]].astype(np.float32).reshape(-1, 2)
    for node in set(l1) & set(l2):
        c2 = np.array(l2[node])
        ok2 = (b["mp"][c2] & 1) == 0
        if only_stereo:
            ok2 &= b["ur"][c2] >= 0                      # (mvuRight >= 0 is the test: a NaN is not stereo)
        e = s["ep"][None] - p2[c2]
        near = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) < f32(100) * SF[b["kps"]["octave"][c2]]
        for i1 in l1[node]:
            if a["mp"][i1] & 1 or (only_stereo and not a["ur"][i1] >= 0):
                continue
            dist = POPCOUNT[a["desc"][i1][None] ^ b["desc"][c2]].sum(1)
            ok = ok2 & (dist <= th_low)
            if not a["ur"][i1] >= 0:
                ok &= ~(near & ~(b["ur"][c2] >= 0))
            if not coarse:
                ok &= np.array([bool(ok[j]) and epipolar_constrain(a["kps"]["x"][i1], a["kps"]["y"][i1], p2[i2, 0], p2[i2, 1], s["F"],
                                                                   SIG2[b["kps"]["octave"][i2]]) for j, i2 in enumerate(c2)], bool)
            if ok.any():
                d = np.where(ok, dist, 999)
                m12[i1] = c2[len(d) - 1 - int(np.argmin(d[::-1]))]
    if check_orientation:
        idx = np.nonzero(m12 >= 0)[0]
        rot = a["kps"]["angle"][idx] - b["kps"]["angle"][m12[idx]]
        rot = np.where(rot < 0, rot + f32(360), rot).astype(np.float32)
        bins = np.floor((rot * (f32(1) / f32(30))).astype(np.float64) + 0.5).astype(int) % 30
        keep = three_maxima(np.bincount(bins, minlength=30).tolist())
        m12[idx[~np.isin(bins, [k for k in keep if k >= 0])]] = -1
    return int((m12 >= 0).sum()), m12.tolist()


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
@pytest.mark.parametrize("kind", STANDARD + DEGENERATE)
def test_walk_equals_the_independent_per_feature_statement(kind):
    s = get(kind)
    for opt in OPTIONS:
        w = walk(s, **opt)
        n, m12 = brute(s, **opt)
        assert w["n"] == n and w["matches12"] == m12, opt
        assert w["n"] == len(w["pairs"]) == sum(m >= 0 for m in w["matches12"])
        assert w["pairs"] == sorted(w["pairs"]) and all(w["matches12"][i] == m for i, m in w["pairs"])


def test_scenes_reach_every_filter_and_both_tie_cases():
    """the condition of the GPU tests, asserted on exactly their scenes and options"""
    base = {k: walk(get(k)) for k in STANDARD}
    for k, w in base.items():
        assert w["n"] > 100, (k, w["n"])
    for counter in ("mp", "disc", "epi", "equal", "shared", "removals"):
        assert any(w[counter] > 0 for w in base.values()), counter
    assert base["forward"]["disc"] > 0 and base["twins"]["equal"] > 0 and base["twins"]["shared"] > 0
    assert any(walk(get(k), only_stereo=True)["stereo"] > 0 for k in STANDARD)
    assert any(walk(get(k), coarse=True)["matches12"] != base[k]["matches12"] for k in STANDARD)
    assert any(walk(get(k), check_orientation=False)["n"] > base[k]["n"] for k in STANDARD)
    assert all(walk(get(k), th_low=0)["n"] < base[k]["n"] and walk(get(k), th_low=256)["matches12"] != base[k]["matches12"] for k in STANDARD)
    assert any(walk(get(k), use_u_right=False)["matches12"] != base[k]["matches12"] for k in STANDARD)


def test_neighbourhood_and_capacity_scenes_match_enough():
    """the counts the GPU tests of kf1_step = 0, kf2_step = 0 and of the capacities assert, on their scenes"""
    for s in neighbourhood(21, 9, True) + neighbourhood(22, 5, False):
        assert walk(s)["n"] > 100
    for n in (1000, 1200, 2000):
        for s in capacity_scenes(n):
            assert walk(s)["n"] > 100


def test_degenerate_scenes_match_nothing():
    for k in DEGENERATE:
        for opt in OPTIONS:
            w = walk(get(k), **opt)
            assert w["n"] == 0 and w["pairs"] == [] and all(m == -1 for m in w["matches12"])


def test_epipolar_test_rounds_as_binary32_and_compares_in_double():
    F12, _ = fundamental(*SIDE)
    rng = np.random.default_rng(3)
    agree = differ = 0
    for _ in range(400):
        x1, y1, x2, y2 = rng.uniform(0, 640, 4).astype(np.float32)
        a, b, c = (np.array([x1, y1, 1.0]) @ F12.astype(np.float64))
        d64 = (a * x2 + b * y2 + c) ** 2 / (a * a + b * b)
        got = epipolar_constrain(x1, y1, x2, y2, F12, SIG2[2])
        agree += got == (d64 < 3.84 * float(SIG2[2])); differ += 1
    assert agree >= differ - 2                       # the float64 evaluation differs only at the threshold
    assert not epipolar_constrain(1.0, 1.0, 5.0, 5.0, np.zeros((3, 3), np.float32), 1.0)      # den == 0 -> false


def test_entry_is_declared_in_the_header():
    assert "orbx_search_for_triangulation_device" in X.header_symbols()
    text = open(X.orbextractor._HEADER).read()
    pos = text.index("int orbx_search_for_triangulation_device(")
    doc = text[text.rindex("/*", 0, pos):pos]
    assert "ORBX_ERR_UNSUPPORTED" in doc and "28 * ((capacity + 15) & ~15) + 64" in doc and "60 * ((capacity + 15) & ~15) + 64" in doc
    assert "vbMatched2" in doc and "LAST" in doc and "CLAMPED" in doc


def test_entry_is_exported_and_rejects_a_null_handle():
    L = X.load_library()
    assert hasattr(L, "orbx_search_for_triangulation_device")
    z = C.c_void_p(16)      # never dereferenced: the handle is checked first
    assert L.orbx_search_for_triangulation_device(None, 1, 0, 1, 1, 1, z, z, z, z, z, z, z, z, z, 16, z, z, 0, 0, 50, 1, z, z, z) == -2


def test_python_method_exists():
    assert callable(getattr(X.ORBextractor, "search_for_triangulation_device", None))


def test_lds_formula_admits_the_capacities_of_the_usual_extractors():
    # orbx_max_keypoints() = sum over the levels of max(quota + 3, 4 * nIni) + 8 * nlevels: about nfeatures + 100 at 640 x 480 (1302 for 1200
    # features); what the handles of 1000-, 1200- and 2000-feature extractors report is asserted against the formula on the GPU
    assert LDS_LIMIT == helpers.entry_lds_budget()
    for cap in (1024, 1100, CAP_1200, 2024, 2200, 4080):
        assert lds_bytes(cap) <= LDS_LIMIT
    for cap in (1024, 1100, CAP_1200, 2024, 2200):
        assert lds_bytes(cap, staged=True) <= LDS_LIMIT
    largest = max(c for c in range(1, 9000) if lds_bytes(c) <= LDS_LIMIT)
    assert largest == 5824 and max(c for c in range(1, 9000) if lds_bytes(c, True) <= LDS_LIMIT) == 2720


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda()


def pack(keyframes, cap):
    """the batch: frame f = keyframes[f]"""
    B = len(keyframes)
    desc = np.zeros((B, cap, 32), np.uint8); kps = np.zeros((B, cap), X.KEYPOINT_DTYPE); ur = np.full((B, cap), -1, np.float32)
    fn = np.zeros((B, cap), np.uint32); fi = np.zeros((B, cap), np.uint32)
    nfeat = np.zeros(B, np.int32); nout = np.zeros(B, np.int32)
    for f, k in enumerate(keyframes):
        n = len(k["desc"])
        desc[f, :n] = k["desc"]; kps[f, :n] = k["kps"]; ur[f, :n] = k["ur"]; nout[f] = n
        fn[f, :len(k["fv"][0])] = k["fv"][0]; fi[f, :len(k["fv"][1])] = k["fv"][1]; nfeat[f] = len(k["fv"][0])
    return dict(fn=_dev(fn.view(np.int32)), fi=_dev(fi.view(np.int32)), nfeat=_dev(nfeat), kps=_dev(kps), ur=_dev(ur), desc=_dev(desc), nout=_dev(nout))


def run(ex, dv, searches, kf1, kf2, cap, use_u_right=True, **opt):
    """searches: per pair the scene dict (its flags, F12 and epipole are uploaded per pair)"""
    import torch
    n = len(searches)
    fl1 = np.zeros((n, cap), np.uint8); fl2 = np.zeros((n, cap), np.uint8)
    for p, s in enumerate(searches):
        fl1[p, :len(s["kf1"]["mp"])] = s["kf1"]["mp"]; fl2[p, :len(s["kf2"]["mp"])] = s["kf2"]["mp"]
    d_f = _dev(np.stack([s["F"].reshape(9) for s in searches]).astype(np.float32)); d_e = _dev(np.stack([s["ep"] for s in searches]).astype(np.float32))
    d_m = torch.full((n, cap), POISON, dtype=torch.int32, device="cuda"); d_p = torch.full((n, cap, 2), POISON, dtype=torch.int32, device="cuda")
    d_nm = torch.full((n,), POISON, dtype=torch.int32, device="cuda")
    d_fl1, d_fl2 = _dev(fl1), _dev(fl2)
    torch.cuda.synchronize()                            # torch's copies and fills have landed before the handle's stream runs
    ex.search_for_triangulation_device(n, kf1, kf2, dv["fn"], dv["fi"], dv["nfeat"], d_fl1, d_fl2, dv["kps"], dv["ur"] if use_u_right else None,
                                       dv["desc"], dv["nout"], cap, d_f, d_e, d_m, d_p, d_nm, **opt)
    ex.synchronize()
    return d_m.cpu().numpy(), d_p.cpu().numpy(), d_nm.cpu().numpy()


def assert_equals_walk(s, m, pairs, nm, what="", use_u_right=True, **opt):
    want = walk(s, use_u_right, **opt)
    n1 = len(s["kf1"]["desc"])
    print("%s: %d matches (walk %d)" % (what, int(nm), want["n"]))
    assert int(nm) == want["n"], what
    assert m[:n1].tolist() == want["matches12"] and (m[n1:] == -1).all(), what
    assert [tuple(r) for r in pairs[:want["n"]].tolist()] == want["pairs"], what
    assert (pairs[want["n"]:] == POISON).all(), what
    return want


@pytest.mark.gpu
def test_gpu_batch_of_scenes_equals_the_walk_under_every_option_set():
    """one call per option set, every scene in each (frames 2p, 2p + 1 = the keyframes of pair p)"""
    ex = X.ORBextractor(1200)
    cap = ex.capacity
    assert cap == CAP_1200
    searches = [get(k) for k in STANDARD + DEGENERATE]
    dv = pack([k for s in searches for k in (s["kf1"], s["kf2"])], cap)
    for opt in OPTIONS:
        m, pr, nm = run(ex, dv, searches, (0, 2), (1, 2), cap, **opt)
        for i, s in enumerate(searches):
            assert_equals_walk(s, m[i], pr[i], nm[i], "scene %d %r" % (i, opt), **opt)


def check_gpu_on_seed(seed, **opt):
    """the body tools/fuzz_matchers.py runs with seeds outside the committed ones: the three scenes of one seed as one batch"""
    ex = X.ORBextractor(1200)
    searches = [scene(k, seed) for k in STANDARD]
    dv = pack([k for s in searches for k in (s["kf1"], s["kf2"])], CAP_1200)
    m, pr, nm = run(ex, dv, searches, (0, 2), (1, 2), CAP_1200, **opt)
    for i, s in enumerate(searches):
        assert_equals_walk(s, m[i], pr[i], nm[i], "seed %d scene %d %r" % (seed, i, opt), **opt)


@pytest.mark.gpu
def test_gpu_without_u_right_no_feature_is_stereo():
    ex = X.ORBextractor(1200)
    searches = [get(k) for k in STANDARD]
    dv = pack([k for s in searches for k in (s["kf1"], s["kf2"])], CAP_1200)
    m, pr, nm = run(ex, dv, searches, (0, 2), (1, 2), CAP_1200, use_u_right=False)
    for i, s in enumerate(searches):
        assert_equals_walk(s, m[i], pr[i], nm[i], "scene %d" % i, use_u_right=False)
    m, pr, nm = run(ex, dv, searches, (0, 2), (1, 2), CAP_1200, use_u_right=False, only_stereo=True)
    assert (nm == 0).all() and (m == -1).all()


def neighbourhood(seed, n_views, shared_first):
    """one keyframe and n_views others that see the same points from poses of their own; shared_first: the shared one is keyframe 1"""
    w = world(seed, 1200, 100)
    rng = np.random.default_rng(seed + 500)
    home = (rot_y(0.0), np.zeros(3))
    shared = view(w, home, 0.3 if shared_first else 0.5, 0.0, off_line=0.0 if shared_first else 0.25)
    out = []
    for v in range(n_views):
        pose = (rot_y(rng.uniform(-0.04, 0.04)), np.array([rng.choice([-1, 1]) * rng.uniform(0.3, 0.7), rng.uniform(-0.05, 0.05), rng.uniform(-0.1, 0.1)]))
        other = view(w, pose, 0.5 if shared_first else 0.3, rng.uniform(-20, 20), off_line=0.25 if shared_first else 0.0, n_seen=1200 - 23 * v)
        if shared_first:
            out.append(pair_of(shared, other, *fundamental(home, pose)))
        else:
            mine = dict(shared, mp=(rng.random(len(shared["mp"])) < 0.4).astype(np.uint8))      # GetMapPoint of the shared keyframe as this pair sees it
            out.append(pair_of(other, mine, *fundamental(pose, home)))
    return out


@pytest.mark.gpu
def test_gpu_one_keyframe_against_its_neighbours_and_many_against_one_twice():
    ex = X.ORBextractor(1200)
    cap = CAP_1200
    # kf1_step = 0, LocalMapping's shape: the new keyframe (batch frame 0) against nine neighbours (frames 1..9)
    searches = neighbourhood(21, 9, True)
    dv = pack([searches[0]["kf1"]] + [s["kf2"] for s in searches], cap)
    a = run(ex, dv, searches, (0, 0), (1, 1), cap)
    b = run(ex, dv, searches, (0, 0), (1, 1), cap)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    for i, s in enumerate(searches):
        assert assert_equals_walk(s, a[0][i], a[1][i], a[2][i], "neighbour %d" % i)["n"] > 100
    assert len(set(int(v) for v in a[2])) >= 5
    # kf2_step = 0: five keyframes (frames 1..5) against one (frame 0), whose MapPoint flags differ per pair
    searches = neighbourhood(22, 5, False)
    dv = pack([searches[0]["kf2"]] + [s["kf1"] for s in searches], cap)
    a = run(ex, dv, searches, (1, 1), (0, 0), cap)
    b = run(ex, dv, searches, (1, 1), (0, 0), cap)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    for i, s in enumerate(searches):
        assert assert_equals_walk(s, a[0][i], a[1][i], a[2][i], "keyframe %d" % i)["n"] > 100


def capacity_scenes(n):
    return [scene("twins", 31, n, max(n // 12, 1)), scene("forward", 32, n - 40, max(n // 12, 1))]


@pytest.mark.gpu
@pytest.mark.parametrize("nfeatures,cap,n", [(1000, 1024, 1000), (1200, CAP_1200, 1200), (2000, 2024, 2000), (2000, 3000, 2000)])
def test_gpu_capacities_staged_and_unstaged(nfeatures, cap, n):
    """1024 / 1302 / 2024 stage keyframe 2's descriptors in LDS; 3000 is above the staged bound (2720) and reads them from L2"""
    assert (lds_bytes(cap, staged=True) <= LDS_LIMIT) == (cap != 3000) and lds_bytes(cap) <= LDS_LIMIT
    ex = X.ORBextractor(nfeatures)
    assert lds_bytes(ex.capacity) <= LDS_LIMIT and lds_bytes(ex.capacity, staged=True) <= LDS_LIMIT      # orbx_max_keypoints() of this extractor
    searches = capacity_scenes(n)
    dv = pack([k for s in searches for k in (s["kf1"], s["kf2"])], cap)
    m, pr, nm = run(ex, dv, searches, (0, 2), (1, 2), cap)
    for i, s in enumerate(searches):
        assert assert_equals_walk(s, m[i], pr[i], nm[i], "capacity %d scene %d" % (cap, i))["n"] > 100


@pytest.mark.gpu
def test_gpu_on_the_producers_own_output():
    """extract_batch_device -> frame_finish_device -> compute_bow_device -> the search: the layouts the header documents are the ones the
    producers write.  F12 comes from a fixed arbitrary pose (the frames are shifted views of one picture, not a rigid scene), so the loose
    search (coarse) finds the shifted features and the strict one fewer; both are exact against the walk on the downloaded arrays."""
    import torch
    from test_frame_finish import TUM1
    rng = np.random.default_rng(12)
    voc = X.Vocabulary(arrays=make_vocab(rng, k=10, L=4, ragged=False))
    base = synth.frames("textured", 70, 1, 520, 720)[0]
    crop = lambda y, x: base[y:y + 480, x:x + 640]      # noqa: E731
    fr = np.stack([crop(20, 30), crop(20, 42), crop(22, 33), crop(14, 38)])
    B = 4
    ex = X.ORBextractor(1200, max_batch=B)
    cap = ex.capacity
    ex.set_stream(torch.cuda.current_stream().cuda_stream)
    d_k = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda"); d_d = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda"); d_mono = torch.zeros(B, dtype=torch.int32, device="cuda")
    ex.extract_batch_device(torch.from_numpy(np.ascontiguousarray(fr)).cuda(), B, 480, 640, d_k, d_d, d_n, d_mono, cap)
    cam = X.camera(**TUM1)
    bounds = X.compute_image_bounds(cam, 640, 480)
    d_un = torch.zeros_like(d_k); d_off = torch.zeros((B, 64 * 48 + 1), dtype=torch.int32, device="cuda")
    d_idx = torch.zeros((B, cap), dtype=torch.int32, device="cuda"); d_in = torch.zeros(B, dtype=torch.int32, device="cuda")
    ex.frame_finish_device(B, d_k, d_n, cap, cam, bounds, d_un, d_off, d_idx, d_in)
    d_wid = torch.zeros((B, cap), dtype=torch.int32, device="cuda"); d_ww = torch.zeros((B, cap), dtype=torch.float64, device="cuda")
    d_nw = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_fn = torch.zeros((B, cap), dtype=torch.int32, device="cuda"); d_fi = torch.zeros((B, cap), dtype=torch.int32, device="cuda")
    d_nf = torch.zeros(B, dtype=torch.int32, device="cuda")
    ex.compute_bow_device(voc, B, d_d, d_n, cap, d_wid, d_ww, d_nw, d_fn, d_fi, d_nf, levels_up=2)
    flags = (rng.random((2, 3, cap)) < 0.2).astype(np.uint8)      # [kf1 | kf2][pair]
    ur = np.where(rng.random((B, cap)) < 0.3, 10.0, -1.0).astype(np.float32)
    F12, ep = fundamental(*SIDE)                         # a fixed arbitrary pose
    F12 = np.tile(F12.reshape(1, 9), (3, 1)); ep = np.tile(ep.reshape(1, 2), (3, 1))
    d_ur, d_f, d_e = _dev(ur), _dev(F12), _dev(ep)
    d_fl1, d_fl2 = _dev(flags[0]), _dev(flags[1])
    n = d_n.cpu().numpy(); nf = d_nf.cpu().numpy()
    kk = d_un.cpu().numpy(); dd = d_d.cpu().numpy(); fnn = d_fn.cpu().numpy().astype(np.uint32); fii = d_fi.cpu().numpy().astype(np.uint32)
    kp = lambda f: kk[f, :n[f]].copy().view(np.uint8).reshape(-1, 28).copy().view(X.KEYPOINT_DTYPE).reshape(-1)      # noqa: E731
    total = {}
    for coarse in (False, True):
        d_m = torch.full((3, cap), POISON, dtype=torch.int32, device="cuda"); d_p = torch.full((3, cap, 2), POISON, dtype=torch.int32, device="cuda")
        d_nm = torch.full((3,), POISON, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ex.search_for_triangulation_device(3, (0, 0), (1, 1), d_fn, d_fi, d_nf, d_fl1, d_fl2, d_un, d_ur, d_d, d_n, cap, d_f, d_e, d_m, d_p, d_nm,
                                           coarse=coarse)
        ex.synchronize()
        m, pr, nm = d_m.cpu().numpy(), d_p.cpu().numpy(), d_nm.cpu().numpy()
        total[coarse] = 0
        for p in range(3):
            f2 = 1 + p
            kf = lambda f, fl: dict(kps=kp(f), desc=dd[f, :n[f]], fv=(fnn[f, :nf[f]], fii[f, :nf[f]]), mp=fl[:n[f]], ur=ur[f, :n[f]])      # noqa: E731
            s = pair_of(kf(0, flags[0, p]), kf(f2, flags[1, p]), F12[p].reshape(3, 3), ep[p])
            total[coarse] += assert_equals_walk(s, m[p], pr[p], nm[p], "pair %d coarse %d" % (p, coarse), coarse=coarse)["n"]
    assert total[True] > 30 and total[True] >= total[False]      # shifted views of one picture share most of their corners


@pytest.mark.gpu
def test_gpu_capacity_above_the_bound_is_refused_before_any_launch():
    import torch
    ex = X.ORBextractor(1000)
    cap = max(c for c in range(1, 9000) if lds_bytes(c) <= LDS_LIMIT)
    assert lds_bytes(cap + 1) > LDS_LIMIT and cap >= 4080
    s = scene("side", 41, 600, 50)
    dv = pack([s["kf1"], s["kf2"]], cap)
    ex.profile(True)
    m, pr, nm = run(ex, dv, [s], (0, 1), (1, 1), cap)                  # the largest accepted capacity runs
    assert_equals_walk(s, m[0], pr[0], nm[0], "capacity %d" % cap)
    launches = sum(v[1] for v in ex.profile_read().values())
    assert launches >= 1
    dv = pack([s["kf1"], s["kf2"]], cap + 1)
    with pytest.raises(X.OrbxError) as e:                              # the first refused one
        run(ex, dv, [s], (0, 1), (1, 1), cap + 1)
    assert e.value.code == -8
    ex.synchronize()
    assert sum(v[1] for v in ex.profile_read().values()) == launches   # nothing was launched


@pytest.mark.gpu
def test_gpu_argument_errors_are_rejected_before_any_launch():
    import torch
    ex = X.ORBextractor(1000)
    z = torch.zeros(4096, dtype=torch.int32, device="cuda")
    nm = torch.full((4,), POISON, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    good = dict(n_pairs=1, kf1=(0, 1), kf2=(1, 1), d_feat_nodes=z, d_feat_idx=z, d_n_feat=z, d_kf1_mp_flags=z, d_kf2_mp_flags=z, d_kps_un=z,
                d_u_right=z, d_desc=z, d_n=z, capacity=16, d_f12=z, d_epipole=z, d_matches12=z, d_pairs=z, d_n_matches=nm)
    bad = [dict(n_pairs=0), dict(kf1=(-1, 1)), dict(kf2=(-1, 1)), dict(n_pairs=3, kf1=(1, -1)), dict(n_pairs=3, kf2=(1, -1)), dict(capacity=0),
           dict(d_feat_nodes=None), dict(d_feat_idx=None), dict(d_n_feat=None), dict(d_kf1_mp_flags=None), dict(d_kf2_mp_flags=None),
           dict(d_kps_un=None), dict(d_desc=None), dict(d_n=None), dict(d_f12=None), dict(d_epipole=None), dict(d_matches12=None),
           dict(d_pairs=None), dict(d_n_matches=None)]
    for change in bad:
        with pytest.raises(X.OrbxError) as e:
            ex.search_for_triangulation_device(**dict(good, **change))
        assert e.value.code == -2, change
    ex.synchronize()
    assert (nm == POISON).all()
