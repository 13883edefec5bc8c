"""ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vpMapPointMatches) for two-camera frames (reference src/ORBmatcher.cc:269-471,
F.Nleft != -1; callers Tracking::TrackReferenceKeyFrame and Tracking::Relocalization).  CPU: the checker (tests/two_eyes_bow_walk.py)
against the C++ oracle where the right eyes are empty and against an independent per-node numpy statement; the per-eye FeatureVectors
merged equal the FeatureVector of the stacked descriptors; the synthetic inputs reach every branch the twin adds; the C entry exists.
GPU: orbx_search_by_bow_two_eyes_device against the walk, exact (matches of both eyes and the count)."""
import ctypes as C

import numpy as np
import pytest

import helpers
import oracle_lib as O
import extractorb_amd as X
import two_eyes_bow_walk as W
from extractorb_amd import synth
from test_bow import make_vocab
from test_search_bow import synthetic_pair

CAP_1200 = 1302                # orbx_max_keypoints() of a 1200-feature extractor (asserted on the GPU)
LDS_LIMIT = 160 * 1024 - 512


def lds_bytes(capacity):
    """the bound the header documents: 40 * ((capacity + 15) & ~15) + 64 <= 163 328"""
    return 40 * ((capacity + 15) & ~15) + 64


def feature_vector(node, keep):
    idx = np.nonzero(keep)[0]
    order = np.lexsort((idx, node[idx]))
    return node[idx][order].astype(np.uint32), idx[order].astype(np.uint32)


def flip_bits(rng, d, counts):
    for i in range(len(d)):
        for b in rng.integers(0, 256, counts[i]):
            d[i, b >> 3] ^= np.uint8(1 << (b & 7))


def keyframe_pair(rng, n_kl=600, n_kr=600, n_nodes=60, flag_rate=0.8):
    """A keyframe pair, arrays stacked left over right: 40 % of the right descriptors are copies of left ones in the same node (one
    MapPoint seen by both eyes); 5 % of the features are in no node (stopped words); flag bit 1 is noise."""
    n_k = n_kl + n_kr
    dk = rng.integers(0, 256, (n_k, 32), dtype=np.uint8)
    node = rng.integers(1, n_nodes + 1, n_k).astype(np.uint32) * 7
    twin = np.nonzero(rng.random(n_kr) < 0.4)[0]
    if n_kl:
        of = rng.integers(0, n_kl, len(twin))
        dk[n_kl + twin] = dk[of]; node[n_kl + twin] = node[of]
    flags = (rng.random(n_k) < flag_rate).astype(np.uint8) | (rng.integers(0, 2, n_k).astype(np.uint8) << 1)
    return dict(d=dk, node=node, keep=rng.random(n_k) > 0.05, angle=rng.uniform(0, 360, n_k).astype(np.float32), flags=flags, n_left=n_kl,
                n_nodes=n_nodes)


def related_keyframe_pair(rng, K, share=0.6):
    """Another keyframe pair of the same shape that shares `share` of its features with K (a few bits flipped, same node, nearly the same
    angle): a frame derived from K matches it as well, differently"""
    n_k = len(K["d"])
    R = keyframe_pair(rng, K["n_left"], n_k - K["n_left"], K["n_nodes"])
    same = np.nonzero(rng.random(n_k) < share)[0]
    d = K["d"][same].copy()
    flip_bits(rng, d, rng.integers(0, 6, len(same)))
    R["d"][same] = d; R["node"][same] = K["node"][same]
    R["angle"][same] = np.mod(K["angle"][same] + rng.normal(0, 3, len(same)), 360).astype(np.float32)
    R["angle"][R["angle"] >= 360] = 0
    return R


def frame_pair(rng, K, n_fl=650, n_fr=640, tie_heavy=False):
    """A frame pair for keyframe pair K: descriptors are noisy copies of K's descriptors of either eye, in the same node most of the time"""
    n_k, n_f, n_nodes = len(K["d"]), n_fl + n_fr, K["n_nodes"]
    if n_k:
        src = rng.integers(0, n_k, n_f)
        df = K["d"][src].copy(); node = K["node"][src].copy()
    else:
        df = rng.integers(0, 256, (n_f, 32), dtype=np.uint8)
        node = rng.integers(1, n_nodes + 1, n_f).astype(np.uint32) * 7
    flip_bits(rng, df, rng.integers(0, 3 if tie_heavy else 40, n_f))
    if tie_heavy:      # many identical descriptors inside a node, in each eye: best == second best, the first position must win
        for lo, n in ((0, n_fl), (n_fl, n_fr)):
            if n >= 16:
                df[lo:lo + n // 2] = df[lo + rng.integers(0, 8, n // 2)]
    wrong = rng.random(n_f) < 0.15
    node[wrong] = rng.integers(1, n_nodes + 40, wrong.sum()).astype(np.uint32) * 7      # other (sometimes keyframe-less) nodes
    angle = rng.uniform(0, 360, n_f).astype(np.float32)
    if n_k:
        angle = np.where(rng.random(n_f) < 0.8, np.mod(K["angle"][src] + rng.normal(12, 4, n_f), 360), angle).astype(np.float32)
    angle[angle >= 360] = 0
    return dict(d=df, node=node, keep=rng.random(n_f) > 0.05, angle=angle, n_left=n_fl)


def search_of(K, F):
    """the search keyframe pair K -> frame pair F, every array PER EYE (index 0 left, 1 right) with eye-local indices; FeatureVectors in
    (node, index) order"""
    def kp(a):
        k = np.zeros(len(a), X.KEYPOINT_DTYPE)
        k["angle"] = a
        return k
    cut = lambda P, key: [P[key][:P["n_left"]], P[key][P["n_left"]:]]
    fv = lambda P: [feature_vector(n, k) for n, k in zip(cut(P, "node"), cut(P, "keep"))]
    return dict(dk=cut(K, "d"), df=cut(F, "d"), kps_k=[kp(a) for a in cut(K, "angle")], kps_f=[kp(a) for a in cut(F, "angle")],
                flags=cut(K, "flags"), fv_k=fv(K), fv_f=fv(F))


def synthetic_two_eyes(rng, n_kl=600, n_kr=600, n_fl=650, n_fr=640, n_nodes=60, tie_heavy=False, flag_rate=0.8):
    """A keyframe pair and a frame pair with planted correspondences"""
    K = keyframe_pair(rng, n_kl, n_kr, n_nodes, flag_rate)
    return search_of(K, frame_pair(rng, K, n_fl, n_fr, tie_heavy))


def shared_keyframe_searches():
    """kf_step = 0: ONE keyframe pair against four frame pairs, each derived from it on its own"""
    rng = np.random.default_rng(40)
    K = keyframe_pair(rng)
    return [search_of(K, frame_pair(rng, K, 650 - 20 * i, 640 - 30 * i)) for i in range(4)]


def shared_frame_searches():
    """cur_step = 0 (relocalisation): four keyframe pairs against ONE frame pair; the frame is derived from the first keyframe, the others
    share 60 % of their features with it, each its own 60 %"""
    rng = np.random.default_rng(44)
    K = keyframe_pair(rng)
    F = frame_pair(rng, K)
    return [search_of(Ki, F) for Ki in [K] + [related_keyframe_pair(rng, K) for _ in range(3)]]


def walk(s, nnratio=0.7, th_low=50, check=True):
    """the checker on a search given per eye"""
    nlk, nlf = len(s["dk"][0]), len(s["df"][0])
    cat = lambda two, field=None: np.concatenate([a[field] if field else a for a in two])
    return W.search_by_bow_two_eyes(W.merge_feature_vectors(s["fv_k"][0], s["fv_k"][1], nlk), W.merge_feature_vectors(s["fv_f"][0], s["fv_f"][1], nlf),
                                    cat(s["flags"]), cat(s["kps_k"], "angle"), cat(s["dk"]), cat(s["kps_f"], "angle"), cat(s["df"]), nlf,
                                    nnratio, th_low, check)


def brute(s, nnratio, th_low, check):
    """Independent statement: nodes are independent; inside a node the keyframe's left features go first, then its right ones, each in list
    order; per eye of the frame the open features of the node sorted by distance (stable: the first position wins)."""
    nlk, nlf = len(s["dk"][0]), len(s["df"][0])
    bits_k = [np.unpackbits(d, axis=1).astype(np.int16) for d in s["dk"]]; bits_f = [np.unpackbits(d, axis=1).astype(np.int16) for d in s["df"]]
    m = [np.full(len(d), -1, np.int64) for d in s["df"]]
    bins = {}
    nodes_k = set(s["fv_k"][0][0].tolist()) | set(s["fv_k"][1][0].tolist())
    nodes_f = set(s["fv_f"][0][0].tolist()) | set(s["fv_f"][1][0].tolist())
    for node in sorted(nodes_k & nodes_f):
        cand = [s["fv_f"][e][1][s["fv_f"][e][0] == node] for e in (0, 1)]
        for ek in (0, 1):
            for k in s["fv_k"][ek][1][s["fv_k"][ek][0] == node]:
                if not s["flags"][ek][k] & 1:
                    continue
                best = []
                for e in (0, 1):
                    free = [int(f) for f in cand[e] if m[e][f] < 0]
                    if not free:
                        best.append((256, 256, -1))
                        continue
                    dist = np.abs(bits_f[e][free] - bits_k[ek][k]).sum(1)
                    order = np.argsort(dist, kind="stable")
                    best.append((int(dist[order[0]]), int(dist[order[1]]) if len(free) > 1 else 256, free[int(order[0])]))
                if best[0][0] > th_low:
                    continue
                take = [np.float32(best[0][0]) < np.float32(nnratio) * np.float32(best[0][1]), best[1][0] <= th_low]
                for e in (0, 1):
                    if take[e]:
                        f = best[e][2]
                        m[e][f] = k + ek * nlk
                        rot = np.float32(s["kps_k"][ek]["angle"][k]) - np.float32(s["kps_f"][e]["angle"][f])
                        if rot < 0:
                            rot = np.float32(rot + np.float32(360.0))
                        bins[(e, f)] = int(np.floor(float(np.float32(rot * np.float32(1.0 / 30))) + 0.5)) % 30
    if check:
        # ComputeThreeMaxima restated: the three largest bins, the earliest bin first among equals; the second and third only from 10 % of the first
        cnt = np.bincount(list(bins.values()), minlength=30)
        top = [int(i) for i in np.argsort(-cnt, kind="stable")[:3] if cnt[i] > 0]
        keep = [i for r, i in enumerate(top) if r == 0 or not np.float32(cnt[i]) < np.float32(0.1) * np.float32(cnt[top[0]])]
        for (e, f), b in bins.items():
            if b not in keep:
                m[e][f] = -1
    both = np.concatenate(m)
    return int((both >= 0).sum()), both


# the synthetic searches of the GPU batch test: generator arguments and search parameters
CASES = [dict(seed=1), dict(seed=2, nnratio=0.9, check=False), dict(seed=3, tie_heavy=True),
         dict(seed=4, n_nodes=3, n_kl=200, n_kr=180, n_fl=300, n_fr=280), dict(seed=5, n_nodes=2000), dict(seed=6, th_low=100, nnratio=0.6),
         dict(seed=7, n_kl=1302, n_kr=1302, n_fl=1302, n_fr=1302, n_nodes=100), dict(seed=8, n_kl=610, n_kr=40, n_fl=300, n_fr=900, n_nodes=12)]
GEN_KEYS = ("n_kl", "n_kr", "n_fl", "n_fr", "n_nodes", "tie_heavy", "flag_rate")
# degenerate shapes: an empty right eye on the keyframe only, on the frame only, on both; an empty left eye of the frame; all flags 0
DEGENERATE = [dict(seed=21, n_kr=0), dict(seed=22, n_fr=0), dict(seed=23, n_kr=0, n_fr=0), dict(seed=24, n_fl=0), dict(seed=25, flag_rate=0.0)]


def make(case):
    return synthetic_two_eyes(np.random.default_rng(case["seed"]), **{k: case[k] for k in GEN_KEYS if k in case})


def params(case):
    return case.get("nnratio", 0.7), case.get("th_low", 50), case.get("check", True)


# ---------------------------------------------------------------- CPU: the checker ----------------------------------------------------------------
@pytest.mark.parametrize("seed", [11, 12])
def test_walk_with_empty_right_eyes_equals_the_one_eye_oracle(seed):
    rng = np.random.default_rng(seed)
    p = synthetic_pair(rng)
    n, m = O.search_by_bow(p["fv_k"], p["fv_f"], p["flags"], p["kps_k"], p["dk"], p["kps_f"], p["df"], 0.7, 50, True)
    got = W.search_by_bow_two_eyes(p["fv_k"], p["fv_f"], p["flags"], p["kps_k"]["angle"], p["dk"], p["kps_f"]["angle"], p["df"], len(p["df"]))
    assert got["n"] == n and got["matches"] == m.tolist()
    assert n > 100 and got["right_writes"] == 0 and got["left_writes"] - got["removals"] == n


@pytest.mark.parametrize("case", CASES + DEGENERATE, ids=[str(c) for c in CASES + DEGENERATE])
def test_walk_equals_independent_statement(case):
    s = make(case)
    nn, th, chk = params(case)
    got = walk(s, nn, th, chk)
    bn, bm = brute(s, nn, th, chk)
    assert got["n"] == bn and got["matches"] == bm.tolist()
    assert got["n"] == sum(1 for v in got["matches"] if v >= 0) == got["left_writes"] + got["right_writes"] - got["removals"]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_merged_eye_feature_vectors_equal_the_feature_vector_of_the_stacked_descriptors(seed):
    rng = np.random.default_rng(seed)
    v = make_vocab(rng, k=6, L=4, ragged=seed == 3)
    words = v["desc"][v["is_leaf"] > 0]
    pick = lambda n: words[rng.integers(0, len(words), n)] ^ (rng.random((n, 32)) < 0.03).astype(np.uint8)      # near words: nodes repeat
    dl, dr = pick(300 + 10 * seed), pick(280)
    for levelsup in (1, 2, 4):
        fl, fr, fc = (O.compute_bow(v, d, levelsup)[2:] for d in (dl, dr, np.concatenate([dl, dr])))
        nodes, idx = W.merge_feature_vectors(fl, fr, len(dl))
        assert nodes.tolist() == fc[0].tolist() and idx.tolist() == fc[1].tolist()
        assert len(fc[0]) > 400
        if levelsup < 4:                                # (levelsup = L: every feature under the root, one node)
            assert len(set(fl[0].tolist()) & set(fr[0].tolist())) > 3


CAPACITY_CASE = dict(seed=51)      # the search of the capacity test


def branch_inputs():
    """every non-degenerate synthetic search a GPU test runs, AS IT IS COMBINED there, with its parameters"""
    out = [("case %s" % c, lambda c=c: make(c), params(c)) for c in CASES + [CAPACITY_CASE]]
    out += [("one keyframe, frame pair %d" % i, lambda i=i: shared_keyframe_searches()[i], (0.7, 50, True)) for i in range(4)]
    out += [("one frame, keyframe pair %d" % i, lambda i=i: shared_frame_searches()[i], (0.7, 50, True)) for i in range(4)]
    return out


@pytest.mark.parametrize("name,build,par", branch_inputs(), ids=[b[0] for b in branch_inputs()])
def test_synthetic_cases_reach_every_branch_of_the_twin(name, build, par):
    """A condition on the INPUTS of the GPU tests (the walk's counters), not on the code under test.  The degenerate shapes are exempt by
    construction (an empty eye has no writes), and a search without orientation check has no histogram removals."""
    nn, th, chk = par
    got = walk(build(), nn, th, chk)
    for key in ("left_writes", "right_writes", "right_without_left", "right_own_ratio_fail", "stopped_by_left"):
        assert got[key] >= 1, key
    if chk:
        assert got["removals"] >= 1


@pytest.mark.parametrize("searches", [shared_keyframe_searches, shared_frame_searches])
def test_searches_that_share_a_side_all_match_and_all_differ(searches):
    """the inputs of the kf_step = 0 / cur_step = 0 test: a wrong pair index cannot give the expected result of any of the four searches"""
    want = [walk(s) for s in searches()]
    for w in want:
        assert w["n"] > 100 and w["left_writes"] > 50 and w["right_writes"] > 20
    for i in range(4):
        for j in range(i + 1, 4):
            assert want[i]["matches"] != want[j]["matches"] and want[i]["n"] != want[j]["n"]


def test_degenerate_shapes_match_nothing_where_they_must():
    assert walk(make(DEGENERATE[3]))["n"] == 0 and walk(make(DEGENERATE[4]))["n"] == 0
    assert walk(make(DEGENERATE[1]))["right_writes"] == 0 and walk(make(DEGENERATE[0]))["right_writes"] >= 1


def test_entry_is_declared_exported_and_rejects_a_null_handle():
    assert "orbx_search_by_bow_two_eyes_device" in X.header_symbols()
    L = X.load_library()
    assert hasattr(L, "orbx_search_by_bow_two_eyes_device")
    z = C.c_void_p(16)      # never dereferenced: the handle is checked first
    assert L.orbx_search_by_bow_two_eyes_device(None, 1, 0, 1, 1, 1, z, z, z, z, z, z, z, 16, C.c_float(0.7), 50, 1, z, z) == -2
    text = open(X.orbextractor._HEADER).read()
    pos = text.index("int orbx_search_by_bow_two_eyes_device(")
    doc = text[text.rindex("/*", 0, pos):pos]
    assert "ORBX_ERR_UNSUPPORTED" in doc and "40 * ((capacity + 15) & ~15) + 64" in doc


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda()


def pack(pairs, cap):
    """pairs: per batch pair X (frame 2X = left eye, 2X + 1 = right eye) the per-eye (descriptors, keypoints, FeatureVectors)"""
    B = 2 * len(pairs)
    desc = np.zeros((B, cap, 32), np.uint8); kps = np.zeros((B, cap), X.KEYPOINT_DTYPE)
    fn = np.zeros((B, cap), np.uint32); fi = np.zeros((B, cap), np.uint32)
    nfeat = np.zeros(B, np.int32); nout = np.zeros(B, np.int32)
    for x, (d2, k2, fv2) in enumerate(pairs):
        for e in (0, 1):
            f = 2 * x + e
            desc[f, :len(d2[e])] = d2[e]; kps[f, :len(k2[e])] = k2[e]; nout[f] = len(d2[e])
            fn[f, :len(fv2[e][0])] = fv2[e][0]; fi[f, :len(fv2[e][1])] = fv2[e][1]; nfeat[f] = len(fv2[e][0])
    return dict(fn=_dev(fn.view(np.int32)), fi=_dev(fi.view(np.int32)), nfeat=_dev(nfeat), kps=_dev(kps), desc=_dev(desc), nout=_dev(nout))


def kf_of(s):
    return (s["dk"], s["kps_k"], s["fv_k"])


def cur_of(s):
    return (s["df"], s["kps_f"], s["fv_f"])


def flag_table(flag_pairs, cap):
    t = np.zeros((len(flag_pairs), 2, cap), np.uint8)
    for p, two in enumerate(flag_pairs):
        for e in (0, 1):
            t[p, e, :len(two[e])] = two[e]
    return t


def run(ex, dv, n, kf, cur, flags, cap, nnratio=0.7, th_low=50, check=True):
    import torch
    d_m = torch.full((n, 2, cap), -7, dtype=torch.int32, device="cuda"); d_nm = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    d_fl = _dev(flags)
    torch.cuda.synchronize()                            # torch's copies and fills have landed before the handle's stream runs
    ex.search_by_bow_two_eyes_device(n, kf, cur, dv["fn"], dv["fi"], dv["nfeat"], d_fl, dv["kps"], dv["desc"], dv["nout"], cap, d_m, d_nm,
                                     nnratio=nnratio, th_low=th_low, check_orientation=check)
    ex.synchronize()
    return d_m.cpu().numpy(), d_nm.cpu().numpy()


def run_searches(ex, searches, cap, nnratio=0.7, th_low=50, check=True):
    """search p: keyframe pair 2p against frame pair 2p + 1"""
    dv = pack([x for s in searches for x in (kf_of(s), cur_of(s))], cap)
    return run(ex, dv, len(searches), (0, 2), (1, 2), flag_table([s["flags"] for s in searches], cap), cap, nnratio, th_low, check)


def assert_equals_walk(s, m, nm, nnratio=0.7, th_low=50, check=True, what=""):
    want = walk(s, nnratio, th_low, check)
    nl, nr = len(s["df"][0]), len(s["df"][1])
    assert int(nm) == want["n"] == int((m >= 0).sum()), what
    assert m[0, :nl].tolist() == want["matches"][:nl] and m[1, :nr].tolist() == want["matches"][nl:], what
    assert (m[0, nl:] == -1).all() and (m[1, nr:] == -1).all(), what
    return want


@pytest.mark.gpu
def test_gpu_batch_of_synthetic_searches_equals_the_walk():
    """one call per parameter set, all thirteen searches in each: every search is checked under every parameter set"""
    ex = X.ORBextractor(1200)
    cap = ex.capacity
    assert cap == CAP_1200
    searches = [make(c) for c in CASES + DEGENERATE]
    for nn, th, chk in sorted(set(params(c) for c in CASES)):
        m, nm = run_searches(ex, searches, cap, nn, th, chk)
        for i, s in enumerate(searches):
            assert_equals_walk(s, m[i], nm[i], nn, th, chk, "search %d nnratio %g th_low %d check %d" % (i, nn, th, chk))
    assert int(nm[len(CASES) + 3]) == 0 and int(nm[len(CASES) + 4]) == 0      # empty left eye of the frame; all flags 0


@pytest.mark.gpu
def test_gpu_empty_right_eyes_equal_the_one_eye_entry_and_the_oracle():
    import torch
    ex = X.ORBextractor(1000)
    cap = 1024
    rng = np.random.default_rng(31)
    ps = [synthetic_pair(rng, 900 - 17 * i, 1000 - 31 * i, 60, tie_heavy=i == 2) for i in range(3)]
    z = lambda dt, shape=(0,): np.zeros(shape, dt)
    empty = (z(np.uint8, (0, 32)), z(X.KEYPOINT_DTYPE), (z(np.uint32), z(np.uint32)))
    two = lambda d, k, fv: ([d, empty[0]], [k, empty[1]], [fv, empty[2]])
    dv = pack([x for p in ps for x in (two(p["dk"], p["kps_k"], p["fv_k"]), two(p["df"], p["kps_f"], p["fv_f"]))], cap)
    m, nm = run(ex, dv, 3, (0, 2), (1, 2), flag_table([[p["flags"], z(np.uint8)] for p in ps], cap), cap)
    d_m1 = torch.full((3, cap), -7, dtype=torch.int32, device="cuda"); d_nm1 = torch.zeros(3, dtype=torch.int32, device="cuda")
    fl1 = np.zeros((3, cap), np.uint8)
    for i, p in enumerate(ps):
        fl1[i, :len(p["flags"])] = p["flags"]
    torch.cuda.synchronize()
    ex.search_by_bow_device(3, (0, 4), (2, 4), dv["fn"], dv["fi"], dv["nfeat"], _dev(fl1), dv["kps"], dv["desc"], dv["nout"], cap, d_m1, d_nm1)
    ex.synchronize()
    assert np.array_equal(m[:, 0], d_m1.cpu().numpy()) and np.array_equal(nm, d_nm1.cpu().numpy()) and (m[:, 1] == -1).all()
    for i, p in enumerate(ps):
        n, want = O.search_by_bow(p["fv_k"], p["fv_f"], p["flags"], p["kps_k"], p["dk"], p["kps_f"], p["df"])
        assert int(nm[i]) == n and m[i, 0, :len(want)].tolist() == want.tolist() and n > 100


@pytest.mark.gpu
def test_gpu_one_keyframe_against_many_frames_many_keyframes_against_one_frame_and_repeatability():
    ex = X.ORBextractor(1200)
    cap = CAP_1200
    # kf_step = 0: one keyframe pair (batch pair 0) against four frame pairs derived from it (batch pairs 1..4)
    searches = shared_keyframe_searches()
    dv = pack([kf_of(searches[0])] + [cur_of(s) for s in searches], cap)
    flags = flag_table([searches[0]["flags"]] * 4, cap)
    m, nm = run(ex, dv, 4, (0, 0), (1, 1), flags, cap)
    m2, nm2 = run(ex, dv, 4, (0, 0), (1, 1), flags, cap)
    assert np.array_equal(m, m2) and np.array_equal(nm, nm2)
    for i, s in enumerate(searches):
        want = assert_equals_walk(s, m[i], nm[i], what="frame pair %d" % i)
        assert want["n"] > 100 and int((m[i, 0] >= 0).sum()) > 50 and int((m[i, 1] >= 0).sum()) > 20
    assert len(set(int(v) for v in nm)) == 4
    # cur_step = 0 (relocalisation): four keyframe pairs that share features (batch pairs 1..4) against one frame pair (batch pair 0)
    searches = shared_frame_searches()
    dv = pack([cur_of(searches[0])] + [kf_of(s) for s in searches], cap)
    flags = flag_table([s["flags"] for s in searches], cap)
    m, nm = run(ex, dv, 4, (1, 1), (0, 0), flags, cap)
    m2, nm2 = run(ex, dv, 4, (1, 1), (0, 0), flags, cap)
    assert np.array_equal(m, m2) and np.array_equal(nm, nm2)
    for i, s in enumerate(searches):
        want = assert_equals_walk(s, m[i], nm[i], what="keyframe pair %d" % i)
        assert want["n"] > 100 and int((m[i, 0] >= 0).sum()) > 50 and int((m[i, 1] >= 0).sum()) > 20
    assert len(set(int(v) for v in nm)) == 4


@pytest.mark.gpu
def test_gpu_th_low_above_255_is_taken_as_255():
    """the documented clamp: from 256 on the reference would index vpMapPointMatches[-1] for a node without an open candidate"""
    ex = X.ORBextractor(1200)
    searches = [make(c) for c in CASES[:2]]
    m0, nm0 = run_searches(ex, searches, CAP_1200, 0.7, 255, True)
    m1, nm1 = run_searches(ex, searches, CAP_1200, 0.7, 300, True)
    assert np.array_equal(m0, m1) and np.array_equal(nm0, nm1)
    for i, s in enumerate(searches):
        assert_equals_walk(s, m1[i], nm1[i], 0.7, 255, True, "search %d" % i)


@pytest.mark.gpu
def test_gpu_descriptors_read_from_l2_equal_the_staged_form():
    """the form of capacities whose frame descriptors do not fit the LDS, forced at the 1200-feature capacity by the test aid"""
    cap = CAP_1200
    searches = [make(c) for c in CASES[:3]]
    m0, nm0 = run_searches(X.ORBextractor(1200), searches, cap)
    X.debug_set_option("two_eyes_bow_stage", 0)
    try:
        ex = X.ORBextractor(1200)
    finally:
        X.debug_set_option("two_eyes_bow_stage", -1)
    m1, nm1 = run_searches(ex, searches, cap)
    assert np.array_equal(m0, m1) and np.array_equal(nm0, nm1)
    for i, s in enumerate(searches):
        assert_equals_walk(s, m1[i], nm1[i], what="search %d" % i)


@pytest.mark.gpu
def test_gpu_on_extracted_stereo_pairs():
    """extract_batch_device (8 frames: keyframe pair, frame pair, twice) -> compute_bow_device per eye -> the two-eye search, against the
    walk fed with the downloaded arrays"""
    import torch
    rng = np.random.default_rng(12)
    voc = X.Vocabulary(arrays=make_vocab(rng, k=10, L=4, ragged=False))
    base = synth.frames("textured", 70, 1, 520, 720)[0]
    crop = lambda y, x: base[y:y + 480, x:x + 640]
    fr = np.stack([crop(20, 30), crop(20, 42), crop(22, 33), crop(22, 45),      # keyframe pair 0, frame pair 1 (right eyes 12 px further)
                   crop(20, 30), crop(20, 42), crop(14, 38), crop(14, 50)])     # keyframe pair 2, frame pair 3
    B = 8
    ex = X.ORBextractor(1200, max_batch=B)
    cap = ex.capacity
    ex.set_stream(torch.cuda.current_stream().cuda_stream)
    d_k = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda"); d_d = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda"); d_mono = torch.zeros(B, dtype=torch.int32, device="cuda")
    ex.extract_batch_device(torch.from_numpy(np.ascontiguousarray(fr)).cuda(), B, 480, 640, d_k, d_d, d_n, d_mono, cap)
    d_wid = torch.zeros((B, cap), dtype=torch.int32, device="cuda"); d_ww = torch.zeros((B, cap), dtype=torch.float64, device="cuda")
    d_nw = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_fn = torch.zeros((B, cap), dtype=torch.int32, device="cuda"); d_fi = torch.zeros((B, cap), dtype=torch.int32, device="cuda")
    d_nf = torch.zeros(B, dtype=torch.int32, device="cuda")
    ex.compute_bow_device(voc, B, d_d, d_n, cap, d_wid, d_ww, d_nw, d_fn, d_fi, d_nf, levels_up=2)
    flags = (rng.random((2, 2, cap)) < 0.85).astype(np.uint8)
    d_m = torch.full((2, 2, cap), -7, dtype=torch.int32, device="cuda"); d_nm = torch.zeros(2, dtype=torch.int32, device="cuda")
    ex.search_by_bow_two_eyes_device(2, (0, 2), (1, 2), d_fn, d_fi, d_nf, torch.from_numpy(flags).cuda(), d_k, d_d, d_n, cap, d_m, d_nm)
    ex.synchronize()
    n = d_n.cpu().numpy(); nf = d_nf.cpu().numpy(); m = d_m.cpu().numpy(); nm = d_nm.cpu().numpy()
    kk = d_k.cpu().numpy(); dd = d_d.cpu().numpy(); fnn = d_fn.cpu().numpy().astype(np.uint32); fii = d_fi.cpu().numpy().astype(np.uint32)
    kp = lambda f: kk[f, :n[f]].copy().view(np.uint8).reshape(-1, 28).copy().view(X.KEYPOINT_DTYPE).reshape(-1)
    eyes = lambda x, fun: [fun(2 * x), fun(2 * x + 1)]
    left = right = 0
    for p in range(2):
        K, Cp = 2 * p, 2 * p + 1
        s = dict(dk=eyes(K, lambda f: dd[f, :n[f]]), df=eyes(Cp, lambda f: dd[f, :n[f]]), kps_k=eyes(K, kp), kps_f=eyes(Cp, kp),
                 fv_k=eyes(K, lambda f: (fnn[f, :nf[f]], fii[f, :nf[f]])), fv_f=eyes(Cp, lambda f: (fnn[f, :nf[f]], fii[f, :nf[f]])),
                 flags=eyes(K, lambda f: flags[p, f & 1, :n[f]]))
        assert_equals_walk(s, m[p], nm[p], what="pair %d" % p)
        left += int((m[p, 0] >= 0).sum()); right += int((m[p, 1] >= 0).sum())
    assert left >= 1 and right >= 1


@pytest.mark.gpu
def test_gpu_capacity_bound_both_sides():
    import torch
    ex = X.ORBextractor(1000)
    cap = max(c for c in range(1, 8000) if lds_bytes(c) <= LDS_LIMIT)
    assert lds_bytes(cap + 1) > LDS_LIMIT and cap >= CAP_1200 and LDS_LIMIT == helpers.entry_lds_budget()
    s = make(CAPACITY_CASE)
    m, nm = run_searches(ex, [s], cap)                  # the largest accepted capacity runs
    assert_equals_walk(s, m[0], nm[0])
    m, nm = run_searches(X.ORBextractor(1200), [s], CAP_1200)      # the required one
    assert_equals_walk(s, m[0], nm[0])
    dv = pack([kf_of(s), cur_of(s)], cap + 1)
    d_m = torch.full((1, 2, cap + 1), -7, dtype=torch.int32, device="cuda"); d_nm = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    d_fl = _dev(flag_table([s["flags"]], cap + 1))
    torch.cuda.synchronize()
    with pytest.raises(X.OrbxError) as e:               # the first refused one
        ex.search_by_bow_two_eyes_device(1, (0, 2), (1, 2), dv["fn"], dv["fi"], dv["nfeat"], d_fl, dv["kps"], dv["desc"], dv["nout"], cap + 1,
                                         d_m, d_nm)
    assert e.value.code == -8
    ex.synchronize()
    assert (d_m == -7).all() and (d_nm == -7).all()     # nothing ran


@pytest.mark.gpu
def test_gpu_argument_errors_are_rejected_before_any_launch():
    import torch
    ex = X.ORBextractor(1000)
    z = torch.zeros(4096, dtype=torch.int32, device="cuda")
    nm = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    good = dict(n_pairs=1, kf=(0, 1), cur=(1, 1), d_feat_nodes=z, d_feat_idx=z, d_n_feat=z, d_kf_mp_flags=z, d_kps=z, d_desc=z, d_n=z, capacity=16,
                d_matches=z, d_n_matches=nm)
    bad = [dict(n_pairs=0), dict(kf=(-1, 1)), dict(cur=(-1, 1)), dict(n_pairs=3, kf=(1, -1)), dict(n_pairs=3, cur=(1, -1)), dict(capacity=0),
           dict(d_feat_nodes=None), dict(d_feat_idx=None), dict(d_n_feat=None), dict(d_kf_mp_flags=None), dict(d_kps=None), dict(d_desc=None),
           dict(d_n=None), dict(d_matches=None), dict(d_n_matches=None)]
    for change in bad:
        with pytest.raises(X.OrbxError) as e:
            ex.search_by_bow_two_eyes_device(**dict(good, **change))
        assert e.value.code == -2, change
    ex.synchronize()
    assert (nm == -7).all()                             # nothing ran
