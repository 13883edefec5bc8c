"""The Sim3 overloads of ORBmatcher::SearchByProjection (reference src/ORBmatcher.cc:473-586 and :588-704; loop closing;
orbx_search_by_projection_sim3_device) - the CPU side.
(a) the sequential walk (tests/sim3_projection_walk.py) against an independent statement that is NOT a walk: a certificate check of a given
    result (brute force over all keypoints, levels from the library's breakpoints, the bound from the library's host function); by induction
    on the list index exactly one result passes it.  A result with two entries swapped is shown not to pass;
(b) scenes with contention (several MapPoints per keypoint), initially occupied keypoints, other settings and bounds, real sizes, the Fuse edge
    scene under this search;
(c) crafted scenes, each asserted to reach what it was planted for: a cascade that needs one round per request, the same chain reversed, a
    window with more equal candidates than a key list, the bounds and gates;
(d) k_project_sim3.hip's own source compiled for the host (tests/cpp/sim3_host_check.cpp) against the walk on every scene, and under
    ASan + UBSan as a stand-alone program;
(e) the surface.
The GPU tests are in tests/test_sim3_projection_gpu.py and use the cases, the packing and the walks of this module."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import extractorb_amd as X
import fuse_walk as W
import sim3_projection_walk as S
import test_fuse as T
from fuse_walk import f32, f64

ROOT = T.ROOT
CALLERS = dict(kf_window=dict(th=8.0, th_low=50, ratio_hamming=1.5),       # src/LoopClosing.cc:730 (the second overload)
               bow=dict(th=5.0, th_low=50, ratio_hamming=1.0),             # :755
               place=dict(th=3.0, th_low=50, ratio_hamming=1.5))           # :1008


# ---------------------------------------------------------------- cases ----------------------------------------------------------------
def from_fuse_scene(s, opt, occupied_share=0.0, density=None):
    """pair k = list 0 into keyframe k under keyframe k's pose (kf step 1, mp step 0)"""
    pairs = []
    for k, kf in enumerate(s["kfs"]):
        n = len(s["lists"][0]["world"])
        flags = T.flags_for(s, k, n) if density is None else np.ones(n, np.uint8)
        occ = None
        if occupied_share:
            occ = (np.random.default_rng(900 + k).random(len(kf["kps"])) < occupied_share).astype(np.uint8)
        pairs.append(dict(kf=k, lst=0, pose=kf["pose"], flags=flags, occupied=occ))
    return dict(scene=s, pairs=pairs, kf=(0, 1), mp=(0, 0), opt=opt)


def few_words(s, seed, words=4):
    """rewrites the descriptors of a random scene from a vocabulary of a few words (plus flipped bits): a MapPoint is within the bound of
    EVERY keypoint of its word, so a request whose keypoint was taken falls back to a neighbour - the contention the closing rule is about.
    (With the scene's own random descriptors a displaced request finds nothing else within 75 bits.)"""
    rng = np.random.default_rng(seed)
    vocab = rng.integers(0, 256, (words, 32), dtype=np.uint8)

    def noisy(n, most):
        out = vocab[rng.integers(0, words, n)].copy()
        for row in out:
            for b in rng.integers(0, 256, rng.integers(0, most + 1)):
                row[b >> 3] ^= 1 << (b & 7)
        return out
    for kf in s["kfs"]:
        kf["desc"] = noisy(len(kf["kps"]), 20)
    for m in s["lists"]:
        m["desc"] = noisy(len(m["world"]), 40)
    return s


def real_case():
    """1200 keypoints x 4000 MapPoints x 2 pairs with different poses into the same keyframe (kf step 0, mp step 1)"""
    s = few_words(T.random_scene(41, 1200, 4000, 1, lists=2), 141)
    pose = s["kfs"][0]["pose"]
    other = pose.copy(); other[:, 3] += np.array([0.004, -0.003, 0.002], f32)
    pairs = [dict(kf=0, lst=l, pose=p, flags=T.flags_for(s, l, 4000), occupied=None) for l, p in enumerate((pose, other))]
    return dict(scene=s, pairs=pairs, kf=(0, 0), mp=(0, 1), opt=CALLERS["kf_window"])


def crafted(kp, mp, opt, occupied=()):
    """identity pose, CAM of powers of two, level 0 everywhere: kp = [(x, y, descriptor)], mp = [(u, v, descriptor)] or [(world point, descriptor)]"""
    tab = W.tables()
    kps = np.zeros(len(kp), X.KEYPOINT_DTYPE)
    kps["x"] = [k[0] for k in kp]; kps["y"] = [k[1] for k in kp]
    off, idx, cell = W.build_grid(kps, T.BOUNDS)
    assert (cell >= 0).all()
    pose = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(f32)
    kf = dict(pose=pose, kps=kps, ur=None, desc=np.stack([k[2] for k in kp]), grid_off=off, grid_idx=idx)
    world = np.stack([T.at(m[0], m[1]) if len(m) == 3 else np.asarray(m[0], f32) for m in mp])
    d = np.array([T.dist3d_of(p) for p in world], f32)
    mps = dict(world=world, normal=(world / d[:, None]).astype(f32), dist=np.stack([np.zeros_like(d), np.full_like(d, 1e9), d], axis=1),
               desc=np.stack([m[-1] for m in mp]))
    s = dict(tab=tab, setting=(1.2, 8), cam=T.CAM, bounds=T.BOUNDS, mbf=T.MBF, kfs=[kf], lists=[mps], seed=77)
    occ = None
    if len(occupied):
        occ = np.zeros(len(kp), np.uint8); occ[list(occupied)] = 1
    return dict(scene=s, pairs=[dict(kf=0, lst=0, pose=pose, flags=np.ones(len(mp), np.uint8), occupied=occ)], kf=(0, 1), mp=(0, 0), opt=opt)


def flip(desc, bits, start=0):
    d = desc.copy()
    for b in range(start, start + bits):
        d[(b % 256) >> 3] ^= 1 << (b & 7)
    return d


CHAIN = 47          # chain requests; with the request in front 48 requests on 48 keypoints


def chain_parts():
    """keypoints k_0 .. k_47 in a row, 6 px apart; chain request c_j sits between k_j and k_j+1 (radius 5: its window holds exactly those two),
    carries k_j's descriptor (distance 0) and finds k_j+1 at distance 10; `front` sits where c_0 sits and carries k_0's descriptor too"""
    rng = np.random.default_rng(51)
    d = [rng.integers(0, 256, 32, dtype=np.uint8)]
    for j in range(CHAIN):
        d.append(flip(d[-1], 10, 10 * j))
    kp = [(30.0 + 6.0 * j, 100.0, d[j]) for j in range(CHAIN + 1)]
    chain = [(33.0 + 6.0 * j, 100.0, d[j]) for j in range(CHAIN)]
    front = (33.0, 100.0, d[0])
    return kp, chain, front


def cascade_case():
    kp, chain, front = chain_parts()
    return crafted(kp, [front] + chain, CALLERS["bow"])


def reversed_case():
    kp, chain, front = chain_parts()
    return crafted(kp, chain[::-1] + [front], CALLERS["bow"])


def overflow_case():
    """one window with K + 3 keypoints of one descriptor; K + 5 requests with it"""
    K = X.load_library().orbx_debug_sim3_search_list_length()
    d = np.random.default_rng(52).integers(0, 256, 32, dtype=np.uint8)
    kp = [(300.0 + 0.5 * (j % 4), 200.0 + 0.5 * (j // 4), d) for j in range(K + 3)]
    return crafted(kp, [(300.5, 200.5, d)] * (K + 5), CALLERS["place"])


def projection_probe():
    """a world point (identity pose) whose u differs between the two projection forms: fl(x/z) against fl(x*fl(1/z)), a difference in the last
    bit that survives the addition of cx; found by search, fixed by the seed.  u lies in [256, 512): u + 3 is exact there"""
    rng = np.random.default_rng(53)
    cam = T.CAM
    while True:
        p = np.array([rng.uniform(0.05, 0.5), rng.uniform(-0.3, 0.3), rng.uniform(2.5, 7.5)], f32)
        u0, v0 = S.project(p, cam, 0); u1, v1 = S.project(p, cam, 1)
        if u0 != u1 and 280 < u0 < 500 and 60 < v0 < 440:
            return p, (u0, v0), (u1, v1)


GATE_NAMES = {}


def gates_case(opt):
    """bounds and gates; GATE_NAMES: name -> MapPoint index, "kp_" + name -> keypoint index"""
    rng = np.random.default_rng(54)
    rnd = lambda: rng.integers(0, 256, 32, dtype=np.uint8)      # noqa: E731
    kp, mp, names = [], [], {}

    def add_kp(name, x, y, d):
        names["kp_" + name] = len(kp); kp.append((x, y, d))

    def add_mp(name, *m):
        names[name] = len(mp); mp.append(m)
    for k, bits in enumerate((75, 76, 50, 51)):                                       # distance exactly at and one above the two bounds
        d = rnd(); add_kp("dist_%d" % bits, 40.0 + 40.0 * k, 40.0, d); add_mp("dist_%d" % bits, 40.0 + 40.0 * k, 40.0, flip(d, bits))
    d = rnd(); add_kp("taken", 240.0, 40.0, d)                                        # the only candidate within the bound goes to the earlier request
    add_mp("taker", 240.0, 40.0, d); add_mp("too_late", 240.0, 40.0, flip(d, 5))
    d = rnd(); add_kp("occupied_zero", 300.0, 40.0, d); add_kp("open_worse", 301.0, 40.0, flip(d, 7))      # an occupied keypoint at distance 0
    add_mp("skips_occupied", 300.5, 40.0, d)
    d = rnd()
    add_kp("tie_first_index", 64.0, 145.5, d)                                         # cell (6, 15): visited second
    add_kp("tie_second_index", 64.0, 143.5, d)                                        # cell (6, 14): visited first, although its index is larger
    add_mp("tie", 64.0, 144.5, d)
    # the two projection forms: u0 != u1 by one ulp; a keypoint exactly one radius (3 px) beside the smaller one's u: |kx - u| < r fails for it
    # (= 3) and holds for the other
    p, (u0, v0), (u1, v1) = projection_probe()
    lo, hi = (u0, u1) if u0 < u1 else (u1, u0)
    kx = f32(lo + f32(3.0))
    assert f32(kx - lo) == f32(3.0) and f32(kx - hi) < f32(3.0)
    d = rnd(); add_kp("projection", kx, v0, d); add_mp("projection", p, d)
    GATE_NAMES.update(names)
    return crafted(kp, mp, opt, occupied=[names["kp_occupied_zero"]])


def edge_case(opt_extra=None):
    s = T.get("edge")
    n = len(s["lists"][0]["world"])
    c = from_fuse_scene(s, dict(CALLERS["place"], ratio_hamming=1.0, **(opt_extra or {})), density=1.0)
    assert len(c["pairs"]) == 1 and len(c["pairs"][0]["flags"]) == n
    return c


BUILDERS = dict(
    contended=lambda: from_fuse_scene(few_words(T.random_scene(31, 96, 600, 3), 131, words=2), CALLERS["kf_window"]),
    contended_occupied=lambda: from_fuse_scene(few_words(T.random_scene(31, 96, 600, 3), 131, words=2), CALLERS["kf_window"], occupied_share=0.3),
    contended_12=lambda: from_fuse_scene(few_words(T.random_scene(32, 96, 600, 3, setting=(1.1, 12)), 132, words=2), CALLERS["kf_window"]),
    contended_frac=lambda: from_fuse_scene(few_words(T.random_scene(33, 96, 600, 3, bounds=T.FRAC_BOUNDS), 133, words=2), CALLERS["bow"]),
    real=real_case,
    edge=edge_case,
    edge_returns=lambda: edge_case(T.RETURNS),
    cascade=cascade_case,
    reversed=reversed_case,
    overflow=overflow_case,
    gates_15=lambda: gates_case(dict(th=3.0, th_low=50, ratio_hamming=1.5)),
    gates_10=lambda: gates_case(dict(th=3.0, th_low=50, ratio_hamming=1.0)),
)
CASES = tuple(BUILDERS)
_cases, _walks = {}, {}


def get(name):
    if name not in _cases:
        _cases[name] = BUILDERS[name]()
    return _cases[name]


def walk(name, pair, projection=0, n_mp=None, use_occupied=True):
    """the walk of pair `pair` of a case - shared by all tests, never changed"""
    key = (name, pair, projection, n_mp, use_occupied)
    if key not in _walks:
        c = get(name); s = c["scene"]; q = c["pairs"][pair]
        stats = {}
        r = S.search(s["kfs"][q["kf"]], q["pose"], s["lists"][q["lst"]], q["flags"], s["cam"], s["bounds"], s["tab"], projection=projection,
                     occupied=q["occupied"] if use_occupied else None, n_mp=n_mp, stats=stats, **c["opt"])
        r["stats"] = stats
        _walks[key] = r
    return _walks[key]


# ---------------------------------------------------------------- (a) the certificate ----------------------------------------------------------------
def certify(c, pair, projection, res):
    """Is `res` THE result?  No walk: the front end in vector arithmetic, then for every request the set open_i from the RESULT's own earlier
    entries.  Returns (ok, first bad request or -1)."""
    s = c["scene"]; q = c["pairs"][pair]; opt = c["opt"]
    kf = s["kfs"][q["kf"]]; mps = s["lists"][q["lst"]]; tab, cam = s["tab"], s["cam"]
    fb = np.asarray(s["bounds"], f32)
    w_inv = f32(64) / (fb[1] - fb[0]); h_inv = f32(48) / (fb[3] - fb[2])
    minx, maxx, miny, maxy = (f32(int(b)) for b in fb)
    bp = X.predict_scale_breakpoints(*s["setting"])
    bound = X.sim3_hamming_bound(opt["th_low"], opt["ratio_hamming"])
    P = np.asarray(q["pose"], f32); M = len(mps["world"]); w = mps["world"].astype(f32)
    with np.errstate(all="ignore"):
        pc = [(((P[r, 0].astype(f64) * w[:, 0].astype(f64) + P[r, 1].astype(f64) * w[:, 1].astype(f64)) + P[r, 2].astype(f64) * w[:, 2].astype(f64)) * 1.0 +
               P[r, 3].astype(f64)).astype(f32) for r in range(3)]
        Ow = np.array([f32(((f64(P[0, r]) * f64(P[0, 3]) + f64(P[1, r]) * f64(P[1, 3])) + f64(P[2, r]) * f64(P[2, 3])) * -1.0) for r in range(3)], f32)
        if projection:
            invz = f32(1) / pc[2]
            u = cam[0] * (pc[0] * invz) + cam[2]; v = cam[1] * (pc[1] * invz) + cam[3]
        else:
            u = cam[0] * pc[0] / pc[2] + cam[2]; v = cam[1] * pc[1] / pc[2] + cam[3]
        PO64 = (w - Ow[None, :]).astype(f64)
        d3 = np.sqrt((PO64[:, 0] ** 2 + PO64[:, 1] ** 2) + PO64[:, 2] ** 2).astype(f32)
        nv = mps["normal"].astype(f32).astype(f64)
        dot = (PO64[:, 0] * nv[:, 0] + PO64[:, 1] * nv[:, 1]) + PO64[:, 2] * nv[:, 2]
        ratio = mps["dist"][:, 2].astype(f32) / d3
        level = np.searchsorted(bp, np.where(np.isnan(ratio), f32(0), ratio), side="right")
        radius = f32(opt["th"]) * tab["scale"][level]
        code = np.full(M, -1, np.int32)

        def leave(mask, k):
            code[(code < 0) & mask] = k
        leave((q["flags"] & 1) == 0, S.EXIT_FLAG)
        leave(pc[2] < 0, S.EXIT_NEG_DEPTH)
        leave(~((u >= minx) & (u < maxx) & (v >= miny) & (v < maxy)), S.EXIT_NOT_IN_IMAGE)
        leave((d3 < mps["dist"][:, 0]) | (d3 > mps["dist"][:, 1]), S.EXIT_DISTANCE)
        leave(dot < 0.5 * d3.astype(f64), S.EXIT_NORMAL)
        kps = kf["kps"]; n = len(kps)
        _, order, cell = W.build_grid(kps, s["bounds"])
        pos = np.full(n, 1 << 30, np.int64); pos[order] = np.arange(len(order))
        kx, ky, ko = kps["x"].astype(f32), kps["y"].astype(f32), kps["octave"].astype(np.int64)
        free = np.ones(n, bool) if q["occupied"] is None else (np.asarray(q["occupied"][:n]) == 0)
        taken = np.zeros(n, bool)                            # match_idx[j] of the j < i, read from the result under test
        holder = np.full(n, -1, np.int64)
        for i in range(M):
            want_idx, want_dist, want_exit = -1, 256, int(code[i])
            if code[i] < 0:
                r = radius[i]
                lo_x = np.floor((u[i] - minx - r) * w_inv); hi_x = np.ceil((u[i] - minx + r) * w_inv)
                lo_y = np.floor((v[i] - miny - r) * h_inv); hi_y = np.ceil((v[i] - miny + r) * h_inv)
                seen = (cell >= 0) & (lo_x < 64) & (hi_x >= 0) & (lo_y < 48) & (hi_y >= 0)
                seen &= (cell // 48 >= lo_x) & (cell // 48 <= hi_x) & (cell % 48 >= lo_y) & (cell % 48 <= hi_y)
                seen &= (np.abs(kx - u[i]) < r) & (np.abs(ky - v[i]) < r)
                want_exit = S.EXIT_NO_MATCH if seen.any() else S.EXIT_EMPTY_WINDOW
                open_i = np.nonzero(seen & (ko >= level[i] - 1) & (ko <= level[i]) & free & ~taken)[0]
                if len(open_i):
                    dist = W.POPCOUNT[kf["desc"][open_i] ^ mps["desc"][i][None, :]].sum(axis=1)
                    b = np.lexsort((pos[open_i], dist))[0]
                    if dist[b] <= bound:
                        want_idx, want_dist, want_exit = int(open_i[b]), int(dist[b]), S.EXIT_MATCHED
            if (int(res["match_idx"][i]), int(res["match_dist"][i]), int(res["exit"][i])) != (want_idx, want_dist, want_exit):
                return False, i
            if res["match_idx"][i] >= 0:
                taken[res["match_idx"][i]] = True; holder[res["match_idx"][i]] = i
    ok = np.array_equal(res["matches"], holder.astype(np.int32)) and res["n_matches"] == int((holder >= 0).sum())
    return ok, -1


@pytest.mark.parametrize("name", CASES)
def test_walk_passes_the_certificate(name):
    c = get(name)
    for pair in range(len(c["pairs"])):
        for projection in (0, 1):
            ok, bad = certify(c, pair, projection, walk(name, pair, projection))
            assert ok, (name, pair, projection, bad)


def test_certificate_rejects_a_result_with_two_entries_swapped():
    c = get("contended")
    r = walk("contended", 0)
    matched = np.nonzero(r["match_idx"] >= 0)[0]
    assert len(matched) > 20
    rejected = 0
    for a, b in zip(matched[:10], matched[10:20]):
        bad = dict((k, np.array(v)) for k, v in r.items() if k != "stats")
        bad["n_matches"] = r["n_matches"]
        for k in ("match_idx", "match_dist"):
            bad[k][[a, b]] = bad[k][[b, a]]
        bad["matches"][bad["match_idx"][a]] = a; bad["matches"][bad["match_idx"][b]] = b
        rejected += not certify(c, 0, 0, bad)[0]
    assert rejected == 10
    # ... and one that hands a contended keypoint to the LATER of two requests that want it
    stats = r["stats"]
    assert stats.get("closed_skip", 0) > 0


# ---------------------------------------------------------------- (b), (c) reach ----------------------------------------------------------------
def test_contended_scenes_meet_closed_candidates_and_displaced_requests():
    for name in ("contended", "contended_occupied", "contended_12", "contended_frac", "real"):
        c = get(name)
        total = {}
        exits = set()
        for pair in range(len(c["pairs"])):
            r = walk(name, pair)
            exits |= set(r["exit"].tolist())
            for k, v in r["stats"].items():
                total[k] = total.get(k, 0) + v
        need = ["closed_skip", "level_filter", "only_closed_within_bound"]
        need += ["occupied_skip"] if name == "contended_occupied" else []
        need += ["best_closed_worse_taken", "tie_kept_first"] if name == "real" else []      # (a window of the small scenes rarely holds two keypoints)
        assert not [k for k in need if not total.get(k, 0)], (name, total)
        assert exits == set(range(8)), (name, exits)
    assert get("contended_frac")["scene"]["bounds"][0] != np.trunc(get("contended_frac")["scene"]["bounds"][0])
    assert walk("real", 0)["n_matches"] > 300 and not np.array_equal(walk("real", 0)["match_idx"], walk("real", 1)["match_idx"])
    assert sum(walk("contended", p)["n_matches"] for p in range(3)) > 60


def test_edge_probes_end_where_fuses_do():
    s = T.get("edge")
    n = len(s["lists"][0]["world"])
    for extra, case in ((dict(), "edge"), (T.RETURNS, "edge_returns")):
        fuse = W.search(s["kfs"][0], s["lists"][0], np.ones(n, np.uint8), s["cam"], s["bounds"], s["mbf"], s["tab"], reproj_check=False, **extra)
        mine = walk(case, 0)
        early = fuse["exit"] <= W.EXIT_EMPTY_WINDOW
        assert early.sum() >= 10 and np.array_equal(mine["exit"][early], fuse["exit"][early]) and (mine["exit"][~early] > S.EXIT_EMPTY_WINDOW).all()
        if extra:
            for k in ("min_x", "max_x", "min_y", "max_y"):
                assert mine["stats"].get("return_%s_cell_%s" % tuple(k.split("_")), 0) >= 1
            assert not (mine["exit"] > S.EXIT_EMPTY_WINDOW).any()
        else:
            assert set(mine["exit"].tolist()) == set(range(1, 8))      # (every probe's flag is set)


def test_cascade_displaces_every_request_and_the_reversed_chain_nobody():
    r = walk("cascade", 0)
    assert r["match_idx"].tolist() == list(range(CHAIN + 1)) and r["match_dist"].tolist() == [0] + [10] * CHAIN
    assert r["stats"]["best_closed_worse_taken"] == CHAIN and r["n_matches"] == CHAIN + 1
    r = walk("reversed", 0)
    assert r["match_idx"].tolist() == list(range(CHAIN))[::-1] + [-1] and r["match_dist"].tolist() == [0] * CHAIN + [256]
    assert r["exit"][-1] == S.EXIT_NO_MATCH and "best_closed_worse_taken" not in r["stats"] and r["stats"]["only_closed_within_bound"] == 1


def test_overflow_window_holds_more_equal_candidates_than_a_key_list():
    K = X.load_library().orbx_debug_sim3_search_list_length()
    assert K in (4, 8)
    c = get("overflow"); r = walk("overflow", 0)
    kf = c["scene"]["kfs"][0]
    visit = W.features_in_area(kf, T.BOUNDS, f32(300.5), f32(200.5), f32(3.0))
    assert len(visit) == K + 3
    assert r["match_idx"].tolist() == visit + [-1, -1] and r["match_dist"].tolist() == [0] * (K + 3) + [256, 256]
    assert r["exit"].tolist() == [S.EXIT_MATCHED] * (K + 3) + [S.EXIT_NO_MATCH] * 2


def test_bounds_and_gates():
    r15, r10 = walk("gates_15", 0), walk("gates_10", 0)
    N = GATE_NAMES
    e = lambda r, k: (int(r["exit"][N[k]]), int(r["match_dist"][N[k]]))      # noqa: E731
    assert e(r15, "dist_75") == (S.EXIT_MATCHED, 75) and e(r15, "dist_76") == (S.EXIT_NO_MATCH, 256)
    assert e(r15, "dist_50") == (S.EXIT_MATCHED, 50) and e(r15, "dist_51") == (S.EXIT_MATCHED, 51)
    assert e(r10, "dist_50") == (S.EXIT_MATCHED, 50) and e(r10, "dist_51") == (S.EXIT_NO_MATCH, 256) and e(r10, "dist_75") == (S.EXIT_NO_MATCH, 256)
    for r in (r15, r10):
        assert e(r, "taker") == (S.EXIT_MATCHED, 0) and e(r, "too_late") == (S.EXIT_NO_MATCH, 256) and r["match_idx"][N["too_late"]] == -1
        assert r["matches"][N["kp_taken"]] == N["taker"]
        assert r["match_idx"][N["skips_occupied"]] == N["kp_open_worse"] and r["match_dist"][N["skips_occupied"]] == 7
        assert r["matches"][N["kp_occupied_zero"]] == -1 and r["stats"]["occupied_skip"] >= 1
        assert N["kp_tie_second_index"] > N["kp_tie_first_index"] and r["match_idx"][N["tie"]] == N["kp_tie_second_index"] and r["stats"]["tie_kept_first"] >= 1
    # the two projection forms differ in u by one ulp, and the keypoint one radius beside the smaller u is inside the window of the other only
    p, (u0, v0), (u1, v1) = projection_probe()
    assert u0 != u1 and abs(float(u0) - float(u1)) <= float(np.spacing(u0)) * 1.01
    got = sorted((int(walk("gates_15", 0, pr)["exit"][N["projection"]]), pr) for pr in (0, 1))
    assert [g[0] for g in got] == [S.EXIT_EMPTY_WINDOW, S.EXIT_MATCHED] and got[0][1] == (0 if u0 < u1 else 1)


# ---------------------------------------------------------------- packing (shared with the GPU tests) ----------------------------------------------------------------
def pack(c, cap=None, mp_cap=None):
    """the arrays of a case as the entry takes them: frame f = keyframe f, list l = MapPoint list l, poses / flags / occupied per pair"""
    s = c["scene"]; kfs, lists, pairs = s["kfs"], s["lists"], c["pairs"]
    cap = cap or max(len(k["kps"]) for k in kfs) + 3
    mp_cap = mp_cap or max(len(m["world"]) for m in lists)
    B, NL, P = len(kfs), len(lists), len(pairs)
    a = dict(kps=np.zeros((B, cap), X.KEYPOINT_DTYPE), desc=np.zeros((B, cap, 32), np.uint8), nout=np.zeros(B, np.int32),
             off=np.zeros((B, 64 * 48 + 1), np.int32), idx=np.zeros((B, cap), np.int32), poses=np.zeros((P, 12), f32),
             world=np.zeros((NL, mp_cap, 3), f32), normal=np.zeros((NL, mp_cap, 3), f32), dist=np.zeros((NL, mp_cap, 3), f32),
             mdesc=np.zeros((NL, mp_cap, 32), np.uint8), flags=np.ones((P, mp_cap), np.uint8), occupied=np.zeros((P, cap), np.uint8))
    for f, k in enumerate(kfs):
        n = len(k["kps"])
        a["kps"][f, :n] = k["kps"]; a["desc"][f, :n] = k["desc"]; a["nout"][f] = n; a["off"][f] = k["grid_off"]; a["idx"][f, :len(k["grid_idx"])] = k["grid_idx"]
    for l, m in enumerate(lists):
        n = len(m["world"])
        a["world"][l, :n] = m["world"]; a["normal"][l, :n] = m["normal"]; a["dist"][l, :n] = m["dist"]; a["mdesc"][l, :n] = m["desc"]
    for p, q in enumerate(pairs):
        assert (q["kf"], q["lst"]) == (c["kf"][0] + p * c["kf"][1], c["mp"][0] + p * c["mp"][1])
        a["poses"][p] = np.asarray(q["pose"], f32).reshape(12)
        a["flags"][p, :len(q["flags"])] = q["flags"]                 # beyond the list the flags stay SET: d_n_mp must stop them
        if q["occupied"] is not None:
            a["occupied"][p, :len(q["occupied"])] = q["occupied"]
    a["any_occupied"] = any(q["occupied"] is not None for q in pairs)
    a["cap"], a["mp_cap"] = cap, mp_cap
    return a


# ---------------------------------------------------------------- (d) the kernel's own source, on the host ----------------------------------------------------------------
HOST_FLAGS = ["-std=c++17", "-ffp-contract=off", "-I" + os.path.join(ROOT, "tests", "cpp"), "-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"),
              "-I" + os.path.join(ROOT, "extractorb_amd", "csrc"), "-I" + os.path.join(ROOT, "include")]
HOST_SOURCES = [os.path.join(ROOT, "tests", "cpp", "sim3_host_check.cpp"), os.path.join(ROOT, "extractorb_amd", "csrc", "orbx_predict_scale.cpp")]


class HostParams(C.Structure):      # == Sim3SearchParams of extractorb_amd/csrc/orbx_params.hpp
    _fields_ = ([(n, C.c_float) for n in "fx fy cx cy minX maxX minY maxY wInv hInv".split()] +
                [("scale", C.c_float * 16), ("breaks", C.c_float * 16), ("th", C.c_float)] +
                [(n, C.c_int) for n in "nlevels maxDist projection capacity mpCapacity kfFirst kfStep mpFirst mpStep".split()])


def host_params(c, a, projection):
    s = c["scene"]; tab = s["tab"]; opt = c["opt"]
    p = HostParams()
    p.fx, p.fy, p.cx, p.cy = (float(v) for v in s["cam"][:4])
    p.minX, p.maxX, p.minY, p.maxY = (float(int(b)) for b in s["bounds"])      # as the entry fills them: truncated
    p.wInv = f32(64) / (s["bounds"][1] - s["bounds"][0]); p.hInv = f32(48) / (s["bounds"][3] - s["bounds"][2])
    for i in range(tab["nlevels"]):
        p.scale[i] = tab["scale"][i]
    for i, b in enumerate(X.predict_scale_breakpoints(*s["setting"])):
        p.breaks[i] = b
    p.th = opt["th"]; p.nlevels = tab["nlevels"]; p.maxDist = X.sim3_hamming_bound(opt["th_low"], opt["ratio_hamming"]); p.projection = projection
    p.capacity = a["cap"]; p.mpCapacity = a["mp_cap"]; p.kfFirst, p.kfStep = c["kf"]; p.mpFirst, p.mpStep = c["mp"]
    return p


def test_kernel_source_compiled_for_the_host_equals_the_walk(tmp_path):
    """k_project_sim3.hip itself: k_sim3_window one thread at a time, then the shared decision function in emulated rounds"""
    so = str(tmp_path / "libsim3_host.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", *HOST_FLAGS, *HOST_SOURCES, "-o", so])
    L = C.CDLL(so)
    assert L.sim3_host_params_size() == C.sizeof(HostParams) and L.sim3_host_list_length() == X.load_library().orbx_debug_sim3_search_list_length()
    ptr = lambda x: x.ctypes.data_as(C.c_void_p)      # noqa: E731
    compared, rounds_of, rescans_of = 0, {}, {}
    for name in CASES:
        c = get(name); a = pack(c); P = len(c["pairs"])
        for projection in (0, 1):
            p = host_params(c, a, projection)
            matches = np.full((P, a["cap"]), -7, np.int32); mi = np.full((P, a["mp_cap"]), -7, np.int32); md = mi.copy()
            ex = np.full((P, a["mp_cap"]), 99, np.uint8); nm = np.full(P, -7, np.int32); st = np.zeros(2, np.int32)
            L.sim3_host(ptr(a["world"]), ptr(a["normal"]), ptr(a["dist"]), ptr(a["mdesc"]), None, ptr(a["flags"]), ptr(a["poses"]), ptr(a["kps"]),
                        ptr(a["desc"]), ptr(a["nout"]), ptr(a["off"]), ptr(a["idx"]), ptr(a["occupied"]) if a["any_occupied"] else None, C.byref(p),
                        ptr(matches), ptr(mi), ptr(md), ptr(ex), ptr(nm), P, ptr(st))
            rounds_of[name], rescans_of[name] = int(st[0]), int(st[1])
            for q in range(P):
                want = walk(name, q, projection)
                n = len(want["matches"]); m = len(want["exit"])
                what = (name, projection, q)
                assert np.array_equal(matches[q, :n], want["matches"]) and (matches[q, n:] == -1).all(), what
                assert np.array_equal(mi[q, :m], want["match_idx"]) and np.array_equal(md[q, :m], want["match_dist"]), what
                assert np.array_equal(ex[q, :m], want["exit"]) and int(nm[q]) == want["n_matches"], what
                compared += m
    assert compared > 20000
    assert rounds_of["cascade"] >= 40 and rounds_of["reversed"] <= 3 and rescans_of["overflow"] > 0, (rounds_of, rescans_of)


def test_kernel_source_stays_inside_its_arrays_as_a_sanitized_host_program(tmp_path):
    """the same source as a stand-alone program under AddressSanitizer + UBSan: exact-size buffers, valid and corrupt grids"""
    exe = str(tmp_path / "sim3_host_check")
    subprocess.check_call(["g++", "-O1", "-g", "-DSIM3_HOST_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *HOST_FLAGS, *HOST_SOURCES,
                           "-o", exe])
    out = subprocess.check_output([exe], text=True)
    assert out.count("trial") == 6 and out.strip().endswith("clean")
    assert "rescans 0" not in out.splitlines()[1]      # the valid trial with few distinct descriptors takes the re-scan path


# ---------------------------------------------------------------- (e) the surface ----------------------------------------------------------------
def test_entries_are_declared_documented_exported_and_bound():
    names = ("orbx_search_by_projection_sim3_device", "orbx_sim3_hamming_bound", "orbx_debug_sim3_search_stats", "orbx_debug_sim3_search_list_length")
    for n in names:
        assert n in X.header_symbols() and hasattr(X.load_library(), n)
    text = open(X.orbextractor._HEADER).read()
    pos = text.index("int orbx_search_by_projection_sim3_device(")
    doc = text[text.rindex("/*", 0, pos):pos]
    for word in ("473-586", "588-704", "730", "755", "1008", "1735-1959", "PER PAIR", "vpMatchedKF", "ORBX_ERR_UNSUPPORTED", "163 328", "FIRST"):
        assert word in doc, word
    assert "CLAMPS" in text[text.rindex("/*", 0, text.index("int orbx_sim3_hamming_bound(")):text.index("int orbx_sim3_hamming_bound(")]
    for k, v in dict(FLAG=0, NEG_DEPTH=1, NOT_IN_IMAGE=2, DISTANCE=3, NORMAL=4, EMPTY_WINDOW=5, NO_MATCH=6, MATCHED=7).items():
        assert "ORBX_SIM3_SEARCH_%s = %d" % (k, v) in text
    z = C.c_void_p(16)      # never dereferenced: the handle is checked first
    L = X.load_library()
    assert L.orbx_search_by_projection_sim3_device(None, 1, 0, 0, 0, 0, z, z, z, z, z, 16, z, z, z, z, z, 16, z, z, z, z, 8, 0, 3.0, 50, 1.0, z, z, z, z,
                                                   z, z) == -2
    assert L.orbx_debug_sim3_search_stats(None) == -2
    assert callable(getattr(X.ORBextractor, "search_by_projection_sim3_device", None)) and callable(getattr(X.ORBextractor, "debug_sim3_search_stats", None))


def test_the_integer_bound_of_the_float_acceptance():
    assert X.sim3_hamming_bound(50, 1.5) == 75 and X.sim3_hamming_bound(50, 1.0) == 50 and X.sim3_hamming_bound(50, 0.999) == 49
    assert X.sim3_hamming_bound(50, 6.0) == 255 and X.sim3_hamming_bound(50, float("nan")) == -1 and X.sim3_hamming_bound(50, -0.5) == -1
    assert X.sim3_hamming_bound(0, 1.5) == 0 and X.sim3_hamming_bound(50, float("inf")) == 255
    # the definition, against the reference's comparison of an int with the float product
    rng = np.random.default_rng(3)
    for th_low, ratio in zip(rng.integers(0, 120, 300).tolist(), rng.uniform(0, 3, 300).astype(f32).tolist()):
        prod = f32(th_low) * f32(ratio)
        want = max([d for d in range(256) if f32(d) <= prod], default=-1)
        assert X.sim3_hamming_bound(th_low, ratio) == want, (th_low, ratio)


def test_lds_bound_formula_admits_the_stated_shape():
    """(the refusal itself needs a handle: tests/test_sim3_projection_gpu.py) the documented bound, restated"""
    fits = lambda cap, m: 4 * (cap + m) + 64 <= 163328 and cap <= 65536      # noqa: E731
    assert fits(2720, 16384) and fits(1302, 16384) and not fits(2720, 40000)
