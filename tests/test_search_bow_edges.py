"""The one-camera SearchByBoW row (k_search_bow<STAGE>, frame and keyframe overloads) on crafted scenes (tests/search_bow_scenes.py).
CPU: the statement equals the oracle and the older per-node statements of test_search_bow.py on every scene, every named mutant of the statement
is told apart by a named scene, the binary32 ratio test's disagreements with a double product are enumerated.  GPU: every scene against the
oracle at the capacities where the kernel changes form (staged / unstaged descriptors, the last accepted capacity), a full-size unstaged run,
degenerate launches over poisoned outputs, and the three frame walks.  docs/history/r25_bow_edges.md has the tables."""
import functools

import numpy as np
import pytest

import extractorb_amd as X
import search_bow_scenes as S
from test_search_bow import brute, brute_keyframes, synthetic_pair

SCENES = S.crafted_scenes()
BY_NAME = dict((s["name"], s) for s in SCENES)
OVERLOADS = [False, True]          # keyframes?
IDS = ["frame", "keyframes"]

# mutant -> (scene, overload) that tells it from the statement (test_every_mutant_is_caught_by_its_scene)
CAUGHT_BY = {
    "ratio_double": ("ratio_rounding_0.8", True), "ratio_fused": ("ratio_rounding_0.6", False), "th_swapped": ("th_low_boundary", False),
    "last_position": ("first_position_1.5_1_15_16_17", False), "second_is_first": ("th_low_boundary", True), "closed_ignored": ("chains_1.5", False),
    "maxima_ge": ("hist_four_tens", False), "cut_le": ("hist_30_3_3", True), "cut_double": ("hist_10_1_1", False), "round_even": ("histogram_edges", False),
}


def test_the_histogram_cut_in_binary32_and_with_a_double_literal_agree():
    """ComputeThreeMaxima's max2 < 0.1f * (float)max1: for every count a frame can give, the binary32 product and the product with the double
    literal 0.1 decide alike (both round onto max1 / 10 where it is an integer), so only the unrounded product (mutant cut_double) is a form
    the scenes can and must tell apart"""
    for m1 in range(0, 16385):
        single = np.float32(0.1) * np.float32(m1)
        for m2 in {m1 // 10, m1 // 10 + 1, max(m1 // 10 - 1, 0)}:
            assert (np.float32(m2) < single) == (m2 < 0.1 * m1), (m1, m2)


@functools.lru_cache(maxsize=None)
def want(name, keyframes, check):
    s = BY_NAME[name]
    n, m = S.oracle(s, s["nnratio"], s["th_low"], check, keyframes)
    m.setflags(write=False)
    return n, m


def test_scene_names_are_unique_and_small():
    assert len(BY_NAME) == len(SCENES)
    for s in SCENES:
        assert max(len(s["dk"]), len(s["df"])) < 300, s["name"]
        for nodes, idx in (s["fv_k"], s["fv_f"]):      # a FeatureVector: (node, index) ascending
            key = nodes.astype(np.int64) << 32 | idx
            assert (np.diff(key) > 0).all(), s["name"]


def test_ratio_disagreements_enumerated():
    """(float)bestDist1 < nnratio * (float)bestDist2 in binary32 against the same in double, over every distance pair"""
    found = {}
    for nn in (0.8, 0.6, 0.7, 0.75, 0.9):
        pairs, single, double = S.ratio_disagreements(nn)
        found[nn] = pairs
        for b1, b2 in pairs:                  # binary32 rounds the product down onto bestDist1: it rejects what the exact product accepts
            assert not single[b1, b2] and double[b1, b2]
    print("ratio disagreements:", dict((k, len(v)) for k, v in found.items()))
    assert len(found[0.8]) == 51 and len(found[0.6]) == 33
    assert (4, 5) in found[0.8] and (8, 10) in found[0.8] and (40, 50) in found[0.8] and (3, 5) in found[0.6] and (6, 10) in found[0.6]
    assert found[0.7] == [] and found[0.75] == [] and found[0.9] == []      # the frame overload's ratios (0.7, 0.75, 0.9) are safe
    for nn in (0.8, 0.6):                     # the scene plants every pair it can: two nodes each
        planted = [(a, b) for a, b in found[nn] if 1 <= a < 100]
        s = BY_NAME["ratio_rounding_%g" % nn]
        assert len(planted) >= 10 and len(s["dk"]) == 2 * len(planted) and len(s["df"]) == 4 * len(planted)


@pytest.mark.parametrize("keyframes", OVERLOADS, ids=IDS)
@pytest.mark.parametrize("name", list(BY_NAME))
def test_statement_equals_oracle_on_every_scene(name, keyframes):
    s = BY_NAME[name]
    for check in (True, False):
        n, m = want(name, keyframes, check)
        sn, sm = S.statement(s, s["nnratio"], s["th_low"], check, keyframes)
        assert n == sn and m.tolist() == sm.tolist(), (name, check)
        if keyframes:
            bn, bm = brute_keyframes(s, s["flags2"], s["nnratio"], s["th_low"], check)
        else:
            bn, bm = brute(s, s["nnratio"], s["th_low"], check)
        assert n == bn and m.tolist() == bm.tolist(), (name, check)
    # what the scene's own text promises (angles are all 0 in these scenes: the histogram drops nothing)
    n, m = want(name, keyframes, False)
    for k, f in s["expect"][keyframes].items():
        if keyframes:
            assert m[k] == f, (name, k)
        else:
            assert (m == k).sum() == (f >= 0) and (f < 0 or m[f] == k), (name, k)


def test_scenes_reach_what_they_are_for():
    """properties of the oracle's answers that the scenes exist for (a scene that lost its branch must not pass silently)"""
    # chains: several keyframe features of one node are accepted one after the other, and late ones find nothing free
    for keyframes in OVERLOADS:
        n, m = want("chains_1.5", keyframes, False)
        s = BY_NAME["chains_1.5"]
        assert n >= 40 and n < int((s["flags"] & 1).sum()) - 30
        n7, _ = want("chains_0.7", keyframes, False)
        assert 10 <= n7 < n
    assert want("chains_1.5", False, False)[0] > want("chains_1.5", True, False)[0]      # flags2 closes the nearest ones
    # 179 is accepted and 180 is not, alone (1 and 0 matches) and after a closing (the closing one's match + 1 and + 0)
    for keyframes in OVERLOADS:
        assert want("single_candidate_ratio", keyframes, False)[0] == (1 + 2) + (0 + 1)
    # histogram: (10, 1, 1) keeps all, (11, 1, 1) keeps one bin, four tens keep three, (30, 3, 3) keeps all
    assert [want(x, False, True)[0] for x in ("hist_10_1_1", "hist_11_1_1", "hist_30_3_3", "hist_four_tens", "hist_one_bin", "hist_no_matches")] == [12, 11, 36, 30, 5, 0]
    assert [want(x, False, False)[0] for x in ("hist_10_1_1", "hist_11_1_1", "hist_30_3_3", "hist_four_tens", "hist_one_bin", "hist_no_matches")] == [12, 13, 36, 40, 5, 0]
    bins = sorted(set(S.rotation_bin(a, b) for a, b, _ in S.EDGE_ANGLES))
    assert bins == [0, 1, 3, 12] and max(S.rotation_bin(a, 0.0) for a in np.linspace(0, 360, 3601, dtype=np.float32)) == 12
    below = np.nextafter(np.float32(360), np.float32(0))
    assert np.float32(np.float32(0.0) - np.float32(3e-5)) + np.float32(360) == below      # "just below 360" is also reached through the wrap
    assert np.float32(np.float32(0.0) - np.float32(1e-6)) + np.float32(360) == np.float32(360)
    assert want("histogram_edges", False, True)[0] < want("histogram_edges", False, False)[0]
    # degenerate pairs give nothing, the normal pair beside them something
    for keyframes in OVERLOADS:
        assert want("normal", keyframes, True)[0] > 10
        for x in ("empty_keyframe_fv", "empty_frame_fv", "no_common_node", "no_map_points", "no_keyframe_keypoints", "no_frame_keypoints"):
            assert want(x, keyframes, True)[0] == 0
    assert want("second_all_closed", True, True)[0] == 0 and want("second_all_closed", False, True)[0] > 10


def test_every_mutant_is_caught_by_its_scene():
    assert set(CAUGHT_BY) == set(S.MUTANTS)
    caught = {}
    for mutant in S.MUTANTS:
        for s in SCENES:
            for keyframes in OVERLOADS:
                for check in (True, False):
                    n, m = want(s["name"], keyframes, check)
                    mn, mm = S.statement(s, s["nnratio"], s["th_low"], check, keyframes, mutant=mutant)
                    if (n, m.tolist()) != (mn, mm.tolist()):
                        caught.setdefault(mutant, set()).add((s["name"], keyframes))
    print("mutants caught by:", dict((k, sorted(v)) for k, v in caught.items()))
    for mutant, where in CAUGHT_BY.items():
        assert where in caught.get(mutant, ()), (mutant, sorted(caught.get(mutant, ())))


def test_capacities_take_the_forms_the_formula_gives():
    """k_bow_match.hip: staged while 86 * up16(capacity) + 64 <= 150 KB; orbx_rows.cpp accepts while 22 * up16(capacity) + 64 <= 150 KB"""
    assert [S.is_staged(c) for c in S.CAPACITIES] == [True, True, False, False, False]
    assert all(S.is_accepted(c) for c in S.CAPACITIES) and not S.is_accepted(6977)
    assert max(c for c in range(1, 8000) if S.is_staged(c)) == 1776 and max(c for c in range(1, 8000) if S.is_accepted(c)) == 6976
    assert S.lds_bytes(1777, False) == 22 * 1792 + 64 and 1781 % 16 != 0
    from test_entry_rejections_gpu import PAST_LDS
    assert PAST_LDS["orbx_search_by_bow_device"] == 6977


def _compare(nm, m, pairs, nnratio, th_low, check, keyframes, label, wanted=None):
    for i, p in enumerate(pairs):
        n, w = wanted[i] if wanted else S.oracle(p, nnratio, th_low, check, keyframes)
        assert int(nm[i]) == n, (label, i, p.get("name"))
        assert m[i, :len(w)].tolist() == w.tolist(), (label, i, p.get("name"))
        assert (m[i, len(w):] == -1).all(), (label, i, p.get("name"))      # -1 beyond the frame's keypoints, whatever the buffer held


@pytest.mark.gpu
@pytest.mark.parametrize("keyframes", OVERLOADS, ids=IDS)
@pytest.mark.parametrize("cap", S.CAPACITIES)
def test_gpu_crafted_scenes_at_every_form(cap, keyframes):
    """all scenes (degenerate pairs among them, in one batch beside normal ones) over poisoned outputs, at a staged capacity, the last staged,
    the first unstaged, one that is no multiple of 16 and the largest the entry accepts"""
    assert S.is_accepted(cap) and S.is_staged(cap) == (cap <= 1776)
    ex = X.ORBextractor(1000)
    for (nnratio, th_low), pairs in S.groups(SCENES).items():
        for check in (True, False):
            nm, m = S.run_pairs(ex, pairs, nnratio, th_low, check, cap, keyframes)
            _compare(nm, m, pairs, nnratio, th_low, check, keyframes, (nnratio, th_low, check), [want(p["name"], keyframes, check) for p in pairs])


@pytest.mark.gpu
@pytest.mark.parametrize("keyframes", OVERLOADS, ids=IDS)
def test_gpu_full_size_unstaged(keyframes):
    """k_search_bow<false> on frames that fill its tables: capacity 1777, about 1700 keypoints per frame"""
    cap = 1777
    assert not S.is_staged(cap)
    rng = np.random.default_rng(25)
    pairs = [dict(synthetic_pair(rng, 1700 - 9 * i, 1777 - 40 * i, 110, tie_heavy=(i == 1))) for i in range(2)]
    for p in pairs:
        p["flags2"] = (rng.random(len(p["df"])) < 0.7).astype(np.uint8) | 2
    ex = X.ORBextractor(1000)
    nnratio = 0.8 if keyframes else 0.7
    nm, m = S.run_pairs(ex, pairs, nnratio, 50, True, cap, keyframes)
    _compare(nm, m, pairs, nnratio, 50, True, keyframes, "full")
    assert int(nm.sum()) > 400


def _view(rng, d, kps, fv):
    """another view of a frame: a few bits flipped, some features dropped from the FeatureVector, angles jittered"""
    d = d.copy()
    for i in range(len(d)):
        for b in rng.integers(0, 256, rng.integers(0, 12)):
            d[i, b >> 3] ^= np.uint8(1 << (b & 7))
    kps = kps.copy()
    kps["angle"] = np.mod(kps["angle"] + rng.normal(0, 5, len(kps)), 360).astype(np.float32)
    keep = rng.random(len(fv[0])) > 0.1
    return d, kps, (fv[0][keep], fv[1][keep])


@pytest.mark.gpu
@pytest.mark.parametrize("keyframes", OVERLOADS, ids=IDS)
def test_gpu_walks(keyframes):
    """one keyframe against many frames (kf step 0), many keyframes against one frame (cur step 0: Relocalization's shape); the interleaved
    (0, 2), (1, 2) walk is every other test's"""
    rng = np.random.default_rng(31)
    p = synthetic_pair(rng, 200, 240, 12)
    n_pairs, cap = 3, 1024
    nnratio = 0.8 if keyframes else 0.7
    ex = X.ORBextractor(1000)
    kf = (p["dk"], p["kps_k"], p["fv_k"]); fr = (p["df"], p["kps_f"], p["fv_f"])
    # one keyframe, three frames; every pair has its own MapPoint flags
    views = [_view(rng, *fr) for _ in range(n_pairs)]
    pairs = [dict(dk=kf[0], kps_k=kf[1], fv_k=kf[2], df=v[0], kps_f=v[1], fv_f=v[2], flags=(rng.random(200) < 0.8).astype(np.uint8),
                  flags2=(rng.random(240) < 0.7).astype(np.uint8)) for v in views]
    nm, m = S.run_device(ex, [kf] + views, [q["flags"] for q in pairs], [q["flags2"] for q in pairs], (0, 0), (1, 1), n_pairs, nnratio, 50, True, cap,
                         keyframes)
    _compare(nm, m, pairs, nnratio, 50, True, keyframes, "one keyframe")
    assert int(nm.min()) > 20
    # three keyframes, one frame
    views = [_view(rng, *kf) for _ in range(n_pairs)]
    pairs = [dict(dk=v[0], kps_k=v[1], fv_k=v[2], df=fr[0], kps_f=fr[1], fv_f=fr[2], flags=(rng.random(200) < 0.8).astype(np.uint8),
                  flags2=(rng.random(240) < 0.7).astype(np.uint8)) for v in views]
    nm, m = S.run_device(ex, [fr] + views, [q["flags"] for q in pairs], [q["flags2"] for q in pairs], (1, 1), (0, 0), n_pairs, nnratio, 50, True, cap,
                         keyframes)
    _compare(nm, m, pairs, nnratio, 50, True, keyframes, "one frame")
    assert int(nm.min()) > 20
