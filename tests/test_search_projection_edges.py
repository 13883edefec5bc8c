"""The one-camera SearchByProjection row (k_search_proj<TOPLIST>, k_project_last) on crafted scenes (tests/search_projection_scenes.py).
CPU: the statement equals the oracle and the older brute_search of test_search_projection.py on every scene, every named mutant of the statement
is told apart by a named scene (or is shown equivalent), the binary32 ratio test's disagreements with a double product are enumerated, the
chains reach the kernel's re-scan condition.  GPU: every scene against the oracle at the capacities where the kernel changes form, degenerate
pairs over poisoned outputs, the frame / descriptor walks, k_project_last on hand-written requests.  docs/history/r27_search_projection_edges.md
has the tables."""
import functools

import numpy as np
import pytest

import extractorb_amd as X
import oracle_lib as O
import search_projection_scenes as S
from test_search_projection import brute_search, crowd_scene

f32 = np.float32
SCENES = S.crafted_scenes()
BY_NAME = dict((s["name"], s) for s in SCENES)

# mutant -> (scene, ratio mode) that tells it from the statement (test_every_mutant_is_caught_by_its_scene)
CAUGHT_BY = {
    "maxdist_ge": ("th_high_boundary_64", False), "box_le": ("box_boundary", False), "stereo_ge": ("stereo_column", False),
    "uright_ge_zero": ("stereo_column", True), "ratio_double": ("ratio_rounding_0.9", True), "ratio_ge": ("ratio_rounding_0.9", True),
    "ratio_any_level": ("second_level_ties", True), "last_tie": ("first_in_grid_order", False), "second_tie_level": ("second_level_ties", True),
    "closed_ignored": ("chains_5", False), "no_obs_closes": ("chain_with_gaps", False), "first_holder_wins": ("chain_with_gaps", True),
    "round_half_even": ("histogram_edges", False), "cut_gt": ("hist_30_3_3", False), "cut_double": ("hist_10_1_1", False),
    "maxima_ge": ("hist_four_tens", False), "drop_counts_keypoints": ("holders_in_two_bins", False), "level_max_unguarded": ("level_windows", False),
}
# mutants no scene can tell apart, and why
EQUIVALENT = {
    "no_bin_wrap": "factor = 1 / 30, not 30 / 360: rot in [0, 360] reaches bins 0 .. 12 only, bin 30 does not occur",
    "level_check_always": "octaves are >= 0: with bCheckLevels false, minLevel <= 0 excludes nothing and the maxLevel test is guarded by maxLevel >= 0 itself",
}


@functools.lru_cache(maxsize=None)
def want(name, ratio, check, stereo=None):
    return S.oracle(BY_NAME[name], ratio, check, stereo)


def modes(s):
    return [(ratio, check) for ratio, check in s["modes"]]


def test_scene_names_are_unique_and_small():
    assert len(BY_NAME) == len(SCENES)
    for s in SCENES:
        assert len(s["un"]) <= 300 and len(s["q"]) <= 400, s["name"]
        # well-formed: a consistent grid (every index once, in range; ascending offsets that end at the number of keypoints inside)
        assert (np.diff(s["off"]) >= 0).all() and s["off"][0] == 0 and s["off"][-1] == len(s["idx"]), s["name"]
        assert len(set(s["idx"].tolist())) == len(s["idx"]) and (len(s["idx"]) == 0 or (0 <= s["idx"].min() and s["idx"].max() < len(s["un"]))), s["name"]
        assert s["un"]["octave"].min(initial=0) >= 0 and s["un"]["octave"].max(initial=0) <= 7, s["name"]


def test_ratio_disagreements_enumerated():
    """(float)bestDist > mfNNratio * (float)bestDist2 in binary32 against the product in double, over every distance pair"""
    found = {}
    for nn in (0.7, 0.9, 0.6, 0.75, 0.8):
        pairs, single, double = S.ratio_disagreements(nn)
        found[nn] = pairs
        for b1, b2 in pairs:                  # binary32 rounds the product up onto bestDist: it accepts what the exact product rejects
            assert not single[b1, b2] and double[b1, b2]
    print("ratio disagreements:", dict((k, len(v)) for k, v in found.items()))
    assert [len(found[nn]) for nn in (0.7, 0.9, 0.6, 0.75, 0.8)] == [25, 25, 0, 0, 0]
    assert found[0.7] == [(7 * k, 10 * k) for k in range(1, 26)] and found[0.9] == [(9 * k, 10 * k) for k in range(1, 26)]
    s = BY_NAME["ratio_rounding_0.9"]         # the scene plants every pair whose best distance can be accepted: four spots each
    assert s["pairs"] == [(9 * k, 10 * k) for k in range(1, 12)] and len(s["q"]) == 4 * len(s["pairs"]) and len(s["un"]) == 8 * len(s["pairs"])


@pytest.mark.parametrize("name", list(BY_NAME))
def test_statement_equals_oracle_on_every_scene(name):
    s = BY_NAME[name]
    inside = {int(i): p for p, i in enumerate(s["idx"])}
    for ratio, check in modes(s):
        log = {}
        sn, sm, so = S.statement(s, ratio, check, log=log)
        assert (sn, sm, so) == want(name, ratio, check), (name, ratio, check)
        bn, bm, bo = brute_search(s["q"], s["qd"], s["un"], s["d"], inside, s["bounds"], s["ur"] if s["stereo"] else None, s["occ"], ratio, s["nnratio"],
                                  check, s["max_distance"])
        assert (bn, bm, bo) == (sn, sm, so), (name, ratio, check)
        # what the scene's own text promises: where each request is accepted
        if not (check and not ratio and name in ("histogram_edges",)):
            for i, k in s["expect"].items():
                assert log.get(i) == k, (name, ratio, check, i)


def _bins(s):
    log = {}
    S.statement(s, False, True, log=log)
    sizes = [0] * 30
    for i, k in log.items():
        sizes[S.rotation_bin(s["q"]["angle"][i], s["un"]["angle"][k])] += 1
    return sizes


def test_chains_reach_the_rescan_condition():
    """k_search_proj<true> scans a window again only when its four best static keys leave too few open keypoints: all four closed, or in ratio
    mode three of the four (a second best is needed).  The chains reach that from the fifth request on (the fourth in ratio mode), and not before."""
    for k in S.CHAINS:
        s = BY_NAME["chains_%d" % k]
        assert bool(S.rescans(s, False)) == (k >= 5), k
        assert bool(S.rescans(s, True)) == (k >= 4), k
        if k >= 5:
            assert S.rescans(s, False)[0] == 4 and S.rescans(s, True)[0] == 3
    assert len(S.rescans(BY_NAME["chains_40"], False)) == 36 and S.rescans(BY_NAME["chain_with_gaps"], False)
    for name in ("ratio_rounding_0.9", "level_windows", "box_boundary", "hist_30_3_3"):
        assert not S.rescans(BY_NAME[name], BY_NAME[name]["modes"][0][0])


def test_scenes_reach_what_they_are_for():
    """properties of the oracle's answers that the scenes exist for (a scene that lost its branch must not pass silently)"""
    # the distance bound: 99 and 100 (63 and 64) match, 101 (65) does not
    for name in ("th_high_boundary_100", "th_high_boundary_64"):
        for ratio, check in modes(BY_NAME[name]):
            n, m, _ = want(name, ratio, check)
            assert n == 2 and m == [0, 1, -1]
    assert (BY_NAME["th_high_boundary_64"]["q"]["flags"] & 2).all()
    # the box: the four keypoints at exactly u +- r, v +- r are no candidates, their neighbours one float inside are
    s = BY_NAME["box_boundary"]
    n, m, _ = want("box_boundary", False, True)
    assert n == 4 and m == [-1, 1, -1, 3, -1, 5, -1, 7]
    for i in range(0, 8, 2):
        dx, dy = abs(s["un"]["x"][i] - s["q"]["u"][i]), abs(s["un"]["y"][i] - s["q"]["v"][i])
        assert max(dx, dy) == s["q"]["radius"][i] == 8 and len(S.area(s, s["q"]["u"][i], s["q"]["v"][i], 8.0, -1, -1, "box_le")) == 1
    # the stereo column: exactly r is kept, the next float is not; only a positive mvuRight is tested
    assert want("stereo_column", False, True)[1] == [0, -1, 2, -1, 4, 5, 6, -1, 8, -1]
    assert want("stereo_column_without_u_right", False, True)[1] == list(range(10))
    s = BY_NAME["stereo_column"]
    assert [abs(f32(32) - u) > 8 for u in s["ur"][:4]] == [False, True, False, True] and 0 < s["ur"][7] < 1e-44
    # the ratio pairs: (9k, 10k) accepted on one level, (9k + 1, 10k) not, both accepted on two levels; the planted are the best and second
    s = BY_NAME["ratio_rounding_0.9"]
    n, m, _ = want("ratio_rounding_0.9", True, False)
    assert n == 3 * len(s["pairs"])
    trace = []
    S.statement(s, True, trace=trace)
    for i, keys in trace:
        b1, b2 = s["pairs"][i // 4]
        assert [k[0] for k in keys] == [b1 + (i % 4) % 2, b2], i
        assert (s["un"]["octave"][keys[0][1]] == s["un"]["octave"][keys[1][1]]) == (i % 4 < 2)
    # the level ties: accepted exactly where B (the other level) precedes A, whatever the cell layout and the position of the best
    n, m, _ = want("second_level_ties", True, False)
    assert n == 6 and sorted(x for x in m if x >= 0) == list(range(6, 12))
    # equal best distances: where the cells differ the expected keypoint is the HIGHEST index among the tied ones (in one cell, the lowest)
    s = BY_NAME["first_in_grid_order"]
    log, trace = {}, []
    S.statement(s, False, True, log=log, trace=trace)
    assert len(log) == len(s["q"]) == len(s["ties"]) == 10
    for i, keys in trace:
        place, expected, tied = s["ties"][i]
        assert sorted(k for dist, k, _ in keys if dist == keys[0][0]) == sorted(tied) and len(tied) in (2, 3) and log[i] == expected, i
        assert expected == (min(tied) if place == "cell" else max(tied)), i
    # level windows: the nearest keypoint of each window, nothing in the empty window
    n, m, _ = want("level_windows", False, True)
    assert n == len(S.LEVEL_WINDOWS) - 1
    assert [None if i not in m else int(BY_NAME["level_windows"]["un"]["octave"][m.index(i)]) for i in range(len(S.LEVEL_WINDOWS))] == list(S.LEVEL_EXPECT)
    # chains: request i takes the i-th nearest; the late ones run dry
    for k, nk in S.CHAINS.items():
        for ratio, check in modes(BY_NAME["chains_%d" % k]):
            assert want("chains_%d" % k, ratio, check)[0] == min(k, nk), (k, ratio)
    # gaps: the last accepted request holds the keypoint, the count has every acceptance, occupancy only what was closed
    s = BY_NAME["chain_with_gaps"]
    for ratio, check in modes(s):
        n, m, occ = want("chain_with_gaps", ratio, check)
        assert n == s["acceptances"] and all(m[k] == i for k, i in s["holders"].items())
        assert [k for k in range(len(occ)) if occ[k]] == sorted(s["closed"]) and n > sum(x >= 0 for x in m)
    # two holders: -1 and open although the last (or the first) holder's bin is kept; one decrement per dropped entry
    s = BY_NAME["holders_in_two_bins"]
    n, m, occ = want("holders_in_two_bins", False, True)
    n0, m0, occ0 = want("holders_in_two_bins", False, False)
    assert _bins(s)[:7] == [7, 5, 4, 1, 1, 1, 1] and (n0, n) == (20, 16) and sum(x >= 0 for x in m) == 13
    for name, (k, reqs) in s["spots"].items():
        assert m[k] == -1 and occ[k] == 0 and m0[k] == reqs[-1] and occ0[k] == 1, name
    # histogram: the bins named; (10, 1, 1) keeps all, (11, 1, 1) one bin, four tens three, (30, 3, 3) all
    for name, counts in S.HISTOGRAMS.items():
        assert tuple(_bins(BY_NAME[name])[:len(counts)]) == counts and sum(_bins(BY_NAME[name])) == sum(counts)
        assert want(name, False, True)[0] == S.HISTOGRAMS_KEPT[name] and want(name, False, False)[0] == sum(counts)
    for a1, a2, b, _ in S.EDGE_ANGLES:
        assert S.rotation_bin(a1, a2) == b, (a1, a2)
    assert f32(f32(0.0) - f32(3e-5)) + f32(360) == S.BELOW_360 and f32(f32(0.0) - f32(1e-6)) + f32(360) == f32(360)
    assert max(S.rotation_bin(a, 0.0) for a in np.linspace(0, 360, 3601, dtype=f32)) == 12
    assert [b for b, c in enumerate(_bins(BY_NAME["histogram_edges"])) if c] == [0, 1, 2, 3, 12]
    assert _bins(BY_NAME["histogram_edges"])[12] == 5 and want("histogram_edges", False, True)[0] == 14 and want("histogram_edges", False, False)[0] == 18
    assert S.down(15.0) > S.HALF_BELOW > 14.9999 and S.rotation_bin(S.up(S.HALF_BELOW), 0.0) == 1
    # window edges: keypoints outside the grid have no row, whatever aims at them
    s = BY_NAME["window_edges"]
    assert not set(s["left_out"]) & set(s["idx"].tolist()) and len(s["idx"]) == len(s["un"]) - 4
    assert all(want("window_edges", False, True)[1][k] == -1 for k in s["left_out"])
    # degenerate pairs give nothing, the normal pairs beside them something
    pairs = S.degenerate_pairs()
    got = [S.oracle(p, False, True)[0] for p in pairs]
    assert got[0] > 10 and got[-1] > 10 and got[1:-1] == [0, 0, 0, 0]


def test_every_mutant_is_caught_by_its_scene():
    assert set(CAUGHT_BY) | set(EQUIVALENT) == set(S.MUTANTS) and not set(CAUGHT_BY) & set(EQUIVALENT)
    caught = {}
    for mutant in S.MUTANTS:
        for s in SCENES:
            for ratio, check in modes(s):
                if S.statement(s, ratio, check, mutant=mutant) != want(s["name"], ratio, check):
                    caught.setdefault(mutant, set()).add((s["name"], ratio))
    print("mutants caught by:", dict((k, sorted(v)) for k, v in caught.items()))
    for mutant, where in CAUGHT_BY.items():
        assert where in caught.get(mutant, ()), (mutant, sorted(caught.get(mutant, ())))
    for mutant in EQUIVALENT:
        assert mutant not in caught, (mutant, caught.get(mutant))
    # the double product is an equivalent mutant at SearchLocalPoints' 0.8f (and at 0.6f, 0.75f): no distance pair disagrees
    assert S.ratio_disagreements(0.8)[0] == []


def test_capacities_take_the_forms_the_formula_gives():
    """k_project.hip: best-key lists while projSearchLdsBytes(c, c, true) <= kLdsBudget; orbx_rows.cpp accepts while the form without fits"""
    caps = S.capacities()
    print("capacities:", [(c, S.takes_top_list(c), S.lds_bytes(c, c, S.takes_top_list(c))) for c in caps])
    assert [S.takes_top_list(c) for c in caps] == [True, True, False, False, False]
    assert all(S.is_accepted(c) for c in caps) and not S.is_accepted(caps[-1] + 1)
    assert not S.takes_top_list(caps[1] + 1) and caps[2] == caps[1] + 1 and caps[3] % 4 != 0 and caps[2] < caps[3] < caps[4]
    assert all(S.takes_top_list(c) for c in range(1, caps[1] + 1)) and all(S.is_accepted(c) for c in range(1, caps[4] + 1))
    assert S.lds_bytes(1024, 768, True) == 62 * 1024 + 136 + 6148 + 21 * 768 + 64
    assert max(len(s["un"]) for s in SCENES) <= 300 and max(len(s["q"]) for s in SCENES) <= 400


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
def _compare(got, scenes, expected, cap, label):
    nm, m, occ = got
    for p, (s, (wn, wm, wo)) in enumerate(zip(scenes, expected)):
        n = len(s["un"])
        assert int(nm[p]) == wn, (label, p, s["name"])
        assert m[p, :n].tolist() == wm, (label, p, s["name"])
        assert (m[p, n:cap] == -1).all(), (label, p, s["name"])      # -1 up to the capacity, whatever the buffer held
        assert occ[p, :n].tolist() == wo, (label, p, s["name"])
        assert not occ[p, n:].any(), (label, p, s["name"])


@pytest.mark.gpu
@pytest.mark.parametrize("cap", S.capacities())
def test_gpu_crafted_scenes_at_every_form(cap):
    """every scene in every mode it has, over poisoned outputs, with query_capacity == capacity: with best-key lists (1024 and the last such
    capacity), without (the first, one that is no multiple of 4, the largest the entry accepts); one more is refused"""
    assert S.is_accepted(cap)
    ex = X.ORBextractor(1000)
    for key, scenes in S.groups(SCENES).items():
        got = S.run_scenes(ex, scenes, cap, key)
        _compare(got, scenes, [want(s["name"], key[0], key[1]) for s in scenes], cap, key)
    if cap == S.capacities()[-1]:
        key, scenes = next(iter(S.groups(SCENES).items()))
        with pytest.raises(X.OrbxError):
            S.run_scenes(ex, scenes[:1], cap + 1, key)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", S.capacities()[:3:2])
def test_gpu_degenerate_pairs(cap):
    """between two normal pairs: a frame of 0 keypoints, n_queries = 0, all requests inactive, all keypoints closed on entry; n_queries above
    query_capacity is clamped; d_n_queries = None means query_capacity requests"""
    ex = X.ORBextractor(1000)
    pairs = S.degenerate_pairs()
    assert [p["name"] for p in pairs] == ["normal_first", "no_keypoints", "no_requests", "all_inactive", "all_closed", "normal_last"]
    for ratio, check in ((False, True), (True, False)):
        key = (ratio, check, 0.9, 100, False)
        expected = [S.oracle(p, ratio, check) for p in pairs]
        assert expected[4][2] == [1] * len(pairs[4]["un"]) and expected[1][1] == []
        _compare(S.run_scenes(ex, pairs, cap, key), pairs, expected, cap, "n_queries")
        clamped = [dict(p, n_queries_device=cap + 1000) if p.get("n_queries") is None and i % 2 == 1 else p for i, p in enumerate(pairs)]
        _compare(S.run_scenes(ex, clamped, cap, key), pairs, expected, cap, "clamped")
        # without d_n_queries every pair has query_capacity requests (the rows past a scene's own are zero: inactive)
        full = [dict(p) for p in pairs]
        full[2].pop("n_queries")
        _compare(S.run_scenes(ex, full, cap, key, n_queries=None), full, [S.oracle(p, ratio, check) for p in full], cap, "no n_queries")


def _variant(rng, s, bounds4):
    """the scene with other requests: some switched off, some without observations, other radii"""
    q = s["q"].copy()
    q["flags"] = np.where(rng.random(len(q)) < 0.85, 1, 0) | np.where(rng.random(len(q)) < 0.7, 2, 0)
    q["radius"] = rng.choice([9.0, 14.0, 30.0], len(q)).astype(f32)
    return dict(s, q=q, occ=(rng.random(len(s["un"])) < 0.1).astype(np.uint8), bounds=bounds4)


@pytest.mark.gpu
@pytest.mark.parametrize("ratio", [False, True])
def test_gpu_walks(ratio):
    """several request sets against one frame (cur step 0), each with its own occupancy row; one descriptor block for several pairs (desc step 0);
    non-zero first indices with a frame step of 2.  Every pair against the oracle."""
    rng = np.random.default_rng(27)
    base = [dict(crowd_scene(rng, n=int(rng.integers(150, 250)), nq=300, clusters=4, ratio=ratio), name="crowd%d" % i, stereo=False, nnratio=0.8,
                 max_distance=100) for i in range(5)]
    b4 = base[0]["bounds"]
    ex = X.ORBextractor(1000)
    cap, qcap, P = 1024, 512, 3
    run = lambda frames, reqs, cur, desc, blocks: S.run_device(ex, frames, reqs, cur, desc, blocks, len(reqs), cap, qcap, ratio, 0.8, not ratio, 100, False,
                                                               bounds4=b4)
    def exp(reqs):      # the oracle's answers; every pair of every walk really matches
        out = [S.oracle(r, ratio, not ratio) for r in reqs]
        assert min(e[0] for e in out) > 10 and min(sum(x >= 0 for x in e[1]) for e in out) > 10
        return out
    # one frame (device frame 2), three request sets with their own descriptors and occupancy
    reqs = [_variant(rng, base[2], b4) for _ in range(P)]
    for r in reqs:
        r["qd"] = np.where(rng.random((300, 1)) < 0.5, r["qd"], np.roll(r["qd"], 1, axis=0))
    _compare(run(base[:3], reqs, (2, 0), (0, 1), [r["qd"] for r in reqs]), reqs, exp(reqs), cap, "one frame")
    # one descriptor block (block 2 of three) for three pairs on frames 0, 1, 2, three views of one scene (a few descriptor bits differ): the
    # same MapPoint descriptors meet other frames, requests and occupancy
    views = [dict(base[1], d=base[1]["d"] ^ (np.uint8(1) << rng.integers(0, 8, base[1]["d"].shape, dtype=np.uint8)) * (rng.random(base[1]["d"].shape) < 0.03))
             for _ in range(P)]
    reqs = [_variant(rng, v, b4) for v in views]
    _compare(run(views, reqs, (0, 1), (2, 0), [base[0]["qd"][::-1], base[2]["qd"], base[1]["qd"]]), reqs, exp(reqs), cap, "one descriptor block")
    # frames 1 and 3 of five, descriptor blocks 2 and 3 of four
    reqs = [_variant(rng, base[1], b4), _variant(rng, base[3], b4)]
    _compare(run(base, reqs, (1, 2), (2, 1), [base[0]["qd"], base[4]["qd"], reqs[0]["qd"], reqs[1]["qd"]]), reqs, exp(reqs), cap, "first 1, step 2")


# k_project_last: fx = fy = 256, cx = 256, cy = 192, the current pose is the identity, depths and coordinates are powers of two (or one float
# beside them), so u = 256 * x / z + 256 and v = 256 * y / z + 192 are exact and every expected field is written by hand
MB, MBF, TH = 0.125, 32.0, 8.0
_B = f32(2) ** -21        # one float step at 4 .. 8
POINTS = (   # world point, mpFlags, octave, expected (u, v) or None = no request
    ((-4.0, 0.0, 4.0), 3, 0, (0.0, 192.0)),                  # u = mnMinX exactly: kept
    ((-4.0 - 2 * float(_B), 0.0, 4.0), 3, 0, None),          # u = -2^-14 (one float step of the sum's operand 256 + 2^-14): dropped
    ((4.0, 0.0, 4.0), 3, 1, (512.0, 192.0)),                 # u = mnMaxX: kept
    ((4.0 + 2 * float(_B), 0.0, 4.0), 3, 1, None),           # u = the float above 512: dropped
    ((0.0, -3.0, 4.0), 3, 2, (256.0, 0.0)),                  # v = mnMinY
    ((0.0, -3.0 - float(_B), 4.0), 3, 2, None),
    ((0.0, 3.0, 4.0), 3, 3, (256.0, 384.0)),                 # v = mnMaxY
    ((0.0, 3.0 + float(_B), 4.0), 3, 3, None),               # v = the float above 384
    ((0.0, 0.0, -4.0), 3, 0, None),                          # invzc < 0
    ((0.0, 0.0, -1.401298464324817e-45), 3, 0, None),        # the smallest negative float: invzc = -inf < 0
    ((1.0, 1.0, 0.0), 3, 0, None),                           # invzc = +inf is not < 0; u = +inf > mnMaxX
    ((0.0, 0.0, 0.0), 3, 4, "nan"),                          # u = 0 / 0: no comparison drops it; the reference keeps an active request of NaNs
    ((0.0, 0.0, -0.0), 3, 5, "nan"),                         # 0 * 0 + 0 * 0 + 1 * -0 is +0 and stays +0 with tcw.z = -0: z = +0 again
    ((-0.0, -0.0, -0.0), 3, 6, None),                        # three products of -0 and tcw.z = -0: z = -0, invzc = -inf < 0 (z < 0 would keep it)
    ((0.0, 0.0, float("inf")), 3, 1, "nan"),                 # z = +inf: invzc = +0 is not < 0; 0 * inf makes x and y NaN
    ((1.0, 0.5, 4.0), 1, 0, (320.0, 224.0)),                 # octave 0, no observations
    ((1.0, 0.5, 2.0), 3, 7, (384.0, 256.0)),                 # octave 7
    ((1.0, 0.5, 4.0), 0, 2, None),                           # no MapPoint
    ((1.0, 0.5, 4.0), 2, 2, None),                           # bit 0 clear
    ((-1.0, -0.5, 8.0), 3, 5, (224.0, 176.0)),
)
NAN_ROWS = [i for i, p in enumerate(POINTS) if p[3] == "nan"]
TLC_Z = (0.0, MB, float(S.up(MB)), -MB, -float(S.up(MB)))      # tlc.z of the five last frames: neither, == mb: neither, forward, == -mb: neither, backward


def _project_setup():
    n, cap, F = len(POINTS), 24, len(TLC_Z) + 1
    k = np.zeros((F, cap), O.KEYPOINT_DTYPE); flags = np.zeros((F, cap), np.uint8); world = np.zeros((F, cap, 3), f32)
    poses = np.zeros((F, 3, 4), f32); nout = np.full(F, n, np.int32)
    poses[:, :, :3] = np.eye(3, dtype=f32)
    poses[F - 1, 2, 3] = -0.0                             # the current pose: the identity with tcw.z = -0, so that a z of -0 can reach the camera frame
    for f, z in enumerate(TLC_Z):
        poses[f, 2, 3] = z                                # current pose = identity: tlc = Rlw * 0 + tlw
        for i, (xw, fl, o, _) in enumerate(POINTS):
            world[f, i], flags[f, i], k[f, i]["octave"], k[f, i]["angle"] = xw, fl, o, 10.0 * i
        flags[f, n:] = 3                                  # beyond n_out: never read as MapPoints
        world[f, n:] = (0.0, 0.0, 4.0)
    return n, cap, F, k, flags, world, poses, nout


def _project_expected(mono):
    """the requests of every pair, by hand"""
    sc = np.asarray(X.compute_tables(1000, 1.2, 8)["scale_factors"], f32)
    n, cap = len(POINTS), 24
    out = np.zeros((len(TLC_Z), cap), O.PROJ_QUERY_DTYPE)
    for f, z in enumerate(TLC_Z):
        forward, backward = (f == 2 and not mono), (f == 4 and not mono)
        for i, (xw, fl, o, uv) in enumerate(POINTS):
            if uv is None:
                continue
            r = out[f, i]
            if uv == "nan":
                r["u"] = r["v"] = r["ur"] = np.nan
            else:
                r["u"], r["v"] = uv
                r["ur"] = f32(uv[0]) - f32(MBF) / f32(xw[2])      # invzc = 1 / z is a power of two: mbf * invzc is exact
            r["radius"] = f32(TH) * sc[o]
            r["min_level"], r["max_level"] = (o, -1) if forward else (0, o) if backward else (o - 1, o + 1)
            r["flags"], r["angle"] = 1 | (fl & 2), 10.0 * i
    return out


def _same_requests(got, exp):
    """byte for byte, but a NaN equals a NaN: sign and payload of 0 / 0 are not pinned by the reference's arithmetic"""
    for name in got.dtype.names:
        a, b = got[name], exp[name]
        if a.dtype.kind == "f":
            nan = np.isnan(a) & np.isnan(b)
            if not np.array_equal(np.where(nan, 0, a).view(np.uint32), np.where(nan, 0, b).view(np.uint32)):
                return False
        elif not np.array_equal(a, b):
            return False
    return True


def test_project_last_edges_by_hand_equal_the_oracle():
    n, cap, F, k, flags, world, poses, nout = _project_setup()
    assert f32(256) * f32(-4.0 - 2 * float(_B)) / f32(4) + f32(256) == -f32(2) ** -14 and f32(256) * f32(4.0 + 2 * float(_B)) / f32(4) + f32(256) == S.up(512.0)
    assert f32(256) * f32(3.0 + float(_B)) / f32(4) + f32(192) == S.up(384.0) and f32(256) * f32(-3.0 - float(_B)) / f32(4) + f32(192) == -f32(2) ** -15
    sc = np.asarray(X.compute_tables(1000, 1.2, 8)["scale_factors"], f32)
    for mono in (False, True):
        exp = _project_expected(mono)
        for f in range(len(TLC_Z)):
            q = O.project_last_frame(k[f, :n], k[f, :n], flags[f, :n], world[f, :n], poses[F - 1], poses[f], S.CAM, S.bounds(), sc, MBF, MB, TH, mono)
            assert _same_requests(q, exp[f, :n]), (mono, f)
    exp = _project_expected(False)
    assert (exp["flags"][0] != 0).sum() == 10 and not exp["flags"][0, 13] and exp["max_level"][2].min() == -1 and (exp["min_level"][4][exp["flags"][4] != 0] == 0).all()
    assert np.array_equal(exp["min_level"][1], exp["min_level"][0]) and np.array_equal(exp["max_level"][3], exp["max_level"][0])
    assert _same_requests(_project_expected(True)[2], exp[0]) and exp["radius"][0, 16] == f32(8) * sc[7] and exp["radius"][0, 15] == 8 and NAN_ROWS == [11, 12, 14]


@pytest.mark.gpu
@pytest.mark.parametrize("mono", [False, True])
def test_gpu_project_last_edges(mono):
    """k_project_last on the strict comparisons of :1999-2008 and :1981-1982, z = +-0, the three level windows at octaves 0 and 7, the MapPoint
    flags and the rows past n_out: against the hand-written requests and byte for byte (NaN-aware) against the oracle; then the search on
    those requests, where the request of NaNs matches nothing"""
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    n, cap, F, k, flags, world, poses, nout = _project_setup()
    P = len(TLC_Z)
    ex = X.ORBextractor(1000)
    d_q = torch.full((P, cap, 8), -7.0, dtype=torch.float32, device="cuda")
    d_k = dev(k.view(np.uint8))
    ex.project_last_frame_device(P, (0, 1), (F - 1, 0), d_k, d_k, dev(nout), cap, dev(flags), dev(world), dev(poses), S.CAM, S.bounds(), MBF, MB, TH, mono, d_q)
    ex.synchronize()
    got = d_q.cpu().numpy().view(np.uint8).reshape(P, cap, 32).copy().view(O.PROJ_QUERY_DTYPE).reshape(P, cap)
    exp = _project_expected(mono)
    sc = np.asarray(X.compute_tables(1000, 1.2, 8)["scale_factors"], f32)
    for p in range(P):
        assert _same_requests(got[p], exp[p]), (mono, p)
        assert not got[p, n:].view(np.uint8).any()
        q = O.project_last_frame(k[p, :n], k[p, :n], flags[p, :n], world[p, :n], poses[F - 1], poses[p], S.CAM, S.bounds(), sc, MBF, MB, TH, mono)
        assert _same_requests(got[p, :n], q), (mono, p)
        assert np.isnan(got[p, NAN_ROWS]["u"]).all() and (got[p, NAN_ROWS]["flags"] == 3).all()
    # the search on these requests: a frame with a keypoint at every projected position, the requests' descriptors its own
    b = S.Builder("projected", 50)
    qd = np.zeros((n, 32), np.uint8)
    for i, (_, _, o, uv) in enumerate(POINTS):
        qd[i] = b.descriptor()
        if isinstance(uv, tuple) and uv[0] < 500 and uv[1] < 370:
            b.keypoint(uv[0], uv[1], S.away(qd[i], 2), octave=o, angle=10.0 * i)
    for i in NAN_ROWS:
        b.keypoint(256.0, 192.0, qd[i], octave=POINTS[i][2], angle=10.0 * i)   # what a request of NaNs would take if it saw anything
    frame = b.build()
    pairs = [dict(frame, name="pair%d" % p, q=got[p, :n].copy(), qd=qd, stereo=False) for p in range(P)]
    res = S.run_device(ex, [frame], pairs, (0, 0), (0, 0), [qd], P, 64, 32, False, 0.9, True, 100, False)
    for p in range(P):
        wn, wm, wo = S.oracle(pairs[p], False, True)
        assert not set(NAN_ROWS) & set(wm) and wn == 5
    _compare(res, pairs, [S.oracle(pp, False, True) for pp in pairs], 64, "search")
