"""orbx_search_for_triangulation_device on crafted scenes (tests/triangulation_scenes.py): the epipolar gate and the epipole's disc on the
last binary32 value of either side, distances at th_low, ties at chosen list positions and lanes, segment and row counts around the
kernel's 16 lanes and 64 rows, capacities 1 .. 1025 and the two on either side of the staging threshold (2720 staged, 2721 unstaged), raw
octaves outside the tables, the rotation histogram's rules, FeatureVector indices at or above the frame's count and stale counts.

CPU: on every scene under every Run it is searched with, the walk (tests/triangulation_walk.py) equals the independent per-feature
statement (test_search_triangulation.brute), every probe ends where the builder planted it, and the walk's counters are the planted ones.
GPU: every scene that fits a capacity goes in as one pair of one call per Run, under lds_pollute 0xC3 with the outputs pre-filled with
POISON, and equals the walk exactly; the probes are asserted on the device's own output as well.  The device is handed the FeatureVector
with the entries that name no feature and the stale counts; the walk is handed the FeatureVector without them (it is not changed)."""
import numpy as np
import pytest

import extractorb_amd as X
import test_search_triangulation as T
import triangulation_scenes as S
from triangulation_scenes import Run, options

CAPACITIES = (1, 15, 16, 17, 100, 1025, 2720, 2721)      # 2720: the largest staged; 2721: the first unstaged


def expected(expect, run):
    return expect(run) if callable(expect) else expect


def without_u_right(s):
    mono = lambda kf: dict(kf, ur=np.full(len(kf["ur"]), -1, np.float32))      # noqa: E731
    return dict(s, kf1=mono(s["kf1"]), kf2=mono(s["kf2"]))


def runs_of(scenes):
    out = []
    for s in scenes:
        out += [r for r in s["runs"] if r not in out]
    return out


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
def test_every_scene_is_tens_of_features_and_every_probe_names_a_feature():
    scenes = S.scenes()
    assert len(scenes) >= 30 and sum(len(s["probes"]) for s in scenes) >= 250
    for s in scenes:
        n_fv = max(len(s["kf1"]["fv"][0]), len(s["kf2"]["fv"][0]))
        assert n_fv <= 260 and s["probes"], s["name"]
        assert all(0 <= i1 < len(s["kf1"]["desc"]) for i1, _ in s["probes"].values()), s["name"]
        for kf in (s["kf1"], s["kf2"]):                 # a FeatureVector: nodes ascending, every index a feature of the walk's keyframe
            assert (np.diff(kf["fv"][0].astype(np.int64)) >= 0).all() and (kf["fv"][1] < max(len(kf["desc"]), 1)).all(), s["name"]


@pytest.mark.parametrize("index", range(len(S.scenes())), ids=[s["name"] for s in S.scenes()])
def test_walk_equals_the_per_feature_statement_and_every_probe_ends_where_it_was_planted(index):
    s = S.scenes()[index]
    for run in s["runs"]:
        with np.errstate(invalid="ignore"):             # (the scenes with an infinity or a NaN in them)
            w = T.walk(s, run.ur, **options(run))
            n, m12 = T.brute(s if run.ur else without_u_right(s), **options(run))
        assert w["n"] == n and w["matches12"] == m12, (s["name"], run)
        assert w["n"] == len(w["pairs"]) == sum(m >= 0 for m in w["matches12"])
        for name, (i1, expect) in s["probes"].items():
            assert w["matches12"][i1] == expected(expect, run), (name, run, w["matches12"][i1])
        for counter, value in s["counters"].items():
            if value(run) is not None:
                assert w[counter] == value(run), (s["name"], counter, run, w[counter])


def test_gate_and_disc_values_are_neighbours_on_either_side_of_the_bound():
    for o in range(8):
        a, b = S.gate_pair(o)
        lim = 3.84 * float(S.SIG2[o])
        assert b == np.nextafter(a, S.INF) and float(np.float32(a * a)) < lim <= float(np.float32(b * b))
        if o:
            a, b = S.disc_pair(o)
            lim = np.float32(np.float32(100) * S.SF[o])
            assert b == np.nextafter(a, S.INF) and np.float32(a * a) < lim and not np.float32(b * b) < lim


def test_scenes_reach_what_they_are_for():
    by = {s["name"]: s for s in S.scenes()}
    assert T.walk(by["ties"])["equal"] == 5 and T.walk(by["disc"], True, **options(S.COARSE))["disc"] == 12
    assert T.walk(by["disc"], False, **options(Run(ur=False, coarse=True)))["disc"] == 40
    assert T.walk(by["distance"], True, **options(Run(th_low=-1)))["n"] == 0 and T.walk(by["distance"], True, **options(Run(th_low=300)))["n"] == 7
    assert T.walk(by["nothing"])["n"] == 0 and T.walk(by["rotation"])["removals"] == 3
    assert [len(by["full_%d" % n]["kf1"]["fv"][0]) for n in S.FULL] == list(S.FULL)          # M1: one, two and three trips of the 64-row loop
    per_node = np.bincount(by["segments"]["kf2"]["fv"][0])
    assert sorted(per_node[per_node > 0].tolist()) == [1, 15, 16, 17, 32, 33, 100]
    assert len(set(by["one_node"]["kf2"]["fv"][0].tolist())) == 1 and len(by["one_node"]["kf2"]["desc"]) == 100
    assert {i1 for i1, _ in by["compaction_1025"]["probes"].values()} == {0, 1023, 1024} and S.size(by["compaction_1025"]) == 1025
    # what the device is handed beyond the walk's keyframes
    g = by["octaves"]["gpu"]["kf2"]["kps"]["octave"]
    assert {-1, 8, 255} <= set(g.tolist()) and by["octaves"]["kf2"]["kps"]["octave"].max() == 7 and by["octaves"]["kf2"]["kps"]["octave"].min() == 0
    g = by["phantom_candidate"]["gpu"]
    assert (g["kf2"]["fv"][1] >= g["nout"][1]).sum() == 2 and len(by["phantom_candidate"]["kf2"]["fv"][1]) == 2
    g = by["phantom_key"]["gpu"]
    assert (g["kf1"]["fv"][1] >= g["nout"][0]).sum() == 1
    assert all(S.size(by["plus_five_%d" % c]) == c for c in S.PLUS_FIVE) and set(S.PLUS_FIVE) <= set(CAPACITIES)
    assert all(any(S.size(s) <= c for s in S.scenes()) for c in CAPACITIES) and S.size(by["full_1"]) == 1


def test_staging_threshold_is_between_2720_and_2721():
    assert T.lds_bytes(2720, staged=True) <= T.LDS_LIMIT < T.lds_bytes(2721, staged=True) and T.lds_bytes(2721) <= T.LDS_LIMIT


def test_header_states_what_an_index_at_or_above_the_count_means():
    text = open(X.orbextractor._HEADER).read()
    for entry in ("orbx_search_for_triangulation_device", "orbx_search_for_triangulation_two_eyes_device", "orbx_search_by_bow_device",
                  "orbx_search_by_bow_two_eyes_device"):
        pos = text.index("int %s(" % entry)
        doc = text[text.rindex("/*", 0, pos):pos]
        assert "names no feature" in doc, entry


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
def fits(s, cap):
    return S.size(s) == cap if s["name"].startswith("plus_five_") else S.size(s) <= cap      # (counts of capacity + 5 need the scene that fills it)


def run_group(ex, group, cap, run):
    """the scenes of `group` as the pairs of ONE call at capacity cap under `run`: every scene against its walk, every probe on the device's output"""
    views = [S.gpu_view(s) for s in group]
    dv = T.pack([k for v in views for k in (v["kf1"], v["kf2"])], cap)
    for p, s in enumerate(group):                        # stale counts
        g = s.get("gpu", {})
        for key in ("nout", "nfeat"):
            for e, v in enumerate(g.get(key, (None, None))):
                if v is not None:
                    dv[key][2 * p + e] = v
    m, pr, nm = T.run(ex, dv, views, (0, 2), (1, 2), cap, run.ur, **options(run))
    for p, s in enumerate(group):
        what = "%s capacity %d %r" % (s["name"], cap, run)
        T.assert_equals_walk(s, m[p], pr[p], nm[p], what, run.ur, **options(run))
        for name, (i1, expect) in s["probes"].items():
            assert int(m[p][i1]) == expected(expect, run), (name, what)


@pytest.mark.gpu
@pytest.mark.parametrize("cap", CAPACITIES)
def test_gpu_every_scene_that_fits_equals_the_walk_under_pollution(cap):
    assert (T.lds_bytes(cap, staged=True) <= T.LDS_LIMIT) == (cap <= 2720) and T.lds_bytes(cap) <= T.LDS_LIMIT
    import torch
    torch.zeros(1).cuda()                               # torch asks for the GPU first
    X.debug_set_option("lds_pollute", S.POLLUTION)      # before the handle is made; tests/conftest.py resets the aids after the test
    ex = X.ORBextractor(1200)
    assert "lds_pollute:%d" % S.POLLUTION in ex.policy()
    scenes = [s for s in S.scenes() if fits(s, cap)]
    assert scenes
    if cap >= 1025:
        assert len(scenes) == len(S.scenes()) - len(S.PLUS_FIVE)      # every scene but the ones made for one capacity
    before = ex.lds_pollutions()
    calls = 0
    for run in runs_of(scenes):
        group = [s for s in scenes if run in s["runs"]]
        run_group(ex, group, cap, run)
        calls += 1
    assert ex.lds_pollutions() == before + calls         # one kernel per call, each behind a pollution
