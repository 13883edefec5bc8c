"""The triangulation loop of LocalMapping::CreateNewMapPoints without a GPU: extractorb_amd/csrc/k_new_map_points.hpp - the statement of
k_new_map_points.hip - compiled for the host (tests/cpp/new_map_points_host_check.cpp: every thread's staging, every lane's match) against the
sequential walk (tests/new_map_points_walk.py) on the scenes of tests/new_map_points_scenes.py, byte for byte, for both rig kinds:
  (a) the crafted scenes at capacity 32 (per eye), four pairs with kf1_step = 0, one of them (0, 0): exit codes, x3d bits, counts, marks and
      the debug counters; a histogram over orbx_new_point_exit with no zero entry and every kind of match on the exit it was built for;
  (b) edge scenes: a NaN rotation (everything leaves by LOW_PARALLAX), a NaN cosParallaxRays, the monocular call with NULL stereo arrays,
      NLeft = 0, an empty pair list, n_matches past the capacity and negative, bad indices, octaves outside the tables, ZERO_DIST;
  (c) the semantics the header lists: the `else if` of the stereo parallax, UnprojectStereo reading mvKeys, the pose and camera picked per
      match, the marks never cleared;
  (d) the margin condition: on MARGIN_SEEDS the float64 kind of the walk takes the same exit clear of every threshold, and the accepted
      points agree within a bound derived here from the parallax;
  (e) cos(2*atan2f) against the host libm on every float of [pi, 2 pi] and its negative; the sanitizer program; the declarations."""
import collections
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import extractorb_amd as X
import new_map_points_scenes as SC
import new_map_points_walk as NW
from test_kb8_math import HOST_FLAGS, ROOT, settle
from test_kb8_unproject_math import same_floats

f32 = np.float32
VP = C.c_void_p
POISON_EXIT, POISON_X, POISON_N = 0xEE, -7.0, -559038737
KIND_EXIT = dict(tri=NW.TRIANGULATED, tri_s1=NW.TRIANGULATED, tri_s2=NW.TRIANGULATED, tri_both=NW.TRIANGULATED, st1=NW.STEREO_1, st2=NW.STEREO_2,
                 st_both=NW.STEREO_1, empty=NW.EMPTY_STEREO, low=NW.LOW_PARALLAX, behind1=NW.BEHIND_1, behind2=NW.BEHIND_2, reproj1=NW.REPROJ_1,
                 reproj2=NW.REPROJ_2, far=NW.FAR, scale=NW.SCALE, oct=NW.TRIANGULATED, bad=NW.BAD_INDEX, zero_w=NW.ZERO_W, zero_dist=NW.ZERO_DIST)
# What binary32 costs an accepted point against float64, relative to its distance from keyframe 1.  Both kinds read the same binary32
# pixels and poses.  u = 2^-24 is the unit roundoff.  A Pinhole ray component carries 4 roundings (a subtraction and a division, then a product
# and a difference in its row of A): at most 4 u.  A KannalaBrandt8 ray component carries about 17: 2 in pw, 3 in theta_d (two products, a sum;
# the root is exact to 0.5 u), about 8 in the last Newton step (the polynomial, the product, the difference, the quotient: the earlier steps'
# errors are contracted away, the iteration ends below 1e-6), tanf (0.5 u, its argument's error amplified by at most 1.3 below 35 degrees), the
# quotient, the product, and 2 in the row of A.  Their worst case, 17 u = 1.0e-6, is what tests/test_stereo_fisheye.py uses; but the
# roundings are independent and each is uniform over +-0.5 ulp of a value of either binade, a standard deviation of at most 0.41 u, so their
# sum has at most 0.41 * sqrt(17) = 1.7 u and SIX standard deviations are 10 u = 6.0e-7: the bound taken here for some sixty points
# (a worst-case bound would not notice a loss of accuracy below a factor of 17 / 1.7).
# How far a ray error moves the point is the scene's geometry - for two rays about 2 e / parallax of the distance, the distance being baseline /
# parallax angle (0.5 m / 6 m = 0.08 for the farthest ordinary point, 0.05 for the far one) - and is taken from the match itself, not from that
# estimate: triangulation_bound() moves each of the four ray components by e * max(1, |component|) in the FLOAT64 statement and adds up the
# moves of the point (first order, every error at its worst sign).  nullVector4 adds a homogeneous-vector error of 3.44e-8 / sigma_3
# (the residual excess docs/history/r18_two_eyes_triangulation.md measured over 10^5 matrices, over the third singular value of this A),
# which moves x = v[0..2] / v[3] by that times (1 + |x|^2).  UnprojectStereo is two products, a gemm row and no parallax: 4 u of the distance.
RAY_ERROR = {False: 4 * 2.0 ** -24, True: 10 * 2.0 ** -24}


def triangulation_bound(s, p, k, e):
    """the absolute first-order bound of the comment above for match k of pair p of scene s, from the float64 kind of the walk"""
    N = NW.Float64()
    a, b = SC.pair_frames(s)[p]
    two = s["two_eyes"]
    v1, v2 = N.views(s["kfs"][a]["pose"], s["tlr"]), N.views(s["kfs"][b]["pose"], s["tlr"])
    o1, o2 = NW.observation(N, s["kfs"][a], s["pairs"][p][k][0], two), NW.observation(N, s["kfs"][b], s["pairs"][p][k][1], two)
    view1, view2 = v1[o1["eye"]], v2[o2["eye"]]
    cam1, cam2 = (s["cams"][o1["eye"]], s["cams"][o2["eye"]]) if two else (s["cams"], s["cams"])
    xn1, xn2, _ = NW.rays_and_parallax(N, view1, view2, cam1, cam2, o1, o2, two)
    x0, _ = NW.triangulate(N, xn1, xn2, view1, view2)
    x0 = np.array(x0)
    moved = 0.0
    for which in (0, 1):
        for c in (0, 1):
            q = [list(xn1), list(xn2)]
            q[which][c] += e * max(1.0, abs(q[which][c]))
            moved += float(np.linalg.norm(np.array(NW.triangulate(N, q[0], q[1], view1, view2)[0]) - x0))
    rows = []
    for xn, (R, t, _) in ((xn1, view1), (xn2, view2)):
        T = np.hstack([np.asarray(R, np.float64), np.asarray(t, np.float64)[:, None]])
        rows += [xn[0] * T[2] - T[0], xn[1] * T[2] - T[1]]
    sigma3 = float(np.linalg.svd(np.array(rows))[1][2])
    return moved + 3.44e-8 / sigma3 * (1.0 + float(x0 @ x0))


def build_host(directory):
    so = os.path.join(str(directory), "libnew_map_points_host.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", *HOST_FLAGS, os.path.join(ROOT, "tests", "cpp", "new_map_points_host_check.cpp"), "-o", so])
    L = C.CDLL(so)
    L.nmp_host.argtypes = [C.c_int] * 6 + [VP] * 10 + [C.c_int, VP, VP, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, C.c_float] + [VP] * 6
    L.nmp_host.restype = None
    L.nmp_stereo_cos.restype = C.c_float
    L.nmp_stereo_cos.argtypes = [C.c_float, C.c_float]
    L.nmp_check_cos.restype = C.c_long
    L.nmp_check_cos.argtypes = [C.c_int, C.POINTER(C.c_long)]
    L.nmp_check_stereo_cos.restype = C.c_long
    L.nmp_check_stereo_cos.argtypes = [C.c_long, C.c_ulonglong]
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("nmphost"))


def ptr(a):
    return None if a is None else a.ctypes.data_as(VP)


_SCENES, _WALKS = {}, {}


def scene(two_eyes, seed, variant=None):
    key = (two_eyes, seed, variant)
    if key not in _SCENES:
        _SCENES[key] = SC.make(two_eyes, seed) if variant is None else SC.variant(scene(two_eyes, seed), variant)
    return _SCENES[key]


def walk(s):
    """the binary32 walk of a scene, computed once (the scene object is the key) and left unchanged"""
    if id(s) not in _WALKS:
        _WALKS[id(s)] = (s, SC.walk(s))
    return _WALKS[id(s)][1]


def cams16(s):
    c = np.zeros(16, f32)
    if s["two_eyes"]:
        c[:8], c[8:] = s["cams"][0], s["cams"][1]
    else:
        c[:4] = s["cams"][:4]
    return c


def outputs(d, marks=True):
    P, L, cap = d["P"], d["L"], d["cap"]
    return dict(exit=np.full((P, L), POISON_EXIT, np.uint8), x3d=np.full((P, L, 3), POISON_X, f32), n_new=np.full(P, POISON_N, np.int32),
                mark1=np.zeros((P, L), np.uint8) if marks else None, mark2=np.zeros((P, L), np.uint8) if marks else None)


def host_run(host, s, d=None, marks=True, far_points=None):
    d = d or SC.pack(s)
    o = outputs(d, marks)
    stats = np.zeros(2, np.int32)
    far = s["far_points"] if far_points is None else far_points
    host.nmp_host(int(s["two_eyes"]), d["P"], s["kf1"][0], s["kf1"][1], s["kf2"][0], s["kf2"][1], ptr(d["pairs"]), ptr(d["n_matches"]), ptr(d["poses"]),
                  ptr(None if s["tlr"] is None else np.ascontiguousarray(s["tlr"], f32)), ptr(cams16(s)), ptr(d["kps_un"]), ptr(d["kps"]), ptr(d["u_right"]),
                  ptr(d["depth"]), ptr(d["n_out"]), d["cap"], ptr(SC.TAB["scale"]), ptr(SC.TAB["sigma2"]), 8, float(SC.TAB["ratio_factor"]), s["mb"],
                  s["mbf"], int(far), s["th_far"], ptr(o["exit"]), ptr(o["x3d"]), ptr(o["n_new"]), ptr(o["mark1"]), ptr(o["mark2"]), ptr(stats))
    o["stats"] = (int(stats[0]), int(stats[1]))
    return o


def expected_marks(s, w, cap, which):
    """the flag rows the walk's accepted matches set: [p][eye * capacity + i] (one camera: eye 0)"""
    P = len(w)
    m = np.zeros((P, (2 if s["two_eyes"] else 1) * cap), np.uint8)
    for p, r in enumerate(w):
        for eye, i in r[which]:
            m[p, eye * cap + i] = 1
    return m


def assert_equals_walk(o, s, w=None, what="", n_matches=None):
    """exit codes, the bits of x3d, the counts, the marks and the debug counters of every pair; every entry from n_matches on still holds
    the poison.  n_matches: what the call was given when it differs from the lists' lengths (the walk then sees the clamped list)."""
    w = w or walk(s)
    cap = s["cap"]
    L = 2 * cap if s["two_eyes"] else cap
    for p, r in enumerate(w):
        n = len(r["exit"])
        assert o["exit"][p, :n].tolist() == r["exit"], (what, p, [NW.EXIT_NAMES[e] for e in o["exit"][p, :n]], [NW.EXIT_NAMES[e] for e in r["exit"]])
        assert same_floats(o["x3d"][p, :n], r["x3d"].astype(f32)), (what, p)
        assert (o["exit"][p, n:] == POISON_EXIT).all() and (o["x3d"][p, n:] == POISON_X).all(), (what, p, "an entry past n_matches was written")
        assert int(o["n_new"][p]) == r["n_new"], (what, p, int(o["n_new"][p]), r["n_new"])
        assert (o["x3d"][p, :n][np.array(r["exit"]) > NW.STEREO_2] == 0).all(), (what, p, "a rejected match holds a point")
    if o.get("mark1") is not None:
        assert np.array_equal(o["mark1"][:, :L], expected_marks(s, w, cap, "mark1")) and np.array_equal(o["mark2"][:, :L], expected_marks(s, w, cap, "mark2")), what
    if "stats" in o:
        assert o["stats"] == (sum(r["svd"] for r in w), sum(r["stereo"] for r in w)), (what, o["stats"])


def histogram(s):
    h = collections.Counter()
    for r in walk(s):
        h.update(r["exit"])
    return h


# ---- (a) ----
def test_every_exit_and_every_branch_is_reached():
    one, two, zd = scene(False, 1), scene(True, 1), SC.zero_dist_scene()
    h1, h2 = histogram(one) + histogram(zd), histogram(two)
    assert all(h1[e] > 0 for e in range(14)), {NW.EXIT_NAMES[e]: h1[e] for e in range(14)}      # one camera: no zero entry
    never = {NW.STEREO_1, NW.STEREO_2, NW.EMPTY_STEREO, NW.ZERO_DIST}       # two eyes: bStereo is false by construction; ZERO_DIST see zero_dist_scene
    assert all((h2[e] > 0) == (e not in never) for e in range(14)), {NW.EXIT_NAMES[e]: h2[e] for e in range(14)}
    for s in (one, two, zd):
        for p, r in enumerate(walk(s)):
            for kind, e in zip(s["kinds"][p], r["exit"]):
                assert kind == "self" or KIND_EXIT[kind] == e, (s["two_eyes"], p, kind, NW.EXIT_NAMES[e])
    # all four eye combinations made a point (:503-568), told by the stacked indices of the accepted matches of pair (0, 1)
    n0, n1 = len(two["kfs"][0]["eyes"][0]["kps"]), len(two["kfs"][1]["eyes"][0]["kps"])
    combos = {(a >= n0, b >= n1) for (a, b), e in zip(two["pairs"][1], walk(two)[1]["exit"]) if e == NW.TRIANGULATED}
    assert combos == {(False, False), (False, True), (True, False), (True, True)}
    assert len(one["pairs"]) == 4 and SC.pair_frames(one)[0] == (0, 0) and one["kf1"][1] == 0 and one["cap"] == 32


@pytest.mark.parametrize("two_eyes", [False, True])
@pytest.mark.parametrize("seed", SC.MARGIN_SEEDS)
def test_host_kernel_equals_the_walk_on_the_crafted_scenes(host, two_eyes, seed):
    s = scene(two_eyes, seed)
    o = host_run(host, s)
    assert_equals_walk(o, s, what="crafted")
    assert o["stats"][0] > 10 and (o["stats"][1] > 3) == (not two_eyes)
    o2 = host_run(host, s, marks=False)                                                          # d_mark1 = d_mark2 = NULL
    assert_equals_walk(o2, s, what="no marks")


# ---- (b) ----
@pytest.mark.parametrize("two_eyes,name", [(False, "nan_pose"), (True, "nan_pose"), (False, "nan_parallax"), (True, "nan_parallax"), (False, "mono"),
                                           (True, "nleft_zero")])
def test_edge_variants(host, two_eyes, name):
    s = scene(two_eyes, 1, name)
    w = walk(s)
    if name == "nan_pose":                                                                       # every test is false on a NaN
        assert all(e in (NW.LOW_PARALLAX, NW.BAD_INDEX) for e in w[1]["exit"]) and w[1]["n_new"] == 0 and NW.LOW_PARALLAX in w[1]["exit"]
        assert w[2]["n_new"] == walk(scene(two_eyes, 1))[2]["n_new"]
    elif name == "nan_parallax":
        assert w[3]["exit"][0] == NW.LOW_PARALLAX                                                # cosParallaxRays = 0 / 0: not ZERO_W here
    elif name == "mono":
        assert all(e not in (NW.STEREO_1, NW.STEREO_2, NW.EMPTY_STEREO) for r in w for e in r["exit"]) and sum(r["stereo"] for r in w) == 0
        assert SC.pack(s)["u_right"] is None and SC.pack(s)["kps"] is None and SC.pack(s)["depth"] is None
    elif name == "nleft_zero":
        assert len(s["kfs"][1]["eyes"][0]["kps"]) == 0 and w[1]["n_new"] >= 2
    assert_equals_walk(host_run(host, s), s, what=name)


@pytest.mark.parametrize("two_eyes", [False, True])
def test_counts_are_clamped_and_an_empty_list_writes_nothing(host, two_eyes):
    import copy
    s = scene(two_eyes, 1)
    L = (2 if two_eyes else 1) * s["cap"]
    empty = copy.deepcopy(s); empty["pairs"] = [[], [], [], []]; empty["kinds"] = [[], [], [], []]
    o = host_run(host, empty)
    assert (o["n_new"] == 0).all() and (o["exit"] == POISON_EXIT).all()
    assert_equals_walk(o, empty, what="empty")
    for given in (L + 40, 2 ** 31 - 1):                                                          # past the capacity: all L entries, the poison pairs are bad indices
        full = copy.deepcopy(s)
        for p in range(4):
            pad = L - len(full["pairs"][p])
            full["pairs"][p] = list(full["pairs"][p]) + [(SC.POISON_PAIR, SC.POISON_PAIR)] * pad; full["kinds"][p] = list(full["kinds"][p]) + ["bad"] * pad
        o = host_run(host, full, SC.pack(s, n_matches=given))
        assert_equals_walk(o, full, what="n_matches %d" % given)
        assert (o["exit"][1, len(s["pairs"][1]):] == NW.BAD_INDEX).all()
    o = host_run(host, empty, SC.pack(s, n_matches=-3))                                          # negative: clamped to zero
    assert_equals_walk(o, empty, what="negative")


def test_zero_dist(host):
    s = SC.zero_dist_scene()
    assert walk(s)[0]["exit"] == [NW.ZERO_DIST] and walk(s)[0]["stereo"] == 1
    assert (s["kfs"][0]["pose"] != s["kfs"][1]["pose"]).any() and s["kfs"][1]["depth"][0] > 0
    assert_equals_walk(host_run(host, s), s, what="zero_dist")


# ---- (c) ----
def test_stereo_parallax_else_if_and_unproject_stereo_reads_the_raw_keypoints(host):
    import copy
    s = scene(False, 1)
    w = walk(s)[2]
    both = s["kinds"][2].index("st_both")
    i1, i2 = s["pairs"][2][both]
    assert s["kfs"][0]["u_right"][i1] >= 0 and s["kfs"][2]["u_right"][i2] >= 0 and w["exit"][both] == NW.STEREO_1
    # with both stereo only cosParallaxStereo1 is replaced: the point is keyframe 1's UnprojectStereo, bit for bit what it is with a monocular kp2 ...
    t = copy.deepcopy(s); t["kfs"][2]["u_right"][i2] = -1.0
    assert same_floats(SC.walk(t)[2]["x3d"][both], w["x3d"][both])
    # ... and not keyframe 2's
    t = copy.deepcopy(s); t["kfs"][0]["u_right"][i1] = -1.0
    w2 = SC.walk(t)[2]
    assert w2["exit"][both] == NW.STEREO_2 and not same_floats(w2["x3d"][both], w["x3d"][both])
    # UnprojectStereo reads mvKeys (the scene shifts them against mvKeysUn): with the shift taken out the stereo points move, the others stay
    t = copy.deepcopy(s)
    for kf in t["kfs"]:
        kf["kps"] = kf["kps_un"].copy()
    w3 = SC.walk(t)[2]
    for k, e in enumerate(w["exit"]):
        assert (e in (NW.STEREO_1, NW.STEREO_2)) == (not same_floats(w3["x3d"][k], w["x3d"][k])), k
    assert_equals_walk(host_run(host, t), t, w=SC.walk(t), what="raw = undistorted")
    # the stereo cosine is binary32 throughout, the host libm's
    m = NW.Binary32()
    for depth in (2.5, 0.01, -1.0, 0.0, 1e-30, 40.0):
        assert same_floats(np.array([host.nmp_stereo_cos(0.1, depth)], f32), np.array([m.stereo_cos(0.1, depth)], f32)), depth


def test_marks_are_only_ever_set(host):
    s = scene(True, 2)
    d = SC.pack(s)
    o = outputs(d)
    o["mark1"][:] = 0xF0; o["mark2"][:] = 0x02                                                    # other bits and other entries stay
    stats = np.zeros(2, np.int32)
    host.nmp_host(1, d["P"], 0, 0, 0, 1, ptr(d["pairs"]), ptr(d["n_matches"]), ptr(d["poses"]), ptr(np.ascontiguousarray(s["tlr"], f32)), ptr(cams16(s)),
                  ptr(d["kps_un"]), None, None, None, ptr(d["n_out"]), d["cap"], ptr(SC.TAB["scale"]), ptr(SC.TAB["sigma2"]), 8, float(SC.TAB["ratio_factor"]),
                  s["mb"], s["mbf"], 1, s["th_far"], ptr(o["exit"]), ptr(o["x3d"]), ptr(o["n_new"]), ptr(o["mark1"]), ptr(o["mark2"]), ptr(stats))
    w = walk(s)
    assert np.array_equal(o["mark1"], 0xF0 | expected_marks(s, w, s["cap"], "mark1")) and np.array_equal(o["mark2"], 0x02 | expected_marks(s, w, s["cap"], "mark2"))
    # several matches share a keypoint of keyframe 1 in the pair against itself
    assert len(w[0]["mark1"] | w[0]["mark2"]) < 2 * w[0]["n_new"] or w[0]["n_new"] == 0


# ---- (d) ----
@pytest.mark.parametrize("two_eyes", [False, True])
@pytest.mark.parametrize("seed", SC.MARGIN_SEEDS)
def test_float64_statement_agrees_with_margin(two_eyes, seed):
    s = scene(two_eyes, seed)
    margins = []
    w64 = SC.walk(s, NW.Float64(), margins=margins)
    tested, worst, worst_ratio = 0, 0.0, 0.0
    for p, (a, b) in enumerate(zip(walk(s), w64)):
        for k, (e, e64, kind) in enumerate(zip(a["exit"], b["exit"], s["kinds"][p])):
            if kind in SC.NO_MARGIN_KINDS:
                continue
            assert e == e64 and SC.margin_ok(margins[p][k]), (seed, p, k, kind, NW.EXIT_NAMES[e], NW.EXIT_NAMES[e64], margins[p][k])
            tested += 1
            if e > NW.STEREO_2:
                continue
            x32, x64 = a["x3d"][k].astype(np.float64), b["x3d"][k]
            dist = float(np.linalg.norm(x64))                                                    # keyframe 1 is at the origin
            bound = triangulation_bound(s, p, k, RAY_ERROR[two_eyes]) / dist if e == NW.TRIANGULATED else 4 * 2.0 ** -24
            gap = float(np.linalg.norm(x32 - x64)) / dist
            worst, worst_ratio = max(worst, gap), max(worst_ratio, gap / bound)
            assert gap <= bound, (seed, p, k, kind, gap, bound)
    print("%s seed %d: %d matches, worst relative gap of x3d %.3g, %.2f of its bound" % ("two eyes" if two_eyes else "one camera", seed, tested, worst, worst_ratio))
    assert tested >= (18 if two_eyes else 25)      # every crafted match but the kinds of NO_MARGIN_KINDS


# ---- (e) ----
@pytest.mark.parametrize("negative", [0, 1])
def test_cosine_on_every_float_between_pi_and_two_pi(host, negative):
    tested = C.c_long(0)
    bad = host.nmp_check_cos(negative, C.byref(tested))
    assert tested.value == 0x800001
    settle(bad, "kb8SinCos's cosine on every float of %s" % ("[-2 pi, -pi]" if negative else "[pi, 2 pi]"))


def test_stereo_cosine_against_libm(host):
    settle(host.nmp_check_stereo_cos(2_000_000, 3), "cos(2 * atan2f(mb / 2, depth)) on 2 * 10^6 pairs")


def test_the_scenes_tables_are_the_handles():
    t = X.compute_tables(1000, 1.2, 8)
    assert SC.TAB["sigma2"].tobytes() == t["level_sigma2"].tobytes() and SC.TAB["scale"].tobytes() == t["scale_factors"].tobytes()
    assert SC.TAB["ratio_factor"] == f32(1.5) * f32(1.2)


def test_host_program_runs_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "prog")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DNEW_MAP_POINTS_HOST_MAIN", *HOST_FLAGS,
                           os.path.join(ROOT, "tests", "cpp", "new_map_points_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and "runtime error" not in out.stdout and "AddressSanitizer" not in out.stdout, out.stdout[-3000:]
    assert "every access inside its arrays" in out.stdout


def test_the_entries_are_declared_exported_mirrored_and_tabled():
    names = ("orbx_create_new_map_points_device", "orbx_create_new_map_points_two_eyes_device", "orbx_debug_new_map_points_enable",
             "orbx_debug_new_map_points_stats")
    L = X.load_library()
    for n in names:
        assert n in X.header_symbols() and hasattr(L, n), n
    for n in ("create_new_map_points_device", "create_new_map_points_two_eyes_device", "new_map_points_count", "new_map_points_stats"):
        assert hasattr(X.ORBextractor, n), n
    for n, count in (("orbx_create_new_map_points_device", 26), ("orbx_create_new_map_points_two_eyes_device", 23)):      # a NULL handle
        fn = getattr(L, n)
        assert len(fn.argtypes) == count and fn(*[None if t is C.c_void_p else 1 for t in fn.argtypes]) == -2, n
    text = open(os.path.join(ROOT, "include", "orbx.h")).read()
    enum = re.search(r"enum orbx_new_point_exit \{(.*?)\};", text, flags=re.S).group(1)
    assert [(n.lower(), int(v)) for n, v in re.findall(r"ORBX_NEW_POINT_(\w+) = (\d+)", enum)] == list(zip(NW.EXIT_NAMES, range(14)))
    table = json.load(open(os.path.join(ROOT, "extractorb_amd", "csrc", "kernel_table.json")))
    for k in ("k_new_map_points<0>", "k_new_map_points<1>", "k_new_map_points_init"):
        assert table[k]["scratch_bytes"] == 0 and table[k]["sgpr_spill"] == 0 and table[k]["vgpr_spill"] == 0 and table[k]["flat"] == 0, k
