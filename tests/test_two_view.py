"""TwoViewReconstruction::Reconstruct without a GPU: extractorb_amd/csrc/k_two_view.hpp - the statement of k_two_view.hip - compiled for the
host (tests/cpp/two_view_host_check.cpp: the three kernels' bodies with a wave of one lane) against the sequential walk
(tests/two_view_walk.py) on the scenes of tests/two_view_scenes.py, byte for byte: result rows, p3d, flags and pruned matches.
  (a) every scene of two_view_scenes.CASES; a histogram over orbx_two_view_status (what is not reached: docs/history/r23_two_view.md);
  (b) the semantics the header lists, one by one: a tie goes to the lower iteration, vP3D is set with the flag 0 at cosParallax >= 0.99998,
      prune leaves a rejected pair untouched, N < 8 and a bad index write zeros and read nothing else, the set construction against a direct
      transcription of the swap-remove loop at N = 8 (every set a permutation) and at large N;
  (c) the pieces: nullVector9 and svd3 against numpy, acosf against the host libm on every float of [0.9, 1], a stride over [-1, 1] and the
      values outside the domain;
  (d) the float64 kind of the walk on MARGIN_SEEDS: every decision quantity clear of its threshold, the same model, winning iteration, status
      and triangulated set, R21, t21 and the accepted points within a bound derived by perturbing the float64 statement;
  (e) the stand-alone sanitizer program; the header's declarations against the Python argtypes."""
import collections
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import extractorb_amd as X
import two_view_scenes as SC
import two_view_walk as TW
from test_kb8_math import HOST_FLAGS, ROOT

f32 = np.float32
VP = C.c_void_p
SRC = os.path.join(ROOT, "tests", "cpp", "two_view_host_check.cpp")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("tvhost")), "libtwo_view_host.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", *HOST_FLAGS, SRC, "-o", so])
    L = C.CDLL(so)
    L.tv_host.argtypes = [C.c_int] * 5 + [VP, VP, C.c_int, VP, VP, VP, C.c_float, C.c_int, C.c_float, C.c_int, C.c_float, VP, C.c_int, VP, VP, VP]
    L.tv_host.restype = None
    L.tv_check_acos.restype = C.c_long
    L.tv_check_point.argtypes = [VP, VP, VP, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, VP, VP]
    L.tv_check_point.restype = None
    L.tv_rank_hit.argtypes = [VP, VP, C.c_int, C.c_float, C.c_int]
    L.tv_decide.argtypes = [C.c_int, VP, VP, C.c_int, C.c_float, C.c_int, VP]
    L.tv_check_acos.argtypes = [C.c_int, C.POINTER(C.c_long)]
    return L


def ptr(a):
    return a.ctypes.data_as(VP)


def run_host(L, s):
    o = SC.poisoned_outputs(s)
    cam = np.array(s["cam"], f32)
    L.tv_host(s["pairs"], s["frames1"][0], s["frames1"][1], s["frames2"][0], s["frames2"][1], ptr(s["kps"]), ptr(s["n_out"]), s["cap"],
              ptr(o["matches"]), ptr(o["n_matches"]), ptr(cam), s["sigma"], s["iterations"], s["min_parallax"], s["min_triangulated"],
              s["rh_threshold"], ptr(s["rand"]), s["prune"], ptr(o["result"]), ptr(o["p3d"]), ptr(o["tri"]))
    return o


def test_the_result_row_is_the_headers(host):
    assert host.tv_result_bytes() == SC.RESULT_DTYPE.itemsize == X.TWO_VIEW_RESULT_DTYPE.itemsize
    assert SC.RESULT_DTYPE == X.TWO_VIEW_RESULT_DTYPE
    header = open(os.path.join(ROOT, "include", "orbx.h")).read()
    names = re.findall(r"ORBX_TWO_VIEW_(\w+) = (\d+)", header)
    assert [n for n, _ in names] == list(TW.STATUS) == list(X.TWO_VIEW_STATUS) and [int(v) for _, v in names] == list(range(len(TW.STATUS)))


@pytest.mark.parametrize("name", list(SC.CASES))
def test_the_header_equals_the_walk_byte_for_byte(host, name):
    s = SC.case(name)
    _, want = SC.case_expected(name)
    got = run_host(host, s)
    assert SC.differences(got, want) == [], [(TW.STATUS[a], TW.STATUS[b]) for a, b in zip(got["result"]["status"], want["result"]["status"])]


def test_the_scenes_reach_the_statuses():
    """every status but the four docs/history/r23_two_view.md explains, and the scenes built for one end on it"""
    hist = collections.Counter()
    for name in SC.CASES:
        for w in SC.case_expected(name)[0]:
            hist[TW.STATUS[w["status"]]] += 1
    print(dict(hist))
    status = lambda name, p=0: TW.STATUS[SC.case_expected(name)[0][p]["status"]]
    assert status("n7_too_few") == "TOO_FEW_MATCHES"
    assert status("general_n96_it200") == "ACCEPTED_F" and status("plane_n96") == "ACCEPTED_H"
    assert status("zero_translation") == "H_AMBIGUOUS"       # 0.3 px noise separates the singular values: three motions with 85 good points each
    assert status("h_degenerate_exact_rotation") == "H_DEGENERATE" and status("f_low_parallax") == "F_LOW_PARALLAX"
    assert status("h_low_parallax") == "H_LOW_PARALLAX"
    assert status("plane_n48_few_points") == "H_FEW_POINTS" and status("small_baseline_ambiguous") == "F_AMBIGUOUS"
    for need in ("ACCEPTED_H", "ACCEPTED_F", "TOO_FEW_MATCHES", "F_FEW_POINTS", "H_AMBIGUOUS"):
        assert hist[need], (need, dict(hist))


def test_a_bad_index_writes_zeros_and_decides_before_the_count(host):
    s = dict(SC.case("n7_too_few"))
    s["matches"] = s["matches"].copy()
    i = int(np.nonzero(s["matches"][0] >= 0)[0][0])
    s["matches"][0, i] = int(s["n_out"][1])                  # == n of frame 2: one past its last keypoint
    got = run_host(host, s)
    assert SC.differences(got, SC.expected(s)) == []
    r = got["result"][0]
    n1 = int(s["n_out"][0])
    assert TW.STATUS[r["status"]] == "BAD_INDEX" and r["n_matches"] == 7
    assert not got["p3d"][0, :n1].any() and not got["tri"][0, :n1].any() and np.array_equal(got["matches"], s["matches"])


def test_a_tie_goes_to_the_lower_iteration(host):
    s = dict(SC.case("plane_n96"))
    s["rand"] = s["rand"].copy()
    s["rand"][0, :] = s["rand"][0, 5]                        # every iteration draws the same set: every score ties
    got = run_host(host, s)
    assert SC.differences(got, SC.expected(s)) == []
    r = got["result"][0]
    assert r["SH"] > 0 and r["SF"] > 0 and r["best_it_h"] == 0 and r["best_it_f"] == 0


def test_nan_keypoints_end_as_zero_scores(host):
    """one matched keypoint of frame 1 is NaN: every hypothesis of both models sums a NaN term, no score is above 0"""
    s = dict(SC.case("plane_n96"))
    s["kps"] = s["kps"].copy()
    i = int(np.nonzero(s["matches"][0] >= 0)[0][3])
    s["kps"]["x"][0, i] = np.nan
    got, want = run_host(host, s), SC.expected(s)
    assert SC.differences(got, want) == []
    r = got["result"][0]
    assert TW.STATUS[r["status"]] == "ZERO_SCORES" and r["SH"] == 0 and r["SF"] == 0 and r["best_it_h"] == -1 and r["best_it_f"] == -1
    assert not got["tri"][0, :120].any() and np.array_equal(got["matches"], s["matches"])


def test_no_f_score_above_zero_takes_h(host):
    """SF == 0 with SH > 0: RH is 1, H is taken whatever the threshold below 1, and the decision meets no F winner (best_it_f = -1, F21
    zeros).  The F scores are zeroed between the hypotheses and the decision, in the host build and in the walk alike."""
    for name in ("plane_n96", "general_n96_it200"):
        s = dict(SC.case(name), rh_threshold=0.999)
        host.tv_set_zero_f(1)
        try:
            got = run_host(host, s)
        finally:
            host.tv_set_zero_f(0)
        want = SC.expected(s, SC.walk(s, zero_f=True))
        assert SC.differences(got, want) == []
        r = got["result"][0]
        assert r["model"] == 0 and r["RH"] == 1.0 and r["SF"] == 0 and r["SH"] > 0 and r["best_it_f"] == -1 and not r["F21"].any()
        assert r["n_inliers"] > 0 and r["H21"].any()


def check_point(host, R, t, u1, v1, u2, v2):
    out, cos = np.zeros(5, f32), np.zeros(1, f32)
    R, t, cam = np.ascontiguousarray(R, f32), np.ascontiguousarray(t, f32), np.array(SC.CAM, f32)
    host.tv_check_point(ptr(R), ptr(t), ptr(cam), 1.0, u1, v1, u2, v2, ptr(out), ptr(cos))
    return bool(out[0]), bool(out[1]), out[2:], cos[0]


def test_a_non_finite_triangulation_is_not_counted(host):
    """:844-848.  On a NaN point every later test of CheckRT is false (no `continue` is taken): only the isfinite test keeps it out."""
    K32 = TW.Binary32()
    c, s = np.cos(0.05), np.sin(0.05)
    R, t = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], f32), np.array([-0.99, 0.08, 0.16], f32)
    Km = np.array([[SC.CAM[0], 0, SC.CAM[2]], [0, SC.CAM[1], SC.CAM[3]], [0, 0, 1]], f32)
    X = np.array([0.5, -0.3, 9.0])
    a = SC._project(X[None])[0]
    b = SC._project((R.astype(np.float64) @ X + t)[None])[0]
    for u1, v1, u2, v2, counted in ((a[0], a[1], b[0], b[1], True), (np.nan, a[1], b[0], b[1], False), (a[0], a[1], b[0], np.inf, False),
                                    (np.inf, np.inf, np.inf, np.inf, False)):
        got = check_point(host, R, t, u1, v1, u2, v2)
        _, _, per = TW.check_rt(K32, R, t, Km, np.array([[u1, v1]], f32), np.array([[u2, v2]], f32), [True], 1.0, K32.null_vector)
        assert got[0] == per[0][0] == counted and got[1] == per[0][1], (u1, v1, u2, v2, got, per)
        if counted:
            assert got[2].tobytes() == np.asarray(per[0][3], f32).tobytes() and np.allclose(got[2], X * (np.linalg.norm(got[2]) / np.linalg.norm(X)), rtol=1e-3)
        else:
            assert not got[2].any()


def test_a_nan_cosine_sorts_last_and_a_nan_parallax_accepts_nothing(host):
    """the k-th smallest by rank counting against sorted() with the NaNs behind everything; :528's > and :724's >= are false on a NaN"""
    rng = np.random.default_rng(3)
    for trial in range(40):
        N = int(rng.integers(1, 70))
        cosv = rng.uniform(0.99, 1.00001, N).astype(f32)
        cosv[rng.random(N) < 0.2] = np.nan
        if trial % 4 == 0:
            cosv[:] = cosv[0]                                # all ties (or all NaN)
        counted = (rng.random(N) < 0.7).astype(np.uint8)
        vals = [v for v, c in zip(cosv, counted) if c]
        if not vals:
            continue
        order = sorted(v for v in vals if v == v) + [v for v in vals if v != v]
        for idx in {0, len(vals) - 1, min(50, len(vals) - 1), len(vals) // 2}:
            hits = [v for v, c in zip(cosv, counted) if c and host.tv_rank_hit(ptr(cosv), ptr(counted), N, float(v), idx)]
            want = order[idx]
            assert (hits == [] and want != want) or (hits and all(h == want for h in hits)), (trial, idx, hits, want)
    # the scene whose every point is far: cosines at 1 +- an ulp, the largest above 1, its acosf a NaN
    w, want = SC.case_expected("nan_parallax_all_far")
    assert np.isnan(np.asarray(w[0]["parallax"], f32)).any() and SC.differences(run_host(host, SC.case("nan_parallax_all_far")), want) == []
    nan = float("nan")
    for model, n_good, par, N, want_status in ((1, [60, 0, 0, 0], [nan, 0, 0, 0], 60, "F_LOW_PARALLAX"), (0, [60, 0, 0, 0, 0, 0, 0, 0], [nan] + [0] * 7, 60, "H_LOW_PARALLAX")):
        g, pp, ch = np.array(n_good + [0] * (8 - len(n_good)), np.int32), np.array(par + [0] * (8 - len(par)), f32), np.zeros(1, np.int32)
        assert TW.STATUS[host.tv_decide(model, ptr(g), ptr(pp), N, 1.0, 50, ptr(ch))] == want_status == TW.STATUS[TW.decide(model, list(g), list(pp), N, f32(1.0), 50)[0]]
        assert ch[0] == -1


def test_the_conjuncts_of_the_h_decision_are_named_in_source_order(host):
    """:724 on crafted counts: each row fails the named conjunct and every LATER one too, so the name shows the order"""
    rows = ((([60, 50, 0, 0, 0, 0, 0, 0], 0.5, 100), "H_AMBIGUOUS"),            # 50 >= 0.75 * 60; parallax, count and share fail as well
            (([60, 10, 0, 0, 0, 0, 0, 0], 0.5, 100), "H_LOW_PARALLAX"),         # 60 <= 0.9 * 100 and 60 <= 70 fail as well
            (([60, 10, 0, 0, 0, 0, 0, 0], 2.0, 100), "H_FEW_POINTS"),           # min_triangulated 70; 60 <= 0.9 * 100 fails as well
            (([80, 10, 0, 0, 0, 0, 0, 0], 2.0, 100), "H_BELOW_INLIER_SHARE"),   # 80 > 70 but 80 <= 90
            (([95, 10, 0, 0, 0, 0, 0, 0], 2.0, 100), "ACCEPTED_H"))
    for (n_good, par, N), want in rows:
        g, pp, ch = np.array(n_good, np.int32), np.full(8, par, f32), np.zeros(1, np.int32)
        got = TW.STATUS[host.tv_decide(0, ptr(g), ptr(pp), N, 1.0, 70, ptr(ch))]
        assert got == want == TW.STATUS[TW.decide(0, n_good, list(pp), N, f32(1.0), 70)[0]], (n_good, got, want)
    for n_good, par, want in (([40, 0, 0, 0], 5.0, "F_FEW_POINTS"), ([95, 70, 0, 0], 5.0, "F_AMBIGUOUS"), ([40, 30, 0, 0], 5.0, "F_FEW_POINTS"),
                              ([0, 95, 0, 0], 0.5, "F_LOW_PARALLAX"), ([0, 0, 0, 95], 5.0, "ACCEPTED_F")):
        g, pp, ch = np.array(n_good + [0] * 4, np.int32), np.full(8, par, f32), np.zeros(1, np.int32)
        got = TW.STATUS[host.tv_decide(1, ptr(g), ptr(pp), 100, 1.0, 70, ptr(ch))]
        assert got == want == TW.STATUS[TW.decide(1, n_good + [0] * 4, list(pp), 100, f32(1.0), 70)[0]], (n_good, got, want)


def test_a_counted_point_at_low_parallax_has_its_point_and_no_flag():
    s = SC.case("far_points")
    w, want = SC.case_expected("far_points")
    assert w[0]["status"] <= TW.ACCEPTED_F
    p3d, tri = want["p3d"][0], want["tri"][0]
    unflagged = [i for i in range(int(s["n_out"][0])) if p3d[i].any() and not tri[i]]
    assert len(unflagged) == 3 and all(abs(p3d[i][2]) > 100 for i in unflagged), unflagged      # the far points: vP3D written, vbTriangulated false
    assert all(want["matches"][0, i] == -1 for i in unflagged)                    # and pruned by the tracker's next statement
    assert want["n_matches"][0] == (want["matches"][0] >= 0).sum() == tri[:int(s["n_out"][0])].sum()


def test_prune_leaves_a_rejected_pair_untouched_and_zero_writes_nothing(host):
    for name in ("zero_translation", "n7_too_few", "plane_n48_few_points"):
        s = SC.case(name)
        got = run_host(host, s)
        assert got["result"]["status"][0] > TW.ACCEPTED_F and s["prune"] == 1
        assert np.array_equal(got["matches"], s["matches"]) and np.array_equal(got["n_matches"], s["n_matches"])
    s = dict(SC.case("general_n96_it200"), prune=0)
    got = run_host(host, s)
    assert SC.differences(got, SC.expected(s, SC.case_expected("general_n96_it200")[0])) == []
    assert got["result"]["status"][0] == TW.ACCEPTED_F and np.array_equal(got["matches"], s["matches"]) and np.array_equal(got["n_matches"], s["n_matches"])
    assert got["tri"][0, :120].sum() > 50
    pruned = run_host(host, SC.case("general_n96_it200"))
    assert pruned["n_matches"][0] == pruned["tri"][0, :120].sum() < s["n_matches"][0] and pruned["tri"].tobytes() == got["tri"].tobytes()


def test_the_sets_are_the_swap_remove_loops(host):
    rng = np.random.default_rng(5)
    for N in (8, 9, 17, 96, 10000):
        for trial in range(200):
            r8 = rng.integers(0, 2 ** 31, 8).astype(np.int32)
            if trial % 10 == 0:
                r8[rng.integers(0, 8)] = 2 ** 31 - 1
            if trial % 10 == 1:
                r8[:] = 0
            if trial % 10 == 2:
                r8[:] = 2 ** 31 - 1
            got = np.zeros(8, np.int32)
            host.tv_draw_set(ptr(r8), N, ptr(got))
            want = TW.draw_set(r8, N)
            assert list(got) == want and len(set(want)) == 8 and (N > 8 or sorted(want) == list(range(8)))


def test_the_null_vector_and_the_svd_against_numpy(host):
    rng = np.random.default_rng(7)
    for rows in (16, 8):
        for _ in range(20):
            A = rng.normal(size=(rows, 9)).astype(f32)
            if rows == 16:                                   # a 16x9 system of a noisy minimal set: a small last singular value
                u, sv, vt = np.linalg.svd(A.astype(np.float64), full_matrices=False)
                sv[8] = 1e-3 * sv[7]
                A = ((u * sv) @ vt).astype(f32)
            out = np.zeros(9, f32)
            host.tv_null9(ptr(A), rows, ptr(out))
            assert out.tobytes() == TW.jacobi_null_vector(f32, A).tobytes()
            sigma = np.linalg.svd(A.astype(np.float64))[1]
            smallest = sigma[8] if rows == 16 else 0.0
            assert abs(np.linalg.norm(out) - 1) < 1e-5 and np.linalg.norm(A.astype(np.float64) @ out) < smallest + 4e-6 * sigma[0]
    for k in range(30):
        A = rng.normal(size=(3, 3)).astype(f32)
        if k % 3 == 0:                                       # an essential matrix: two equal singular values and a zero
            u, _, vt = np.linalg.svd(A.astype(np.float64))
            A = (u @ np.diag([1.0, 1.0, 0.0]) @ vt).astype(f32)
        U, w, Vt = np.zeros((3, 3), f32), np.zeros(3, f32), np.zeros((3, 3), f32)
        host.tv_svd3(ptr(A), ptr(U), ptr(w), ptr(Vt))
        Uw, ww, Vtw = TW.jacobi_svd3(f32, A)
        assert U.tobytes() == np.ascontiguousarray(Uw).tobytes() and w.tobytes() == ww.tobytes() and Vt.tobytes() == np.ascontiguousarray(Vtw).tobytes()
        assert w[0] >= w[1] >= w[2] >= 0 and np.allclose(w, np.linalg.svd(A.astype(np.float64))[1], atol=4e-7 * w[0])
        assert np.abs(U.astype(np.float64) @ np.diag(w.astype(np.float64)) @ Vt - A).max() < 1e-6 * w[0]
        assert np.abs(U.T @ U - np.eye(3)).max() < 1e-6 and np.abs(Vt @ Vt.T - np.eye(3)).max() < 1e-6


def test_acosf_is_the_host_libms(host):
    n = C.c_long()
    assert host.tv_check_acos(97, C.byref(n)) == 0
    assert n.value > 1677721 + 2 * (0x3f800000 // 97)         # every float of [0.9, 1] and the stride over [-1, 1]


MARGIN_SEEDS = ("general_n96_it200", "plane_n96", "far_points")      # cases of two_view_scenes.CASES (their seeds), pair 0 of each
U = 2.0 ** -24                                           # the unit roundoff of binary32
# What binary32 costs R21, t21 and an accepted point against float64; both kinds read the same binary32 pixels.
#  * the fit: a normalised sample coordinate carries 2 roundings, its entry of A one more, and nullVector9 leaves the null vector within
#    4e-6 sigma_1 (67 u) of the exact one (test_the_null_vector_and_the_svd_against_numpy): taken together as SAMPLE_UNITS = 64 u of each of
#    the 32 pixel coordinates of the eight sample matches, relative to the coordinate.  perturbation_bound() moves each by that much in the
#    FLOAT64 statement, refits, decomposes, takes the motion nearest the chosen one and adds up the moves of R21, t21 and of every point
#    (first order, every error at its worst sign);
#  * the decomposition: three gemm3 and an svd3 on unit-scale 3x3 matrices, DECOMPOSE_UNITS = 16 u on every element of R21 and t21;
#  * a point's own rays: 4 roundings per row of A (RAY_UNITS = 4 u of each of its four pixel coordinates) and nullVector4's residual excess
#    3.44e-8 / sigma_3 * (1 + |x|^2) (tests/test_new_map_points.py: triangulation_bound).
SAMPLE_UNITS, DECOMPOSE_UNITS, RAY_UNITS = 64, 16, 4


def _triangulate64(Km, R, t, a, b):
    P1 = np.hstack([Km, np.zeros((3, 1))])
    P2 = Km @ np.hstack([R, t.reshape(3, 1)])
    A = np.array([a[0] * P1[2] - P1[0], a[1] * P1[2] - P1[1], b[0] * P2[2] - P2[0], b[1] * P2[2] - P2[1]])
    sv, vt = np.linalg.svd(A)[1:]
    return vt[3, :3] / vt[3, 3], sv[2]


def perturbation_bound(s, w64, tr):
    """(bound on |dR21|, |dt21| elementwise, bound on |dx| per keypoint index of frame 1) from the float64 statement"""
    K64 = TW.Float64()
    k1, k2, _ = SC.pair_inputs(s, 0)
    norm1, T1 = TW.normalize(np.float64, np.asarray(k1, np.float64))
    norm2, T2 = TW.normalize(np.float64, np.asarray(k2, np.float64))
    model, Km = w64["model"], np.asarray(tr["Km"], np.float64)
    idx8 = tr["sets"][w64["best_it_h"] if model == 0 else w64["best_it_f"]]
    R0, t0 = np.asarray(w64["R21"], np.float64).reshape(3, 3), np.asarray(w64["t21"], np.float64)
    good = [k for k in range(len(tr["first"])) if w64["triangulated"][tr["first"][k]]]
    x0 = dict((k, _triangulate64(Km, R0, t0, tr["p1"][k], tr["p2"][k])) for k in good)
    move_rt, move_x = 0.0, dict((k, 0.0) for k in good)
    for i in idx8:
        for which in (0, 1):
            for c in (0, 1):
                p = [np.array(tr["p1"], np.float64), np.array(tr["p2"], np.float64)]
                p[which][i, c] += SAMPLE_UNITS * U * abs(p[which][i, c])
                M21, _ = TW.hypothesis(K64, model, idx8, p[0], p[1], norm1, norm2, T1, T2)
                mots = TW.motions_h(K64, M21, Km) if model == 0 else TW.motions_f(K64, M21, Km)
                R, t = min(mots, key=lambda m: np.abs(m[0] - R0).max() + np.abs(m[1] - t0).max())
                move_rt += max(np.abs(R - R0).max(), np.abs(t - t0).max())
                for k in good:
                    move_x[k] += float(np.linalg.norm(_triangulate64(Km, R, t, tr["p1"][k], tr["p2"][k])[0] - x0[k][0]))
    bound_x = {}
    for k in good:
        x, sigma3 = x0[k]
        own = 0.0
        for which in (0, 1):
            for c in (0, 1):
                q = [np.array(tr["p1"][k], np.float64), np.array(tr["p2"][k], np.float64)]
                q[which][c] += RAY_UNITS * U * abs(q[which][c])
                own += float(np.linalg.norm(_triangulate64(Km, R0, t0, q[0], q[1])[0] - x))
        bound_x[int(tr["first"][k])] = move_x[k] + own + 3.44e-8 / sigma3 * (1.0 + float(x @ x))
    return move_rt + DECOMPOSE_UNITS * U, bound_x


def clear_of(value, threshold, rel=1e-4):
    return abs(float(value) - float(threshold)) > rel * max(1.0, abs(float(threshold)))


@pytest.mark.parametrize("name", MARGIN_SEEDS)
def test_the_float64_kind_takes_the_same_decisions(name):
    """On MARGIN_SEEDS both kinds take the same model, the same winning iterations, the same status, the same motion (np.linalg.svd may
    number the motions differently: the motion is compared, not its index) and the same triangulated set, and R21, t21 and the accepted
    points agree within perturbation_bound().  The condition on the inputs, asserted in the float64 statement: the winner leads the
    runner-up of another set by more than LEAD times the chain's accumulated rounding 2N u S (2N adds, each off by at most u times a partial
    sum below S; LEAD = 64 stands for the terms' own roundings, some thirty binary32 operations per term); RH is 0.02 clear of the
    threshold; every chi-square of the winner, every depth, reprojection error and cosine of the chosen motion's CheckRT, d1/d2 and d2/d3,
    the counts against 0.7 maxGood, 0.75 bestGood, 0.9 N and the minimum, and the parallax are clear of their thresholds (clear_of)."""
    LEAD = 64
    s = SC.case(name)
    tr64 = []
    w64, w32 = SC.walk(s, TW.Float64(), tr64)[0], SC.case_expected(name)[0][0]
    tr = tr64[0]
    model = w64["model"]
    scores = tr["scores"][model]
    best = int(np.argmax(scores))
    rivals = [sc for it, sc in enumerate(scores) if sorted(tr["sets"][it]) != sorted(tr["sets"][best])]
    assert scores[best] - max(rivals) > LEAD * 2 * w64["n_matches"] * U * scores[best], (scores[best], max(rivals))
    assert abs(float(w64["RH"]) - s["rh_threshold"]) > 0.02
    # the winner's inlier tests
    M = np.asarray(w64["H21"] if model == 0 else w64["F21"], np.float64).reshape(3, 3)
    terms = TW.score(np.float64, model, M, TW.inv3(np.float64, M) if model == 0 else None, s["sigma"], tr["p1"], tr["p2"])[2]
    th = 5.991 if model == 0 else 3.841
    assert all(clear_of(5.991 - term, th) for term in terms if term != 0), "a chi-square at its threshold"
    # the decomposition and the chosen motion's CheckRT
    if model == 0:
        assert clear_of(tr["d12"], 1.00001) and clear_of(tr["d23"], 1.00001)
    R0, t0 = np.asarray(w64["R21"]).reshape(3, 3), np.asarray(w64["t21"])
    margins = []
    TW.check_rt(TW.Float64(), R0, t0, tr["Km"], tr["p1"], tr["p2"], tr["inliers"], s["sigma"], TW.Float64().null_vector, margins)
    assert margins and all(clear_of(v, t, 2.4e-7 if what == "cos" else 1e-4) for what, v, t in margins), [m for m in margins if not clear_of(m[1], m[2])]
    g, n_inl = sorted(w64["n_good"], reverse=True), w64["n_inliers"]
    if model == 0:
        assert clear_of(g[1], 0.75 * g[0]) and clear_of(g[0], 0.9 * n_inl) and g[0] != s["min_triangulated"]
    else:
        assert all(clear_of(v, 0.7 * g[0]) for v in g[:4]) and g[0] != max(int(0.9 * n_inl), s["min_triangulated"]) and clear_of(0.9 * n_inl, round(0.9 * n_inl))
    assert clear_of(max(w64["parallax"]), s["min_parallax"])
    # the same decisions
    for f in ("status", "model", "best_it_h" if model == 0 else "best_it_f", "n_inliers"):
        assert w64[f] == w32[f], (f, w64[f], w32[f])
    assert w64["status"] <= TW.ACCEPTED_F and np.array_equal(w64["triangulated"], w32["triangulated"])
    assert sorted(w64["n_good"]) == sorted(w32["n_good"])
    # R21, t21 and the points within the derived bound
    bound_rt, bound_x = perturbation_bound(s, w64, tr)
    worst = max(np.abs(np.asarray(w64["R21"]) - w32["R21"]).max(), np.abs(np.asarray(w64["t21"]) - w32["t21"]).max())
    used = [float(np.linalg.norm(np.asarray(w64["p3d"][i], np.float64) - w32["p3d"][i])) / b for i, b in bound_x.items()]
    print(name, "|dR|, |dt|: %.3g of %.3g (%.1f %%); points: worst %.1f %% of its bound, %d points" % (worst, bound_rt, 100 * worst / bound_rt, 100 * max(used), len(used)))
    assert worst <= bound_rt
    assert len(used) > 50 and max(used) <= 1.0


def test_the_sanitizer_program(tmp_path):
    exe = os.path.join(str(tmp_path), "two_view_host_check")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DTWO_VIEW_HOST_MAIN", *HOST_FLAGS, SRC,
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "every access inside its arrays" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]
