"""Sim3Solver without a GPU: extractorb_amd/csrc/k_sim3_solver.hpp - the statement of k_sim3_solver.hip - compiled for the host
(tests/cpp/sim3_solver_host_check.cpp: the three kernels' bodies with a wave of one lane) against the sequential walk
(tests/sim3_solver_walk.py) on the scenes of tests/sim3_solver_scenes.py, byte for byte: result rows and flag rows.
  (a) every scene of sim3_solver_scenes.CASES; the parallel form (first count above the bar, else the last arg-max) against the chunked loop
      on every scene, for chunks of 20, 1 and 7;
  (b) the statuses and rules, crafted: TOO_FEW, N == min_inliers, NO_MORE on pure outliers with the LAST arg-max, convergence at iteration 0
      and at a late one, a tie below the bar, an exact identity (the NaN rotation), three collinear sample points, a point behind both
      cameras, errors on each side of the truncated thresholds 9 and 13;
  (c) the pieces: its[N] against the reference's expression for every N up to 2000, the draws against the swap-remove loop, the top
      eigenvector against numpy, Rodrigues against the closed form, the double atan2 / sin / cos against the walk's statement bit for bit
      and against the host libm after rounding to float (the counts are printed: docs/history/r24_sim3_solver.md);
  (d) the float64 statement WITHOUT a quaternion (Umeyama's rotation by SVD) on MARGIN_SEEDS: every reprojection error clear of its
      threshold, the same status, winning iteration, counts and flag set, R, t, s within a bound derived by perturbing the float64 statement;
  (e) the stand-alone sanitizer program; the header's declarations against the Python mirror."""
import collections
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import extractorb_amd as X
import sim3_solver_scenes as SC
import sim3_solver_walk as SW
from test_kb8_math import HOST_FLAGS, ROOT

f32, f64 = np.float32, np.float64
VP = C.c_void_p
SRC = os.path.join(ROOT, "tests", "cpp", "sim3_solver_host_check.cpp")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("sshost")), "libsim3_solver_host.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", *HOST_FLAGS, SRC, "-o", so])
    L = C.CDLL(so)
    L.ss_host.argtypes = [C.c_int, VP, C.c_int, VP, VP, VP, VP, C.c_double, C.c_int, C.c_int, C.c_int, VP, VP, VP]
    L.ss_host.restype = None
    L.ss_ransac_iterations.argtypes = [C.c_double, C.c_int, C.c_int]
    L.ss_atan2.argtypes = [C.c_double, C.c_double]
    L.ss_atan2.restype = C.c_double
    L.ss_sincos.argtypes = [C.c_double, VP, VP]
    L.ss_max_error.argtypes = [C.c_float]
    L.ss_max_error.restype = C.c_float
    L.ss_draw3.argtypes = [VP, C.c_int, VP]
    L.ss_eigen_top4.argtypes = [VP, VP]
    L.ss_rodrigues.argtypes = [VP, VP]
    L.ss_compute_sim3.argtypes = [VP, VP, C.c_int, VP]
    L.ss_check_math.argtypes = [C.c_int, VP, VP]
    return L


def ptr(a):
    return a.ctypes.data_as(VP)


def run_host(L, s):
    o = SC.poisoned_outputs(s)
    L.ss_host(len(s["list"]), ptr(s["problems"]), s["cap"], ptr(s["x1w"]), ptr(s["x2w"]), ptr(s["oct1"]), ptr(s["oct2"]), s["probability"],
              s["min_inliers"], s["max_iterations"], s["nlevels"], ptr(s["rand"]), ptr(o["result"]), ptr(o["inliers"]))
    return o


def both(L, s):
    """the header and the walk on scene s, equal byte for byte; returns (host outputs, walked)"""
    walked = SC.walk(s)
    got = run_host(L, s)
    assert SC.differences(got, SC.expected(s, walked)) == []
    return got, walked


def test_the_rows_are_the_headers(host):
    assert host.ss_result_bytes() == SC.RESULT_DTYPE.itemsize == X.SIM3_RESULT_DTYPE.itemsize == 144
    assert host.ss_problem_bytes() == SC.PROBLEM_DTYPE.itemsize == X.SIM3_PROBLEM_DTYPE.itemsize == 240
    assert SC.RESULT_DTYPE == X.SIM3_RESULT_DTYPE and SC.PROBLEM_DTYPE == X.SIM3_PROBLEM_DTYPE
    header = open(os.path.join(ROOT, "include", "orbx.h")).read()
    names = re.findall(r"ORBX_SIM3_SOLVE_(\w+) = (\d+)", header)
    assert [n for n, _ in names] == list(SW.STATUS) == list(X.SIM3_STATUS) and [int(v) for _, v in names] == list(range(len(SW.STATUS)))
    assert "orbx_sim3_solve_device" in X.header_symbols()


@pytest.mark.parametrize("name", list(SC.CASES))
def test_the_header_equals_the_walk_byte_for_byte(host, name):
    got = run_host(host, SC.case(name))
    want = SC.case_expected(name)[1]
    assert SC.differences(got, want) == [], [(a, SW.STATUS[b]) for a, b in zip(got["result"]["status"], want["result"]["status"])]


def _same(a, b):
    for k in a:
        if k == "flags":
            assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]), k
        else:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), (k, a[k], b[k])


@pytest.mark.parametrize("name", list(SC.CASES))
def test_the_parallel_form_is_the_chunked_loop(name):
    """every iteration on its own, then the first count above min_inliers or else the last arg-max: the reference's loop in chunks of 20, and
    in chunks of 1 and 7 (the split into calls changes nothing)"""
    s = SC.case(name)
    loop = SC.case_expected(name)[0]
    for a, b in zip(loop, SC.walk(s, SW.solve_parallel)):
        _same(a, b)
    for chunk in (1, 7):
        form = lambda *a, **k: SW.solve(*a, chunk=chunk, **k)
        for a, b in zip(loop, SC.walk(s, form)):
            _same(a, b)


def test_the_scenes_reach_the_statuses():
    hist, sizes, its = collections.Counter(), set(), set()
    for name in SC.CASES:
        for w in SC.case_expected(name)[0]:
            hist[SW.STATUS[w["status"]]] += 1
            sizes.add(w["n"])
        its.add(SC.case(name)["max_iterations"])
    print(dict(hist))
    assert sizes >= {3, 14, 15, 16, 20, 63, 64, 65, 130, 300} and its >= {1, 20, 21, 300}
    assert all(hist[k] for k in ("CONVERGED", "NO_MORE", "TOO_FEW"))
    first = lambda name: SC.case_expected(name)[0][0]
    w = first("n14_too_few")
    assert SW.STATUS[w["status"]] == "TOO_FEW" and w["n"] == 14 and w["iterations"] == 0 and not w["flags"].any()
    # N == min_inliers: ONE iteration (:142-143), which cannot count more than N: NO_MORE with a best
    for name in ("n15_equals_min_inliers", "n3_min3_one_iteration"):
        w = first(name)
        assert SW.STATUS[w["status"]] == "NO_MORE" and w["max_its"] == w["iterations"] == 1 and w["best_it"] == 0
        assert w["best_inliers"] == w["n"] and w["n_inliers"] == 0 and not w["flags"].any() and abs(float(w["scale"]) - SC.TRUE_SCALE) < 0.02
    # pure outliers: all 300 iterations, the LAST of the greatest count
    w = first("n64_pure_outliers_it300")
    top = max(w["counts"])
    assert SW.STATUS[w["status"]] == "NO_MORE" and w["iterations"] == 300 and len(w["counts"]) == 300 and top <= 15
    assert w["best_it"] == max(i for i, c in enumerate(w["counts"]) if c == top) and w["best_inliers"] == top
    # both fix_scale values at a true scale of 1.7: free, the scale is found; fixed, nothing converges
    assert abs(float(first("n64_it300")["scale"]) - SC.TRUE_SCALE) < 0.02 and SW.STATUS[first("n64_it300")["status"]] == "CONVERGED"
    assert first("n65_it21_fix_scale")["scale"] == 1 and SW.STATUS[first("n65_it21_fix_scale")["status"]] == "NO_MORE"
    assert SW.STATUS[first("n65_it300_fix_scale_true_scale_1")["status"]] == "CONVERGED"
    # the compaction is not the identity
    s = SC.case("n64_it300")
    assert (np.nonzero((s["oct1"][0][:s["list"][0]["n1"]] >= 0) & (s["oct2"][0][:s["list"][0]["n1"]] >= 0))[0] != np.arange(64)).any()


def _inliers_of(name):
    """(scene, compacted indices of the converged flag set, of the rest)"""
    s = SC.case(name)
    w = SC.case_expected(name)[0][0]
    assert w["status"] == SW.CONVERGED
    idx1 = np.nonzero((s["oct1"][0][:s["list"][0]["n1"]] >= 0) & (s["oct2"][0][:s["list"][0]["n1"]] >= 0))[0]
    inl = np.nonzero(w["flags"][idx1])[0]
    return s, inl, np.setdiff1d(np.arange(len(idx1)), inl)


def test_convergence_at_iteration_0_and_at_a_late_iteration(host):
    s, inl, out = _inliers_of("n64_it300")
    rng = np.random.default_rng(5)
    good = tuple(int(v) for v in inl[[0, len(inl) // 2, len(inl) - 1]])
    for late in (0, 257):
        triples = [tuple(int(v) for v in rng.choice(out, 3, replace=False)) for _ in range(300)]
        triples[late] = good
        s2 = dict(s, rand=SC.rand_for(triples, 64)[None])
        got, walked = both(host, s2)
        w = walked[0]
        assert w["status"] == SW.CONVERGED and w["best_it"] == late and w["iterations"] == late + 1 and got["result"]["iterations"][0] == late + 1
        assert all(c <= 15 for c in w["counts"][:late]) and w["n_inliers"] == w["best_inliers"] > 15
        assert int(got["inliers"][0][:s["list"][0]["n1"]].sum()) == w["n_inliers"]


def test_a_tie_below_the_bar_goes_to_the_later_iteration(host):
    s = SC.case("n20_it21")
    w = SC.case_expected("n20_it21")[0][0]
    assert w["status"] == SW.NO_MORE and w["max_its"] == 9
    counts = w["counts"]
    src = int(np.argmax(counts))
    rand = s["rand"].copy()
    rand[0, 1], rand[0, 7] = rand[0, src], rand[0, src]      # the same draws three times: the same count three times
    rand[0, 8] = rand[0, 0] if counts[0] < counts[src] or src == 0 else rand[0, 8]
    got, walked = both(host, dict(s, rand=rand))
    c = walked[0]["counts"]
    assert c[1] == c[7] == max(c) and walked[0]["best_it"] == max(i for i, v in enumerate(c) if v == max(c)) >= 7
    assert walked[0]["status"] == SW.NO_MORE and got["result"]["best_it"][0] == walked[0]["best_it"]


def test_an_exact_identity_is_the_references_nan_rotation(host):
    """P1 == P2 exactly: M is symmetric, N12 = N13 = N14 = 0, the top eigenvector is (1, 0, 0, 0) exactly, its imaginary part has norm 0, ang
    is 0 and 2 * ang * vec / norm(vec) is 0 / 0.  The reference goes on with a NaN rotation: no error compares below its threshold, the count
    is 0, and `0 >= mnBestInliers` makes every such iteration the new "best".  The statement keeps that: NO_MORE, best_inliers 0, the LAST
    iteration, every NaN of the row the one quiet NaN."""
    s = SC.make([20], 31, max_iterations=21, outliers=0.0, noise=0.0)
    pb = dict(s["list"][0])
    pb["Tcw2"], pb["x2w"] = pb["Tcw1"].copy(), pb["x1w"].copy()
    s2 = SC.scene([pb], np.random.default_rng(1), 21)
    got, walked = both(host, s2)
    r = got["result"][0]
    assert SW.STATUS[r["status"]] == "NO_MORE" and r["best_inliers"] == 0 and r["n_inliers"] == 0 and r["best_it"] == r["max_its"] - 1 == 8
    assert walked[0]["counts"] == [0] * 9 and not got["inliers"][0][:pb["n1"]].any()
    assert (r["R"].view(np.uint32) == 0x7fc00000).all() and (r["t"].view(np.uint32) == 0x7fc00000).all() and r["scale"].view(np.uint32) == 0x7fc00000
    assert (r["T12"][:12].view(np.uint32) == 0x7fc00000).all() and list(r["T12"][12:]) == [0, 0, 0, 1]
    # the quaternion itself
    P = np.array([[1.0, -2.0, 0.5], [0.25, 1.5, -1.0], [4.0, 5.5, 7.0]], f32)
    out = np.zeros(37, f32)
    host.ss_compute_sim3(ptr(P), ptr(P.copy()), 0, ptr(out))
    assert np.isnan(out[:9]).all()


def test_three_collinear_sample_points(host):
    """two equal top eigenvalues: any unit vector of their plane is an eigenvector and the iteration's own is taken.  The header and the walk
    take the same one, it is a rotation, and it carries the line's direction over"""
    d2 = np.array([0.3, -0.2, 1.0])
    Pb = (np.array([[0.5], [1.0], [5.0]]) + d2[:, None] * np.array([-1.0, 0.25, 2.0])).astype(f32)
    R, t = SC.rot((0.3, 1.0, -0.2), 0.4), np.array([[0.3], [-0.2], [0.4]])
    Pa = (1.7 * R @ Pb.astype(f64) + t).astype(f32)
    out = np.zeros(37, f32)
    host.ss_compute_sim3(ptr(Pa), ptr(Pb), 0, ptr(out))
    Rw, tw, sw, T12, T21 = SW.compute_sim3(Pa, Pb, False, SW.HEADER_MATH)
    assert out[:9].tobytes() == Rw.tobytes() and out[9:12].tobytes() == tw.tobytes() and out[12:13].tobytes() == f32(sw).tobytes()
    assert out[13:25].tobytes() == T12[:3].tobytes() and out[25:37].tobytes() == T21[:3].tobytes()
    Rh = out[:9].reshape(3, 3).astype(f64)
    assert np.abs(Rh @ Rh.T - np.eye(3)).max() < 1e-5 and abs(np.linalg.det(Rh) - 1) < 1e-5
    assert np.abs(Rh @ d2 / np.linalg.norm(d2) - R @ d2 / np.linalg.norm(d2)).max() < 1e-4 and abs(out[12] - 1.7) < 1e-4


def _exact_problem(extra, cap=16):
    """three exact correspondences under the true Sim3 with identity poses, then `extra`: (X2c, displacement in camera 1, octave1, octave2)"""
    R12, t12, sc = SC.rot((0.3, 1.0, -0.2), 0.12), np.array([0.3, -0.2, 0.4]), SC.TRUE_SCALE
    X2 = [np.array(v) for v in ((-1.5, -1.0, 5.0), (1.6, -0.4, 6.5), (0.2, 1.2, 4.5))] + [np.array(e[0], float) for e in extra]
    X1 = [sc * R12 @ x + t12 for x in X2]
    for k, e in enumerate(extra):
        X1[3 + k] = X1[3 + k] + np.array(e[1], float)
    n = len(X2)
    eye = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(f32).reshape(-1)
    full = lambda a, fill: np.concatenate([np.array(a, f32), np.full((cap - n, 3), fill, f32)])
    o1 = np.array([3, 3, 3] + [e[2] for e in extra] + [-1] * (cap - n), np.int32)
    o2 = np.array([3, 3, 3] + [e[3] for e in extra] + [-1] * (cap - n), np.int32)
    pb = dict(n1=n, fix_scale=0, model1=0, model2=0, cam1=np.array(SC.PINHOLE, f32), cam2=np.array(SC.PINHOLE, f32), Tcw1=eye, Tcw2=eye.copy(),
              sigma2=SC.SIGMA2.copy(), x1w=full(X1, 0), x2w=full(X2, 0), oct1=o1, oct2=o2)
    s = SC.scene([pb], np.random.default_rng(0), 5, min_inliers=3)
    s["rand"][0] = SC.rand_for([(0, 1, 2)] * 5, n)
    return s


def test_the_thresholds_are_truncated_integers(host):
    """9.210 * sigma2 truncated: 9 at level 0, 13 at level 1 (9.21 * 1.44 = 13.26).  Errors of about 8.6, 9.1 (between 9 and 9.21: an
    outlier only because of the truncation), 12.6 and 13.1 in image 1, the other image's threshold wide (level 3: 27)"""
    assert [float(host.ss_max_error(f32(v))) for v in SC.SIGMA2[:4]] == [9.0, 13.0, 19.0, 27.0] == [float(SW.max_error(v)) for v in SC.SIGMA2[:4]]
    z = 6.0
    X2 = np.array([0.4, 0.3, z])
    z1 = float((SC.TRUE_SCALE * SC.rot((0.3, 1.0, -0.2), 0.12) @ X2 + np.array([0.3, -0.2, 0.4]))[2])
    dx = lambda err: (np.sqrt(err) * z1 / SC.PINHOLE[0], 0.0, 0.0)
    s = _exact_problem([(X2, dx(8.6), 0, 3), (X2, dx(9.1), 0, 3), (X2, dx(12.6), 1, 3), (X2, dx(13.1), 1, 3), (X2, dx(9.1), 1, 3)])
    got, walked = both(host, s)
    h = SW.Evaluator(s["list"][0], SW.construct(s["list"][0], SC.NLEVELS), s["rand"][0], SW.HEADER_MATH).run(0)
    e = [float(v) for v in h["err1"][3:]]
    assert 8.4 < e[0] < 9 < e[1] < 9.21 and 12.4 < e[2] < 13 < e[3] < 13.26 and (h["err2"][3:] < 27).all(), e
    assert list(got["inliers"][0][:8]) == [1, 1, 1, 1, 0, 1, 0, 1] and walked[0]["status"] == SW.CONVERGED and walked[0]["n_inliers"] == 6


def test_a_point_behind_both_cameras(host):
    """z <= 0 after the transform: the reference has no depth test here.  A correspondence that lies behind both cameras consistently
    projects through the centre onto the same pixel in both ways and counts as an inlier; the statement keeps that"""
    s = _exact_problem([((0.4, 0.3, -6.0), (0.0, 0.0, 0.0), 0, 0), ((0.4, 0.3, 6.0), (0.0, 0.0, -40.0), 0, 0)])
    got, walked = both(host, s)
    con = SW.construct(s["list"][0], SC.NLEVELS)
    assert con["X2"][3, 2] < 0 and con["X1"][3, 2] < 0 and con["X1"][4, 2] < 0 < con["X2"][4, 2]
    assert list(got["inliers"][0][:5]) == [1, 1, 1, 1, 0] and walked[0]["n_inliers"] == 4


def test_out_of_range_problems(host):
    base = SC.case("batch3")
    rows, oct1 = base["problems"].copy(), base["oct1"].copy()
    rows["n1"][0], rows["model2"][1] = base["cap"] + 1, 2
    oct1[2, 1] = SC.NLEVELS
    lst = [dict(pb) for pb in base["list"]]
    lst[0]["n1"], lst[1]["model2"], lst[2]["oct1"] = base["cap"] + 1, 2, oct1[2]
    got, walked = both(host, dict(base, problems=rows, oct1=oct1, list=lst))
    assert (got["result"]["status"] == SW.BAD_ARGUMENT).all() and (got["inliers"][0] == SC.POISON_B).all() and not got["inliers"][1, :lst[1]["n1"]].any()
    # fewer than three correspondences with N >= min_inliers: RandomInt(0, -1) in the reference
    s = SC.make([2], 40, min_inliers=2, outliers=0.0)
    got, walked = both(host, s)
    assert got["result"]["status"][0] == SW.BAD_ARGUMENT and got["result"]["n"][0] == 2


def test_the_iteration_table_is_the_references_expression(host):
    """its[N] for every N from 1 to 2000 at the call site's parameters and at others; the conversion of a double outside the int range"""
    import math
    for prob, mn in ((0.99, 15), (0.99, 3), (0.5, 20), (0.999, 100), (0.99, 1)):
        for N in range(1, 2001):
            want = 1 if mn == N else math.ceil(math.log(1 - prob) / math.log(1 - math.pow(float(f32(mn) / f32(N)), 3))) if N > mn else None
            want = SW.INT_MIN if want is not None and not -2 ** 31 <= want < 2 ** 31 else want      # `int nIterations = ceil(..)` on x86-64
            got = host.ss_ransac_iterations(prob, mn, N)
            assert got == SW.ransac_iterations(prob, mn, N), (prob, mn, N)
            if want is not None:
                assert got == want, (prob, mn, N, got, want)
    assert host.ss_ransac_iterations(0.99, 15, 64) == 356 and host.ss_ransac_iterations(0.99, 15, 20) == 9
    for prob, mn, N in ((0.99, 0, 50), (1.0, 15, 50), (0.99, 15, 4000000), (0.0, 15, 50), (0.99, -3, 50), (0.99, 60, 50)):
        assert host.ss_ransac_iterations(prob, mn, N) == SW.ransac_iterations(prob, mn, N), (prob, mn, N)
    assert host.ss_ransac_iterations(0.99, 15, 4000000) == SW.INT_MIN and host.ss_ransac_iterations(0.99, 0, 50) == SW.INT_MIN


def test_the_draws_are_the_swap_remove_loop(host):
    rng = np.random.default_rng(3)
    for N in (3, 4, 5, 64, 300):
        for _ in range(200):
            r = rng.integers(-2 ** 31, 2 ** 31, 3).astype(np.int32) if N == 5 else rng.integers(0, 2 ** 31, 3).astype(np.int32)
            idx = np.zeros(3, np.int32)
            host.ss_draw3(ptr(r), N, ptr(idx))
            assert list(idx) == SW.draw3(r, N) and len(set(idx)) == 3 and 0 <= idx.min() and idx.max() < N


def _horn(rng):
    Pb = rng.normal(0, 2, (3, 3))
    Pa = 1.3 * SC.rot(rng.normal(0, 1, 3), rng.uniform(0, 3.1)) @ Pb + rng.normal(0, 1, (3, 1))
    Pr1, Pr2 = Pa - Pa.mean(axis=1, keepdims=True), Pb - Pb.mean(axis=1, keepdims=True)
    M = Pr2 @ Pr1.T
    return np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                     [M[1, 2] - M[2, 1], M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                     [M[2, 0] - M[0, 2], M[0, 1] + M[1, 0], -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                     [M[0, 1] - M[1, 0], M[2, 0] + M[0, 2], M[1, 2] + M[2, 1], -M[0, 0] - M[1, 1] + M[2, 2]]])


def test_the_eigenvector_and_rodrigues_against_numpy(host):
    rng = np.random.default_rng(8)
    worst = 0.0
    for _ in range(200):
        N = _horn(rng).astype(f32)
        q = np.zeros(4, f32)
        host.ss_eigen_top4(ptr(N), ptr(q))
        assert q.tobytes() == SW.eigen_top4(N).tobytes()
        lam, vec = np.linalg.eigh(N.astype(f64))
        gap = (lam[3] - lam[2]) / np.abs(lam).max()
        v = vec[:, 3] * np.sign(vec[0, 3])
        assert q[0] >= 0 and abs(np.linalg.norm(q.astype(f64)) - 1) < 1e-5
        err = np.abs(q - v).max() * gap
        worst = max(worst, err)
    print("eigenvector: worst |dq| * relative gap = %.3g (%.0f u)" % (worst, worst / 2.0 ** -24))
    assert worst < 64 * 2.0 ** -24
    for _ in range(100):
        rv = (rng.normal(0, 1, 3) * rng.choice([1e-20, 1e-3, 1.0, 3.0])).astype(f32)
        R = np.zeros(9, f32)
        host.ss_rodrigues(ptr(rv), ptr(R))
        assert R.tobytes() == SW.rodrigues(rv, SW.HEADER_MATH).tobytes()
        th = np.linalg.norm(rv.astype(f64))
        want = np.eye(3) if th < 2.2e-16 else SC.rot(rv.astype(f64), th)
        assert np.abs(R.reshape(3, 3) - want).max() < 2e-7


def test_the_double_functions(host):
    """the header's atan2 / sin / cos: bit for bit the walk's statement of them, and against the host libm after rounding to float over a
    sweep - the counts of differing floats are a measurement (printed), the double results lie within 16 units of libm's"""
    rng = np.random.default_rng(2)
    s, c = C.c_double(), C.c_double()
    for _ in range(2000):
        y, x, th = abs(rng.normal()), rng.normal(), rng.uniform(0, 7)
        assert host.ss_atan2(y, x) == float(SW.header_atan2(y, x))
        host.ss_sincos(th, C.byref(s), C.byref(c))
        ws, wc = SW.header_sincos(th)
        assert (s.value, c.value) == (float(ws), float(wc))
    for y, x in ((0.0, 0.0), (0.0, 1.0), (1.0, 0.0), (0.0, -1.0), (1.0, 1.0), (float("inf"), float("inf")), (1e-300, 1e300)):
        assert abs(host.ss_atan2(y, x) - np.arctan2(y, x)) < 1e-15
    assert np.isnan(host.ss_atan2(float("nan"), 1.0)) and np.isnan(host.ss_atan2(1.0, float("nan")))
    for th in (float("nan"), float("inf"), -1.0, 2.0 ** 21):
        host.ss_sincos(th, C.byref(s), C.byref(c))
        assert np.isnan(s.value) and np.isnan(c.value)
    out, worst = np.zeros(6, np.int64), np.zeros(3, f64)
    host.ss_check_math(700, ptr(out), ptr(worst))
    print("atan2: %d of %d floats differ; sin: %d of %d; cos: %d of %d; worst double difference %.1f / %.1f / %.1f ulp" %
          (out[1], out[0], out[3], out[2], out[5], out[4], worst[0], worst[1], worst[2]))
    assert out[0] > 900000 and out[2] == out[4] > 5000 and worst.max() < 16


# ---- the float64 statement without a quaternion ------------------------------------------------------------------------------------------
MARGIN_SEEDS = ("n64_it300", "n300_it300", "n65_it300_fix_scale_true_scale_1", "n20_it21", "n65_it21_fix_scale")      # cases of sim3_solver_scenes.CASES, problem 0
UNIT = 2.0 ** -24                                        # the unit roundoff of binary32
# What binary32 costs R, t and s of the winning iteration against float64; both read the same binary32 world points and poses.
#  * the sample: an X3Dc coordinate is one gemmRow (one rounding), the centroid three more, the centred coordinate one, an element of M one,
#    an entry of N up to three: SAMPLE_UNITS = 16 u of each of the 18 coordinates of the three sample pairs, relative to the coordinate.
#    perturbation_bound() moves each by that much in the FLOAT64 statement, aligns again, and adds up the moves of R, t and s (first order,
#    every error at its worst sign);
#  * the eigenvector: the Jacobi iteration leaves q within EIGEN_UNITS = 64 u / (relative gap of the two top eigenvalues) of the exact one
#    (test_the_eigenvector_and_rodrigues_against_numpy measures it), and a change dq of a unit quaternion moves R by at most 4 |dq|;
#    atan2, the scaling and Rodrigues add ROTATE_UNITS = 8 u on every element of R;
#  * s = nom / den moves with R by at most s |dR| * 3, t = O1 - s R O2 by (s |dR| * 3 + |ds|) |O2|, each with 4 u of its own.
SAMPLE_UNITS, EIGEN_UNITS, ROTATE_UNITS = 16, 64, 8


def clear_of(value, threshold, rel):
    return abs(float(value) - float(threshold)) > rel * max(float(value), float(threshold))


def perturbation_bound(pb, w64, X1, X2, idx):
    R0, t0, s0 = w64["R"], w64["t"], w64["scale"]
    move_R = move_t = move_s = 0.0
    for which in (0, 1):
        for i in range(3):
            for c in range(3):
                P = [X1[idx].T.copy(), X2[idx].T.copy()]
                P[which][c, i] += SAMPLE_UNITS * UNIT * abs(P[which][c, i])
                R, t, s = SW.align_float64(P[0], P[1], bool(pb["fix_scale"]))
                move_R += np.abs(R - R0).max(); move_t += np.abs(t - t0).max(); move_s += abs(s - s0)
    Pr1, Pr2 = X1[idx].T - X1[idx].T.mean(axis=1, keepdims=True), X2[idx].T - X2[idx].T.mean(axis=1, keepdims=True)
    M = Pr2 @ Pr1.T
    sv = np.linalg.svd(M)[1]
    gap = 2 * sv[1] / (sv[0] + sv[1])                        # the eigenvalues of N are +-(s1 + s2), +-(s1 - s2)
    bound_R = move_R + 4 * EIGEN_UNITS * UNIT / gap + ROTATE_UNITS * UNIT
    O2 = np.abs(X2[idx].mean(axis=0)).max()
    bound_s = move_s + 3 * s0 * bound_R + 4 * UNIT * s0
    bound_t = move_t + (3 * s0 * bound_R + bound_s) * O2 * 3 + 4 * UNIT * np.abs(t0).max()
    return bound_R, bound_t, bound_s


@pytest.mark.parametrize("name", MARGIN_SEEDS)
def test_the_float64_statement_takes_the_same_decisions(name):
    """On MARGIN_SEEDS the float64 alignment by SVD, no quaternion anywhere, gives the same status, winning iteration, iteration count,
    inlier counts of every iteration run and flag set as the binary32 walk, and R, t, s agree within perturbation_bound().  The condition on
    the inputs, asserted in the float64 statement: every reprojection error of every iteration run is clear of its threshold by 1 % of the
    larger of the two (a wild hypothesis has large errors in both kinds; a relative margin covers it)."""
    s = SC.case(name)
    pb, rand = s["list"][0], s["rand"][0]
    w64 = SW.solve_float64(pb, rand, s["probability"], s["min_inliers"], s["max_iterations"], s["nlevels"])
    w32 = SC.case_expected(name)[0][0]
    for run in w64["runs"]:
        for err, mx in ((run["err1"], w64["max1"]), (run["err2"], w64["max2"])):
            close = [(float(e), float(m)) for e, m in zip(err, mx) if not clear_of(e, m, 0.01)]
            assert not close, close
    for f in ("status", "best_it", "iterations", "n_inliers", "best_inliers", "n", "max_its"):
        assert w64[f] == w32[f], (f, w64[f], w32[f])
    assert w64["counts"] == w32["counts"] and np.array_equal(w64["flags"], w32["flags"])
    con = SW.construct(pb, s["nlevels"])
    bound_R, bound_t, bound_s = perturbation_bound(pb, w64, con["X1"].astype(f64), con["X2"].astype(f64), SW.draw3(rand[w64["best_it"]], w64["n"]))
    dR = np.abs(w64["R"] - w32["R"].reshape(3, 3)).max()
    dt = np.abs(w64["t"] - w32["t"]).max()
    ds = abs(w64["scale"] - float(w32["scale"]))
    print("%s: |dR| %.3g of %.3g (%.1f %%), |dt| %.3g of %.3g (%.1f %%), |ds| %.3g of %.3g (%.1f %%)" %
          (name, dR, bound_R, 100 * dR / bound_R, dt, bound_t, 100 * dt / bound_t, ds, bound_s, 100 * ds / bound_s if bound_s else 0))
    assert dR <= bound_R and dt <= bound_t and ds <= bound_s


def test_the_walk_with_the_host_libm_decides_the_same():
    """the double functions are parameters of the walk: with the host libm's atan2 / sin / cos in place of the header's the scenes take the
    same decisions (the rotation may differ in its last place)"""
    for name in ("n64_it300", "n63_it20_kb8", "batch3"):
        for a, b in zip(SC.case_expected(name)[0], SC.walk(SC.case(name), m=SW.LIBM_MATH)):
            assert (a["status"], a["best_it"], a["counts"]) == (b["status"], b["best_it"], b["counts"])
            assert np.allclose(np.asarray(a["R"]), np.asarray(b["R"]), atol=3e-7, equal_nan=True)


def test_the_sanitizer_program(tmp_path):
    exe = os.path.join(str(tmp_path), "sim3_solver_host_check")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSIM3_SOLVER_HOST_MAIN", *HOST_FLAGS, SRC,
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "every access inside its arrays" in out.stdout and "FAILED" not in out.stdout, out.stdout + out.stderr
