"""Optimizer::PoseOptimization without a GPU: extractorb_amd/csrc/k_pose_optimization.hpp - the statement of k_pose_optimization.hip -
compiled for the host (tests/cpp/pose_optimization_host_check.cpp: the kernel's body with the 256 sum slots in a loop) against the
sequential walk (tests/pose_optimization_walk.py) on the scenes of tests/pose_optimization_scenes.py, byte for byte: poses, flag rows,
result rows, the poison beyond N and on keypoints without a MapPoint.
  (a) every scene of pose_optimization_scenes.CASES;
  (b) the exits and events, crafted or found, each asserted to be reached: N = 2, N = 9, a rejected last trial whose stale errors classify
      differently from a fresh computeError, an inlier Huber keeps that round 3 flags, an outlier of round 0 that returns in round 1, a round
      without an active edge, an update below theta = 1e-5, z < 0 and z == 0, chi2 on each side of 5.991f and 7.815f (planted within 4e-3), the _nBad >= 3 stop,
      ten failed trials;
  (c) the pieces: the Huber triple, exp in both branches, the quaternion of a matrix and back, the 6x6 solve against numpy.linalg.solve,
      each projectJac against a central difference of its project, the order of the sums against a plain Python loop;
  (d) the float64 statement in g2o's OWN order (edge-by-edge sums, numpy.linalg, libm) on MARGIN_SEEDS: its margins first, then the same
      statuses, counts and flag sets, and the pose within a bound derived by perturbing the sums;
  (e) the header's declarations against the Python mirror; (f) the stand-alone sanitizer program."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import extractorb_amd as X
import pose_optimization_scenes as SC
import pose_optimization_walk as PW
from test_kb8_math import HOST_FLAGS, ROOT

f32, f64 = np.float32, np.float64
VP = C.c_void_p
SRC = os.path.join(ROOT, "tests", "cpp", "pose_optimization_host_check.cpp")
UNIT = 2.0 ** -53


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("pohost")), "libpose_optimization_host.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", *HOST_FLAGS, SRC, "-o", so])
    L = C.CDLL(so)
    L.po_host.argtypes = [C.c_int] * 4 + [VP] * 4 + [C.c_int, VP, VP, C.c_int, C.c_int, VP, VP, VP]
    L.po_host.restype = None
    L.po_exp.argtypes = [VP, VP]
    L.po_quat.argtypes = [VP, VP, VP]
    L.po_solve6.argtypes = [VP, C.c_double, VP, VP]
    L.po_huber.argtypes = [C.c_int, C.c_int, C.c_double, VP]
    L.po_project.argtypes = [C.c_int, VP, VP, VP]
    L.po_project_jac.argtypes = [C.c_int, VP, VP, VP]
    L.po_sum.argtypes = [VP, C.c_int]
    L.po_sum.restype = C.c_double
    return L


def ptr(a):
    return None if a is None else a.ctypes.data_as(VP)


def run_host(L, s):
    o = SC.poisoned_outputs(s)
    L.po_host(s["n_problems"], s["first"], s["step"], s["eyes"], ptr(s["problems"]), ptr(s["kps"]), ptr(s["n_out"]), ptr(s["u_right"]), s["cap"],
              ptr(s["matches"]), ptr(s["world"]), len(s["world"]), s["nlevels"], ptr(o["poses"]), ptr(o["outlier"]), ptr(o["result"]))
    return o


def both(L, name):
    """the header and the walk on a named scene, equal byte for byte; returns (scene, host outputs, walked)"""
    s = SC.case(name)
    walked, want = SC.case_expected(name)
    got = run_host(L, s)
    assert SC.differences(got, want) == [], name
    return s, got, walked


# ---- (e) ------------------------------------------------------------------------------------------------------------------------------
def test_the_rows_and_names_are_the_headers(host):
    assert host.po_result_bytes() == SC.RESULT_DTYPE.itemsize == X.POSE_RESULT_DTYPE.itemsize == 120
    assert host.po_problem_bytes() == SC.PROBLEM_DTYPE.itemsize == X.POSE_PROBLEM_DTYPE.itemsize == 188
    assert SC.RESULT_DTYPE == X.POSE_RESULT_DTYPE and SC.PROBLEM_DTYPE == X.POSE_PROBLEM_DTYPE and SC.KEYPOINT_DTYPE == X.KEYPOINT_DTYPE
    header = open(os.path.join(ROOT, "include", "orbx.h")).read()
    names = re.findall(r"ORBX_POSE_OPTIMIZATION_(\w+) = (\d+)", header)
    assert [n for n, _ in names] == list(PW.STATUS) == list(X.POSE_OPTIMIZATION_STATUS) and [int(v) for _, v in names] == list(range(len(PW.STATUS)))
    assert "orbx_optimize_pose_device" in X.header_symbols() and "orbx_debug_pose_optimization_launches" in X.header_symbols()
    assert host.po_slots() == PW.SLOTS == 256 and host.po_lds_bytes() == 4 * PW.SUMS * 8 == 896
    assert "896 bytes" in header                                  # the LDS statement of the declaration's comment


# ---- (a) ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SC.CASES))
def test_the_header_equals_the_walk_byte_for_byte(host, name):
    s, got, walked = both(host, name)
    cap = s["cap"]
    for p in range(s["n_problems"]):                             # the poison: beyond N, and on keypoints without a MapPoint
        for e in range(s["eyes"]):
            row, n = (p * s["eyes"] + e) * cap, int(s["n_out"][(s["first"] + p * s["step"]) * s["eyes"] + e])
            flags, held = got["outlier"][row:row + cap], s["matches"][row:row + cap] >= 0
            assert (flags[n:] == SC.POISON_FLAG).all() and (flags[:n][~held[:n]] == SC.POISON_FLAG).all() and (flags[:n][held[:n]] <= 1).all()


def test_the_cases_cover_what_the_issue_lists():
    counts, batches = set(), set()
    for name in SC.CASES:
        walked = SC.case_expected(name)[0]
        batches.add(len(walked))
        counts.update(w["n_initial"] for w in walked)
    assert counts >= {2, 3, 9, 10, 11, 63, 64, 65, 257, 300} and batches >= {1, 3, 17} and 257 == PW.SLOTS + 1
    kinds = lambda name: set(np.unique(PW.Edges(SC.problem(SC.case(name), 1 if SC.case(name)["n_problems"] > 1 else 0)).kind)) - {0}
    assert kinds("mono_n64") == {1} and kinds("mixed_stereo_batch3") == {1, 2} and kinds("kb8_mono_batch3") == {1} and kinds("kb8_rig_batch3") == {1, 3}
    assert SC.case("kb8_mono_batch3")["problems"]["model"][0] == 1 and SC.case("mono_n64")["problems"]["model"][0] == 0
    # outlier shares 0, 30 % and 100 %; the optimiser finds the planted ones
    for name, share in (("mono_n64_clean", 0.0), ("mono_n64", 0.3), ("mono_n64_all_outliers", 1.0)):
        s, w = SC.case(name), SC.case_expected(name)[0][0]
        assert int(s["planted"].sum()) == round(share * 64)
        if share < 1:
            assert abs(w["n_bad"] - int(s["planted"].sum())) <= 3 and np.abs(w["pose"] - s["true_pose"][0]).max() < 0.02


# ---- (b) ------------------------------------------------------------------------------------------------------------------------------
def test_two_correspondences_leave_the_pose_untouched(host):
    s, got, walked = both(host, "mono_n2")
    r = got["result"][0]
    assert PW.STATUS[r["status"]] == "TOO_FEW" and r["n_initial"] == 2 and r["n_inliers"] == 0 and r["rounds"] == 0
    assert got["poses"].tobytes() == s["poses"].tobytes()
    held = s["matches"][:s["n_out"][0]] >= 0
    assert (got["outlier"][:s["n_out"][0]][held] == 0).all()      # mvbOutlier[i] = false ran before the return


def test_nine_correspondences_run_one_round(host):
    s, got, walked = both(host, "mono_n9")
    r = got["result"][0]
    assert PW.STATUS[r["status"]] == "FEW_EDGES" and r["n_initial"] == 9 and r["rounds"] == 1 and r["its"][0] > 0 and list(r["its"][1:]) == [0, 0, 0]
    assert got["poses"].tobytes() != s["poses"].tobytes() and r["n_inliers"] == 9 - r["n_bad"]
    assert PW.STATUS[both(host, "mono_n10")[1]["result"][0]["status"]] == "ALL_ROUNDS"


def test_a_rejected_last_trial_leaves_stale_errors_and_they_classify_differently(host):
    """nothing recomputes the errors after the last trial.  Here that trial's pose is not finite: its errors are NaN, not > 5.991f, and all
    twelve gross outliers stay inliers, where a fresh computeError at the returned pose flags all twelve"""
    s, got, walked = both(host, "non_finite_trial")
    w, r = walked[0], got["result"][0]
    assert all(t["rejected_last"] for t in w["trace"]) and len(w["trace"]) == 4
    for t in w["trace"]:
        assert t["fresh_flags"].sum() == 12 and t["flags"].sum() == 0 and (t["flags"] != t["fresh_flags"]).sum() == 12
    assert r["n_bad"] == 0 and r["n_inliers"] == 12 and list(r["its"]) == [3, 3, 3, 3] and [t["terminate"] for t in w["trace"]] == ["nbad"] * 4
    assert np.isfinite(got["poses"]).all() and np.abs(got["poses"][:12] - s["poses"][:12]).max() < 1e-6      # every trial was popped
    # the same rule at convergence: ten failed trials end a round of this scene, the last of them rejected
    w = both(host, "mixed_stereo_batch3")[2][1]
    assert [t["terminate"] for t in w["trace"]][1] == "trials" and w["trace"][1]["rejected_last"]


def test_huber_keeps_an_inlier_that_round_3_flags_and_an_outlier_returns(host):
    s, got, walked = both(host, "huber_keeps_round3_flags")
    fl = [t["flags"] for t in walked[0]["trace"]]
    assert (~fl[0] & ~fl[1] & ~fl[2] & fl[3]).sum() >= 1          # inlier under Huber three times, flagged without it
    assert (fl[0] & ~fl[1]).sum() >= 1                            # outlier of round 0, inlier again in round 1


def test_a_round_without_an_active_edge(host):
    for name, p in (("no_active_edge_n100", 0), ("kb8_mono_batch3", 2), ("kb8_rig_batch3", 2)):
        s, got, walked = both(host, name)
        r = got["result"][p]
        assert PW.STATUS[r["status"]] == "ALL_ROUNDS" and r["empty_rounds"] == 0b1110 and list(r["its"][1:]) == [-1, -1, -1] and r["its"][0] > 0
        assert r["n_bad"] == r["n_initial"] and r["n_inliers"] == 0 and list(r["trials"][1:]) == [0, 0, 0]
        f = s["first"] + p * s["step"]
        T0 = PW.se3_to_float(PW.se3_from_float(s["poses"][f * 12:(f + 1) * 12]))
        assert got["poses"][f * 12:(f + 1) * 12].tobytes() == T0.tobytes()      # the estimate stayed the initial pose (through the quaternion)


def test_an_update_below_theta_1e_5(host):
    w = both(host, "mono_n64_clean")[2][0]
    assert all(t["small_theta"] >= 1 for t in w["trace"])


def test_points_behind_the_camera_and_at_z_zero(host):
    s, got, walked = both(host, "behind_the_camera")
    pb = SC.problem(s, 0)
    ed = PW.Edges(pb)
    z = PW.se3_map(walked[0]["T"], [ed.X[:, c] for c in range(3)])[2][ed.kind != 0]
    assert (z < 0).sum() == 3 and PW.STATUS[walked[0]["status"]] == "ALL_ROUNDS" and np.isfinite(got["poses"]).all()
    assert walked[0]["trace"][3]["flags"][np.nonzero(ed.kind)[0][:3]].all()      # they contributed, and ended as outliers
    s, got, walked = both(host, "z_zero")
    r = got["result"][0]
    assert list(r["its"]) == [10] * 4 and list(r["trials"]) == [10] * 4 and all(t["rejected_last"] and t["accepted"] == 0 for t in walked[0]["trace"])
    assert (r["chi2"].view(np.uint64) == 0x7ff8000000000000).all() and (r["lambda"].view(np.uint64) == 0x7ff8000000000000).all()
    assert got["poses"][:12].tobytes() == SC.pose12(np.eye(3), [0, 0, 0]).tobytes()
    ed = PW.Edges(SC.problem(s, 0))
    k = int(np.nonzero((ed.X[:, 2] == 0) & (ed.kind != 0))[0][0])
    assert not walked[0]["trace"][3]["flags"][k] and np.isnan(PW.errors(SC.problem(s, 0), ed, walked[0]["T"], PW.HEADER_MATH)[1][k])


def test_chi2_a_hair_on_each_side_of_both_thresholds(host):
    """round 1 of this scene has no active edge and classifies at the initial pose, where four observations were planted"""
    s, got, walked = both(host, "thresholds")
    w = walked[0]
    assert w["empty_rounds"] & 2 and w["its"][1] == -1
    pb = SC.problem(s, 0)
    ed = PW.Edges(pb)
    chi2 = PW.errors(pb, ed, PW.se3_from_float(pb["pose"]), PW.HEADER_MATH)[1]
    for k, thr, sign in s["planted_thresholds"]:
        print("edge %d kind %d: chi2 %.5f against %.3f" % (k, ed.kind[k], chi2[k], thr))
        assert abs(chi2[k] - thr) < 4e-3 and (chi2[k] > thr) == (sign > 0) and ed.kind[k] == (1 if thr < 7 else 2)
        assert bool(w["trace"][1]["flags"][k]) == (sign > 0) and w["trace"][0]["flags"][k]      # an outlier of round 0, decided anew in round 1


def test_chi2_on_each_side_of_both_thresholds(host):
    s, got, walked = both(host, "mixed_stereo_batch3")
    seen = []
    PW.solve(SC.problem(s, 2), observe=lambda name, **v: seen.append((v["values"], v["thresholds"])) if name == "chi2" else None)
    chi, thr = np.concatenate([a for a, _ in seen]), np.concatenate([b for _, b in seen])
    for t in (PW.CHI2_MONO, PW.CHI2_STEREO):
        mine = chi[thr == f64(t)]
        assert (mine.astype(f32) > t).any() and (mine.astype(f32) <= t).any()
        print("threshold %.3f: nearest below %.4f, nearest above %.4f" % (t, mine[mine <= t].max(), mine[mine > t].min()))
    # the comparison is a float's: the double just above 5.991f's double value rounds to 5.991f and is NOT an outlier
    assert f32(np.nextafter(f64(PW.CHI2_MONO), 10.0)) == PW.CHI2_MONO and not f32(np.nextafter(f64(PW.CHI2_MONO), 10.0)) > PW.CHI2_MONO


def test_the_nbad_stop_and_ten_failed_trials(host):
    w = both(host, "mono_n64")[2][0]
    assert [t["terminate"] for t in w["trace"]] == ["nbad"] * 4 and all(0 < i < 10 for i in w["its"])
    w = both(host, "mixed_stereo_batch3")[2][1]
    assert w["trace"][1]["terminate"] == "trials" and w["trials"][1] >= w["its"][1] - 1 + 10
    w = both(host, "mono_batch17")[2][1]
    assert w["trace"][0]["terminate"] is None and w["its"][0] == 10      # all ten iterations


# ---- (c) ------------------------------------------------------------------------------------------------------------------------------
def test_the_huber_triple(host):
    out = np.zeros(2, f64)
    for stereo, delta in ((0, PW.DELTA_MONO), (1, PW.DELTA_STEREO)):
        assert delta == f64(f32(np.sqrt(5.991 if not stereo else 7.815)))
        for e in (0.0, 1.0, float(delta * delta), float(np.nextafter(delta * delta, 100.0)), 7.0, 8.0, 1e6, np.inf):
            host.po_huber(stereo, 1, e, ptr(out))
            ed = type("E", (), {"kind": np.array([2 if stereo else 1])})
            r0, r1 = PW.robust(ed, True, np.array([e], f64))
            assert out.tobytes() == np.array([r0[0], r1[0]], f64).tobytes()
            if e <= delta * delta:
                assert out[0] == e and out[1] == 1.0
            elif np.isfinite(e):
                assert abs(out[0] - (2 * np.sqrt(e) * delta - delta * delta)) <= 4 * UNIT * out[0] and abs(out[1] - delta / np.sqrt(e)) <= 4 * UNIT
            host.po_huber(stereo, 0, e, ptr(out))
            assert out[0] == e and out[1] == 1.0


def _closed_exp(x):
    w, u = np.asarray(x[:3], f64), np.asarray(x[3:], f64)
    th = np.linalg.norm(w)
    Om = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    R = np.eye(3) + np.sin(th) / th * Om + (1 - np.cos(th)) / th ** 2 * Om @ Om
    V = np.eye(3) + (1 - np.cos(th)) / th ** 2 * Om + (th - np.sin(th)) / th ** 3 * Om @ Om
    return R, V @ u


def test_exp_in_both_branches(host):
    out = np.zeros(7, f64)
    rng = np.random.default_rng(3)
    for scale in (0.3, 1e-3, 2e-5, 0.9e-5 / np.sqrt(3), 1e-9, 0.0):
        x = np.concatenate([rng.uniform(-1, 1, 3) * scale, rng.uniform(-1, 1, 3)])
        host.po_exp(ptr(x), ptr(out))
        q, t = PW.se3_exp(x)
        assert out.tobytes() == np.array(list(q) + list(t), f64).tobytes()
        R = np.array(PW.rot_matrix(list(out[:4])), f64).reshape(3, 3)
        if np.linalg.norm(x[:3]) >= 1e-5:
            Rc, tc = _closed_exp(x)
            assert np.abs(R - Rc).max() < 1e-14 and np.abs(out[4:] - tc).max() < 1e-14
        else:                                                   # R = I + Omega + Omega^2 (NOT half the square), V = R
            w = x[:3]
            Om = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
            assert np.abs(out[4:] - (np.eye(3) + Om + Om @ Om) @ x[3:]).max() < 1e-15 and abs(np.linalg.norm(out[:4]) - 1) < 1e-15
            assert np.abs(R - (np.eye(3) + Om)).max() < 1e-9


def test_the_quaternion_of_a_matrix_and_back(host):
    q, back = np.zeros(4, f64), np.zeros(9, f64)
    branches = set()
    for angles in ((0.1, 0.2, -0.3), (3.0, 0.1, 0.1), (0.1, 3.0, 0.1), (0.1, 0.1, 3.0), (3.1, 0.0, 3.1), (2.0, 2.5, -2.2)):
        R = np.ascontiguousarray(SC.rotation(*angles), f64)
        host.po_quat(ptr(R), ptr(q), ptr(back))
        want = PW.normalize(PW.quat_from_matrix(R))
        assert q.tobytes() == np.array(want, f64).tobytes() and q[3] >= 0
        assert np.abs(back.reshape(3, 3) - R).max() < 1e-14
        branches.add("trace" if np.trace(R) > 0 else int(np.argmax(np.diag(R))))
    assert branches == {"trace", 0, 1, 2}


def test_the_6x6_solve_against_numpy(host):
    rng = np.random.default_rng(4)
    for trial in range(20):
        J = rng.normal(0, 1, (40, 6)) * rng.uniform(0.1, 100, 6)
        H = J.T @ J
        b = rng.normal(0, 10, 6)
        lam = 1e-5 * np.abs(np.diag(H)).max()
        Hu = np.array([H[r, c] for r, c in PW.UPPER], f64)
        x = np.zeros(6, f64)
        assert host.po_solve6(ptr(Hu), lam, ptr(b), ptr(x)) == 1
        ok, xw = PW.solve6(list(Hu), f64(lam), list(b), [f64(0)] * 6)
        assert ok and x.tobytes() == np.array(xw, f64).tobytes()
        A = H + lam * np.eye(6)
        ref = np.linalg.solve(A, b)
        assert np.abs(x - ref).max() <= 64 * UNIT * np.linalg.cond(A) * np.abs(ref).max()      # a backward-stable solve's forward error
    # not positive definite, and a NaN: the solve fails and x is untouched
    x = np.full(6, 7.0, f64)
    Hu = np.array([(-1.0 if r == c == 2 else float(r == c)) for r, c in PW.UPPER], f64)
    assert host.po_solve6(ptr(Hu), 0.0, ptr(np.ones(6)), ptr(x)) == 0 and (x == 7.0).all()
    Hu[0] = np.nan
    assert host.po_solve6(ptr(Hu), 0.0, ptr(np.ones(6)), ptr(x)) == 0 and (x == 7.0).all() and not PW.solve6(list(Hu), f64(0), [f64(1)] * 6, list(x))[0]


@pytest.mark.parametrize("model, cam", [(0, SC.PINHOLE), (1, SC.KB8_L), (1, SC.KB8_R)])
def test_project_jac_is_the_derivative_of_project(host, model, cam):
    cam32 = np.array(cam, f32)
    rng = np.random.default_rng(6)
    uv, J = np.zeros(2, f64), np.zeros(6, f64)
    for trial in range(30):
        X = np.array([rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(2, 12)], f64)
        host.po_project(model, ptr(cam32), ptr(X), ptr(uv))
        host.po_project_jac(model, ptr(cam32), ptr(X), ptr(J))
        cols = [np.array([X[0]]), np.array([X[1]]), np.array([X[2]])]
        assert uv.tobytes() == np.array([v[0] for v in PW.project(model, cam32, cols)], f64).tobytes()
        assert J.tobytes() == np.array([np.asarray(v).reshape(-1)[0] for v in PW.project_jac(model, cam32, cols)], f64).tobytes()
        # KannalaBrandt8::project takes atan2f of floats: its value carries a float's rounding (6e-8 * 300 px), so the step is wide and the
        # difference is taken of the float64 camera of the scenes, whose agreement with project is asserted first
        assert np.abs(uv - SC.project64(model, np.array(cam32, f64), X[None])[0]).max() < (1e-9 if not model else 2e-4)
        h = 1e-5
        for c in range(3):
            d = np.zeros(3)
            d[c] = h
            num = (SC.project64(model, np.array(cam32, f64), (X + d)[None])[0] - SC.project64(model, np.array(cam32, f64), (X - d)[None])[0]) / (2 * h)
            assert np.abs(num - J[[c, 3 + c]]).max() < 1e-5 * max(1.0, np.abs(J).max())


def test_the_order_of_the_sums_is_the_declared_one(host):
    rng = np.random.default_rng(8)
    for n in (1, 2, 255, 256, 257, 300, 513, 1000):
        terms = (rng.normal(0, 1, n) * 10.0 ** rng.uniform(-8, 8, n)).astype(f64)
        slots = [0.0] * 256
        for k in range(n):                                        # slot k % 256, ascending k, onto 0.0
            slots[k % 256] = slots[k % 256] + float(terms[k])
        stride = 1
        while stride < 256:                                       # level by level v[s] = v[s] + v[s ^ stride]
            slots = [slots[s] + slots[s ^ stride] for s in range(256)]
            stride *= 2
        got = host.po_sum(ptr(terms), n)
        assert f64(got).tobytes() == f64(slots[0]).tobytes() == PW.slot_sum(terms[:, None], np.ones(n, bool))[0].tobytes()
        assert len(set(slots)) == 1                               # every lane of the tree ends with the same bits
    # an order, not an exact sum: (1 + 1e-17) + (-1 + 0) in the tree's first two levels loses what a sequential sum of this list keeps
    assert host.po_sum(ptr(np.array([1.0, 1e-17, -1.0, 0.0, 1e-17])), 5) == 1e-17 and ((1.0 + 1e-17) + -1.0) + 1e-17 == 1e-17
    assert host.po_sum(ptr(np.array([1.0, -1.0, 1e-17])), 3) == 1e-17 and host.po_sum(ptr(np.array([1.0, 1e-17, -1.0])), 3) == 0.0


# ---- (d) ------------------------------------------------------------------------------------------------------------------------------
# (case of pose_optimization_scenes.CASES, problem): Pinhole mono, mono + stereo, KannalaBrandt8 mono, a rig, rounds without an active edge
MARGIN_SEEDS = (("mono_batch17", 11), ("mixed_stereo_first2_step3", 0), ("mixed_stereo_first2_step3", 2), ("kb8_mono_batch3", 0),
                ("kb8_mono_batch3", 2), ("kb8_rig_batch3", 2))
# The two statements differ by roundings only.  A sum of n <= 300 terms in another order moves by at most n * 2^-53 * sum|terms|, 3.3e-14 of
# its size (the robust chi2 has no cancellation: its terms are positive); numpy's solve and the Cholesky differ by a few 2^-53 * cond(H +
# lambda I) in x, which moves a trial's chi2 only in second order near the optimum; libm and the header's sin / cos / atan2 by a few units.
#   MARGIN_SUMS  for a comparison BETWEEN such sums - rho's sign is that of currentChi - tempChi, Raul's stop compares (iniChi - currentChi)
#                * 1e3 with iniChi, whose left side carries 1e3 roundings of the sums: 3.3e-11 of iniChi.  1e-9 of the sums' size is thirty
#                times that, and four orders above a single sum's rounding;
#   MARGIN_CHI2  for an edge's chi2 against its threshold: the chi2 moves with the POSE, by |d chi2 / d pose| (up to 1e3 per radian or
#                metre on these scenes) times the poses' difference, which (3) below bounds by 1e-10: 1e-7 in chi2.  1e-6 of the
#                threshold (6e-6) is sixty times that.
# Most converged problems are NOT such seeds: g2o stops after three iterations that improve chi2 by less than a thousandth, and near the
# optimum the last of them often improve it by 1e-15 of its size - the sign of that rho is rounding noise in ANY statement (80 Pinhole seeds
# were searched: none is clear by 1e-9).  The list holds the problems of CASES whose every decision is clear.
MARGIN_SUMS, MARGIN_CHI2 = 1e-9, 1e-6


def g2o_order(pb, **kw):
    return PW.solve(pb, math=PW.LIBM_MATH, order="sequential", solver="numpy", **kw)


@pytest.mark.parametrize("name, p", MARGIN_SEEDS)
def test_the_float64_statement_in_g2os_own_order(name, p):
    s = SC.case(name)
    walk = SC.case_expected(name)[0][p]
    seen = []
    w64 = g2o_order(SC.problem(s, p), observe=lambda kind, **v: seen.append((kind, v)))
    # 1. the margins, on that statement alone
    for kind, v in seen:
        if kind == "chi2":
            assert (np.abs(v["values"] - v["thresholds"]) > MARGIN_CHI2 * v["thresholds"]).all(), name
        elif kind == "rho":
            assert abs(v["current"] - v["temp"]) > MARGIN_SUMS * abs(v["current"]) and np.isfinite(v["value"]), (name, v)
        else:
            assert abs(v["lhs"] - v["rhs"]) > MARGIN_SUMS * abs(v["rhs"]), (name, v)
    # 2. the same decisions
    assert w64["status"] == walk["status"] and w64["its"] == walk["its"] and w64["trials"] == walk["trials"] and w64["n_bad"] == walk["n_bad"]
    assert w64["n_initial"] == walk["n_initial"] and w64["empty_rounds"] == walk["empty_rounds"]
    for a, b in zip(w64["trace"], walk["trace"]):
        assert np.array_equal(a["flags"], b["flags"]) and a["terminate"] == b["terminate"]
    # 3. the pose, within a bound derived here: every sum of the float64 statement is moved by eps * sum|terms|, each of the 28 (and the
    #    trial's one) on its own and in every pass, and the pose's moves are added up - first order, the worst signs.  A sum's rounding is at
    #    most n * 2^-53 * sum|terms| in ANY order; the solve's backward error is that of 36 more such units on H and b.  The quaternion
    #    chain (exp, product, normalisation, ten iterations) adds its own roundings directly.
    n = w64["n_initial"]
    eps = 2.0 ** -40                                             # small enough to stay on the statement's path, 1e4 roundings large
    base = np.concatenate([np.array(w64["T"][0], f64), np.array(w64["T"][1], f64)])
    move = np.zeros(7)
    for j in range(PW.SUMS):
        def perturb(sums, terms, active, j=j):
            if terms.shape[1] == 1 and j != 0:
                return sums
            out = sums.copy()
            out[j if terms.shape[1] > 1 else 0] += eps * np.abs(terms[active][:, j if terms.shape[1] > 1 else 0]).sum()
            return out
        wp = g2o_order(SC.problem(s, p), perturb=perturb)
        assert wp["its"] == w64["its"] and wp["trials"] == w64["trials"], (name, j)      # the same path: the move is the derivative's
        move += np.abs(np.concatenate([np.array(wp["T"][0], f64), np.array(wp["T"][1], f64)]) - base)
    bound = move / eps * ((n + 36) * 2 * UNIT) + 64 * 2 * UNIT * (1 + np.abs(base))
    mine = np.concatenate([np.array(walk["T"][0], f64), np.array(walk["T"][1], f64)])
    diff = np.abs(mine - base)
    used = float((diff / bound).max())
    print("%s %d: |dq| %.3g, |dt| %.3g, bound q %.3g t %.3g, %.2f %% of the bound used" % (name, p, diff[:4].max(), diff[4:].max(), bound[:4].max(), bound[4:].max(), 100 * used))
    assert (diff <= bound).all()
    assert np.abs(walk["pose"].astype(f64) - w64["pose"].astype(f64)).max() <= 2.0 ** -22      # and so the float poses, to a float's last places


# ---- (f) ------------------------------------------------------------------------------------------------------------------------------
def test_the_sanitizer_program(tmp_path):
    exe = str(tmp_path / "pose_optimization_host_check")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DPOSE_OPTIMIZATION_HOST_MAIN",
                           *HOST_FLAGS, SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "every access inside its arrays" in out.stdout and "ERROR" not in out.stderr, out.stdout + out.stderr
