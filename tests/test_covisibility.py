"""KeyFrame::UpdateConnections, the vote of Tracking::UpdateLocalKeyFrames and the redundancy test of LocalMapping::KeyFrameCulling without a
GPU: extractorb_amd/csrc/k_covisibility.hpp - the statement of k_covisibility.hip - compiled for the host
(tests/cpp/covisibility_host_check.cpp: cvRank frame by frame, cvVote and rdKeyFrame subject by subject) against the walk
(tests/covisibility_walk.py: KeyFrame and MapPoint objects, std::map in address order, the vector of pairs, sort and push_front) on the scenes
of tests/covisibility_scenes.py, byte for byte: list rows, result rows, the poison beyond the counts, the slot states.
  (a) every scene of covisibility_scenes.CASES;
  (b) the mutants of the walk: for each a NAMED scene whose output it changes, or the reason why none can;
  (c) the crafted scenes, each asserted - on the HEADER's output - to reach what it was made for;
  (d) the sizes, both sides of the entries' bounds, the entries' rejections (orbx_entry.hpp) for every required pointer and range;
  (e) the header's declarations against the Python mirror; (f) the stand-alone sanitizer program."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import extractorb_amd as X
import covisibility_scenes as SC
import covisibility_walk as CW
from test_kb8_math import HOST_FLAGS, ROOT

f32 = np.float32
VP = C.c_void_p
SRC = os.path.join(ROOT, "tests", "cpp", "covisibility_host_check.cpp")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("cvhost")), "libcovisibility_host.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", *HOST_FLAGS, SRC, "-o", so])
    L = C.CDLL(so)
    L.cv_host.argtypes = [C.c_int, C.c_int, VP, VP, VP, C.c_int, VP, VP, VP, C.c_int, VP, VP, C.c_int, VP, VP, C.c_int, C.c_int, VP, VP, VP, VP, VP]
    L.cv_host.restype = None
    L.rd_host.argtypes = [C.c_int, VP, VP, VP, VP, C.c_int, VP, VP, VP, VP, VP, C.c_int, VP, VP, C.c_int, VP, C.c_int, C.c_int, C.c_float, VP, VP]
    L.rd_host.restype = None
    L.cv_bad_argument.argtypes = [VP] + [C.c_int] * 6
    L.rd_bad_argument.argtypes = [VP] + [C.c_int] * 5 + [C.c_float]
    L.cv_unsupported.argtypes = L.rd_unsupported.argtypes = L.cv_vote_lds_bytes.argtypes = L.rd_lds_bytes.argtypes = [C.c_int]
    L.cv_vote_lds_bytes.restype = L.rd_lds_bytes.restype = C.c_long
    return L


def ptr(a):
    return None if a is None else a.ctypes.data_as(VP)


def run_host(L, s, slot_state=True):
    o = SC.poisoned_outputs(s)
    if s["kind"] == "vote":
        L.cv_host(s["mode"], s["n_points"], ptr(s["obs_off"]), ptr(s["obs"]), ptr(s["mp_flags"]), s["n_frames"], ptr(s["kf_flags"]), ptr(s["kf_map"]),
                  ptr(s["kf_key"]), s["n_subjects"], ptr(s["subject_mp"]), ptr(s["subject_n"]), s["capacity"], ptr(s["subject_kf"]),
                  ptr(s["subject_map"]), s["th"], s["conn_capacity"], ptr(o["counter_kf"]), ptr(o["counter_w"]), ptr(o["ordered_kf"]),
                  ptr(o["ordered_w"]), ptr(o["result"]))
    else:
        L.rd_host(s["n_points"], ptr(s["obs_off"]), ptr(s["obs"]), ptr(s["mp_flags"]), ptr(s["mp_nobs"]), s["n_frames"], ptr(s["kf_flags"]),
                  ptr(s["kps_un"]), ptr(s["n_out"]), ptr(s["depth"]), ptr(s["th_depth"]), s["n_subjects"], ptr(s["subject_mp"]), ptr(s["subject_n"]),
                  s["capacity"], ptr(s["subject_kf"]), int(s["monocular"]), s["th_obs"], float(s["redundant_th"]), ptr(o["result"]),
                  ptr(o["slot_state"]) if slot_state else None)
    return o


# ---- (a) ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SC.CASES))
def test_the_header_equals_the_walk_byte_for_byte(host, name):
    s, want = SC.case(name), SC.case_expected(name)
    got = run_host(host, s)
    assert SC.differences(got, want) == [], name
    r = want["result"]
    # what "byte for byte" covers: the poison beyond the counts, and everything of a subject that was refused
    for j in range(s["n_subjects"]):
        if s["kind"] == "vote":
            assert (got["counter_kf"][j, r["n_counter"][j]:] == SC.POISON).all() and (got["counter_w"][j, r["n_counter"][j]:] == SC.POISON).all()
            assert (got["ordered_kf"][j, r["n_ordered"][j]:] == SC.POISON).all() and (got["ordered_w"][j, r["n_ordered"][j]:] == SC.POISON).all()
        else:
            n = min(max(int(s["subject_n"][j]), 0), s["capacity"]) if r["status"][j] == CW.RD_OK else 0
            assert (got["slot_state"][j, n:] == 0xEE).all() and (got["slot_state"][j, :n] <= 2).all()
    if s["kind"] == "redundancy":                             # d_slot_state is optional
        without = run_host(host, s, slot_state=False)
        assert (without["slot_state"] == 0xEE).all() and without["result"].tobytes() == want["result"].tobytes()


# ---- (b) ------------------------------------------------------------------------------------------------------------------------------
KILLED_BY = {
    "frame_order": "update_none_reach_th_tie",
    "ties_key_ascending": "update_three_equal_weights",
    "th_gt": "update_th_14_15_16",
    "nmax_ge": "update_none_reach_th_tie",
    "no_self_test": "update_other_map_and_self",
    "map_test_in_frame_mode": "local_other_map_and_self",
    "self_test_in_frame_mode": "local_other_map_and_self",
    "bad_listed_in_frame_mode": "local_bad_observer",
    "bad_counted_in_update": "update_bad_observer",
    "other_map_counted": "update_other_map_and_self",
    "bad_map_point_votes": "update_bad_map_point",
    "slots_once": "update_point_in_two_slots",
    "single_pair_dropped": "update_none_reach_th_tie",
    "list_length_for_observations": "redundancy_observations_3_and_4",
    "observations_ge": "redundancy_observations_3_and_4",
    "octave_lt": "redundancy_octave_edges",
    "octave_plus_two": "redundancy_octave_edges",
    "subject_counts_itself": "redundancy_subject_one_of_four",
    "slot_ge": "redundancy_octave_edges",
    "bad_observers_skipped_in_culling": "redundancy_subject_one_of_four",
    "final_ge": "redundancy_10_9",
    "product_double": "redundancy_10_9",
    "depth_ge": "redundancy_depth_edges",
    "depth_le_zero": "redundancy_depth_edges",
    "nan_depth_skipped": "redundancy_depth_edges",
}
EQUIVALENT = {
    "bad_excluded_from_frame_count": "UpdateLocalKeyFrames reads a bad keyframe's counter at one place, :3091, where it is skipped: it is not listed "
                                     "and cannot be pKFmax, whatever its count.  Whether it was counted shows nowhere in mvpLocalKeyFrames, max or pKFmax",
}


def test_every_mutant_is_killed_or_declared_equivalent():
    assert set(KILLED_BY) | set(EQUIVALENT) == set(CW.MUTANTS) and not set(KILLED_BY) & set(EQUIVALENT) and len(CW.MUTANTS) >= 12
    assert set(KILLED_BY.values()) <= set(SC.CASES)
    expected = {"frame_order", "ties_key_ascending", "th_gt", "nmax_ge", "no_self_test", "map_test_in_frame_mode", "bad_excluded_from_frame_count",
                "list_length_for_observations", "octave_lt", "final_ge", "product_double"}
    assert expected <= set(CW.MUTANTS)


@pytest.mark.parametrize("mutant", list(KILLED_BY))
def test_a_mutant_of_the_walk_changes_its_scene(mutant):
    name = KILLED_BY[mutant]
    assert SC.differences(CW.walk_scene(SC.case(name), mutant), SC.case_expected(name)) != [], (mutant, name)


@pytest.mark.parametrize("mutant", list(EQUIVALENT))
def test_an_equivalent_mutant_changes_no_scene(mutant):
    for name in SC.CASES:
        assert SC.differences(CW.walk_scene(SC.case(name), mutant), SC.case_expected(name)) == [], (mutant, name)


# ---- (c) ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def header(host):
    """the HEADER's outputs on a named scene, not the walk's: every rule below is asserted on the code and not only on its second statement"""
    cache = {}

    def run(name):
        if name not in cache:
            cache[name] = run_host(host, SC.case(name))
        return cache[name], cache[name]["result"]
    return run


def row(r, j=0):
    return tuple(int(v) for v in r[j])


def test_counts_of_14_15_and_16(header):
    o, r = header("update_th_14_15_16")
    assert row(r) == (CW.OK, 3, 2, 16, 3)
    assert o["counter_kf"][0, :3].tolist() == [3, 2, 1] and o["counter_w"][0, :3].tolist() == [16, 15, 14]      # key ascending: the frames' order reversed
    assert o["ordered_kf"][0, :2].tolist() == [3, 2] and o["ordered_w"][0, :2].tolist() == [16, 15]


def test_no_count_reaches_th_and_the_first_in_key_order_wins_the_tie(header):
    o, r = header("update_none_reach_th_tie")
    s = SC.case("update_none_reach_th_tie")
    assert s["kf_key"][2] < s["kf_key"][1]
    assert row(r) == (CW.OK, 3, 1, 5, 2) and o["ordered_kf"][0, 0] == 2 and o["ordered_w"][0, 0] == 5
    assert o["counter_kf"][0, :3].tolist() == [3, 2, 1] and o["counter_w"][0, :3].tolist() == [3, 5, 5]


def test_equal_weights_stand_in_descending_key_order(header):
    o, r = header("update_three_equal_weights")
    # keys: frame 1 30, frame 3 10, frame 5 20 hold weight 20: 1 (30), 5 (20), 3 (10)
    assert row(r) == (CW.OK, 6, 5, 25, 2) and o["ordered_kf"][0, :5].tolist() == [2, 1, 5, 3, 4] and o["ordered_w"][0, :5].tolist() == [25, 20, 20, 20, 16]
    assert o["counter_kf"][0, :6].tolist() == [3, 5, 1, 6, 4, 2]


def test_an_empty_counter_writes_nothing(header):
    o, r = header("update_empty_counter")
    assert row(r, 0) == (CW.EMPTY, 0, 0, 0, -1) and row(r, 1) == (CW.OK, 1, 1, 3, 1)
    assert all((o[k][0] == SC.POISON).all() for k in ("counter_kf", "counter_w", "ordered_kf", "ordered_w"))


def test_slots_bad_map_points_and_observers(header):
    o, r = header("update_point_in_two_slots")
    assert o["counter_w"][0, :2].tolist() == [4, 3] and o["counter_kf"][0, :2].tolist() == [2, 1]           # MapPoint 0 votes three times
    o, r = header("update_bad_map_point")
    assert o["counter_w"][0, :2].tolist() == [1, 1] and row(r)[1] == 2
    o, r = header("update_bad_observer")
    assert row(r) == (CW.OK, 2, 1, 16, 1) and o["counter_kf"][0, :2].tolist() == [3, 1]                    # frame 2, bad, holds 18: skipped
    o, r = header("local_bad_observer")
    assert row(r) == (CW.OK, 2, 0, 16, 1) and o["counter_kf"][0, :2].tolist() == [3, 1] and o["counter_w"][0, :2].tolist() == [4, 16]
    assert (o["ordered_kf"] == SC.POISON).all()
    o, r = header("update_other_map_and_self")
    assert row(r) == (CW.OK, 2, 1, 16, 1) and o["counter_kf"][0, :2].tolist() == [2, 1]
    o, r = header("local_other_map_and_self")
    assert row(r) == (CW.OK, 4, 0, 17, 3) and o["counter_kf"][0, :4].tolist() == [3, 2, 1, 0] and o["counter_w"][0, :4].tolist() == [17, 2, 16, 17]


def test_a_short_capacity_truncates_and_says_the_true_counts(header):
    full, r = header("update_conn_capacity_exact")
    assert row(r) == (CW.OK, 5, 4, 20, 1)
    o, r = header("update_conn_capacity_one_short")
    assert row(r) == (CW.TRUNCATED, 5, 4, 20, 1)
    assert o["counter_kf"][0].tolist() == full["counter_kf"][0, :4].tolist() and o["ordered_kf"][0].tolist() == full["ordered_kf"][0, :4].tolist()
    o, r = header("update_conn_capacity_ordered_fits")
    assert row(r) == (CW.TRUNCATED, 5, 2, 20, 1) and (o["ordered_kf"][0, 2:] == SC.POISON).all()
    assert row(header("update_conn_capacity_0")[1]) == (CW.TRUNCATED, 5, 4, 20, 1)


def test_duplicate_keys_and_bad_indices_have_names(header):
    o, r = header("update_duplicate_keys")
    assert r["status"].tolist() == [CW.DUPLICATE_KEY] * 2 and (o["counter_kf"] == SC.POISON).all()
    for kind in SC.VOTE_BAD:
        o, r = header("update_bad_" + kind)
        assert r["status"].tolist() == [CW.BAD_INDEX, CW.OK], kind
        assert (o["counter_kf"][0] == SC.POISON).all() and (o["ordered_w"][0] == SC.POISON).all() and o["counter_w"][1, :2].tolist() == [2, 14]
    assert header("update_bad_map_point_unchecked")[1]["status"].tolist() == [CW.OK, CW.OK]
    assert header("local_bad_frame_high")[1]["status"].tolist() == [CW.BAD_INDEX, CW.OK]
    assert header("local_subject_kf_ignored")[1]["status"].tolist() == [CW.OK, CW.OK]
    for kind in SC.REDUNDANCY_BAD:
        o, r = header("redundancy_bad_" + kind)
        assert r["status"].tolist() == [CW.RD_BAD_INDEX, CW.RD_OK], kind
        assert (o["slot_state"][0] == 0xEE).all() and o["slot_state"][1].tolist() == [2, 0, 1]
    o, r = header("redundancy_not_examined_unchecked")
    assert r["status"].tolist() == [CW.RD_OK, CW.RD_OK] and o["slot_state"][0].tolist() == [1, 2, 1]


def test_observations_octaves_and_the_subject_itself(header):
    o, r = header("redundancy_observations_3_and_4")
    assert row(r) == (CW.RD_OK, 3, 1, 0) and o["slot_state"][0, :3].tolist() == [1, 2, 1]
    o, r = header("redundancy_octave_edges")
    assert row(r) == (CW.RD_OK, 2, 1, 0) and o["slot_state"][0, :2].tolist() == [2, 1]
    o, r = header("redundancy_subject_one_of_four")
    assert row(r) == (CW.RD_OK, 2, 1, 0) and o["slot_state"][0].tolist() == [1, 2]              # three others; four others, a bad one among them


def test_the_depth_test_is_the_one_written(header):
    o, r = header("redundancy_depth_edges")
    # th, just above, -0.0, negative, NaN, 0, just below
    assert o["slot_state"][0].tolist() == [2, 0, 2, 0, 2, 2, 2] and row(r) == (CW.RD_OK, 5, 5, 1)


def test_the_share_is_one_float_product(header):
    assert f32(0.9) * f32(10) == f32(9) and float(f32(0.9)) * 10 < 9
    assert row(header("redundancy_10_9")[1]) == (CW.RD_OK, 10, 9, 0)
    assert row(header("redundancy_10_10")[1]) == (CW.RD_OK, 10, 10, 1)
    assert row(header("redundancy_half_7_4")[1]) == (CW.RD_OK, 7, 4, 1) and row(header("redundancy_half_7_3")[1]) == (CW.RD_OK, 7, 3, 0)
    assert row(header("redundancy_no_map_points")[1]) == (CW.RD_OK, 0, 0, 0)
    o, r = header("redundancy_initial_and_bad")
    assert r["status"].tolist() == [CW.RD_SKIPPED, CW.RD_SKIPPED, CW.RD_OK, CW.RD_SKIPPED] and row(r, 2) == (CW.RD_OK, 1, 1, 1)
    assert (o["slot_state"][[0, 1, 3]] == 0xEE).all()


# ---- (d) ------------------------------------------------------------------------------------------------------------------------------
def test_the_cases_cover_the_sizes(host, header):
    for tag in ("update", "local", "redundancy"):
        mine = [SC.case(n) for n in SC.CASES if n.startswith(tag + "_frames")]
        assert {s["n_frames"] for s in mine} >= {1, 2, 63, 64, 65, 257} and {s["n_subjects"] for s in mine} >= {1, 3, 17}
        assert {int(n) for s in mine for n in s["subject_n"]} >= {0, 1, 63, 64, 65, 300}
        lens = {int(n) for s in mine for n in np.diff(s["obs_off"])}
        assert lens >= {0, 1, 4, 5, 64, 65, 3000}, tag
    assert SC.case("update_frames%d" % SC.MAX_FRAMES)["n_frames"] == SC.MAX_FRAMES == SC.case("local_frames%d" % SC.MAX_FRAMES)["n_frames"]
    # key order opposite to the frame order, and a permutation; lists longer than a workgroup, with counts on both sides of th
    assert (np.diff(SC.case("update_frames64_n64")["kf_key"].astype(np.float64)) < 0).all()
    keys = SC.case("update_frames257_n300_x17")["kf_key"]
    assert (keys >> np.uint64(63)).any() and not (keys >> np.uint64(63)).all() and len(set(np.sign(np.diff(keys.astype(np.float64))))) == 2
    r = header("update_frames257_n300_x17")[1]
    assert (r["n_ordered"] > 64).sum() >= 12 and (r["n_ordered"] < r["n_counter"]).sum() >= 12 and (r["status"] == CW.OK).all()      # (every fifth subject lives in the small map)
    r = header("update_frames%d" % SC.MAX_FRAMES)[1]
    assert (r["n_counter"] > 4096).all() and (r["n_ordered"] > 2048).all() and (r["n_ordered"] < r["n_counter"]).all()
    assert (header("update_frames257_short")[1]["status"] == CW.TRUNCATED).all()
    # both sides of the launch-time bounds
    budget = 160 * 1024 - 512
    assert host.cv_max_frames() == SC.MAX_FRAMES and host.rd_max_capacity() == SC.MAX_CAPACITY
    assert host.cv_vote_lds_bytes(SC.MAX_FRAMES) == 12 * SC.MAX_FRAMES + 48 <= budget < host.cv_vote_lds_bytes(SC.MAX_FRAMES + 1)
    assert host.rd_lds_bytes(SC.MAX_CAPACITY) == SC.MAX_CAPACITY + 48 == budget < host.rd_lds_bytes(SC.MAX_CAPACITY + 1)
    assert host.cv_unsupported(SC.MAX_FRAMES) == 0 and host.cv_unsupported(SC.MAX_FRAMES + 1) == 1 and host.cv_unsupported(2 ** 31 - 1) == 1
    assert host.rd_unsupported(SC.MAX_CAPACITY) == 0 and host.rd_unsupported(SC.MAX_CAPACITY + 1) == 1 and host.rd_unsupported(2 ** 31 - 1) == 1


VOTE_POINTERS = ("d_obs_off", "d_obs", "d_mp_flags", "d_kf_flags", "d_kf_map_id", "d_kf_key", "d_subject_mp", "d_subject_n", "d_subject_kf",
                 "d_subject_map_id", "d_counter_kf", "d_counter_w", "d_ordered_kf", "d_ordered_w", "d_result")
REDUNDANCY_POINTERS = ("d_obs_off", "d_obs", "d_mp_flags", "d_kf_flags", "d_kps_un", "d_n_out", "d_depth", "d_th_depth", "d_subject_mp", "d_subject_n",
                       "d_subject_kf", "d_result")


def pointers(names, null=()):
    return (VP * len(names))(*[None if n in null else 4096 for n in names])


def test_the_votes_rejections(host):
    ok = dict(mode=0, n_points=90, n_frames=37, n_subjects=5, capacity=41, conn_capacity=37)
    bad = lambda null=(), **kw: host.cv_bad_argument(pointers(VOTE_POINTERS, null), *[dict(ok, **kw)[k] for k in ok])
    assert bad() == 0 and bad(mode=1) == 0 and bad(n_points=0) == 0 and bad(conn_capacity=0) == 0 and bad(n_subjects=65535) == 0
    local_only = {"d_kf_map_id", "d_subject_kf", "d_subject_map_id", "d_ordered_kf", "d_ordered_w"}
    lists = {"d_counter_kf", "d_counter_w", "d_ordered_kf", "d_ordered_w"}
    for name in VOTE_POINTERS:
        assert bad(null=[name]) == 1, name
        assert bad(null=[name], mode=1) == (0 if name in local_only else 1), name
        assert bad(null=[name], conn_capacity=0) == (0 if name in lists else 1), name
    for kw in (dict(mode=2), dict(mode=-1), dict(n_points=-1), dict(n_frames=0), dict(n_subjects=0), dict(n_subjects=65536), dict(capacity=0),
               dict(conn_capacity=-1), dict(n_subjects=65535, capacity=32769), dict(n_subjects=65535, conn_capacity=32769)):
        assert bad(**kw) == 1, kw


def test_the_redundancy_tests_rejections(host):
    ok = dict(n_points=90, n_frames=37, n_subjects=5, capacity=41, monocular=0)
    bad = lambda null=(), th=0.9, **kw: host.rd_bad_argument(pointers(REDUNDANCY_POINTERS, null), *[dict(ok, **kw)[k] for k in ok], th)
    assert bad() == 0 and bad(monocular=1) == 0 and bad(n_points=0) == 0 and bad(th=0.5) == 0 and bad(th=float("inf")) == 0
    for name in REDUNDANCY_POINTERS:
        assert bad(null=[name]) == 1, name
        assert bad(null=[name], monocular=1) == (0 if name in ("d_depth", "d_th_depth") else 1), name
    for kw in (dict(n_points=-1), dict(n_frames=0), dict(n_subjects=0), dict(n_subjects=65536), dict(capacity=0), dict(th=float("nan")),
               dict(n_subjects=65535, capacity=32769)):
        assert bad(**kw) == 1, kw


# ---- (e) ------------------------------------------------------------------------------------------------------------------------------
def struct_fields(header, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, re.S).group(1)
    return [n for _, n in re.findall(r"^\s*(int32_t|float) (\w+);", body, re.M)]


def test_the_rows_and_names_are_the_headers(host):
    assert host.cv_result_bytes() == CW.RESULT_DTYPE.itemsize == X.COVIS_RESULT_DTYPE.itemsize == 20 and CW.RESULT_DTYPE == X.COVIS_RESULT_DTYPE
    assert host.rd_result_bytes() == CW.REDUNDANCY_DTYPE.itemsize == X.REDUNDANCY_RESULT_DTYPE.itemsize == 16 and CW.REDUNDANCY_DTYPE == X.REDUNDANCY_RESULT_DTYPE
    assert CW.KEYPOINT_DTYPE == X.KEYPOINT_DTYPE
    header = open(os.path.join(ROOT, "include", "orbx.h")).read()
    assert struct_fields(header, "orbx_covis_result") == list(X.COVIS_RESULT_DTYPE.names)
    assert struct_fields(header, "orbx_redundancy_result") == list(X.REDUNDANCY_RESULT_DTYPE.names)
    names = re.findall(r"ORBX_COVIS_(\w+) = (\d+)", header)
    assert [n for n, _ in names] == ["UPDATE_CONNECTIONS", "LOCAL_KEYFRAMES"] + list(CW.STATUS) and list(X.COVIS_STATUS) == list(CW.STATUS)
    assert [int(v) for _, v in names] == [0, 1] + list(range(len(CW.STATUS))) and host.cv_statuses() == len(CW.STATUS)
    names = re.findall(r"ORBX_REDUNDANCY_(\w+) = (\d+)", header)
    assert [n for n, _ in names] == list(CW.REDUNDANCY_STATUS) == list(X.REDUNDANCY_STATUS) and [int(v) for _, v in names] == [0, 1, 2]
    assert host.rd_statuses() == 3 and (X.COVIS_UPDATE_CONNECTIONS, X.COVIS_LOCAL_KEYFRAMES) == (CW.UPDATE_CONNECTIONS, CW.LOCAL_KEYFRAMES) == (0, 1)
    symbols = X.header_symbols()
    assert {"orbx_covisibility_device", "orbx_keyframe_redundancy_device", "orbx_debug_covisibility_launches"} <= set(symbols)
    L = X.load_library()
    assert len(L.orbx_covisibility_device.argtypes) == 23 and len(L.orbx_keyframe_redundancy_device.argtypes) == 22
    assert L.orbx_debug_covisibility_launches(3) == -2 and L.orbx_debug_covisibility_launches(-1) == -2 and L.orbx_debug_covisibility_launches(0) >= 0
    assert "n_frames <= 8192" in header and "capacity <= 163280" in header          # the bounds of the declarations' comments


# ---- (f) ------------------------------------------------------------------------------------------------------------------------------
def test_the_standalone_program_is_clean_under_sanitizers(tmp_path):
    exe = str(tmp_path / "covisibility_host_check")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *HOST_FLAGS,
                           "-DCOVISIBILITY_HOST_MAIN", SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "every access inside its arrays" in out.stdout and "FAILED" not in out.stdout
