"""KeyFrameDatabase::DetectNBestCandidates / DetectRelocalizationCandidates without a GPU: extractorb_amd/csrc/k_place_recognition.hpp - the
statement of k_place_recognition.hip - compiled for the host (tests/cpp/place_recognition_host_check.cpp: prPair pair by pair, prQuery query
by query) against the walk (tests/place_recognition_walk.py: an inverted file, lists, a set, L1Scoring::score with its iterators) on the
scenes of tests/place_recognition_scenes.py, byte for byte: candidates, counts, result rows, the whole score row with its untouched entries,
the poison beyond the counts, and the shared-word counts.
  (a) every scene of place_recognition_scenes.CASES;
  (b) the mutants of the walk: for each a scene whose output it changes, or the reason why none can;
  (c) the crafted scenes, each asserted - on the HEADER's output - to reach what it was made for;
  (d) the sizes: n_db 1, 63, 64, 65, 257, rows of 0, 1, 63, 64, 65 and capacity words, 1 and 3 queries with q_first / q_step, lists longer than a
      workgroup, both sides of the entry's bounds (a database of 8192 rows, a query of 13610 words);
  (e) the walk's own pieces: add and erase, the order of first encounter, two queries chained through one score row;
  (f) the header's declarations against the Python mirror; (g) the stand-alone sanitizer program, the entry's rejections among its cases."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import extractorb_amd as X
import place_recognition_scenes as SC
import place_recognition_walk as PW
from test_kb8_math import HOST_FLAGS, ROOT

f32, f64 = np.float32, np.float64
VP = C.c_void_p
SRC = os.path.join(ROOT, "tests", "cpp", "place_recognition_host_check.cpp")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = os.path.join(str(tmp_path_factory.mktemp("prhost")), "libplace_recognition_host.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", *HOST_FLAGS, SRC, "-o", so])
    L = C.CDLL(so)
    L.pr_host.argtypes = [C.c_int, C.c_int, VP, VP, VP, C.c_int, VP, VP, VP, C.c_int, C.c_int, C.c_int, VP, VP, VP, C.c_int, VP, VP, C.c_int, VP, VP,
                          VP, VP, VP, C.c_int, VP]
    L.pr_host.restype = None
    L.pr_fits.argtypes = [C.c_int, C.c_int]
    L.pr_unsupported.argtypes = [C.c_int, C.c_int, C.c_int]
    L.pr_pair_lds_bytes.argtypes = L.pr_query_lds_bytes.argtypes = [C.c_int]
    L.pr_pair_lds_bytes.restype = L.pr_query_lds_bytes.restype = C.c_long
    return L


def ptr(a):
    return None if a is None else a.ctypes.data_as(VP)


def run_host(L, s, common_words=True):
    o = SC.poisoned_outputs(s)
    L.pr_host(s["mode"], s["n_db"], ptr(s["db_ids"]), ptr(s["db_w"]), ptr(s["db_n"]), s["capacity"], ptr(s["db_map"]), ptr(s["db_flags"]),
              ptr(s["db_covis"]), s["n_queries"], s["q_first"], s["q_step"], ptr(s["q_ids"]), ptr(s["q_w"]), ptr(s["q_n"]), s["q_capacity"],
              ptr(s["q_map"]), ptr(s["connected"]), s["n_candidates"], ptr(o["score"]), ptr(o["result"]), ptr(o["loop"]), ptr(o["merge"]),
              ptr(o["cand"]), s["cand_capacity"], ptr(o["common_words"]) if common_words else None)
    return o


# ---- (a) ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SC.CASES))
def test_the_header_equals_the_walk_byte_for_byte(host, name):
    s, want = SC.case(name), SC.case_expected(name)
    got = run_host(host, s)
    assert SC.differences(got, want) == [], name
    r = want["result"]
    # what "byte for byte" covers: the poison beyond the counts, the untouched part of the score row
    for q in range(s["n_queries"]):
        if s["mode"] == PW.N_BEST:
            assert (got["loop"][q, r["n_loop"][q]:] == SC.POISON).all() and (got["merge"][q, r["n_merge"][q]:] == SC.POISON).all()
            assert (got["cand"] == SC.POISON).all()
        else:
            assert (got["cand"][q, r["n_loop"][q]:] == SC.POISON).all() and (got["loop"] == SC.POISON).all() and (got["merge"] == SC.POISON).all()
        changed = got["score"][q].view(np.uint32) != s["score_in"][q].view(np.uint32)
        assert changed.sum() <= r["n_scored"][q]
    without = run_host(host, s, common_words=False)              # d_common_words is optional
    assert (without["common_words"] == SC.POISON).all() and SC.differences(dict(without, common_words=want["common_words"]), want) == []


# ---- (b) ------------------------------------------------------------------------------------------------------------------------------
KILLED_BY = {
    "tree_sum": "nbest_sum_last_bit",
    "float_sum": "nbest_db63_q3",
    "threshold_ge": "nbest_threshold_max5",
    "connected_in_maximum": "nbest_connected_rows",
    "connected_as_neighbours": "nbest_connected_rows",
    "stale_zero": "nbest_stale_best",
    "stale_fresh": "reloc_stale_best",
    "unstable_sort": "nbest_tie_list_order",
    "row_order": "reloc_tie_list_order",
    "reloc_sorted": "reloc_order",
    "retain_ge": "reloc_retain_boundary",
}
EQUIVALENT = {
    "point8_double": "maxCommonWords * 0.8 is an integer only for multiples of 5, where the float product rounds onto the same integer (0.8f is "
                     "1.5e-8 above 0.8 and a float near k has a spacing of 6e-8 k or more); elsewhere the fraction is at least 0.2",
    "point8_times4_over5": "the floor of 4 m / 5 is the truncation of 0.8 m for the same reason",
    "map_after_set": "a duplicate is the SAME keyframe and so of the same map: whether the map is tested in front of or behind the set, a "
                     "keyframe of another map is never pushed and one of the query's map is pushed at its first occurrence",
    "full_loop_list_skips_set": "the lists never shrink: a same-map keyframe met when the loop list is full would meet a full list again at "
                                "its next occurrence, in the set or not",
}


def test_every_mutant_is_killed_or_declared_equivalent():
    assert set(KILLED_BY) | set(EQUIVALENT) == set(PW.MUTANTS) and not set(KILLED_BY) & set(EQUIVALENT) and len(PW.MUTANTS) >= 12


@pytest.mark.parametrize("mutant", list(KILLED_BY))
def test_a_mutant_of_the_walk_changes_its_scene(mutant):
    name = KILLED_BY[mutant]
    assert SC.differences(PW.walk_scene(SC.case(name), mutant), SC.case_expected(name)) != [], (mutant, name)


@pytest.mark.parametrize("mutant", list(EQUIVALENT))
def test_an_equivalent_mutant_changes_no_scene(mutant):
    for name in SC.CASES:
        if SC.case(name)["n_db"] <= 700:
            assert SC.differences(PW.walk_scene(SC.case(name), mutant), SC.case_expected(name)) == [], (mutant, name)
    if mutant.startswith("point8"):
        assert all(PW.min_common_words(m, mutant) == PW.min_common_words(m) for m in range(0, 70000))


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


def test_equal_scores_are_decided_by_the_order_of_first_encounter(header):
    o, r = header("nbest_tie_list_order")
    assert r["n_scored"][0] == 4 and o["loop"][0].tolist() == [1]               # B, met at word 1, in front of A (row 0), met at word 10
    s = SC.case("nbest_tie_list_order")
    assert len(set(o["score"][0, [0, 1, 2, 5]].tolist())) == 1 and (s["db_ids"][2, :2] == s["db_ids"][5, :2]).all()
    o, r = header("reloc_tie_list_order")
    assert o["cand"][0, :4].tolist() == [1, 0, 2, 5] and r["n_loop"][0] == 4   # not the row order; identical rows in row order
    o, r = header("reloc_order")
    assert o["cand"][0].tolist() == [1, 0] and o["score"][0, 1] < o["score"][0, 0]      # RELOCALIZATION never sorts


def test_a_stale_score_below_the_threshold_becomes_the_best_keyframe(header):
    for name, out in (("nbest_stale_best", "loop"), ("reloc_stale_best", "cand")):
        o, r = header(name)
        assert r["n_sharing"][0] == 2 and r["n_scored"][0] == 1 and r["max_common_words"][0] == 10 and r["min_common_words"][0] == 8
        assert o[out][0, 0] == 1 and r["n_loop"][0] == 1
        assert o["score"][0].tolist() == [0.625, f32(0.9), f32(0.7)] and r["best_acc_score"][0] == f32(0.625) + f32(0.9)


def test_a_best_keyframe_reached_from_several_entries_is_returned_once(header):
    for name, out in (("nbest_duplicate_best", "loop"), ("reloc_duplicate_best", "cand")):
        o, r = header(name)
        assert r["n_scored"][0] == 4 and r["n_loop"][0] == 2 and sorted(o[out][0, :2].tolist()) == [1, 3]


def test_the_walk_goes_on_behind_a_full_loop_list(header):
    o, r = header("nbest_three_loops_then_merge")
    assert o["loop"][0].tolist() == [3, 0, 1] and o["merge"][0].tolist() == [5, 6, 8] and r["status"][0] == PW.OK
    o, r = header("nbest_bad_map")
    assert o["loop"][0, 0] == 1 and o["merge"][0, 0] == 3 and (r["n_loop"][0], r["n_merge"][0]) == (1, 1)
    o, r = header("nbest_no_candidates")
    assert r["status"][0] == PW.OK and r["n_scored"][0] == 9 and o["loop"].size == 0


def test_only_a_bad_keyframe_in_front_of_the_walks_end_stops_it(header):
    o, r = header("nbest_bad_front")
    assert r["status"][0] == PW.BAD_KEYFRAME and (r["n_loop"][0], r["n_merge"][0]) == (0, 0) and (o["loop"] == SC.POISON).all()
    o, r = header("nbest_bad_middle")
    assert r["status"][0] == PW.BAD_KEYFRAME and o["loop"][0, :2].tolist() == [0, 1] and r["n_merge"][0] == 0
    o, r = header("nbest_bad_behind")
    assert r["status"][0] == PW.OK and o["loop"][0].tolist() == [0] and o["merge"][0].tolist() == [1]


def test_the_early_returns_have_names(header):
    for tag in ("nbest", "reloc"):
        assert header(tag + "_no_shared_word")[1]["status"].tolist() == [PW.NO_SHARING]
        assert header(tag + "_empty_query")[1]["status"].tolist() == [PW.EMPTY_QUERY, PW.OK]
        o, r = header(tag + "_empty_database")
        assert r["status"].tolist() == [PW.EMPTY_DATABASE] and o["score"].size == 0
    o, r = header("nbest_all_connected")
    assert r["status"].tolist() == [PW.NO_SHARING] and (o["common_words"][0] == 8).all()
    # NONE_SCORED cannot be reached: the row that holds the maximum passes its own threshold
    assert all(m > PW.min_common_words(m) for m in range(1, 70000))
    assert not any((header(name)[1]["status"] == PW.NONE_SCORED).any() for name in SC.CASES)


def test_connected_rows_neither_count_nor_score_nor_accumulate(header):
    o, r = header("nbest_connected_rows")
    assert r["max_common_words"][0] == 6 and r["n_sharing"][0] == 3 and r["n_scored"][0] == 3 and o["common_words"][0].tolist() == [10, 6, 5, 5]
    assert o["score"][0, 0] == f32(0.95) and r["best_acc_score"][0] < 0.95 + 0.75      # row 0's planted score was not added
    o, r = header("reloc_connected_rows")                                          # RELOCALIZATION has no such test
    assert r["max_common_words"][0] == 10 and r["n_sharing"][0] == 4 and r["n_scored"][0] == 1


@pytest.mark.parametrize("m", range(1, 11))
def test_the_word_threshold(header, m):
    s = SC.case("nbest_threshold_max%d" % m)
    o, r = header("nbest_threshold_max%d" % m)
    lo = int(f32(m) * f32(0.8))
    assert r["max_common_words"][0] == m and r["min_common_words"][0] == lo == [0, 1, 2, 3, 4, 4, 5, 6, 7, 8][m - 1]
    counts = o["common_words"][0]
    assert set(counts.tolist()) == {c for c in (m, lo, lo + 1, lo - 1) if 1 <= c <= m}
    scored = o["score"][0] != 0
    assert (scored == (counts > lo)).all() and r["n_scored"][0] == scored.sum()
    assert (s["score_in"] == 0).all()


def test_the_sum_is_sequential(header):
    bow_of = lambda seed: list(enumerate(SC.last_bit_weights(seed)))
    differs = lambda b: f32(PW.l1_score(b, b)) != f32(PW.l1_score(b, b, "tree_sum"))
    found = [seed for seed in range(100) if differs(bow_of(seed))]
    assert found[0] == SC.SUM_SEED and 0 < len(found) < 100                            # the recorded seed is the search's first result
    bow = bow_of(SC.SUM_SEED)
    seq, tree = PW.l1_score(bow, bow), PW.l1_score(bow, bow, "tree_sum")
    assert tree - seq == 2.0 ** -53 and f32(seq) == f32(0.5) and f32(tree) == np.nextafter(f32(0.5), f32(1))
    assert header("nbest_sum_last_bit")[0]["score"][0, 0] == f32(0.5)


def test_the_retained_share_and_the_other_map(header):
    o, r = header("reloc_retain_boundary")
    assert r["best_acc_score"][0] == 0.5 and o["score"][0, 1] == f32(0.375) and o["cand"][0, :2].tolist() == [0, 2] and r["n_loop"][0] == 2
    o, r = header("reloc_other_map")
    assert o["cand"][0, :1].tolist() == [0] and r["n_loop"][0] == 1 and r["best_acc_score"][0] == 1.5


# ---- (d) ------------------------------------------------------------------------------------------------------------------------------
def test_the_cases_cover_the_sizes(host, header):
    for tag in ("nbest", "reloc"):
        sizes = {(SC.case(n)["n_db"], SC.case(n)["n_queries"]) for n in SC.CASES if n.startswith(tag + "_db")}
        assert {a for a, _ in sizes} >= {1, 63, 64, 65, 257, 700, SC.MAX_DB} and {b for _, b in sizes} >= {1, 3}
        s = SC.case(tag + "_db257_q3")
        assert set(s["db_n"].tolist()) == {0, 1, 63, 64, 65, 130} and s["capacity"] == 130
        assert any(SC.case(n)["q_step"] < 0 for n in SC.CASES if n.startswith(tag)) and any(SC.case(n)["q_first"] > 0 for n in SC.CASES)
        assert SC.case(tag + "_capacity256")["capacity"] == 256 == SC.case(tag + "_capacity256")["db_n"].max()
    assert all(SC.case(n)["capacity"] <= 256 for n in SC.CASES)
    for tag in ("nbest", "reloc"):                         # a query that fills the largest q_capacity the entry takes, and a short one beside it
        s = SC.case("%s_q_capacity%d" % (tag, SC.MAX_QUERY_WORDS))
        assert s["q_capacity"] == SC.MAX_QUERY_WORDS == s["q_n"][0] and s["q_n"][2] == 5 and s["q_step"] == 2
        assert header("%s_q_capacity%d" % (tag, SC.MAX_QUERY_WORDS))[1]["max_common_words"].tolist() == [87, 3]
    # lists longer than a workgroup of 256 lanes, and not a power of two
    assert header("nbest_db%d" % SC.MAX_DB)[1]["n_scored"].min() > 512 and header("reloc_db700")[1]["n_scored"].max() > 64
    long_walk = header("nbest_db700_long_walk")[1]
    assert long_walk["n_loop"][0] + long_walk["n_merge"][0] > 50 and long_walk["status"].tolist() == [PW.OK, PW.BAD_KEYFRAME]
    # both sides of the launch-time bounds, and of the candidate capacity
    assert host.pr_max_db() == SC.MAX_DB and host.pr_max_query_words() == SC.MAX_QUERY_WORDS
    assert host.pr_unsupported(0, SC.MAX_DB, SC.MAX_QUERY_WORDS) == 0 and host.pr_unsupported(1, 63, 130) == 1      # L1_NORM only
    assert host.pr_unsupported(0, SC.MAX_DB + 1, 130) == 1 and host.pr_unsupported(0, 63, SC.MAX_QUERY_WORDS + 1) == 1
    assert host.pr_fits(SC.MAX_DB, SC.MAX_QUERY_WORDS) == 1 and host.pr_fits(SC.MAX_DB + 1, 1) == 0 and host.pr_fits(1, SC.MAX_QUERY_WORDS + 1) == 0
    budget = 160 * 1024 - 512
    assert host.pr_query_lds_bytes(SC.MAX_DB) == 16 * SC.MAX_DB + 80 <= budget < host.pr_query_lds_bytes(SC.MAX_DB + 1)
    assert host.pr_pair_lds_bytes(SC.MAX_QUERY_WORDS) == 12 * SC.MAX_QUERY_WORDS <= budget < host.pr_pair_lds_bytes(SC.MAX_QUERY_WORDS + 1)
    assert header("reloc_cand_capacity_4")[1]["status"].tolist() == [PW.OK]
    o, r = header("reloc_cand_capacity_3")
    assert r["status"].tolist() == [PW.TRUNCATED] and r["n_loop"][0] == 4 and o["cand"][0].tolist() == header("reloc_cand_capacity_4")[0]["cand"][0, :3].tolist()
    assert header("reloc_cand_capacity_0")[1]["status"].tolist() == [PW.TRUNCATED]


# ---- (e) ------------------------------------------------------------------------------------------------------------------------------
def test_erase_leaves_the_lists_of_the_other_keyframes_in_add_order():
    rng = np.random.default_rng(1)
    kfs = [PW.KeyFrame(k, sorted({int(w): 1.0 for w in rng.integers(0, 12, 5)}.items()), None, False) for k in range(20)]
    full, kept = PW.KeyFrameDatabase(), PW.KeyFrameDatabase()
    for kf in kfs:
        full.add(kf)
    gone = {3, 4, 11, 19}
    for k in gone:
        full.erase(kfs[k])
    for kf in kfs:
        if kf.row not in gone:
            kept.add(kf)
    rows = lambda db: {w: [kf.row for kf in lst] for w, lst in db.mvInvertedFile.items() if lst}
    assert rows(full) == rows(kept) and all(r == sorted(r) for r in rows(full).values())


def test_first_encounter_order_is_smallest_shared_word_then_row():
    """the claim the device stands on, on the walk alone: the order of lKFsSharingWords against a sort by (smallest shared word, row)"""
    s = SC.case("reloc_db257_q3")
    kfs = [PW.KeyFrame(k, PW.bow_of(s["db_ids"][k], s["db_w"][k], s["db_n"][k], s["capacity"]), None, False) for k in range(s["n_db"])]
    db = PW.KeyFrameDatabase()
    for kf in kfs:
        db.add(kf)
    bow = PW.bow_of(s["q_ids"][0], s["q_w"][0], s["q_n"][0], s["q_capacity"])
    order = []
    for word, _ in bow:
        for kf in db.mvInvertedFile.get(word, []):
            if kf.row not in order:
                order.append(kf.row)
    mine = {w for w, _ in bow}
    keyed = sorted((min(mine & {w for w, _ in kf.mBowVec}), kf.row) for kf in kfs if mine & {w for w, _ in kf.mBowVec})
    assert len(order) > 100 and order == [k for _, k in keyed] and order != sorted(order)


def test_two_queries_chained_through_one_score_row(host):
    """the reference's consecutive queries: the second reads what the first left in the keyframes' score fields"""
    for name in ("nbest_chained", "reloc_chained"):
        s = SC.case(name)
        one = lambda q, state: dict(s, n_queries=1, q_first=s["q_first"] + q * s["q_step"], q_map=s["q_map"][q:q + 1].copy(),
                                    connected=None if s["connected"] is None else s["connected"][q:q + 1].copy(), score_in=state)
        first = one(0, s["score_in"][0:1].copy())
        left = PW.walk_scene(first)["score"]
        second = one(1, left.copy())
        want, got = PW.walk_scene(second), run_host(host, second)
        assert SC.differences(got, want) == [] and SC.differences(run_host(host, first), PW.walk_scene(first)) == []
        assert (left != s["score_in"][0:1]).any() and (want["score"] != left).any()
        assert (want["score"] == left).sum() > 0                                      # ... and part of the first query's row survives the second


# ---- (f) ------------------------------------------------------------------------------------------------------------------------------
def test_the_rows_and_names_are_the_headers(host):
    assert host.pr_result_bytes() == SC.RESULT_DTYPE.itemsize == X.PLACE_RESULT_DTYPE.itemsize == 32 and SC.RESULT_DTYPE == X.PLACE_RESULT_DTYPE
    header = open(os.path.join(ROOT, "include", "orbx.h")).read()
    body = re.search(r"typedef struct orbx_place_result \{(.*?)\} orbx_place_result;", header, re.S).group(1)
    fields = re.findall(r"^\s*(int32_t|float) (\w+);", body, re.M)
    assert [n for _, n in fields] == list(X.PLACE_RESULT_DTYPE.names)
    for i, (t, n) in enumerate(fields):
        assert X.PLACE_RESULT_DTYPE.fields[n][1] == 4 * i and X.PLACE_RESULT_DTYPE.fields[n][0] == np.dtype("<f4" if t == "float" else "<i4")
    names = re.findall(r"ORBX_PLACE_(\w+) = (\d+)", header)
    assert [n for n, _ in names] == ["N_BEST", "RELOCALIZATION"] + list(PW.STATUS) and list(X.PLACE_STATUS) == list(PW.STATUS)
    assert [int(v) for _, v in names] == [0, 1] + list(range(len(PW.STATUS))) and host.pr_statuses() == len(PW.STATUS)
    assert (X.PLACE_N_BEST, X.PLACE_RELOCALIZATION) == (PW.N_BEST, PW.RELOCALIZATION) == (0, 1)
    assert "orbx_detect_candidates_device" in X.header_symbols() and "orbx_debug_place_recognition_launches" in X.header_symbols()
    L = X.load_library()
    assert hasattr(L, "orbx_detect_candidates_device") and len(L.orbx_detect_candidates_device.argtypes) == 28
    assert L.orbx_debug_place_recognition_launches(2) == -2 and L.orbx_debug_place_recognition_launches(0) >= 0
    assert "n_db <= 8192" in header and "q_capacity\n * <= 13610" in header          # the bounds of the declaration's comment


# ---- (g) ------------------------------------------------------------------------------------------------------------------------------
def test_the_standalone_program_is_clean_under_sanitizers(tmp_path):
    exe = str(tmp_path / "place_recognition_host_check")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *HOST_FLAGS,
                           "-DPLACE_RECOGNITION_HOST_MAIN", SRC, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "every access inside its arrays" in out.stdout and "FAILED" not in out.stdout
