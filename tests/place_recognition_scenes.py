"""Scenes for orbx_detect_candidates_device (KeyFrameDatabase::DetectNBestCandidates / DetectRelocalizationCandidates): plain arrays in the
entry's layout, crafted ones - one per rule of the reference the entry has to keep (docs/history/r31_place_recognition.md lists them) - and
seeded ones at the sizes where the kernels can go wrong.  A scene is a dict; case(name) builds it, case_expected(name) walks it ONCE with
tests/place_recognition_walk.py; both are cached and nothing changes them afterwards."""
import functools

import numpy as np

import place_recognition_walk as PW

f32, f64 = np.float32, np.float64
N_BEST, RELOCALIZATION = PW.N_BEST, PW.RELOCALIZATION
RESULT_DTYPE = PW.RESULT_DTYPE
POISON = np.int32(-286331154)                            # 0xEEEEEEEE
OUTPUTS = ("result", "loop", "merge", "cand", "score", "common_words")
MAX_DB, MAX_QUERY_WORDS = 8192, 13610                    # the entry's two launch-time bounds (include/orbx.h)
SUM_SEED = 0                                             # sum_last_bit: the first seed of last_bit_weights whose two sums narrow to different floats


def poisoned_outputs(s):
    nq, n_db = s["n_queries"], s["n_db"]
    return dict(result=np.frombuffer(bytes([0xEE]) * (RESULT_DTYPE.itemsize * nq), RESULT_DTYPE).copy(),
                loop=np.full((nq, s["n_candidates"]), POISON, np.int32), merge=np.full((nq, s["n_candidates"]), POISON, np.int32),
                cand=np.full((nq, s["cand_capacity"]), POISON, np.int32), score=s["score_in"].copy(),
                common_words=np.full((nq, n_db), POISON, np.int32))


def differences(got, want):
    """the outputs that are not equal byte for byte"""
    return [k for k in OUTPUTS if got[k].tobytes() != want[k].tobytes()]


def pack(bows, capacity, rng):
    """BoW vectors ({word: weight} or [(word, weight)]) in the three-array layout; the slots past a row's count hold junk"""
    ids = rng.integers(0, 1 << 20, (len(bows), capacity)).astype(np.uint32)
    w = rng.random((len(bows), capacity))
    n = np.zeros(len(bows), np.int32)
    for k, b in enumerate(bows):
        items = sorted(b.items()) if isinstance(b, dict) else list(b)
        n[k] = len(items)
        for j, (word, weight) in enumerate(items):
            ids[k, j], w[k, j] = word, weight
    return ids, w, n


def craft(mode, rows, queries, capacity=None, q_capacity=None, n_candidates=3, cand_capacity=None, q_first=0, q_step=1, seed=0):
    """rows: dict(words, map=0, flags=0, covis=[]) in KeyFrameDatabase::add order; queries: dict(words, map=0, connected=[rows],
    state={row: score})"""
    rng = np.random.default_rng(seed)
    n_db, nq = len(rows), len(queries)
    longest = lambda seq: max([len(x["words"]) for x in seq] + [1])
    capacity = capacity or longest(rows)
    q_capacity = q_capacity or longest(queries)
    ids, w, n = pack([r["words"] for r in rows], capacity, rng)
    covis = np.full((n_db, PW.COVIS), -1, np.int32)
    for k, r in enumerate(rows):
        c = r.get("covis", [])
        covis[k, :len(c)] = c
    n_frames = q_first + (nq - 1) * q_step + 1 if q_step >= 0 else q_first + 1
    frames = [{} for _ in range(n_frames)]
    for f in range(n_frames):                            # the frames between the queries hold words of their own
        frames[f] = {int(x): float(rng.random()) for x in rng.integers(0, 50, min(3, q_capacity))}
    for q, qu in enumerate(queries):
        frames[q_first + q * q_step] = qu["words"]
    q_ids, q_w, q_n = pack(frames, q_capacity, rng)
    connected = None
    if any("connected" in qu for qu in queries):
        connected = np.zeros((nq, n_db), np.uint8)
        for q, qu in enumerate(queries):
            connected[q, qu.get("connected", [])] = 1 + q
    score_in = np.zeros((nq, n_db), f32)
    for q, qu in enumerate(queries):
        for k, v in qu.get("state", {}).items():
            score_in[q, k] = v
    return dict(mode=mode, n_db=n_db, capacity=capacity, db_ids=ids, db_w=w, db_n=n, db_map=np.array([r.get("map", 0) for r in rows], np.int32),
                db_flags=np.array([r.get("flags", 0) for r in rows], np.uint8), db_covis=covis, n_queries=nq, q_first=q_first, q_step=q_step,
                q_capacity=q_capacity, q_ids=q_ids, q_w=q_w, q_n=q_n, q_map=np.array([qu.get("map", 0) for qu in queries], np.int32),
                connected=connected, n_candidates=n_candidates, cand_capacity=len(rows) if cand_capacity is None else cand_capacity,
                score_in=score_in)


def normalised(rng, words):
    """a BoW vector over the given words: positive weights with full mantissas that sum to about one, as transform() leaves them"""
    w = rng.random(len(words)) + 0.05
    w = w / w.sum()
    return {int(a): float(b) for a, b in zip(words, w)}


def seeded(seed, mode, n_db, row_words, n_queries, capacity, q_first=0, q_step=1, n_candidates=3, cand_capacity=None, places=None,
           query_words=None):
    """rows drawn from a few places (a place is a set of words; its rows take most of them and some others), queries drawn the same way:
    several rows pass the word threshold, neighbours are scored, stale and absent, two maps, a bad map, bad keyframes, connected rows, and a
    state row of planted scores.  row_words: the words of row k is row_words[k % len(row_words)]."""
    rng = np.random.default_rng(seed)
    places = places or max(1, n_db // 8)
    vocab = 6 * capacity
    base = [rng.permutation(vocab)[:capacity] for _ in range(places)]

    def draw(place, n):
        own = rng.permutation(base[place])[:int(round(0.8 * n))]
        rest = np.setdiff1d(rng.permutation(vocab), own, assume_unique=True)[:n - len(own)]
        return normalised(rng, np.concatenate([own, rest]).astype(np.int64))

    rows = []
    for k in range(n_db):
        nb = [int(x) for x in rng.integers(-1, n_db, rng.integers(0, PW.COVIS + 1))]
        if k % 5 == 0 and n_db > 1:
            nb = [int(x) for x in rng.permutation(n_db)[:min(n_db, PW.COVIS)]]
        rows.append(dict(words=draw(k % places, row_words[k % len(row_words)]), map=2 if k % 13 == 6 else int(k % 7 == 3), flags=0, covis=nb))
    for r in rows:
        if r["map"] == 2:
            r["flags"] |= 2                              # map 2 is bad
    for k in rng.permutation(n_db)[:n_db // 16]:
        rows[k]["flags"] |= 1                            # a few bad keyframes
    queries = []
    for q in range(n_queries):
        n = (query_words or capacity * 3 // 4) if q != 2 else 1
        queries.append(dict(words=draw(int(rng.integers(places)), n), map=int(q == 1),
                            connected=[int(x) for x in rng.permutation(n_db)[:n_db // 6]],
                            state={int(k): float(f32(rng.random())) for k in rng.permutation(n_db)[:n_db // 2 + 1]}))
    return craft(mode, rows, queries, capacity=capacity, q_capacity=capacity, n_candidates=n_candidates, cand_capacity=cand_capacity,
                 q_first=q_first, q_step=q_step, seed=seed)


# ---- crafted scenes -----------------------------------------------------------------------------------------------------------------------
def words(ids, weight=0.125):
    return {int(i): weight for i in ids}


def tie_list_order(mode):
    """Row 0 (A) shares words 10, 11 with the query, row 1 (B) shares 1 and 12, rows 2 and 5 are identical and share 20, 21; every shared
    weight equals the query's 0.125, so every score is exactly 0.25.  First encounter: B (word 1), A (word 10), 2, 5 (word 20) - not the row
    order.  N_BEST with one candidate returns B; RELOCALIZATION returns B, A, 2, 5."""
    rows = [dict(words=words([10, 11, 100, 101])), dict(words=words([1, 12, 102])), dict(words=words([20, 21])), dict(words=words([300])),
            dict(words=words([301])), dict(words=words([20, 21]))]
    return craft(mode, rows, [dict(words=words([1, 10, 11, 12, 20, 21, 400]))], n_candidates=1)


def reloc_order():
    """RELOCALIZATION never sorts: the first entry of the list has the LOWER score (0.1875 + 1/64 against 0.25) and stays in front"""
    q = words([1, 2, 10, 11, 12, 13])
    rows = [dict(words=words([10, 11, 12, 13], 0.0625)), dict(words={**words([1, 2, 12], 0.0625), 13: 1 / 64})]
    return craft(RELOCALIZATION, rows, [dict(words=q)])


def stale_best(mode):
    """Row 0 shares ten words (max 10, min 8), row 1 shares three: it is below the threshold, is never scored, carries the query's id and is
    row 0's neighbour.  Row 0 scores 0.625; row 1's planted state score 0.9 makes it pBestKF; its fresh score would be 0.1875.  Row 2 shares
    nothing and keeps its planted 0.7."""
    w = 0.0625
    rows = [dict(words=words(range(1, 11), w), covis=[1]), dict(words=words([3, 4, 5], w)), dict(words=words([500]), covis=[0])]
    return craft(mode, rows, [dict(words=words(range(1, 11), w), state={1: 0.9, 2: 0.7})])


def duplicate_best(mode):
    """All four rows are scored; row 1 has the highest score and is the neighbour of rows 0 and 2: pBestKF is row 1 three times.  Row 3
    names itself as its neighbour: its own score is added once more and it stays its own pBestKF."""
    rows = [dict(words=words(range(1, 10)), covis=[1]), dict(words=words(range(1, 11)), covis=[]), dict(words=words(range(2, 11)), covis=[-1, 1]),
            dict(words=words(range(1, 10)), covis=[3])]
    return craft(mode, rows, [dict(words=words(range(1, 11)))])


def scored_rows(scores, maps, flags=None, covis=None):
    """rows that all share words 1 .. 8 of an eight-word query (all scored) and whose scores are in the given order of size: row k's weights
    are scores[k] / 8 on each shared word, the query's are 0.125"""
    rows = []
    for k, sc in enumerate(scores):
        rows.append(dict(words=words(range(1, 9), sc / 8.0), map=maps[k], flags=(flags or {}).get(k, 0), covis=(covis or {}).get(k, [])))
    return rows, dict(words=words(range(1, 9)), map=0)


def three_loops_then_merge():
    """Sorted by accumulated score: row 4's entry (0.5 + its neighbour row 3's 0.75; pBestKF is row 3), rows 0, 1 (same map: with row 3
    three loop candidates), row 2 (same map, list full: not pushed, enters the set), row 3's own entry (a duplicate), rows 5, 6 (other map:
    merge candidates), row 7 (bad map: not pushed), row 8 (other map: the third merge candidate, the walk's last entry)."""
    rows, q = scored_rows([0.9, 0.85, 0.8, 0.75, 0.5, 0.45, 0.4, 0.35, 0.3], [0, 0, 0, 0, 0, 1, 1, 2, 1], flags={7: 2}, covis={4: [3]})
    return craft(N_BEST, rows, [q])


def bad_map():
    rows, q = scored_rows([0.9, 0.8, 0.7, 0.6], [2, 0, 2, 1], flags={0: 2, 2: 2})
    return craft(N_BEST, rows, [q])


def bad_keyframe(where):
    """front: the best row is bad, nothing is collected.  middle: two loop candidates are taken, then a bad keyframe stops the walk.  behind:
    both lists are full (n_candidates 1) before the bad keyframe: the walk never sees it."""
    if where == "front":
        rows, q = scored_rows([0.9, 0.8, 0.7], [0, 0, 1], flags={0: 1})
        return craft(N_BEST, rows, [q])
    if where == "middle":
        rows, q = scored_rows([0.9, 0.8, 0.7, 0.6, 0.5], [0, 0, 1, 0, 1], flags={2: 1})
        return craft(N_BEST, rows, [q])
    rows, q = scored_rows([0.9, 0.8, 0.7, 0.6], [0, 1, 0, 1], flags={2: 1})
    return craft(N_BEST, rows, [q], n_candidates=1)


def no_shared_word(mode):
    return craft(mode, [dict(words=words([1, 2])), dict(words=words([3]))], [dict(words=words([4, 5]))])


def empty_query(mode):
    return craft(mode, [dict(words=words([1, 2])), dict(words={})], [dict(words={}), dict(words=words([2]))])


def empty_database(mode):
    return craft(mode, [], [dict(words=words([4, 5]))], capacity=4, cand_capacity=2)


def all_connected():
    rows, q = scored_rows([0.9, 0.8, 0.7], [0, 0, 1], covis={0: [1, 2]})
    return craft(N_BEST, rows, [dict(q, connected=[0, 1, 2])])


def connected_rows(mode):
    """Row 0 shares most words but is connected: the maximum is row 1's 6, so rows 2 (5 words) and 3 (5 words) pass the threshold 4; were
    row 0 counted (10 words, threshold 8) they would not.  Row 0 is row 1's neighbour with a planted state score of 0.95: it is skipped."""
    rows = [dict(words=words(range(1, 11))), dict(words=words(range(1, 7)), covis=[0, 2]), dict(words=words(range(2, 7))),
            dict(words=words(range(3, 8)), covis=[0])]
    return craft(mode, rows, [dict(words=words(range(1, 11)), connected=[0], state={0: 0.95})])


def threshold(max_common):
    """A query of max_common words; row 0 shares all of them; then rows that share exactly minCommonWords, one more and one fewer (where such
    a count exists).  Only words > minCommonWords is scored."""
    m = PW.min_common_words(max_common)
    rows = [dict(words=words(range(1, max_common + 1)))]
    for c in (m, m + 1, m - 1):
        if 1 <= c <= max_common:
            rows.append(dict(words=words(range(1, c + 1))))
    return craft(N_BEST, rows, [dict(words=words(range(1, max_common + 1)))], n_candidates=4)


def last_bit_weights(seed):
    """four common words whose terms are -2v exactly (equal weights on both sides): 1/2, the half float ulp 2^-25, and two values below half the double ulp of the sum.  One after
    the other the two small ones vanish and the sum is a float tie, rounded to even; added to each other first they carry it over the tie
    when together they exceed half an ulp, which not every seed's pair does."""
    rng = np.random.default_rng(seed)
    small = (0.1 + 0.4 * rng.random(2)) * 2.0 ** -53
    return [0.5, 2.0 ** -25, float(small[0]), float(small[1])]


def sum_last_bit(mode):
    v = last_bit_weights(SUM_SEED)
    bow = {7 + 3 * i: x for i, x in enumerate(v)}
    return craft(mode, [dict(words=bow), dict(words=words([900]))], [dict(words={**bow, 5: 0.25, 1000: 0.25})])


def retain_boundary():
    """RELOCALIZATION: bestAccScore 0.5, an entry at exactly 0.75f * 0.5 = 0.375 is not retained, one a float ulp above is"""
    up = float(np.nextafter(f32(0.375), f32(1)))
    rows, q = scored_rows([0.5, 0.375, up, 0.25], [0, 0, 0, 0])
    return craft(RELOCALIZATION, rows, [q])


def other_map_before_set():
    """RELOCALIZATION: entries of another map are skipped; pBestKF of rows 0 and 2 is row 1 (other map: both are retained and skipped), of
    row 3 it is row 0 (accScore 1.15 against the bound 1.125): the one candidate"""
    rows, q = scored_rows([0.6, 0.9, 0.5, 0.55], [0, 1, 0, 0], covis={0: [1], 2: [1], 3: [0]})
    return craft(RELOCALIZATION, rows, [q])


def cand_capacity(n):
    """RELOCALIZATION with four candidates and room for n"""
    rows, q = scored_rows([0.9, 0.85, 0.8, 0.75], [0, 0, 0, 0])
    return craft(RELOCALIZATION, rows, [q], cand_capacity=n)


def chained_queries(mode):
    """two queries as the reference would run them one after the other: the second one's state row is what the first one left (the tests
    chain them); here each has its own planted row"""
    s = seeded(77, mode, 40, [12, 20, 9], 2, 24)
    return s


def many_rows(n_db, mode=N_BEST, n_candidates=3):
    """many rows of two words each, hundreds of them scored: lists longer than a workgroup, sorts of several thousand keys with many equal
    scores (a quarter of the rows are copies of an earlier row).  n_db = 8192 is the largest database the entry takes."""
    rng = np.random.default_rng(n_db)
    rows = []
    for k in range(n_db):
        bow = normalised(rng, rng.permutation(40)[:2]) if k % 4 or k == 0 else rows[int(rng.integers(k))]["words"]
        rows.append(dict(words=bow, map=2 if k % 10 == 9 else int(k % 3 == 0), flags=2 if k % 10 == 9 else 0,
                         covis=[int(x) for x in rng.integers(-1, n_db, 3)]))
    rows[n_db // 2]["flags"] |= 1
    q = dict(words=normalised(rng, np.arange(0, 40, 3)), map=0, connected=[int(x) for x in rng.permutation(n_db)[:n_db // 10]],
             state={int(k): float(f32(rng.random())) for k in rng.permutation(n_db)[:n_db // 2]})
    return craft(mode, rows, [q, dict(q, map=1, words=normalised(rng, np.arange(1, 40, 2)))], capacity=2, n_candidates=n_candidates, seed=n_db)


def longest_query(mode):
    """q_capacity at the entry's bound: k_place_pairs stages 12 * 13610 = 163 320 bytes, eight short of the LDS budget, in 54 trips of its
    staging loop.  Query 0 fills the capacity, query 1 holds five words; the frame between them is junk.  The rows hold a few of the
    query's words each - some from its last slots - and words of their own."""
    rng = np.random.default_rng(13610 + mode)
    ids = np.sort(rng.permutation(3 * MAX_QUERY_WORDS)[:MAX_QUERY_WORDS])
    long_q = normalised(rng, ids)
    rows = []
    for k in range(9):
        mine = np.concatenate([rng.choice(ids, 20 + 7 * k, replace=False), ids[-3 - k:], 3 * MAX_QUERY_WORDS + rng.permutation(500)[:30]])
        rows.append(dict(words=normalised(rng, np.unique(mine)), map=int(k == 4), covis=[int(x) for x in rng.integers(-1, 9, 4)]))
    short_q = {w: 0.2 for w in list(rows[2]["words"])[:3] + list(rows[7]["words"])[-2:]}
    return craft(mode, rows, [dict(words=long_q, state={1: 0.4, 3: 0.8}), dict(words=short_q, map=1)], q_capacity=MAX_QUERY_WORDS, q_first=0, q_step=2,
                 seed=13610)


def hostile_words(mode):
    """n_words negative and past the capacity: the entry reads max(0, min(n, capacity)) words"""
    s = seeded(5, mode, 20, [8], 2, 8, query_words=8)
    s["db_n"][3], s["db_n"][4], s["q_n"][s["q_first"] + s["q_step"]] = -7, 1000, 999
    return s


ROW_WORDS = [0, 1, 63, 64, 65, 130]
CASES = {}
for _mode, _tag in ((N_BEST, "nbest"), (RELOCALIZATION, "reloc")):
    for _n, _q, _first, _step in ((1, 1, 0, 1), (63, 3, 1, 2), (64, 1, 2, 0), (65, 3, 4, -2), (257, 3, 0, 1)):
        CASES["%s_db%d_q%d" % (_tag, _n, _q)] = functools.partial(seeded, 100 + _n, _mode, _n, ROW_WORDS, _q, 130, _first, _step,
                                                                  cand_capacity=max(1, _n // 3))
    CASES[_tag + "_tie_list_order"] = functools.partial(tie_list_order, _mode)
    CASES[_tag + "_stale_best"] = functools.partial(stale_best, _mode)
    CASES[_tag + "_duplicate_best"] = functools.partial(duplicate_best, _mode)
    CASES[_tag + "_no_shared_word"] = functools.partial(no_shared_word, _mode)
    CASES[_tag + "_empty_query"] = functools.partial(empty_query, _mode)
    CASES[_tag + "_empty_database"] = functools.partial(empty_database, _mode)
    CASES[_tag + "_connected_rows"] = functools.partial(connected_rows, _mode)
    CASES[_tag + "_sum_last_bit"] = functools.partial(sum_last_bit, _mode)
    CASES[_tag + "_chained"] = functools.partial(chained_queries, _mode)
    CASES[_tag + "_hostile_words"] = functools.partial(hostile_words, _mode)
    CASES[_tag + "_q_capacity%d" % MAX_QUERY_WORDS] = functools.partial(longest_query, _mode)
    CASES[_tag + "_capacity256"] = functools.partial(seeded, 256, _mode, 33, [256, 200, 17], 3, 256, 0, 1)
CASES["reloc_order"] = reloc_order
CASES["reloc_retain_boundary"] = retain_boundary
CASES["reloc_other_map"] = other_map_before_set
CASES["reloc_cand_capacity_4"] = functools.partial(cand_capacity, 4)
CASES["reloc_cand_capacity_3"] = functools.partial(cand_capacity, 3)
CASES["reloc_cand_capacity_0"] = functools.partial(cand_capacity, 0)
CASES["nbest_three_loops_then_merge"] = three_loops_then_merge
CASES["nbest_bad_map"] = bad_map
CASES["nbest_bad_front"] = functools.partial(bad_keyframe, "front")
CASES["nbest_bad_middle"] = functools.partial(bad_keyframe, "middle")
CASES["nbest_bad_behind"] = functools.partial(bad_keyframe, "behind")
CASES["nbest_all_connected"] = all_connected
CASES["nbest_no_candidates"] = lambda: dict(three_loops_then_merge(), n_candidates=0)
CASES["nbest_db%d" % MAX_DB] = functools.partial(many_rows, MAX_DB)
CASES["nbest_db700_long_walk"] = functools.partial(many_rows, 700, N_BEST, 150)
CASES["reloc_db700"] = functools.partial(many_rows, 700, RELOCALIZATION)
CASES["reloc_db%d" % MAX_DB] = functools.partial(many_rows, MAX_DB, RELOCALIZATION)
for _m in range(1, 11):
    CASES["nbest_threshold_max%d" % _m] = functools.partial(threshold, _m)


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def case_expected(name):
    return PW.walk_scene(case(name))


# ---- the scenes on the device: shared by tests/test_place_recognition_gpu.py and tools/place_recognition_rate.py ---------------------------
INPUTS = ("db_ids", "db_w", "db_n", "db_map", "db_flags", "db_covis", "q_ids", "q_w", "q_n", "q_map", "connected")


def to_device(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype.fields:
        a = a.view(np.uint8)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a).cuda()


def upload(s):
    """(poisoned outputs, inputs) of a scene as device tensors"""
    o = poisoned_outputs(s)
    return dict((k, to_device(v)) for k, v in o.items()), dict((k, None if s[k] is None else to_device(s[k])) for k in INPUTS)


def call(ex, voc, s, d, ins):
    ex.detect_candidates_device(voc, s["mode"], s["n_db"], ins["db_ids"], ins["db_w"], ins["db_n"], s["capacity"], ins["db_map"], ins["db_flags"],
                                ins["db_covis"], s["n_queries"], (s["q_first"], s["q_step"]), ins["q_ids"], ins["q_w"], ins["q_n"], s["q_capacity"],
                                ins["q_map"], d["score"], d["result"], d_connected=ins["connected"], n_candidates=s["n_candidates"], d_loop=d["loop"],
                                d_merge=d["merge"], d_cand=d["cand"], cand_capacity=s["cand_capacity"], d_common_words=d["common_words"])


def download(s, d):
    o = poisoned_outputs(s)
    return dict((k, d[k].cpu().numpy().view(o[k].dtype).reshape(o[k].shape)) for k in o)
