"""KeyFrameDatabase::DetectNBestCandidates and KeyFrameDatabase::DetectRelocalizationCandidates (reference src/KeyFrameDatabase.cc:612-780,
:783-895) stated with the reference's OWN structures: an inverted file of lists filled by add and erase (:39-66), mutable per-keyframe
query / words / score fields, a list with a stable sort, a set, and L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) with
its two iterators and lower_bound jumps, in binary64 and float32.  It is NOT written in the kernel's pair form: that the order of first
encounter equals (smallest shared word, row), that a connected row behaves like a row that shares nothing, and that the walk over the sorted
list is two ordered counts are what tests/test_place_recognition.py checks by comparing extractorb_amd/csrc/k_place_recognition.hpp with
this file byte for byte.

Where the entry differs from the reference it is by a declared rule, stated here once more:
  * `if(pKFi->isBad()) continue;` (:735-736) never returns once a bad keyframe reaches the front of the walk; the entry stops there, keeps
    what was collected and says BAD_KEYFRAME;
  * the early returns have names (STATUS);
  * RELOCALIZATION writes the first cand_capacity candidates and says TRUNCATED when there are more.

MUTANTS names one-line changes of this walk; tests/test_place_recognition.py names, for each, a scene whose output it changes, or the reason
why no scene can."""
import bisect
import functools

import numpy as np

f32, f64 = np.float32, np.float64
N_BEST, RELOCALIZATION = 0, 1
STATUS = ("OK", "NO_SHARING", "NONE_SCORED", "EMPTY_DATABASE", "EMPTY_QUERY", "BAD_KEYFRAME", "TRUNCATED")
OK, NO_SHARING, NONE_SCORED, EMPTY_DATABASE, EMPTY_QUERY, BAD_KEYFRAME, TRUNCATED = range(7)
COVIS = 10
RESULT_DTYPE = np.dtype([("status", "<i4"), ("n_sharing", "<i4"), ("max_common_words", "<i4"), ("min_common_words", "<i4"),
                         ("n_scored", "<i4"), ("best_acc_score", "<f4"), ("n_loop", "<i4"), ("n_merge", "<i4")])

MUTANTS = ("tree_sum", "float_sum", "threshold_ge", "point8_double", "point8_times4_over5", "connected_in_maximum", "connected_as_neighbours",
           "stale_zero", "stale_fresh", "unstable_sort", "row_order", "map_after_set", "full_loop_list_skips_set", "reloc_sorted", "retain_ge")


class Map:
    def __init__(self, ident, bad=False):
        self.ident, self.bad = ident, bad

    def IsBad(self):
        return self.bad


class KeyFrame:
    """what KeyFrameDatabase reads and writes of a KeyFrame"""

    def __init__(self, row, bow, kf_map, bad):
        self.row = row                                   # the database row: output only
        self.mBowVec = bow                               # [(word id, weight)], ascending ids: std::map<WordId, WordValue>
        self.map, self.bad = kf_map, bad
        self.covisible = []                              # GetBestCovisibilityKeyFrames(10)
        self.mnPlaceRecognitionQuery = self.mnRelocQuery = -1
        self.mnPlaceRecognitionWords = self.mnRelocWords = 0
        self.mPlaceRecognitionScore = self.mRelocScore = f32(0)
        self.encounters = 0                              # not the reference's: how often the inverted file led here (d_common_words)

    def isBad(self):
        return self.bad

    def GetMap(self):
        return self.map

    def GetBestCovisibilityKeyFrames(self, n):
        return self.covisible[:n]


class KeyFrameDatabase:
    def __init__(self):
        self.mvInvertedFile = {}                         # word -> list<KeyFrame*>

    def add(self, kf):
        for word, _ in kf.mBowVec:
            self.mvInvertedFile.setdefault(word, []).append(kf)

    def erase(self, kf):
        for word, _ in kf.mBowVec:
            lst = self.mvInvertedFile.get(word, [])
            for i, other in enumerate(lst):
                if other is kf:
                    del lst[i]
                    break


def l1_score(v1, v2, mutant=None):
    """L1Scoring::score: two iterators, lower_bound jumps, a double sum of three-rounding terms"""
    k1, k2 = [w for w, _ in v1], [w for w, _ in v2]
    i1 = i2 = 0
    score = f64(0)
    terms = []
    while i1 < len(v1) and i2 < len(v2):
        vi, wi = f64(v1[i1][1]), f64(v2[i2][1])
        if k1[i1] == k2[i2]:
            term = np.abs(vi - wi) - np.abs(vi) - np.abs(wi)
            if mutant == "float_sum":
                score = f64(f32(score) + f32(term))
            else:
                score = score + term
            terms.append(term)
            i1 += 1
            i2 += 1
        elif k1[i1] < k2[i2]:
            i1 = bisect.bisect_left(k1, k2[i2])
        else:
            i2 = bisect.bisect_left(k2, k1[i1])
    if mutant == "tree_sum":
        while len(terms) > 1:
            terms = [terms[i] + terms[i + 1] if i + 1 < len(terms) else terms[i] for i in range(0, len(terms), 2)]
        score = terms[0] if terms else f64(0)
    return -score / f64(2.0)


def comp_first(a, b):
    """list::sort(compFirst): a stable sort on a.first > b.first"""
    return -1 if a[0] > b[0] else (1 if b[0] > a[0] else 0)


def min_common_words(max_common, mutant=None):
    if mutant == "point8_double":
        return int(max_common * 0.8)
    if mutant == "point8_times4_over5":
        return max_common * 4 // 5
    return int(f32(max_common) * f32(0.8))


def detect(db, mode, query_id, bow, query_map, connected, n_candidates, mutant=None):
    """both functions: the two differ in the connected test, in what follows the accumulation, and in which fields they use (here one set of
    fields serves both: a KeyFrame object lives for one query).  Returns (result fields, loop, merge) or (result fields, candidates, None)."""
    r = dict(status=OK, n_sharing=0, max_common_words=0, min_common_words=0, n_scored=0, best_acc_score=f32(0), n_loop=0, n_merge=0)
    n_best = mode == N_BEST
    lKFsSharingWords = []
    for word, _ in bow:
        for pKFi in db.mvInvertedFile.get(word, []):
            pKFi.encounters += 1
            if pKFi.mnPlaceRecognitionQuery != query_id:
                pKFi.mnPlaceRecognitionWords = 0
                if not (n_best and pKFi in connected):
                    pKFi.mnPlaceRecognitionQuery = query_id
                    lKFsSharingWords.append(pKFi)
                elif mutant == "connected_as_neighbours":
                    pKFi.mnPlaceRecognitionQuery = query_id
            pKFi.mnPlaceRecognitionWords += 1
    if mutant == "row_order":
        lKFsSharingWords.sort(key=lambda kf: kf.row)
    r["n_sharing"] = len(lKFsSharingWords)
    if not lKFsSharingWords:
        r["status"] = NO_SHARING
        return r, [], []
    maxCommonWords = 0
    for kf in lKFsSharingWords:
        if kf.mnPlaceRecognitionWords > maxCommonWords:
            maxCommonWords = kf.mnPlaceRecognitionWords
    if mutant == "connected_in_maximum":
        maxCommonWords = max([maxCommonWords] + [kf.encounters for kf in connected])
    minCommonWords = min_common_words(maxCommonWords, mutant)
    r["max_common_words"], r["min_common_words"] = maxCommonWords, minCommonWords
    lScoreAndMatch = []
    for pKFi in lKFsSharingWords:
        if pKFi.mnPlaceRecognitionWords >= minCommonWords if mutant == "threshold_ge" else pKFi.mnPlaceRecognitionWords > minCommonWords:
            si = f32(l1_score(bow, pKFi.mBowVec, mutant))
            pKFi.mPlaceRecognitionScore = si
            lScoreAndMatch.append((si, pKFi))
    r["n_scored"] = len(lScoreAndMatch)
    if not lScoreAndMatch:
        r["status"] = NONE_SCORED
        return r, [], []
    scored = {id(kf) for _, kf in lScoreAndMatch}
    lAccScoreAndMatch = []
    bestAccScore = f32(0)
    for si, pKFi in lScoreAndMatch:
        bestScore = accScore = si
        pBestKF = pKFi
        for pKF2 in pKFi.GetBestCovisibilityKeyFrames(COVIS):
            if pKF2.mnPlaceRecognitionQuery != query_id:
                continue
            s2 = pKF2.mPlaceRecognitionScore
            if id(pKF2) not in scored and mutant == "stale_zero":
                s2 = f32(0)
            if id(pKF2) not in scored and mutant == "stale_fresh":
                s2 = f32(l1_score(bow, pKF2.mBowVec))
            accScore = f32(accScore + s2)
            if s2 > bestScore:
                pBestKF, bestScore = pKF2, s2
        lAccScoreAndMatch.append((accScore, pBestKF))
        if accScore > bestAccScore:
            bestAccScore = accScore
    r["best_acc_score"] = bestAccScore
    spAlreadyAddedKF = set()
    if not n_best:
        if mutant == "reloc_sorted":
            lAccScoreAndMatch.sort(key=functools.cmp_to_key(comp_first))
        minScoreToRetain = f32(0.75) * bestAccScore
        vpRelocCandidates = []
        for si, pKFi in lAccScoreAndMatch:
            if si >= minScoreToRetain if mutant == "retain_ge" else si > minScoreToRetain:
                if mutant == "map_after_set":
                    if pKFi not in spAlreadyAddedKF:
                        if pKFi.GetMap() is query_map:
                            vpRelocCandidates.append(pKFi)
                        spAlreadyAddedKF.add(pKFi)
                    continue
                if pKFi.GetMap() is not query_map:
                    continue
                if pKFi not in spAlreadyAddedKF:
                    vpRelocCandidates.append(pKFi)
                    spAlreadyAddedKF.add(pKFi)
        r["n_loop"] = len(vpRelocCandidates)
        return r, vpRelocCandidates, None
    if mutant == "unstable_sort":
        lAccScoreAndMatch = sorted(reversed(lAccScoreAndMatch), key=functools.cmp_to_key(comp_first))
    else:
        lAccScoreAndMatch.sort(key=functools.cmp_to_key(comp_first))
    vpLoopCand, vpMergeCand = [], []
    i = 0
    while i < len(lAccScoreAndMatch) and (len(vpLoopCand) < n_candidates or len(vpMergeCand) < n_candidates):
        pKFi = lAccScoreAndMatch[i][1]
        if pKFi.isBad():
            r["status"] = BAD_KEYFRAME                  # the reference spins here for ever: `continue` advances neither i nor it
            break
        if pKFi not in spAlreadyAddedKF:
            if query_map is pKFi.GetMap() and len(vpLoopCand) < n_candidates:
                vpLoopCand.append(pKFi)
            elif query_map is not pKFi.GetMap() and len(vpMergeCand) < n_candidates and not pKFi.GetMap().IsBad():
                vpMergeCand.append(pKFi)
            elif mutant == "full_loop_list_skips_set" and query_map is pKFi.GetMap():
                i += 1
                continue
            spAlreadyAddedKF.add(pKFi)
        i += 1
    r["n_loop"], r["n_merge"] = len(vpLoopCand), len(vpMergeCand)
    return r, vpLoopCand, vpMergeCand


def bow_of(ids, weights, n, capacity):
    n = max(0, min(int(n), capacity))
    return [(int(ids[j]), f64(weights[j])) for j in range(n)]


def walk_scene(s, mutant=None):
    """the entry's outputs for a scene (place_recognition_scenes.py) from poisoned arrays: result rows, candidate rows, the score rows
    (state in, state out) and the shared-word counts"""
    import place_recognition_scenes as SC
    o = SC.poisoned_outputs(s)
    n_db, cap = s["n_db"], s["capacity"]
    for q in range(s["n_queries"]):
        # a KeyFrame object lives for one query: its score field starts as the state row says, no row carries the query's id
        maps = {}
        kfs = []
        for k in range(n_db):
            mid = int(s["db_map"][k])
            if mid not in maps:
                maps[mid] = Map(mid)
            # bit 1 is the MAP's (include/orbx.h: the same on every row of a map); a Map object has one IsBad()
            maps[mid].bad = maps[mid].bad or bool(s["db_flags"][k] & 2)
            kfs.append(KeyFrame(k, bow_of(s["db_ids"][k], s["db_w"][k], s["db_n"][k], cap), maps[mid], bool(s["db_flags"][k] & 1)))
        db = KeyFrameDatabase()
        for k, kf in enumerate(kfs):
            kf.covisible = [kfs[j] for j in s["db_covis"][k] if 0 <= j < n_db]
            kf.mPlaceRecognitionScore = o["score"][q, k]
            db.add(kf)
        qmap_id = int(s["q_map"][q])
        query_map = maps.get(qmap_id) or Map(qmap_id)
        frame = s["q_first"] + q * s["q_step"]
        bow = bow_of(s["q_ids"][frame], s["q_w"][frame], s["q_n"][frame], s["q_capacity"])
        connected = set()
        if s["mode"] == N_BEST and s["connected"] is not None:
            connected = {kfs[k] for k in range(n_db) if s["connected"][q, k]}
        r, first, second = detect(db, s["mode"], 1000000 + q, bow, query_map, connected, s["n_candidates"], mutant)
        if n_db == 0:
            r["status"] = EMPTY_DATABASE
        elif r["status"] == NO_SHARING and not bow:
            r["status"] = EMPTY_QUERY
        if s["mode"] == N_BEST:
            for i, kf in enumerate(first):
                o["loop"][q, i] = kf.row
            for i, kf in enumerate(second):
                o["merge"][q, i] = kf.row
        else:
            if len(first) > s["cand_capacity"]:
                r["status"] = TRUNCATED
            for i, kf in enumerate(first[:s["cand_capacity"]]):
                o["cand"][q, i] = kf.row
        for name in RESULT_DTYPE.names:
            o["result"][name][q] = r[name]
        for k, kf in enumerate(kfs):
            o["score"][q, k] = kf.mPlaceRecognitionScore
            o["common_words"][q, k] = kf.encounters
    return o
