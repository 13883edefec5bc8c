"""orbx_detect_candidates_device on the GPU: the scenes of tests/place_recognition_scenes.py through the ctypes wrapper against the walk
(tests/place_recognition_walk.py), byte for byte - candidates, counts, result rows, the whole score row, the poison beyond the counts, the
shared-word counts -; the launch counters of the entry's one form; two calls back to back on one handle; two queries chained through one
score row; the chain orbx_compute_bow_device -> this entry -> orbx_search_by_bow_keyframes_device on the same device arrays; the entry's
rejections."""
import numpy as np
import pytest

import bow_scenes
import extractorb_amd as X
import place_recognition_scenes as SC
import place_recognition_walk as PW
from test_bow import make_vocab

_dev, upload, call, download = SC.to_device, SC.upload, SC.call, SC.download


def gpu_run(ex, voc, s):
    import torch
    d, ins = upload(s)
    torch.cuda.synchronize()                            # torch's copies have landed before the handle's stream runs
    call(ex, voc, s, d, ins)
    ex.synchronize()
    return download(s, d)


@pytest.fixture(scope="module")
def ex():
    import torch
    torch.zeros(1).cuda()                               # torch asks for the GPU first
    return X.ORBextractor(1000, 1.2, 8)


@pytest.fixture(scope="module")
def voc():
    import torch
    torch.zeros(1).cuda()
    return X.Vocabulary(arrays=make_vocab(np.random.default_rng(3), k=3, L=2))      # L1_NORM


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SC.CASES))
def test_gpu_scene_equals_the_walk(ex, voc, name):
    s, want = SC.case(name), SC.case_expected(name)
    before = [ex.debug_place_recognition_launches(w) for w in (0, 1)]
    got = gpu_run(ex, voc, s)
    # the one launch form: k_place_pairs unless the database is empty, k_place_query always
    assert [ex.debug_place_recognition_launches(w) for w in (0, 1)] == [before[0] + (s["n_db"] > 0), before[1] + 1]
    assert SC.differences(got, want) == [], [(PW.STATUS[a], PW.STATUS[b]) for a, b in zip(got["result"]["status"], want["result"]["status"])]


@pytest.mark.gpu
def test_gpu_two_calls_back_to_back_on_one_handle(ex, voc):
    """no synchronisation between them: both use the handle's workspace, the second one a larger one, and both results stand"""
    import torch
    names = ("nbest_db63_q3", "reloc_db257_q3", "nbest_db65_q3")
    runs = [(SC.case(n),) + upload(SC.case(n)) for n in names]
    torch.cuda.synchronize()
    for s, d, ins in runs:
        call(ex, voc, s, d, ins)
    ex.synchronize()
    for (s, d, _), name in zip(runs, names):
        assert SC.differences(download(s, d), SC.case_expected(name)) == [], name


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["nbest_chained", "reloc_chained"])
def test_gpu_two_queries_chained_through_one_score_row(ex, voc, name):
    """the reference's consecutive queries: ONE device row of scores, the second call reads what the first left"""
    import torch
    s = SC.case(name)
    one = lambda q, state: dict(s, n_queries=1, q_first=s["q_first"] + q * s["q_step"], q_map=s["q_map"][q:q + 1].copy(),
                                connected=None if s["connected"] is None else s["connected"][q:q + 1].copy(), score_in=state)
    first = one(0, s["score_in"][0:1].copy())
    left = PW.walk_scene(first)["score"]
    second = one(1, left.copy())
    want = PW.walk_scene(second)
    d1, ins1 = upload(first)
    d2, ins2 = upload(second)
    d2["score"] = d1["score"]                           # the state row itself
    torch.cuda.synchronize()
    call(ex, voc, first, d1, ins1)
    call(ex, voc, second, d2, ins2)
    ex.synchronize()
    assert SC.differences(download(second, d2), want) == []
    assert (want["score"] != left).any() and (left != s["score_in"][0:1]).any()


@pytest.mark.gpu
def test_gpu_the_chain_from_compute_bow_to_search_by_bow(ex):
    """orbx_compute_bow_device writes the BoW vectors of six frames; the SAME device arrays are the database rows (frames 0 .. 4) and the
    query rows (frame 5) of orbx_detect_candidates_device; its first loop candidate is the keyframe orbx_search_by_bow_keyframes_device
    matches the query against.  Nothing but the candidate's index crosses to the host in between."""
    import torch
    rng = np.random.default_rng(31)
    v = bow_scenes.exponent_weights(make_vocab(rng, k=10, L=3), rng, spread=4)
    voc = X.Vocabulary(arrays=v)
    B, cap, n = 6, 320, 300
    desc = np.zeros((B, cap, 32), np.uint8)
    for f in range(B - 1):
        desc[f, :n] = bow_scenes.near_leaves(v, rng, n)
    desc[5, :n] = desc[2, :n]                            # the query sees the place of keyframe 2 again: a tenth of its features are new
    desc[5, :n // 10] = bow_scenes.near_leaves(v, rng, n // 10)
    kps = np.zeros((B, cap), X.KEYPOINT_DTYPE)
    kps["angle"] = rng.uniform(0, 360, (B, cap)).astype(np.float32)
    kps["angle"][5] = kps["angle"][2]
    zeros = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")
    d_desc, d_n, d_kps = _dev(desc), _dev(np.full(B, n, np.int32)), _dev(kps)
    d_wid, d_ww, d_nw = zeros((B, cap), torch.int32), zeros((B, cap), torch.float64), zeros(B, torch.int32)
    d_fn, d_fi, d_nf = zeros((B, cap), torch.int32), zeros((B, cap), torch.int32), zeros(B, torch.int32)
    n_db = B - 1
    covis = np.full((n_db, 10), -1, np.int32)
    covis[2, :2] = [1, 3]
    d_map, d_flags, d_covis, d_qmap = zeros(n_db, torch.int32), zeros(n_db, torch.uint8), _dev(covis), zeros(1, torch.int32)
    d_score, d_result = zeros((1, n_db), torch.float32), zeros(32, torch.uint8)
    d_loop, d_merge = torch.full((1, 3), int(SC.POISON), dtype=torch.int32, device="cuda"), torch.full((1, 3), int(SC.POISON), dtype=torch.int32, device="cuda")
    flags = torch.ones((1, cap), dtype=torch.uint8, device="cuda")
    d_m, d_nm = torch.full((1, cap), -7, dtype=torch.int32, device="cuda"), zeros(1, torch.int32)
    pointers = [t.data_ptr() for t in (d_wid, d_ww, d_nw, d_fn, d_fi, d_nf)]
    torch.cuda.synchronize()
    ex.compute_bow_device(voc, B, d_desc, d_n, cap, d_wid, d_ww, d_nw, d_fn, d_fi, d_nf, levels_up=2)
    ex.detect_candidates_device(voc, X.PLACE_N_BEST, n_db, d_wid, d_ww, d_nw, cap, d_map, d_flags, d_covis, 1, (5, 1), d_wid, d_ww, d_nw, cap, d_qmap,
                                d_score, d_result, n_candidates=3, d_loop=d_loop, d_merge=d_merge)
    ex.synchronize()
    cand = int(d_loop[0, 0])                             # the one value that crosses: the entry's kf2_first is a host integer
    ex.search_by_bow_keyframes_device(1, (5, 1), (cand, 1), d_fn, d_fi, d_nf, flags, flags, d_kps, d_desc, d_n, cap, d_m, d_nm, nnratio=0.8)
    ex.synchronize()
    assert pointers == [t.data_ptr() for t in (d_wid, d_ww, d_nw, d_fn, d_fi, d_nf)]
    # the walk on what compute_bow wrote
    s = dict(mode=PW.N_BEST, n_db=n_db, capacity=cap, db_ids=d_wid.cpu().numpy().view(np.uint32), db_w=d_ww.cpu().numpy(), db_n=d_nw.cpu().numpy(),
             db_map=np.zeros(n_db, np.int32), db_flags=np.zeros(n_db, np.uint8), db_covis=covis, n_queries=1, q_first=5, q_step=1, q_capacity=cap,
             q_ids=d_wid.cpu().numpy().view(np.uint32), q_w=d_ww.cpu().numpy(), q_n=d_nw.cpu().numpy(), q_map=np.zeros(1, np.int32), connected=None,
             n_candidates=3, cand_capacity=0, score_in=np.zeros((1, n_db), np.float32))
    want = PW.walk_scene(s)
    assert d_loop.cpu().numpy().tobytes() == want["loop"].tobytes() and d_score.cpu().numpy().tobytes() == want["score"].tobytes()
    assert d_result.cpu().numpy().tobytes() == want["result"].tobytes() and want["result"]["status"][0] == PW.OK
    assert cand == 2 and want["result"]["max_common_words"][0] > 100
    assert int(d_nm[0]) > 100                            # the matcher finds the place's features in the candidate


@pytest.mark.gpu
def test_gpu_rejections_return_before_any_launch(ex, voc):
    import torch
    s = SC.case("nbest_db63_q3")
    o = SC.poisoned_outputs(s)
    d, ins = upload(s)
    l2 = X.Vocabulary(arrays=make_vocab(np.random.default_rng(3), k=3, L=2, scoring=1))
    torch.cuda.synchronize()
    good = dict(vocab=voc, mode=s["mode"], n_db=s["n_db"], d_db_word_ids=ins["db_ids"], d_db_word_weights=ins["db_w"], d_db_n_words=ins["db_n"],
                capacity=s["capacity"], d_db_map_id=ins["db_map"], d_db_flags=ins["db_flags"], d_db_covis=ins["db_covis"], n_queries=s["n_queries"],
                queries=(s["q_first"], s["q_step"]), d_q_word_ids=ins["q_ids"], d_q_word_weights=ins["q_w"], d_q_n_words=ins["q_n"],
                q_capacity=s["q_capacity"], d_q_map_id=ins["q_map"], d_score=d["score"], d_result=d["result"], d_connected=ins["connected"],
                n_candidates=3, d_loop=d["loop"], d_merge=d["merge"], d_cand=d["cand"], cand_capacity=s["cand_capacity"],
                d_common_words=d["common_words"])
    before = [ex.debug_place_recognition_launches(w) for w in (0, 1)]
    bad = [dict(mode=2), dict(mode=-1), dict(n_db=-1), dict(n_queries=0), dict(n_queries=65536), dict(capacity=0), dict(q_capacity=0),
           dict(queries=(-1, 1)), dict(queries=(1, -1)), dict(n_candidates=-1), dict(d_loop=None), dict(d_merge=None), dict(d_score=None),
           dict(d_result=None), dict(d_db_word_ids=None), dict(d_db_word_weights=None), dict(d_db_n_words=None), dict(d_db_map_id=None),
           dict(d_db_flags=None), dict(d_db_covis=None), dict(d_q_word_ids=None), dict(d_q_word_weights=None), dict(d_q_n_words=None),
           dict(d_q_map_id=None), dict(mode=X.PLACE_RELOCALIZATION, d_cand=None), dict(mode=X.PLACE_RELOCALIZATION, cand_capacity=-1)]
    unsupported = [dict(vocab=l2), dict(n_db=SC.MAX_DB + 1), dict(q_capacity=SC.MAX_QUERY_WORDS + 1)]
    for change, code in [(c, -2) for c in bad] + [(c, -8) for c in unsupported]:
        with pytest.raises(X.OrbxError) as err:
            ex.detect_candidates_device(**dict(good, **change))
        assert err.value.code == code, change
    ex.synchronize()
    assert [ex.debug_place_recognition_launches(w) for w in (0, 1)] == before
    for k, t in d.items():                              # nothing ran: the poison stands
        assert t.cpu().numpy().tobytes() == np.ascontiguousarray(o[k]).tobytes(), k
