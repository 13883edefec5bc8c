"""orbx_covisibility_device and orbx_keyframe_redundancy_device on the GPU: the scenes of tests/covisibility_scenes.py through the ctypes
wrappers against the walk (tests/covisibility_walk.py), byte for byte - list rows, result rows, the poison beyond the counts, the slot
states -; the launch counters of the entries' one form each; calls back to back on one handle; the entries' rejections; and two chains on
device arrays: orbx_optimize_pose_device's match rows into the frame-mode vote, the new keyframe's vote, its ordered lists as the d_db_covis
rows of orbx_detect_candidates_device; the observation table orbx_update_map_points_device consumed into the redundancy test."""
import numpy as np
import pytest

import covisibility_scenes as SC
import covisibility_walk as CW
import extractorb_amd as X

_dev, upload, call, download = SC.to_device, SC.upload, SC.call, SC.download


def gpu_run(ex, s):
    import torch
    d, ins = upload(s)
    torch.cuda.synchronize()                            # torch's copies have landed before the handle's stream runs
    call(ex, s, d, ins)
    ex.synchronize()
    return download(s, d)


def launches(ex):
    return [ex.debug_covisibility_launches(w) for w in (0, 1, 2)]


@pytest.fixture(scope="module")
def ex():
    import torch
    torch.zeros(1).cuda()                               # torch asks for the GPU first
    return X.ORBextractor(1000, 1.2, 8)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SC.CASES))
def test_gpu_scene_equals_the_walk(ex, name):
    s, want = SC.case(name), SC.case_expected(name)
    before = launches(ex)
    got = gpu_run(ex, s)
    # the one launch form of each entry: the rank kernel and the vote, or the redundancy kernel
    vote = s["kind"] == "vote"
    assert launches(ex) == [before[0] + vote, before[1] + vote, before[2] + (not vote)]
    assert SC.differences(got, want) == [], (got["result"]["status"].tolist(), want["result"]["status"].tolist())


@pytest.mark.gpu
def test_gpu_calls_back_to_back_on_one_handle(ex):
    """no synchronisation between them: the votes share the handle's rank tables - the second call's are larger, the third's smaller and of
    other keys - and every result stands"""
    import torch
    names = ("update_frames65_n65", "local_frames257_n300_x17", "update_three_equal_weights", "redundancy_frames65_n65", "update_frames257_n300")
    runs = [(SC.case(n),) + upload(SC.case(n)) for n in names]
    torch.cuda.synchronize()
    for s, d, ins in runs:
        call(ex, s, d, ins)
    ex.synchronize()
    for (s, d, _), name in zip(runs, names):
        assert SC.differences(download(s, d), SC.case_expected(name)) == [], name


@pytest.mark.gpu
def test_gpu_the_chain_from_pose_optimization_to_place_recognition(ex):
    """Three tracked frames are optimised by orbx_optimize_pose_device; the SAME device rows of MapPoint indices are the subjects of the
    frame-mode vote.  The third frame becomes keyframe 11 (its observations are in the table): its row of the keyframes' table is a device
    copy of its match row, and UpdateConnections runs for all twelve keyframes with a capacity of ten over blocks that hold -1 - which makes
    the ordered block, untouched beyond each count, the d_db_covis table of orbx_detect_candidates_device.  Only integers would cross to
    the host in between, and none does."""
    import torch
    import place_recognition_scenes as PSC
    import place_recognition_walk as PW
    import pose_optimization_scenes as PS
    from test_bow import make_vocab
    rng = np.random.default_rng(34)
    ps = PS.make(counts=[40, 55, 64], seed=5)
    cap, n_mp, nF = ps["cap"], len(ps["world"]), 12
    matches = ps["matches"].reshape(3, cap)
    # the map: every MapPoint is seen from a few of keyframes 0 .. 10, those of the third frame also from keyframe 11
    pts = SC.neighbourhood_points(rng, n_mp, nF - 1, (5, 4, 3, 6, 2), width=3)
    for m in matches[2][matches[2] >= 0]:
        pts[m] = pts[m] + [nF - 1]
    kf_rows = np.full((nF, cap), -1, np.int32)
    kf_n = np.zeros(nF, np.int32)
    for m, p in enumerate(pts):
        for f in p:
            if f != nF - 1:
                kf_rows[f, kf_n[f]] = m
                kf_n[f] += 1
    kf_n[nF - 1] = ps["n_out"][2]
    assert kf_n.max() <= cap
    flags = np.zeros(nF, np.uint8)
    flags[7] = 1
    vote = SC.craft_vote(CW.LOCAL_KEYFRAMES, nF, pts, [dict(mp=list(matches[j]), n=int(ps["n_out"][j])) for j in range(3)], keys=SC.permuted_keys(nF, 3),
                         kf_flags=flags, capacity=cap)
    # the devices' arrays
    o = PS.poisoned_outputs(ps)
    d_pose = dict((k, _dev(v)) for k, v in o.items())
    pins = dict((k, _dev(ps[k])) for k in ("problems", "kps", "n_out", "matches", "world"))
    d_vote, vins = upload(vote)
    vins["subject_mp"], vins["subject_n"] = pins["matches"], pins["n_out"]              # the optimiser's own rows
    d_kf_rows, d_kf_n = _dev(kf_rows), _dev(kf_n)
    d_kf_self, d_kf_mapid = _dev(np.arange(nF, dtype=np.int32)), _dev(np.zeros(nF, np.int32))
    blocks = [torch.full((nF, 10), -1, dtype=torch.int32, device="cuda") for _ in range(4)]
    d_kf_result = torch.zeros(nF * 20, dtype=torch.uint8, device="cuda")
    place = PSC.seeded(7, PW.N_BEST, nF, [20, 25], 1, 30)
    voc = X.Vocabulary(arrays=make_vocab(np.random.default_rng(3), k=3, L=2))
    d_place, lins = PSC.upload(place)
    lins["db_covis"] = blocks[2]                                                         # the ordered keyframes
    torch.cuda.synchronize()
    ex.optimize_pose_device(3, (0, 1), pins["problems"], pins["kps"], pins["n_out"], None, cap, pins["matches"], pins["world"], n_mp, d_pose["poses"],
                            d_pose["outlier"], d_pose["result"])
    call(ex, vote, d_vote, vins)
    d_kf_rows[nF - 1].copy_(pins["matches"].view(3, cap)[2])                            # the new keyframe's mvpMapPoints, on the device
    ex.synchronize()                                    # (torch's copy runs on torch's stream: the handle's work before it, and it before the next call)
    torch.cuda.synchronize()
    ex.covisibility_device(CW.UPDATE_CONNECTIONS, n_mp, vins["obs_off"], vins["obs"], vins["mp_flags"], nF, vins["kf_flags"], vins["kf_key"], nF, d_kf_rows,
                           d_kf_n, cap, 10, blocks[0], blocks[1], d_kf_result, d_kf_map_id=d_kf_mapid, d_subject_kf=d_kf_self,
                           d_subject_map_id=d_kf_mapid, th=3, d_ordered_kf=blocks[2], d_ordered_w=blocks[3])
    PSC.call(ex, voc, place, d_place, lins)
    ex.synchronize()
    # the walks on the same tables
    assert np.array_equal(pins["matches"].cpu().numpy(), ps["matches"])                  # the optimiser left its match rows alone
    assert SC.differences(download(vote, d_vote), CW.walk_scene(vote)) == []
    kf_rows[nF - 1] = matches[2]
    update = dict(vote, mode=CW.UPDATE_CONNECTIONS, n_subjects=nF, subject_mp=kf_rows, subject_n=kf_n, subject_kf=np.arange(nF, dtype=np.int32),
                  subject_map=np.zeros(nF, np.int32), th=3, conn_capacity=10)
    want = CW.walk_scene(update)
    unpoisoned = lambda a: np.where(a == SC.POISON, -1, a).astype(np.int32)
    for k, t in zip(("counter_kf", "counter_w", "ordered_kf", "ordered_w"), blocks):
        assert np.array_equal(t.cpu().numpy(), unpoisoned(want[k])), k
    assert d_kf_result.cpu().numpy().tobytes() == want["result"].tobytes()
    r = want["result"]
    assert (r["n_ordered"] >= 1).all() and (r["status"] == CW.TRUNCATED).any() and (r["n_ordered"] < 10).any() and r["n_ordered"][nF - 1] > 3
    place_want = PW.walk_scene(dict(place, db_covis=unpoisoned(want["ordered_kf"])))
    assert PSC.differences(PSC.download(place, d_place), place_want) == [] and place_want["result"]["status"][0] == PW.OK


@pytest.mark.gpu
def test_gpu_the_chain_from_map_point_update_to_redundancy(ex):
    """orbx_update_map_points_device consumes an observation table, keypoints and counts; the SAME device arrays, unchanged, are the tables
    of orbx_keyframe_redundancy_device, whose subjects are the table's eight keyframes"""
    import torch
    import map_point_update_scenes as MSC
    import test_map_point_update_gpu as MG
    b = MSC.base(False, 34)
    rng, nF, cap = b["rng"], len(b["n_out"]), b["capacity"]
    slots = [list(rng.permutation(int(n))) for n in b["n_out"]]                        # every keypoint holds one MapPoint at most
    points = []
    for m in range(150):
        fr = [int(f) for f in rng.permutation(nF)[:int(rng.integers(0, nF + 1))] if slots[f]]
        points.append(dict(entries=sorted((f, int(slots[f].pop())) for f in fr), ref=0))
    ms = MSC.with_points(b, points, no_flags=True)
    dv = MG.upload(ms)
    out = MG.poisoned(ms)
    rows = np.full((nF, cap), -1, np.int32)
    for m, pt in enumerate(points):
        for f, row in pt["entries"]:
            rows[f, row] = m
    flags = np.zeros(nF, np.uint8)
    flags[0], flags[5] = 2, 1
    s = dict(kind="redundancy", n_points=len(points), obs_off=ms["obs_off"], obs=ms["obs"], mp_flags=np.zeros(len(points), np.uint8), mp_nobs=None,
             n_frames=nF, kf_flags=flags, kps_un=MG.T.keypoints(ms), n_out=ms["n_out"].astype(np.int32), depth=None, th_depth=None, n_subjects=nF,
             subject_mp=rows, subject_n=ms["n_out"].astype(np.int32), capacity=cap, subject_kf=np.arange(nF, dtype=np.int32), monocular=True, th_obs=3,
             redundant_th=np.float32(0.5))
    d, ins = upload(s)
    ins.update(obs_off=dv["obs_off"], obs=dv["obs"], kps_un=dv["kps"], n_out=dv["n_out"])      # the arrays the update consumes
    pointers = [dv[k].data_ptr() for k in ("obs_off", "obs", "kps", "n_out")]
    torch.cuda.synchronize()
    MG.call(ex, ms, dv, 3, out)
    call(ex, s, d, ins)
    ex.synchronize()
    assert pointers == [dv[k].data_ptr() for k in ("obs_off", "obs", "kps", "n_out")] and np.array_equal(dv["obs"].cpu().numpy(), ms["obs"])
    seen = sum(1 for pt in points if pt["entries"])      # (the keyframes run out of free keypoints: the later MapPoints are seen by nobody)
    assert int((out["status"] == 0).sum()) == seen > 40   # the update ran on the table
    want = CW.walk_scene(s)
    assert SC.differences(download(s, d), want) == []
    r = want["result"]
    assert r["status"].tolist() == [CW.RD_SKIPPED] + [CW.RD_OK] * 4 + [CW.RD_SKIPPED] + [CW.RD_OK] * 2 and (r["n_redundant"] > 0).sum() >= 5


@pytest.mark.gpu
def test_gpu_rejections_return_before_any_launch(ex):
    import torch
    s = SC.case("update_frames65_n65")
    o = SC.poisoned_outputs(s)
    d, ins = upload(s)
    torch.cuda.synchronize()
    before = launches(ex)
    bad = [dict(mode=2), dict(mode=-1), dict(n_points=-1), dict(n_frames=0), dict(n_subjects=0), dict(n_subjects=65536), dict(capacity=0),
           dict(conn_capacity=-1), dict(d_obs_off=None), dict(d_obs=None), dict(d_mp_flags=None), dict(d_kf_flags=None), dict(d_kf_key=None),
           dict(d_subject_mp=None), dict(d_subject_n=None), dict(d_result=None), dict(d_kf_map_id=None), dict(d_subject_kf=None),
           dict(d_subject_map_id=None), dict(d_counter_kf=None), dict(d_counter_w=None), dict(d_ordered_kf=None), dict(d_ordered_w=None),
           dict(mode=CW.LOCAL_KEYFRAMES, d_counter_kf=None)]
    for change, code in [(c, -2) for c in bad] + [(dict(n_frames=SC.MAX_FRAMES + 1), -8)]:
        with pytest.raises(X.OrbxError) as err:
            call(ex, s, d, ins, **change)
        assert err.value.code == code, change
    r = SC.case("redundancy_frames65_n65")
    ro = SC.poisoned_outputs(r)
    rd, rins = upload(r)
    torch.cuda.synchronize()
    bad = [dict(n_points=-1), dict(n_frames=0), dict(n_subjects=0), dict(n_subjects=65536), dict(capacity=0), dict(redundant_th=float("nan")),
           dict(d_obs_off=None), dict(d_obs=None), dict(d_mp_flags=None), dict(d_kf_flags=None), dict(d_kps_un=None), dict(d_n_out=None),
           dict(d_subject_mp=None), dict(d_subject_n=None), dict(d_subject_kf=None), dict(d_result=None), dict(monocular=False, d_depth=None),
           dict(monocular=False, d_th_depth=None)]
    for change, code in [(c, -2) for c in bad] + [(dict(capacity=SC.MAX_CAPACITY + 1, n_subjects=1), -8)]:
        with pytest.raises(X.OrbxError) as err:
            call(ex, r, rd, rins, **change)
        assert err.value.code == code, change
    ex.synchronize()
    assert launches(ex) == before
    for outs, poison in ((d, o), (rd, ro)):             # nothing ran: the poison stands
        for k, t in outs.items():
            assert t.cpu().numpy().tobytes()[:poison[k].nbytes] == np.ascontiguousarray(poison[k]).tobytes(), k
