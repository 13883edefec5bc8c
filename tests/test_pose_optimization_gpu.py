"""orbx_optimize_pose_device on the GPU: the scenes of tests/pose_optimization_scenes.py - CASES and the crafted ones - through the C ABI
against the binary64 walk (tests/pose_optimization_walk.py), byte for byte: poses, flag rows, result rows, poison beyond N and on keypoints
without a MapPoint; a non-zero frame_first / frame_step; the handle's stream adopted from torch; two calls back to back on one handle; the
entry's rejections; and the chain - the entry's pose, in place, into orbx_frustum_requests_device on a synthetic local map, and the flag row
applied as the tracker applies it.  The entry has ONE launch form: every accepted call is one launch."""
import numpy as np
import pytest

import extractorb_amd as X
import pose_optimization_scenes as SC
import pose_optimization_walk as PW

ALL = list(SC.CASES) + list(SC.CRAFTED)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda()


def gpu_run(ex, s, keep=None):
    """one call on the scene's arrays; returns the outputs as host arrays shaped like SC.expected's (keep: the device arrays, for a chain)"""
    import torch
    o = SC.poisoned_outputs(s)
    d = dict((k, _dev(v)) for k, v in o.items())
    ins = dict((k, None if s[k] is None else _dev(s[k])) for k in ("problems", "kps", "n_out", "u_right", "matches", "world"))
    torch.cuda.synchronize()                            # torch's copies have landed before the handle's stream runs
    ex.optimize_pose_device(s["n_problems"], (s["first"], s["step"]), ins["problems"], ins["kps"], ins["n_out"], ins["u_right"], s["cap"],
                            ins["matches"], ins["world"], len(s["world"]), d["poses"], d["outlier"], d["result"], eyes=s["eyes"])
    ex.synchronize()
    out = dict((k, v.cpu().numpy()) for k, v in d.items())
    out["result"] = out["result"].view(SC.RESULT_DTYPE).reshape(-1)
    if keep is not None:
        keep.update(d)
    return out


@pytest.fixture(scope="module")
def ex():
    import torch
    torch.zeros(1).cuda()                               # torch asks for the GPU first
    return X.ORBextractor(1000, 1.2, SC.NLEVELS)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_gpu_scene_equals_the_walk(ex, name):
    s = SC.case(name)
    walked, want = SC.case_expected(name)
    before = ex.debug_pose_optimization_launches()
    got = gpu_run(ex, s)
    assert ex.debug_pose_optimization_launches() == before + 1      # the one launch form
    assert SC.differences(got, want) == [], [(a, PW.STATUS[b]) for a, b in zip(got["result"]["status"], want["result"]["status"])]


@pytest.mark.gpu
def test_gpu_two_calls_back_to_back_on_one_handle(ex):
    """no synchronisation between them: the second call's problems are other frames' and both results stand"""
    import torch
    a, b = SC.case("mixed_stereo_batch3"), SC.case("mono_batch17")
    runs = []
    for s in (a, b):
        o = SC.poisoned_outputs(s)
        d = dict((k, _dev(v)) for k, v in o.items())
        ins = dict((k, None if s[k] is None else _dev(s[k])) for k in ("problems", "kps", "n_out", "u_right", "matches", "world"))
        runs.append((s, d, ins))
    torch.cuda.synchronize()
    for s, d, ins in runs:
        ex.optimize_pose_device(s["n_problems"], (s["first"], s["step"]), ins["problems"], ins["kps"], ins["n_out"], ins["u_right"], s["cap"],
                                ins["matches"], ins["world"], len(s["world"]), d["poses"], d["outlier"], d["result"], eyes=s["eyes"])
    ex.synchronize()
    for (s, d, _), name in zip(runs, ("mixed_stereo_batch3", "mono_batch17")):
        got = dict((k, v.cpu().numpy()) for k, v in d.items())
        got["result"] = got["result"].view(SC.RESULT_DTYPE).reshape(-1)
        assert SC.differences(got, SC.case_expected(name)[1]) == [], name


@pytest.mark.gpu
def test_gpu_on_a_stream_adopted_from_torch():
    import torch
    torch.zeros(1).cuda()
    stream = torch.cuda.Stream()
    ex2 = X.ORBextractor(1000, 1.2, SC.NLEVELS)
    s = SC.case("mixed_stereo_first2_step3")
    with torch.cuda.stream(stream):
        ex2.set_stream(torch.cuda.current_stream().cuda_stream)
        got = gpu_run(ex2, s)
    assert SC.differences(got, SC.case_expected("mixed_stereo_first2_step3")[1]) == []


@pytest.mark.gpu
def test_gpu_out_of_range_problems_are_named(ex):
    """N past the capacity, a camera model that is neither, a match outside the MapPoint table, an octave outside the level table:
    BAD_ARGUMENT for that problem alone, nothing of it written but the result row"""
    base = SC.case("mono_batch17")
    s = dict(base, problems=base["problems"].copy(), n_out=base["n_out"].copy(), matches=base["matches"].copy(), kps=base["kps"].copy())
    cap = s["cap"]
    s["n_out"][3] = cap + 1
    s["problems"]["model"][4] = 2
    s["matches"][5 * cap + int(np.nonzero(s["matches"][5 * cap:6 * cap] >= 0)[0][0])] = len(s["world"])
    s["kps"]["octave"][6 * cap + int(np.nonzero(s["matches"][6 * cap:7 * cap] >= 0)[0][0])] = SC.NLEVELS
    s["n_out"][7] = -1
    got, (walked, want) = gpu_run(ex, s), SC.expected(s)
    assert SC.differences(got, want) == []
    assert [PW.STATUS[v] for v in got["result"]["status"][3:8]] == ["BAD_ARGUMENT"] * 5
    assert (got["outlier"][3 * cap:8 * cap] == SC.POISON_FLAG).all() and np.array_equal(got["poses"][3 * 12:8 * 12], s["poses"][3 * 12:8 * 12])
    assert (got["result"]["status"][:3] != PW.BAD_ARGUMENT).all()


@pytest.mark.gpu
def test_gpu_bad_arguments_are_rejected_before_any_launch(ex):
    import torch
    s = SC.case("mixed_stereo_batch3")
    o = SC.poisoned_outputs(s)
    d = dict((k, _dev(v)) for k, v in o.items())
    ins = dict((k, _dev(s[k])) for k in ("problems", "kps", "n_out", "u_right", "matches", "world"))
    torch.cuda.synchronize()
    good = dict(n_problems=3, frames=(0, 1), d_problems=ins["problems"], d_kps=ins["kps"], d_n=ins["n_out"], d_u_right=ins["u_right"], capacity=s["cap"],
                d_matches=ins["matches"], d_mp_world=ins["world"], n_map_points=len(s["world"]), d_poses=d["poses"], d_outlier=d["outlier"],
                d_result=d["result"], eyes=1)
    before = ex.debug_pose_optimization_launches()
    for change in (dict(n_problems=0), dict(capacity=0), dict(eyes=0), dict(eyes=3), dict(eyes=2), dict(frames=(-1, 1)), dict(frames=(1, -1)),
                   dict(n_map_points=-1), dict(d_problems=None), dict(d_kps=None), dict(d_n=None), dict(d_matches=None), dict(d_mp_world=None),
                   dict(d_poses=None), dict(d_outlier=None), dict(d_result=None)):
        with pytest.raises(X.OrbxError) as err:
            ex.optimize_pose_device(**dict(good, **change))
        assert err.value.code == -2, change                 # ORBX_ERR_BAD_ARGUMENT
    ex.synchronize()
    assert ex.debug_pose_optimization_launches() == before
    for k, v in d.items():                              # nothing ran: the poison stands
        assert v.cpu().numpy().tobytes() == np.ascontiguousarray(o[k]).view(np.uint8).tobytes(), k


@pytest.mark.gpu
def test_gpu_the_chain_into_the_frustum_requests_and_the_trackers_use_of_the_flags(ex):
    """TrackLocalMap's order: the pose the entry wrote, IN PLACE, is what orbx_frustum_requests_device reads as d_poses; the requests equal
    those the walk's pose gives.  The flag row, applied as the tracker applies it (an outlier's MapPoint is dropped), leaves the planted
    inliers and drops the planted outliers."""
    import torch
    s = SC.case("mixed_stereo_first2_step3")
    walked, want = SC.case_expected("mixed_stereo_first2_step3")
    keep = {}
    got = gpu_run(ex, s, keep)
    assert SC.differences(got, want) == []
    # a synthetic local map: the scene's own MapPoints, one list for every frame
    P, M = s["n_problems"], len(s["world"])
    rng = np.random.default_rng(7)
    normal = np.tile(np.array([0, 0, 1], np.float32), (M, 1))            # the cameras look along +z, a few degrees off
    dist = np.tile(np.array([0.5, 60.0, 40.0], np.float32), (M, 1))
    desc = rng.integers(0, 256, (M, 32), dtype=np.uint8)
    flags = np.full(P * M, 3, np.uint8)
    cam = X.camera(*SC.PINHOLE[:4])
    bounds = np.array([0, 752, 0, 480], np.float32)

    def requests(d_poses):
        q = torch.zeros(P * M * X.PROJ_QUERY_DTYPE.itemsize, dtype=torch.uint8).cuda()
        qd = torch.zeros(P * M * 32, dtype=torch.uint8).cuda()
        src = torch.zeros(P * M, dtype=torch.int32).cuda()
        nq = torch.zeros(P, dtype=torch.int32).cuda()
        track = torch.zeros(P * M * X.TRACK_RECORD_DTYPE.itemsize, dtype=torch.uint8).cuda()
        nin = torch.zeros(P, dtype=torch.int32).cuda()
        torch.cuda.synchronize()
        ex.frustum_requests_device(P, (s["first"], s["step"]), (0, 0), _dev(s["world"]), _dev(normal), _dev(dist), _dev(desc), None, None, M, _dev(flags),
                                   d_poses, cam, bounds, q, qd, src, nq, track, nin, mode=X.FRUSTUM_LOCAL_MAP, mbf=SC.MBF, view_cos_limit=0.5)
        ex.synchronize()
        return [t.cpu().numpy().tobytes() for t in (q, src, nq, track, nin)], nq.cpu().numpy()
    mine, n_mine = requests(keep["poses"])
    theirs, _ = requests(_dev(want["poses"]))
    assert mine == theirs and (n_mine > 0).all()
    # the tracker: mvpMapPoints[i] = NULL where mvbOutlier[i] (src/Tracking.cc:2336-2360)
    held = s["matches"] >= 0
    left = held & (got["outlier"] == 0)
    assert (left & s["planted"]).sum() == 0                              # no planted outlier survives
    assert (left & ~s["planted"]).sum() >= 0.9 * (held & ~s["planted"]).sum()
