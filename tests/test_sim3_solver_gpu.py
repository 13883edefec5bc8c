"""orbx_sim3_solve_device on the GPU: the scenes of tests/sim3_solver_scenes.py through the C ABI against the binary32 walk
(tests/sim3_solver_walk.py), byte for byte - result rows, flag rows, poison beyond n1 -, a smaller call after a larger one on the same
workspace, the entry's rejections, and one chain into orbx_search_by_projection_sim3_device on a synthetic keyframe."""
import numpy as np
import pytest

import extractorb_amd as X
import sim3_solver_scenes as SC
import sim3_solver_walk as SW


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda()


def gpu_run(ex, s):
    """one call on the scene's arrays; returns the outputs as host arrays shaped like SC.expected's"""
    import torch
    o = SC.poisoned_outputs(s)
    d = dict((k, _dev(v)) for k, v in o.items())
    ins = [_dev(s[k]) for k in ("problems", "x1w", "x2w", "oct1", "oct2", "rand")]
    torch.cuda.synchronize()                            # torch's copies have landed before the handle's stream runs
    ex.sim3_solve_device(len(s["list"]), ins[0], s["cap"], ins[1], ins[2], ins[3], ins[4], ins[5], d["result"], d["inliers"], s["probability"],
                         s["min_inliers"], s["max_iterations"])
    ex.synchronize()
    out = dict((k, v.cpu().numpy()) for k, v in d.items())
    out["result"] = out["result"].view(SC.RESULT_DTYPE).reshape(-1)
    return out


@pytest.fixture(scope="module")
def ex():
    import torch
    torch.zeros(1).cuda()                               # torch asks for the GPU first
    return X.ORBextractor(1000, 1.2, SC.NLEVELS)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SC.CASES))
def test_gpu_scene_equals_the_walk(ex, name):
    s = SC.case(name)
    walked, want = SC.case_expected(name)
    got = gpu_run(ex, s)
    assert SC.differences(got, want) == [], [(a, SW.STATUS[b]) for a, b in zip(got["result"]["status"], want["result"]["status"])]
    for p, pb in enumerate(s["list"]):                  # nothing beyond n1
        assert (got["inliers"][p, pb["n1"]:] == SC.POISON_B).all()


@pytest.mark.gpu
def test_gpu_a_smaller_call_after_a_larger_one_reuses_the_workspace(ex):
    for name in ("n300_it300", "n16_it20", "batch17", "n3_min3_one_iteration", "batch3"):
        assert SC.differences(gpu_run(ex, SC.case(name)), SC.case_expected(name)[1]) == [], name


@pytest.mark.gpu
def test_gpu_other_ransac_parameters_on_the_same_workspace(ex):
    """(probability, min_inliers) change between calls: the table of iteration counts is made again"""
    for prob, mn in ((0.5, 15), (0.99, 10), (0.99, 15)):
        s = dict(SC.case("batch3"), probability=prob, min_inliers=mn)
        got, want = gpu_run(ex, s), SC.expected(s)
        assert SC.differences(got, want) == [], (prob, mn)


@pytest.mark.gpu
def test_gpu_out_of_range_problems_are_named(ex):
    """n1 past the capacity, a negative n1, a model that is neither, an octave outside the table: BAD_ARGUMENT, and no flag of a problem
    whose n1 is out of range is touched"""
    base = SC.case("batch3")
    rows, oct1 = base["problems"].copy(), base["oct1"].copy()
    rows["n1"][0] = base["cap"] + 1
    rows["model2"][1] = 2
    oct1[2, 1] = SC.NLEVELS
    lst = [dict(pb) for pb in base["list"]]
    lst[0]["n1"], lst[1]["model2"], lst[2]["oct1"] = base["cap"] + 1, 2, oct1[2]
    s = dict(base, problems=rows, oct1=oct1, list=lst)
    got, want = gpu_run(ex, s), SC.expected(s)
    assert SC.differences(got, want) == []
    assert (got["result"]["status"] == SW.BAD_ARGUMENT).all() and (got["inliers"][0] == SC.POISON_B).all()
    assert not got["inliers"][1, :lst[1]["n1"]].any()


@pytest.mark.gpu
def test_gpu_the_entry_refuses_bad_arguments(ex):
    import torch
    s = SC.case("n16_it20")
    o = SC.poisoned_outputs(s)
    d = dict((k, _dev(v)) for k, v in o.items())
    ins = [_dev(s[k]) for k in ("problems", "x1w", "x2w", "oct1", "oct2", "rand")]
    torch.cuda.synchronize()
    call = lambda n=1, cap=s["cap"], it=20, prob=0.99, rnd=ins[5]: ex.sim3_solve_device(n, ins[0], cap, ins[1], ins[2], ins[3], ins[4], rnd, d["result"],
                                                                                      d["inliers"], prob, 15, it)
    for kw in (dict(n=0), dict(cap=0), dict(it=0), dict(it=4097), dict(prob=float("nan")), dict(prob=1.5), dict(rnd=None), dict(n=2 ** 20, it=4096)):
        with pytest.raises(X.OrbxError):
            call(**kw)
    ex.synchronize()
    assert (d["inliers"].cpu().numpy() == SC.POISON_B).all()


def chain_problem():
    """one loop candidate at small size: keyframe 2's MapPoints, the current keyframe 1 that sees them under the true Sim3 (scale 1.7) with a
    quarter of the matches wrong, cameras T.CAM; and keyframe 1 as a synthetic keyframe: one level-0 keypoint per correct match at the
    projection of ITS OWN MapPoint, with the descriptor of keyframe 2's MapPoint, in shuffled order"""
    import fuse_walk as W
    import test_fuse as T
    rng = np.random.default_rng(77)
    cap = 64
    pb = SC.problem(rng, 44, cap, outliers=0.25)
    pb["cam1"] = pb["cam2"] = np.array(list(T.CAM) + [0, 0, 0, 0], np.float32)
    s = SC.scene([pb], rng, 300)
    con = SW.construct(pb, SC.NLEVELS)
    uv = SW.project(0, pb["cam1"], con["X1"])
    inside = (uv[:, 0] > 8) & (uv[:, 0] < 632) & (uv[:, 1] > 8) & (uv[:, 1] < 472)
    slots = con["idx1"][inside]
    order = rng.permutation(len(slots))
    kps = np.zeros(len(slots), X.KEYPOINT_DTYPE)
    kps["x"], kps["y"] = uv[inside][order, 0], uv[inside][order, 1]
    mdesc = rng.integers(0, 256, (pb["n1"], 32), dtype=np.uint8)
    off, idx, cell = W.build_grid(kps, T.BOUNDS)
    assert (cell >= 0).all()
    return s, dict(kps=kps, desc=mdesc[slots[order]], slot_of_kp=slots[order], mdesc=mdesc, off=off, idx=idx)


@pytest.mark.gpu
def test_gpu_chain_into_the_sim3_projection_search(ex):
    """SearchByBoW's matches -> Sim3Solver (here) -> gScm * gSmw on the host (LoopClosing.cc:720-723) -> SearchByProjection(pKF, Scw, ..):
    the entry's mBestT12 composed with keyframe 2's pose into Scw, split as the search does (sRcw / scw | tcw / scw, ORBmatcher.cc:481-487),
    goes into orbx_search_by_projection_sim3_device with keyframe 2's MapPoints; every correspondence the solver flagged comes back as a match
    of its own keypoint, and no keypoint is matched to another MapPoint"""
    import torch
    import test_fuse as T
    import test_sim3_projection as P
    s, k = chain_problem()
    pb = s["list"][0]
    got = gpu_run(ex, s)
    assert SC.differences(got, SC.expected(s)) == []
    r = got["result"][0]
    assert r["status"] == SW.CONVERGED and abs(float(r["scale"]) - SC.TRUE_SCALE) < 0.02
    # gScw = gScm * gSmw, then the search's own split
    Scm = r["T12"].reshape(4, 4).astype(np.float64)
    Smw = np.vstack([pb["Tcw2"].reshape(3, 4).astype(np.float64), [0, 0, 0, 1]])
    Scw = Scm @ Smw
    scw = np.sqrt(Scw[0, :3] @ Scw[0, :3])
    pose = np.hstack([Scw[:3, :3] / scw, Scw[:3, 3:4] / scw]).astype(np.float32)
    n1 = pb["n1"]
    world = pb["x2w"][:n1]
    Ow = -pose[:, :3].T.astype(np.float64) @ pose[:, 3].astype(np.float64)
    d = np.linalg.norm(world - Ow, axis=1).astype(np.float32)
    mps = dict(world=world, normal=((world - Ow) / d[:, None]).astype(np.float32), dist=np.stack([np.zeros_like(d), np.full_like(d, 1e9), d], axis=1),
               desc=k["mdesc"])
    kf = dict(pose=pose, kps=k["kps"], ur=None, desc=k["desc"], grid_off=k["off"], grid_idx=k["idx"])
    case = dict(scene=dict(kfs=[kf], lists=[mps]), pairs=[dict(kf=0, lst=0, pose=pose, flags=np.ones(n1, np.uint8), occupied=None)], kf=(0, 1), mp=(0, 0))
    a = P.pack(case)
    dv = dict((key, _dev(v)) for key, v in a.items() if isinstance(v, np.ndarray))
    d_m = torch.full((1, a["cap"]), -7, dtype=torch.int32, device="cuda")
    d_mi = torch.full((1, a["mp_cap"]), -7, dtype=torch.int32, device="cuda"); d_md = d_mi.clone()
    d_nm = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ex.search_by_projection_sim3_device(1, (0, 1), (0, 0), dv["world"], dv["normal"], dv["dist"], dv["mdesc"], None, a["mp_cap"], dv["flags"], dv["poses"],
                                        dv["kps"], dv["desc"], dv["nout"], a["cap"], dv["off"], dv["idx"], T.BOUNDS, X.camera(*T.CAM), None, d_m, d_mi, d_md,
                                        None, d_nm, projection=0, **P.CALLERS["kf_window"])
    ex.synchronize()
    matches = d_m.cpu().numpy()[0][:len(k["kps"])]
    flagged = got["inliers"][0][:n1] == 1
    wanted = [(j, slot) for j, slot in enumerate(k["slot_of_kp"]) if flagged[slot]]
    assert len(wanted) > 15 and all(matches[j] == slot for j, slot in wanted), (matches, wanted)
    assert all(m == -1 or m == slot for m, slot in zip(matches, k["slot_of_kp"])) and int(d_nm.cpu().numpy()[0]) == int((matches >= 0).sum()) >= len(wanted)
