"""orbx_frustum_requests_device against the sequential walk (tests/frustum_walk.py) on the scenes of tests/frustum_scenes.py: requests,
descriptors, sources, counts and the bytes of every track record exactly; the outputs are poisoned first, and the descriptor slots past the
requests must still hold the poison.  tests/test_frustum_requests.py (c) runs the per-MapPoint header, compiled for the host, against the same
walks; the compaction (ballots, the scan across the waves, the running base) is covered here alone."""
import numpy as np
import pytest

import extractorb_amd as X
import frustum_scenes as S
import frustum_walk as W

f32 = np.float32
POISON8 = 0xA5
TAB = W.tables(*S.SETTING)


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda()


def upload(lists, mp_cap, angles=None):
    NL = len(lists)
    a = dict(world=np.zeros((NL, mp_cap, 3), f32), normal=np.zeros((NL, mp_cap, 3), f32), dist=np.zeros((NL, mp_cap, 3), f32),
             desc=np.zeros((NL, mp_cap, 32), np.uint8), angle=np.zeros((NL, mp_cap), f32))
    for l, m in enumerate(lists):
        n = len(m["world"])
        for k in ("world", "normal", "dist", "desc"):
            a[k][l, :n] = m[k]
        if angles is not None:
            a["angle"][l, :n] = angles[l]
    return dict((k, _dev(v)) for k, v in a.items())


def run(ex, dv, flags, poses, mp_cap, cur, mp, mode, cam, n_mp=None, normal=True, angle=True, **opt):
    """flags [P, mp_cap]; returns dict(queries [P, mp_cap], desc, src, n_queries [P], track, n_in_view [P]) as numpy"""
    import torch
    P = len(flags)
    d_q = torch.full((P, mp_cap, 32), POISON8, dtype=torch.uint8, device="cuda"); d_qd = torch.full((P, mp_cap, 32), POISON8, dtype=torch.uint8, device="cuda")
    d_src = torch.full((P, mp_cap), -7, dtype=torch.int32, device="cuda"); d_tr = torch.full((P, mp_cap, 28), POISON8, dtype=torch.uint8, device="cuda")
    d_nq = torch.full((P,), -7, dtype=torch.int32, device="cuda"); d_nin = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    d_fl = _dev(np.asarray(flags, np.uint8)); d_poses = _dev(np.asarray(poses, f32).reshape(-1, 12))
    d_nmp = None if n_mp is None else _dev(np.asarray(n_mp, np.int32))
    torch.cuda.synchronize()                            # torch's copies and fills have landed before the handle's stream runs
    ex.frustum_requests_device(P, cur, mp, dv["world"], dv["normal"] if normal else None, dv["dist"], dv["desc"], dv["angle"] if angle else None, d_nmp,
                               mp_cap, d_fl, d_poses, X.camera(*cam), S.BOUNDS, d_q, d_qd, d_src, d_nq, d_tr, d_nin, mode=mode, mbf=S.MBF, **opt)
    ex.synchronize()
    return dict(queries=d_q.cpu().numpy().reshape(P, -1).view(X.PROJ_QUERY_DTYPE), desc=d_qd.cpu().numpy(), src=d_src.cpu().numpy(),
                n_queries=d_nq.cpu().numpy(), track=d_tr.cpu().numpy().reshape(P, -1).view(X.TRACK_RECORD_DTYPE), n_in_view=d_nin.cpu().numpy(),
                dev=dict(queries=d_q, desc=d_qd, n_queries=d_nq))


def assert_pair(got, p, want, what):
    """pair p of a device result against a walk over a list of len(want['track']) <= mp_capacity entries"""
    m, n = len(want["track"]), want["n_queries"]
    cap = got["track"].shape[1]
    assert int(got["n_queries"][p]) == n and int(got["n_in_view"][p]) == want["n_in_view"], what
    assert got["track"][p, :m].tobytes() == want["track"].tobytes(), what
    rest = got["track"][p, m:]
    assert (rest["exit"] == 0).all() and (rest["proj_x"] == -1).all() and (rest["level"] == -1).all() and (rest["depth"] == 0).all(), what
    assert got["queries"][p, :n].tobytes() == want["queries"][:n].tobytes() and got["queries"][p, n:].tobytes() == bytes(32 * (cap - n)), what
    assert np.array_equal(got["src"][p, :n], want["src"][:n]) and (got["src"][p, n:] == -1).all(), what
    assert np.array_equal(got["desc"][p, :n], want["desc"]) and (got["desc"][p, n:] == POISON8).all(), what


def extractor(setting=S.SETTING):
    return X.ORBextractor(1000, setting[0], setting[1])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [W.LOCAL_MAP, W.RELOCALIZATION])
def test_gpu_crafted_points_in_both_modes(mode):
    """every comparison of the statement, on it and one float beside it; th == 1 and th != 1; with and without bFarPoints; twice, same bytes"""
    pts = S.crafted()
    mps, flags, angle = S.crafted_arrays(pts)
    ex = extractor()
    n = len(flags)
    dv = upload([mps], n, [angle])
    for th, far in ((1.0, True), (1.5, True), (1.0, False)) if mode == W.LOCAL_MAP else ((15.0, True),):
        opt = dict(th=th, far_points=far, th_far_points=S.TH_FAR)
        got = run(ex, dv, flags[None], S.IDENTITY, n, (0, 1), (0, 1), mode, S.CAM_CRAFTED, normal=mode == 0, angle=mode == 1, **opt)
        want = W.walk(mps, flags, S.IDENTITY, S.CAM_CRAFTED, S.BOUNDS, TAB, mode=mode, mbf=S.MBF, angle=angle, **opt)
        print("mode %d th %.1f far %d: exits %s" % (mode, th, far, np.bincount(want["track"]["exit"], minlength=7).tolist()))
        assert_pair(got, 0, want, (mode, th, far))
        if th == 1.0 and far or mode == 1:
            for i, p in enumerate(pts):
                assert int(got["track"]["exit"][0, i]) == p["want%d" % mode], p["name"]
        again = run(ex, dv, flags[None], S.IDENTITY, n, (0, 1), (0, 1), mode, S.CAM_CRAFTED, **opt)      # the unread pointers given: no difference
        assert all(got[k].tobytes() == again[k].tobytes() for k in ("queries", "desc", "src", "n_queries", "track", "n_in_view"))


@pytest.mark.gpu
def test_gpu_list_lengths_at_the_wave_and_chunk_edges():
    """0, 1, 63, 64, 65, 1023, 1024, 1025 and 2049 entries inside mp_capacity 2304 (three chunks of 1024 threads, the last one partial), one
    list per length and one pose for all; then d_n_mp NULL.  Flags are set on the whole capacity: d_n_mp alone must stop the walk."""
    lengths = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049]
    cap = 2304
    mps, flags, _ = S.uniform_scene(3, cap, box=((-1.5, 1.5), (-1, 1), (2, 8)), noise=0.3)      # most in view: dense requests on both sides of every edge
    flags |= 1
    ex = extractor()
    dv = upload([mps] * len(lengths), cap)
    full = W.walk(mps, flags, S.POSES[0], S.CAM, S.BOUNDS, TAB, mbf=S.MBF)
    assert full["n_queries"] > 600
    got = run(ex, dv, np.tile(flags, (len(lengths), 1)), S.POSES[:1], cap, (0, 0), (0, 1), 0, S.CAM, n_mp=lengths, angle=False)
    for p, n in enumerate(lengths):
        assert_pair(got, p, W.truncate(full, n, mps), "length %d" % n)
    got = run(ex, dv, flags[None], S.POSES[:1], cap, (0, 0), (3, 1), 0, S.CAM, n_mp=None, angle=False)
    assert_pair(got, 0, full, "d_n_mp NULL")
    got = run(ex, dv, np.tile(flags, (2, 1)), S.POSES[:1], cap, (0, 0), (0, 1), 0, S.CAM, n_mp=[cap + 77, -3] + [0] * 7, angle=False)      # clamped
    assert_pair(got, 0, full, "count above the capacity")
    assert_pair(got, 1, W.truncate(full, 0, mps), "negative count")


@pytest.mark.gpu
def test_gpu_three_pairs_with_every_step_combination():
    """n_pairs = 3, mp_step and cur_step 0 and 1 (and -1 from the last frame), three distinct poses, flags that differ per pair, both modes"""
    n = 1100
    scenes = [S.uniform_scene(20 + l, n, pose_index=l) for l in range(3)]
    lists = [s[0] for s in scenes]; angles = [s[2] for s in scenes]
    rng = np.random.default_rng(4)
    flags = rng.integers(0, 4, (3, n)).astype(np.uint8) | np.stack([s[1] for s in scenes]) & 1
    ex = extractor()
    dv = upload(lists, n, angles)
    walks = {}
    for cur, mp, mode in [((0, 1), (0, 0), 0), ((0, 0), (0, 1), 0), ((0, 1), (0, 1), 1), ((2, -1), (0, 1), 0), ((1, 0), (2, 0), 1)]:
        got = run(ex, dv, flags, S.POSES, n, cur, mp, mode, S.CAM, th=1.0 if mode == 0 else 15.0, far_points=True, th_far_points=8.0)
        for p in range(3):
            f, l = cur[0] + p * cur[1], mp[0] + p * mp[1]
            key = (f, l, p, mode)
            if key not in walks:
                walks[key] = W.walk(lists[l], flags[p], S.POSES[f], S.CAM, S.BOUNDS, TAB, mode=mode, mbf=S.MBF, th=1.0 if mode == 0 else 15.0,
                                    far_points=True, th_far_points=8.0, angle=angles[l])
            assert_pair(got, p, walks[key], (cur, mp, mode, p))
    assert len(set(w["n_queries"] for w in walks.values())) > 3


@pytest.mark.gpu
def test_gpu_requests_feed_the_local_map_search_as_they_are():
    """mode 0 on a local map aimed at a synthetic frame, fed straight into search_by_projection_device (ratio_mode = 1); d_matches must equal
    the same search fed with the walk's host-built arrays, and d_query_src maps every match to its list index"""
    import torch
    import test_search_projection as SP
    rng = np.random.default_rng(12)
    frame = SP.random_scene(rng, n=900, nq=4, ratio=True)
    cam = (SP.CAM["fx"], SP.CAM["fy"], SP.CAM["cx"], SP.CAM["cy"])
    T = S.POSES[0]
    n, cap = 1500, 1024
    mps, flags = S.map_for_frame(rng, frame, T, n, cam)
    want = W.walk(mps, flags, T, cam, S.BOUNDS, TAB, mbf=S.MBF, th=3.0, far_points=True, th_far_points=8.0)
    assert 300 < want["n_queries"] < n - 300 and want["n_in_view"] > want["n_queries"]
    ex = extractor()
    got = run(ex, upload([mps], n), flags[None], T, n, (0, 1), (0, 1), 0, cam, angle=False, th=3.0, far_points=True, th_far_points=8.0)
    assert_pair(got, 0, want, "map for the frame")
    fr = SP._frames_to_device([dict(un=frame["un"], d=frame["d"], off=frame["off"], idx=frame["idx"])], cap)
    ur = np.full((1, cap), -1.0, f32); ur[0, :len(frame["ur"])] = frame["ur"]
    occ = np.zeros((1, cap), np.uint8); occ[0, :len(frame["occ"])] = frame["occ"]
    qd_host = np.zeros((1, n, 32), np.uint8); qd_host[0, :want["n_queries"]] = want["desc"]
    results = []
    for q, qd, nq in ((got["dev"]["queries"], got["dev"]["desc"], got["dev"]["n_queries"]),
                      (_dev(want["queries"][None]), _dev(qd_host), _dev(np.array([want["n_queries"]], np.int32)))):
        d_m = torch.full((1, cap), -7, dtype=torch.int32, device="cuda"); d_nm = torch.zeros(1, dtype=torch.int32, device="cuda")
        d_occ = _dev(occ)
        torch.cuda.synchronize()
        ex.search_by_projection_device(1, (0, 1), q, qd, (0, 1), nq, n, fr["un"], fr["d"], fr["n"], cap, fr["off"], fr["idx"], S.BOUNDS, _dev(ur), d_occ,
                                       True, 0.8, False, d_m, d_nm)
        ex.synchronize()
        results.append((d_m.cpu().numpy()[0], int(d_nm[0]), d_occ.cpu().numpy()[0]))
    (m_dev, n_dev, occ_dev), (m_host, n_host, occ_host) = results
    print("%d requests of %d MapPoints, %d in view, %d matches" % (want["n_queries"], n, want["n_in_view"], n_dev))
    assert np.array_equal(m_dev, m_host) and n_dev == n_host and np.array_equal(occ_dev, occ_host) and n_dev > 100
    hit = m_dev[m_dev >= 0]
    assert (hit < want["n_queries"]).all()
    idx = got["src"][0][hit]                                # vpMapPoints[d_query_src[d_matches[i2]]]
    assert np.array_equal(idx, want["src"][hit]) and (want["track"]["exit"][idx] == W.EXIT_REQUEST).all() and len(set(idx.tolist())) == len(idx)


@pytest.mark.gpu
def test_gpu_a_second_handle_with_twelve_levels_of_1_1():
    setting = (1.1, 12)
    tab = W.tables(*setting)
    mps, flags, angle = S.uniform_scene(8, 700)
    ex = extractor(setting)
    got = run(ex, upload([mps], 700, [angle]), flags[None], S.POSES[1], 700, (0, 1), (0, 1), 0, S.CAM)
    want = W.walk(mps, flags, S.POSES[1], S.CAM, S.BOUNDS, tab, mbf=S.MBF)
    assert_pair(got, 0, want, "1.1 x 12")
    assert want["track"]["level"].max() > 8


@pytest.mark.gpu
def test_gpu_argument_errors_are_rejected_before_any_launch():
    import torch
    ex = extractor()
    z = torch.zeros(8192, dtype=torch.int32, device="cuda")
    outs = [torch.full((1024,), -7, dtype=torch.int32, device="cuda") for _ in range(6)]
    torch.cuda.synchronize()
    ex.profile(True)
    good = dict(n_pairs=1, cur=(0, 1), mp=(0, 0), d_mp_world=z, d_mp_normal=z, d_mp_dist=z, d_mp_desc=z, d_mp_angle=z, d_n_mp=None, mp_capacity=16,
                d_mp_flags=z, d_poses=z, cam=X.camera(*S.CAM), bounds=S.BOUNDS, d_queries=outs[0], d_query_desc=outs[1], d_query_src=outs[2],
                d_n_queries=outs[3], d_track=outs[4], d_n_in_view=outs[5])
    bad = [dict(n_pairs=0), dict(n_pairs=-1), dict(cur=(-1, 1)), dict(mp=(-1, 0)), dict(n_pairs=3, cur=(1, -1)), dict(n_pairs=3, mp=(1, -1)),
           dict(mp_capacity=0), dict(mp_capacity=-1), dict(nlevels=7), dict(nlevels=12), dict(mode=2), dict(mode=-1), dict(bounds=None), dict(cam=None),
           dict(d_mp_normal=None, mode=0), dict(d_mp_angle=None, mode=1)]
    bad += [dict([(k, None)]) for k in ("d_mp_world", "d_mp_dist", "d_mp_desc", "d_mp_flags", "d_poses", "d_queries", "d_query_desc", "d_query_src",
                                       "d_n_queries", "d_track", "d_n_in_view")]
    for change in bad:
        with pytest.raises(X.OrbxError) as e:
            ex.frustum_requests_device(**dict(good, **change))
        assert e.value.code == -2, change
    ex.synchronize()
    assert all((o == -7).all() for o in outs)
    assert sum(v[1] for v in ex.profile_read().values()) == 0      # nothing was launched
    for change in (dict(d_mp_angle=None, mode=0), dict(d_mp_normal=None, mode=1)):      # what a mode does not read may be NULL
        ex.frustum_requests_device(**dict(good, **change))
    ex.synchronize()
    assert int(outs[3][0]) == 0 and int(outs[5][0]) == 0 and (outs[2][:16] == -1).all() and (outs[2][16:] == -7).all()
    assert (outs[0][:16 * 8] == 0).all() and (outs[0][16 * 8:] == -7).all() and (outs[1] == -7).all()
    assert sum(v[1] for v in ex.profile_read().values()) == 2
