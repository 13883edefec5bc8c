"""orbx_frustum_requests_two_eyes_device against the sequential walk (tests/frustum_two_eyes_walk.py, host libm) on the scenes of
tests/frustum_two_eyes_scenes.py: both track records of every list entry, the two requests, the descriptor and the source of every slot and
the three counts, by bytes; the outputs are poisoned first, and the descriptor slots past the written ones must still hold the poison.
tests/test_frustum_requests_two_eyes.py (d) runs the per-MapPoint header, compiled for the host, against the same walks; the lane pairs, the
per-workgroup counts and the placement (256 MapPoints per workgroup, 32 per wave) are covered here alone."""
import numpy as np
import pytest

import extractorb_amd as X
import frustum_two_eyes_scenes as S
import frustum_two_eyes_walk as W

f32, f64 = np.float32, np.float64
POISON8 = 0xA5
TAB = W.tables(*S.SETTING)
_cache = {}


def libm():
    return _cache.setdefault("libm", W.libm_math())


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda()


def upload(lists, mp_cap):
    NL = len(lists)
    a = dict(world=np.zeros((NL, mp_cap, 3), f32), normal=np.zeros((NL, mp_cap, 3), f32), dist=np.zeros((NL, mp_cap, 3), f32),
             desc=np.zeros((NL, mp_cap, 32), np.uint8))
    for l, m in enumerate(lists):
        n = len(m["world"])
        for k in a:
            a[k][l, :n] = m[k]
    return dict((k, _dev(v)) for k, v in a.items())


def run(ex, dv, flags, prev, poses, rig, mp_cap, cur, mp, n_mp=None, qcap=None, guard=1, cams=S.CAMS, wanted=True, **opt):
    """flags [P, mp_cap], prev [P, mp_cap] or None; the outputs have `guard` more pair blocks than the call writes.  Returns numpy arrays."""
    import torch
    P = len(flags)
    qcap = mp_cap if qcap is None else qcap
    B = P + guard
    d_q = torch.full((B, qcap, 2, 32), POISON8, dtype=torch.uint8, device="cuda"); d_qd = torch.full((B, qcap, 32), POISON8, dtype=torch.uint8, device="cuda")
    d_src = torch.full((B, qcap), -7, dtype=torch.int32, device="cuda"); d_tr = torch.full((B, mp_cap, 2, 28), POISON8, dtype=torch.uint8, device="cuda")
    d_nq, d_nw, d_nin = (torch.full((B,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    d_fl = _dev(np.asarray(flags, np.uint8)); d_poses = _dev(np.asarray(poses, f32).reshape(-1, 12))
    d_prev = None if prev is None else _dev(np.asarray(prev, f32))
    d_nmp = None if n_mp is None else _dev(np.asarray(n_mp, np.int32))
    torch.cuda.synchronize()                            # torch's copies and fills have landed before the handle's stream runs
    ex.frustum_requests_two_eyes_device(P, cur, mp, dv["world"], dv["normal"], dv["dist"], dv["desc"], d_nmp, mp_cap, d_fl, d_prev, d_poses, rig["trl"],
                                        rig["tlr"], cams[0], cams[1], S.BOUNDS, qcap, d_q, d_qd, d_src, d_nq, d_nw if wanted else None, d_tr, d_nin, **opt)
    ex.synchronize()
    return dict(queries=d_q.cpu().numpy().reshape(B, qcap, 2, 32).view(X.PROJ_QUERY_DTYPE)[..., 0], desc=d_qd.cpu().numpy(), src=d_src.cpu().numpy(),
                n_queries=d_nq.cpu().numpy(), n_wanted=d_nw.cpu().numpy(), track=d_tr.cpu().numpy().view(X.TRACK_RECORD_DTYPE)[..., 0],
                n_in_view=d_nin.cpu().numpy(), pairs=P, dev=dict(queries=d_q, desc=d_qd, n_queries=d_nq))


def assert_guard(got):
    """nothing past the blocks of the call's pairs is written"""
    P = got["pairs"]
    assert (got["queries"][P:].view(np.uint8) == POISON8).all() and (got["desc"][P:] == POISON8).all() and (got["src"][P:] == -7).all()
    assert (got["track"][P:].view(np.uint8) == POISON8).all()
    assert (got["n_queries"][P:] == -7).all() and (got["n_wanted"][P:] == -7).all() and (got["n_in_view"][P:] == -7).all()


def assert_pair(got, p, want, what, wanted=True):
    """pair p of a device result against a walk over a list of len(want['track']) <= mp_capacity entries with the same query capacity"""
    m, n = len(want["track"]), want["n_queries"]
    qcap = got["queries"].shape[1]
    assert int(got["n_queries"][p]) == n and int(got["n_in_view"][p]) == want["n_in_view"], what
    assert int(got["n_wanted"][p]) == (want["n_wanted"] if wanted else -7), what
    assert got["track"][p, :m].tobytes() == want["track"].tobytes(), what
    rest = got["track"][p, m:]
    assert (rest["exit"] == 0).all() and (rest["proj_x"] == -1).all() and (rest["proj_y"] == -1).all() and (rest["level"] == -1).all(), what
    assert (rest["depth"] == 0).all() and (rest["view_cos"] == 0).all() and (rest["proj_xr"] == 0).all(), what
    assert got["queries"][p, :n].tobytes() == want["queries"][:n].tobytes() and got["queries"][p, n:].tobytes() == bytes(64 * (qcap - n)), what
    assert np.array_equal(got["src"][p, :n], want["src"][:n]) and (got["src"][p, n:] == -1).all(), what
    assert np.array_equal(got["desc"][p, :n], want["desc"]) and (got["desc"][p, n:] == POISON8).all(), what


def extractor(setting=S.SETTING):
    return X.ORBextractor(1000, setting[0], setting[1])


def same_bytes(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in ("queries", "desc", "src", "n_queries", "n_wanted", "track", "n_in_view"))


@pytest.mark.gpu
@pytest.mark.parametrize("rig_name", ["narrow", "wide"])
def test_gpu_crafted_points_of_both_rigs(rig_name):
    """every comparison of the statement in each eye, on its two sides; th == 1 and th != 1; with and without bFarPoints; d_mp_prev_depth given
    and NULL; each twice, same bytes"""
    pts = S.crafted(rig_name)
    mps, flags, prev = S.crafted_arrays(rig_name)
    rig = S.RIGS[rig_name]
    ex = extractor()
    n = len(flags)
    dv = upload([mps], n)
    slots = set()
    for th, far, with_prev in ((1.0, True, True), (1.5, True, True), (1.0, False, True), (1.0, True, False), (1.5, False, False)):
        opt = dict(th=th, far_points=far, th_far_points=S.TH_FAR)
        pv = prev if with_prev else None
        got = run(ex, dv, flags[None], None if pv is None else pv[None], S.POSE, rig, n, (0, 1), (0, 1), **opt)
        want = W.walk(libm(), mps, flags, S.POSE, rig["trl"], rig["tlr"], S.CAMS, S.BOUNDS, TAB, prev_depth=pv, **opt)
        print("%s th %.1f far %d prev %d: %d slots, %d in view, exits L %s R %s" % (
            rig_name, th, far, with_prev, want["n_queries"], want["n_in_view"], np.bincount(want["track"]["exit"][:, 0], minlength=7).tolist(),
            np.bincount(want["track"]["exit"][:, 1], minlength=7).tolist()))
        assert_pair(got, 0, want, (th, far, with_prev)); assert_guard(got)
        slots.add(want["n_queries"])
        if th == 1.0 and far and with_prev:
            for i, p in enumerate(pts):
                ex_i = tuple(int(v) for v in got["track"]["exit"][0, i])
                assert (ex_i == tuple(p["want"])) if p["eye"] is None else (ex_i[p["eye"]] == p["want"]), p["name"]
        assert same_bytes(got, run(ex, dv, flags[None], None if pv is None else pv[None], S.POSE, rig, n, (0, 1), (0, 1), **opt))
    assert len(slots) >= (3 if rig_name == "wide" else 2)      # far and, on the wide rig, the earlier depth of a right-only point change the count


def dense_scene(seed, n):
    """most MapPoints in view of both eyes, near: dense slots on both sides of every edge"""
    mps, flags, prev = S.uniform_scene(seed, n, box=((-1.5, 1.5), (-1, 1), (1.0, 6)), noise=0.3)
    return mps, flags | 1, prev


@pytest.mark.gpu
def test_gpu_list_lengths_at_the_wave_and_workgroup_edges():
    """a wave holds 32 MapPoints (one lane pair each), a workgroup 256: 0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257 and 1025 entries inside
    mp_capacity 1280 (five workgroups), one list per length and one pose for all; then d_n_mp NULL, a count above the capacity and a negative
    one.  Flags are set on the whole capacity: d_n_mp alone must stop the walk."""
    lengths = [0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1025]
    cap = 1280
    mps, flags, prev = dense_scene(3, cap)
    rig = S.RIGS["narrow"]
    ex = extractor()
    dv = upload([mps] * len(lengths), cap)
    opt = dict(far_points=True, th_far_points=5.0)
    full = W.walk(libm(), mps, flags, S.POSE, rig["trl"], rig["tlr"], S.CAMS, S.BOUNDS, TAB, prev_depth=prev, **opt)
    assert full["n_queries"] > 500 and full["n_in_view"] > full["n_queries"]
    P = len(lengths)
    got = run(ex, dv, np.tile(flags, (P, 1)), np.tile(prev, (P, 1)), S.POSE, rig, cap, (0, 0), (0, 1), n_mp=lengths, **opt)
    for p, n in enumerate(lengths):
        assert_pair(got, p, W.truncate(full, n, mps), "length %d" % n)
    assert_guard(got)
    got = run(ex, dv, flags[None], prev[None], S.POSE, rig, cap, (0, 0), (3, 1), n_mp=None, **opt)
    assert_pair(got, 0, full, "d_n_mp NULL")
    got = run(ex, dv, np.tile(flags, (2, 1)), np.tile(prev, (2, 1)), S.POSE, rig, cap, (0, 0), (0, 1), n_mp=[cap + 77, -3] + [0] * (P - 2), **opt)      # clamped
    assert_pair(got, 0, full, "count above the capacity")
    assert_pair(got, 1, W.truncate(full, 0, mps), "negative count")


@pytest.mark.gpu
def test_gpu_three_pairs_with_every_step_combination():
    """n_pairs = 3, mp_step and cur_step 0 and 1 (and -1 from the last rig frame), three distinct poses, flags and earlier depths per pair"""
    n = 600
    scenes = [S.uniform_scene(20 + l, n, box=((-5, 5), (-5, 5), (-1, 5)), pose=S.POSES[l]) for l in range(3)]
    lists = [s[0] for s in scenes]
    rng = np.random.default_rng(4)
    flags = rng.integers(0, 4, (3, n)).astype(np.uint8) | np.stack([s[1] for s in scenes]) & 1
    prev = np.stack([s[2] for s in scenes])
    rig = S.RIGS["wide"]
    ex = extractor()
    dv = upload(lists, n)
    opt = dict(th=1.5, far_points=True, th_far_points=5.0)
    walks = {}
    for cur, mp in [((0, 1), (0, 0)), ((0, 0), (0, 1)), ((0, 1), (0, 1)), ((2, -1), (0, 1)), ((1, 0), (2, -1))]:
        got = run(ex, dv, flags, prev, S.POSES, rig, n, cur, mp, **opt)
        for p in range(3):
            f, l = cur[0] + p * cur[1], mp[0] + p * mp[1]
            key = (f, l, p)
            if key not in walks:
                walks[key] = W.walk(libm(), lists[l], flags[p], S.POSES[f], rig["trl"], rig["tlr"], S.CAMS, S.BOUNDS, TAB, prev_depth=prev[p], **opt)
            assert_pair(got, p, walks[key], (cur, mp, p))
        assert_guard(got)
    assert len(set(w["n_queries"] for w in walks.values())) > 3


@pytest.mark.gpu
def test_gpu_query_capacity_below_the_produced_count():
    """two pairs, the first produces more slots than query_capacity holds: its first query_capacity slots are the walk's, d_n_queries is the
    capacity, d_n_wanted the walk's count, and nothing past a pair's block is written (pair 1's block follows pair 0's; a guard block follows
    both).  d_n_wanted = NULL changes nothing else."""
    cap, qcap = 700, 96
    mps, flags, prev = dense_scene(5, cap)
    sparse = flags.copy(); sparse[40:] &= 2
    rig = S.RIGS["wide"]
    ex = extractor()
    dv = upload([mps], cap)
    want = [W.walk(libm(), mps, fl, S.POSE, rig["trl"], rig["tlr"], S.CAMS, S.BOUNDS, TAB, prev_depth=prev, query_capacity=qcap) for fl in (flags, sparse)]
    assert want[0]["n_wanted"] > 3 * qcap and want[0]["n_queries"] == qcap and 0 < want[1]["n_wanted"] == want[1]["n_queries"] < qcap
    got = run(ex, dv, np.stack([flags, sparse]), np.stack([prev, prev]), S.POSE, rig, cap, (0, 0), (0, 0), qcap=qcap)
    for p in (0, 1):
        assert_pair(got, p, want[p], "pair %d" % p)
    assert_guard(got)
    again = run(ex, dv, np.stack([flags, sparse]), np.stack([prev, prev]), S.POSE, rig, cap, (0, 0), (0, 0), qcap=qcap, wanted=False)
    for p in (0, 1):
        assert_pair(again, p, want[p], "pair %d without d_n_wanted" % p, wanted=False)
    got = run(ex, dv, flags[None], prev[None], S.POSE, rig, cap, (0, 0), (0, 0), qcap=1)
    assert int(got["n_queries"][0]) == 1 and int(got["n_wanted"][0]) == want[0]["n_wanted"] and got["queries"][0, 0].tobytes() == want[0]["queries"][0].tobytes()


@pytest.mark.gpu
def test_gpu_a_second_handle_with_twelve_levels_of_1_1():
    setting = (1.1, 12)
    tab = W.tables(*setting)
    mps, flags, prev = S.uniform_scene(8, 500)
    rig = S.RIGS["narrow"]
    ex = extractor(setting)
    got = run(ex, upload([mps], 500), flags[None], prev[None], S.POSES[1], rig, 500, (0, 1), (0, 1))
    want = W.walk(libm(), mps, flags, S.POSES[1], rig["trl"], rig["tlr"], S.CAMS, S.BOUNDS, tab, prev_depth=prev)
    assert_pair(got, 0, want, "1.1 x 12")
    assert want["track"]["level"].max() > 8


def frame_and_map(rng, rig, pose, n, extra=120):
    """A two-eye frame and a local map aimed at it (the method of tests/frustum_scenes.map_for_frame, adapted: KannalaBrandt8 has no
    closed-form ray, so the MapPoints come first and each eye's keypoints sit on their projections, a few pixels off, with a descriptor a few
    bits away and the octave the MapPoint's mfMaxDistance predicts; a share lies behind the rig, outside the images or is seen from the side).
    The eyes and grids are those of tests/test_search_projection_two_eyes.py."""
    import oracle_lib as O
    import test_search_projection_two_eyes as SP
    m = libm()
    T = np.asarray(pose, f64)
    xc = np.stack([rng.uniform(-5, 5, n), rng.uniform(-5, 5, n), rng.uniform(-1.0, 7.0, n)], 1)
    world = ((xc - T[:, 3]) @ T[:, :3]).astype(f32)          # Rcw.t() * (xc - tcw), row by row
    PO = world.astype(f64) - (-T[:, :3].T @ T[:, 3])
    dd = np.linalg.norm(PO, axis=1)
    nrm = PO / dd[:, None] + rng.standard_normal((n, 3)) * np.where(rng.random(n) < 0.25, 0.9, 0.05)[:, None]
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    lvl = rng.integers(0, 8, n)
    mf = dd * 1.2 ** (lvl - 0.5)
    dist = np.stack([0.8 * mf / 1.2 ** 7, 1.2 * mf, mf], 1).astype(f32)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    mps = dict(world=world.astype(f32), normal=nrm.astype(f32), dist=dist, desc=desc)
    flags = ((rng.random(n) < 0.93).astype(np.uint8) | ((rng.random(n) < 0.85).astype(np.uint8) << 1)).astype(np.uint8)
    halves = []
    for e in (0, 1):
        Te = S.eye_pose64(rig, e, pose)
        xs, ys, octs, ds = [], [], [], []
        for i in range(n):
            pc = Te[:, :3] @ world[i].astype(f64) + Te[:, 3]
            if pc[2] < 0.05 or rng.random() < 0.15:
                continue
            u, v = W.kb8_project(m, S.CAMS[e], pc[0], pc[1], pc[2])
            xs.append(float(u) + rng.uniform(-3, 3)); ys.append(float(v) + rng.uniform(-3, 3)); octs.append(int(lvl[i]))
            ds.append(SP.flip(desc[i], rng, int(rng.integers(0, 30))))
        xs += rng.uniform(0, 512, extra).tolist(); ys += rng.uniform(0, 512, extra).tolist(); octs += rng.integers(0, 8, extra).tolist()
        ds += [rng.integers(0, 256, 32, dtype=np.uint8) for _ in range(extra)]
        halves.append((SP.keypoints(xs, ys, octs), np.array(ds, np.uint8)))
    gl, gr = O.assign_features_two_eyes(halves[0][0], halves[1][0], S.BOUNDS)
    scene = dict(left=SP.eye(halves[0][0], halves[0][1], gl), right=SP.eye(halves[1][0], halves[1][1], gr), l2r=None, r2l=None, bounds=S.BOUNDS,
                 occ=[(rng.random(len(h[0])) < 0.1).astype(np.uint8) for h in halves])
    return scene, mps, flags


@pytest.mark.gpu
def test_gpu_requests_feed_the_two_eye_search_as_they_are():
    """the entry's device outputs, fed straight into search_by_projection_two_eyes_device with the same query_capacity; d_matches, d_n_matches
    and d_occupied must equal the same search fed with the walk's host-built arrays, and d_query_src maps every match to its list index"""
    import torch
    import test_search_projection_two_eyes as SP
    rng = np.random.default_rng(12)
    rig = S.RIGS["wide"]
    n, qcap, cap = 1400, 1000, 1302
    scene, mps, flags = frame_and_map(rng, rig, S.POSE, n)
    opt = dict(th=3.0, far_points=True, th_far_points=6.0)
    want = W.walk(libm(), mps, flags, S.POSE, rig["trl"], rig["tlr"], S.CAMS, S.BOUNDS, TAB, query_capacity=qcap, **opt)
    assert 300 < want["n_queries"] == want["n_wanted"] < qcap and want["n_in_view"] > want["n_queries"]
    ex = X.ORBextractor(1200, *S.SETTING)
    got = run(ex, upload([mps], n), flags[None], None, S.POSE, rig, n, (0, 1), (0, 1), qcap=qcap, **opt)
    assert_pair(got, 0, want, "map for the frame")
    host = dict(scene, q=want["queries"][:want["n_queries"]], qd=want["desc"])
    dv = SP.to_device([host], cap, qcap)
    results = []
    for q, qd, nq in ((got["dev"]["queries"], got["dev"]["desc"], got["dev"]["n_queries"]), (dv["q"], dv["qd"], dv["nq"])):
        d_m = torch.full((1, 2, cap), -7, dtype=torch.int32, device="cuda"); d_nm = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        d_occ = dv["occ"].clone()
        torch.cuda.synchronize()
        ex.search_by_projection_two_eyes_device(1, (0, 1), q, qd, (0, 1), nq, qcap, dv["k"], dv["d"], dv["n"], cap, dv["off"], dv["idx"], S.BOUNDS, None,
                                                None, d_occ, 0.8, d_m, d_nm)
        ex.synchronize()
        results.append((d_m.cpu().numpy()[0], int(d_nm[0]), d_occ.cpu().numpy()[0]))
    (m_dev, n_dev, occ_dev), (m_host, n_host, occ_host) = results
    print("%d slots of %d MapPoints, %d in view, %d matches" % (want["n_queries"], n, want["n_in_view"], n_dev))
    assert np.array_equal(m_dev, m_host) and n_dev == n_host and np.array_equal(occ_dev, occ_host) and n_dev > 100
    hit = m_dev[m_dev >= 0]
    assert (hit < want["n_queries"]).all()
    idx = got["src"][0][hit]                                # vpMapPoints[d_query_src[d_matches[...]]]
    assert np.array_equal(idx, want["src"][hit]) and W.is_slot(want["track"])[idx].all()


@pytest.mark.gpu
def test_gpu_argument_errors_are_rejected_before_any_launch():
    import torch
    ex = extractor()
    z = torch.zeros(8192, dtype=torch.int32, device="cuda")
    outs = [torch.full((1024,), -7, dtype=torch.int32, device="cuda") for _ in range(7)]
    torch.cuda.synchronize()
    ex.profile(True)
    rig = S.RIGS["narrow"]
    good = dict(n_pairs=1, cur=(0, 1), mp=(0, 0), d_mp_world=z, d_mp_normal=z, d_mp_dist=z, d_mp_desc=z, d_n_mp=None, mp_capacity=16, d_mp_flags=z,
                d_mp_prev_depth=None, d_poses=z, trl=rig["trl"], tlr=rig["tlr"], cam_left=S.CAM_LEFT, cam_right=S.CAM_RIGHT, bounds=S.BOUNDS,
                query_capacity=16, d_queries=outs[0], d_query_desc=outs[1], d_query_src=outs[2], d_n_queries=outs[3], d_n_wanted=outs[4],
                d_track=outs[5], d_n_in_view=outs[6])
    bad = [dict(n_pairs=0), dict(n_pairs=-1), dict(n_pairs=65536), dict(cur=(-1, 1)), dict(mp=(-1, 0)), dict(n_pairs=3, cur=(1, -1)),
           dict(n_pairs=3, mp=(1, -1)), dict(mp_capacity=0), dict(mp_capacity=-1), dict(query_capacity=0), dict(query_capacity=17), dict(nlevels=7),
           dict(nlevels=12)]
    bad += [dict([(k, None)]) for k in ("d_mp_world", "d_mp_normal", "d_mp_dist", "d_mp_desc", "d_mp_flags", "d_poses", "trl", "tlr", "cam_left",
                                       "cam_right", "bounds", "d_queries", "d_query_desc", "d_query_src", "d_n_queries", "d_track", "d_n_in_view")]
    for change in bad:
        with pytest.raises(X.OrbxError) as e:
            ex.frustum_requests_two_eyes_device(**dict(good, **change))
        assert e.value.code == -2, change
    ex.synchronize()
    assert all((o == -7).all() for o in outs)
    assert sum(v[1] for v in ex.profile_read().values()) == 0      # nothing was launched
    ex.frustum_requests_two_eyes_device(**good)                    # all-zero input: flags 0, nothing is looked at
    ex.frustum_requests_two_eyes_device(**dict(good, d_n_wanted=None, query_capacity=5))
    ex.synchronize()
    assert int(outs[3][0]) == 0 and int(outs[4][0]) == 0 and int(outs[6][0]) == 0 and (outs[2][:16] == -1).all() and (outs[2][16:] == -7).all()
    assert (outs[0][:16 * 16] == 0).all() and (outs[0][16 * 16:] == -7).all() and (outs[1] == -7).all()
    tr = outs[5].cpu().numpy()[:16 * 2 * 7].view(X.TRACK_RECORD_DTYPE)
    assert (tr["exit"] == 0).all() and (tr["proj_x"] == -1).all() and (tr["level"] == -1).all() and (outs[5][16 * 2 * 7:] == -7).all()
    assert sum(v[1] for v in ex.profile_read().values()) == 2
