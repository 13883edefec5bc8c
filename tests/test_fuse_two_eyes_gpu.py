"""orbx_fuse_two_eyes_device against the sequential walk (tests/fuse_two_eyes_walk.py) on the scenes of tests/test_fuse_two_eyes.py: d_best_idx,
d_best_dist, d_exit and d_n_fused exactly, all mp_capacity entries of every eye asked for written and those of an eye not asked for left alone
(the outputs are poisoned first).  tests/test_fuse_two_eyes.py (f) runs the kernel's own source, compiled for the host, against the same walks
on the same scenes."""
import numpy as np
import pytest

import extractorb_amd as X
import test_fuse_two_eyes as T
from fuse_walk import f32

POISON = -559038737
POISON8 = 0xA5


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda()


def upload(scene, cap, mp_cap):
    """the batch: device frames 2r, 2r + 1 = the eyes of rig r of the scene, list l = MapPoint list l"""
    return dict((k, _dev(v)) for k, v in T.pack(scene, cap, mp_cap).items())


def run(ex, scene, dv, pairs, cap, mp_cap, kf, mp, n_mp=None, exits=True, eyes=3, **opt):
    """pairs: (rig, list) per pair - they fix the flags (T.flags_for) and must agree with kf / mp = (first, step)"""
    import torch
    P = len(pairs)
    flags = np.zeros((P, mp_cap), np.uint8)
    for p, (k, l) in enumerate(pairs):
        assert (k, l) == (kf[0] + p * kf[1], mp[0] + p * mp[1])
        n = len(scene["lists"][l]["world"])
        flags[p, :n] = T.flags_for(scene, k, n)
    flags[:, min(len(m["world"]) for m in scene["lists"]):] = 1      # beyond the lists (mp_capacity above them): set, d_n_mp must stop them
    d_fl = _dev(flags)
    d_nmp = None if n_mp is None else _dev(np.asarray(n_mp, np.int32))
    d_bi = torch.full((P, 2, mp_cap), POISON, dtype=torch.int32, device="cuda"); d_bd = torch.full((P, 2, mp_cap), POISON, dtype=torch.int32, device="cuda")
    d_ex = torch.full((P, 2, mp_cap), POISON8, dtype=torch.uint8, device="cuda") if exits else None
    d_nf = torch.full((P, 2), POISON, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                            # torch's copies and fills have landed before the handle's stream runs
    ex.fuse_two_eyes_device(P, kf, mp, dv["world"], dv["normal"], dv["dist"], dv["mdesc"], d_nmp, mp_cap, d_fl, dv["poses"], scene["tlr"],
                            X.camera_kb8(*scene["cams"][0]), X.camera_kb8(*scene["cams"][1]), dv["kps"], dv["desc"], dv["nout"], cap, dv["off"], dv["idx"],
                            scene["bounds"], d_bi, d_bd, d_ex, d_nf, eyes=eyes, **opt)
    ex.synchronize()
    return d_bi.cpu().numpy(), d_bd.cpu().numpy(), None if d_ex is None else d_ex.cpu().numpy(), d_nf.cpu().numpy()


def assert_equals_walk(name, got, pairs, n_mp=None, eyes=3, **opt):
    bi, bd, ex, nf = got
    s = T.get(name)
    for p, (k, l) in enumerate(pairs):
        for e in (0, 1):
            what = "%s pair %d eye %d eyes %d %r" % (name, p, e, eyes, opt)
            if not (eyes >> e) & 1:                                             # not asked for: the poison is still there
                assert (bi[p, e] == POISON).all() and (bd[p, e] == POISON).all() and (ex is None or (ex[p, e] == POISON8).all()) and nf[p, e] == POISON, what
                continue
            n = len(s["lists"][l]["world"]) if n_mp is None else int(n_mp[l])
            want = T.walk(name, k, l, bool(e), n_mp=None if n_mp is None else n, **opt)
            m = len(want["exit"])
            print("%s: %d fused (walk %d), exits %s" % (what, int(nf[p, e]), want["n_fused"], np.bincount(want["exit"], minlength=8).tolist()))
            assert np.array_equal(bi[p, e, :m], want["best_idx"]) and np.array_equal(bd[p, e, :m], want["best_dist"]), what
            assert ex is None or np.array_equal(ex[p, e, :m], want["exit"]), what
            assert int(nf[p, e]) == want["n_fused"], what
            # past the list: written all the same, as flag exits
            assert (bi[p, e, m:] == -1).all() and (bd[p, e, m:] == 256).all() and (ex is None or (ex[p, e, m:] == 0).all()), what


def extractor(setting=(1.2, 8), nfeatures=1000):
    return X.ORBextractor(nfeatures, setting[0], setting[1])


@pytest.mark.gpu
@pytest.mark.parametrize("reproj_check", [True, False])
def test_gpu_one_list_into_three_rigs(reproj_check):
    """capacity 96 per eye x 150 MapPoints x 3 rigs, mp_step = 0 (SearchInNeighbors' first half); 150 and 300 lanes are no multiple of the
    block.  eyes = 3, 1 and 2 (the loop-closing mode has the left eye only); a second run is byte-identical"""
    s = T.get("small")
    ex = extractor()
    dv = upload(s, 96, 150)
    pairs = [(0, 0), (1, 0), (2, 0)]
    for eyes in (3, 1, 2) if reproj_check else (1,):
        got = run(ex, s, dv, pairs, 96, 150, (0, 1), (0, 0), reproj_check=reproj_check, eyes=eyes)
        assert_equals_walk("small", got, pairs, reproj_check=reproj_check, eyes=eyes)
        again = run(ex, s, dv, pairs, 96, 150, (0, 1), (0, 0), reproj_check=reproj_check, eyes=eyes)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


def check_gpu_on_seed(seed, **opt):
    """the body tools/fuzz_matchers.py runs with seeds outside the committed ones: a scene of this seed, one list into both eyes of three rigs"""
    s = T.random_scene(seed, 300, 400, 3)
    ex = extractor()
    bi, bd, exits, nf = run(ex, s, upload(s, 300, 400), [(0, 0), (1, 0), (2, 0)], 300, 400, (0, 1), (0, 0), **opt)
    for k in range(3):
        for e in (0, 1):
            want = T.FW.search(s["kfs"][k], bool(e), s["lists"][0], T.flags_for(s, k, 400), s["tlr"], s["cams"], s["bounds"], s["tab"], **opt)
            assert np.array_equal(bi[k, e], want["best_idx"]) and np.array_equal(bd[k, e], want["best_dist"]) and np.array_equal(exits[k, e], want["exit"]), (seed, k, e)
            assert int(nf[k, e]) == want["n_fused"], (seed, k, e)


@pytest.mark.gpu
def test_gpu_the_soak_body_on_a_committed_seed():
    """check_gpu_on_seed as tools/fuzz_matchers.py calls it, with the wider window (th = 4)"""
    check_gpu_on_seed(21, th=4.0)


@pytest.mark.gpu
def test_gpu_one_list_per_rig_and_one_rig_for_all_lists():
    s = T.get("small_lists")
    ex = extractor()
    dv = upload(s, 96, 150)
    pairs = [(0, 0), (1, 1), (2, 2)]
    assert_equals_walk("small_lists", run(ex, s, dv, pairs, 96, 150, (0, 1), (0, 1)), pairs)
    kw = dict(tlr=s["tlr"], cams=s["cams"], bounds=s["bounds"], tab=s["tab"])
    # kf_step = 0: every list into rig 1; then a rig and lists that are not the first
    for pairs, kf, mp in (([(1, 0), (1, 1), (1, 2)], (1, 0), (0, 1)), ([(2, 1), (2, 2)], (2, 0), (1, 1))):
        bi, bd, exits, nf = run(ex, s, dv, pairs, 96, 150, kf, mp)
        for p, (k, l) in enumerate(pairs):
            for e in (0, 1):
                want = T.FW.search(s["kfs"][k], bool(e), s["lists"][l], T.flags_for(s, k, 150), **kw)
                assert np.array_equal(bi[p, e], want["best_idx"]) and np.array_equal(bd[p, e], want["best_dist"]) and np.array_equal(exits[p, e], want["exit"])
                assert int(nf[p, e]) == want["n_fused"]


@pytest.mark.gpu
def test_gpu_ragged_lists_a_larger_mp_capacity_and_no_exit_array():
    """d_n_mp ragged (0, 1, a middle value, all) against NULL; mp_capacity 300 above the lists' 150 with the flags beyond set; d_exit NULL"""
    s = T.get("small_lists")
    ex = extractor()
    dv = upload(s, 96, 300)
    pairs = [(0, 0), (1, 1), (2, 2)]
    n_mp = [77, 0, 150]
    assert_equals_walk("small_lists", run(ex, s, dv, pairs, 96, 300, (0, 1), (0, 1), n_mp=n_mp), pairs, n_mp=n_mp)
    n_mp = [1, 149, 150]
    assert_equals_walk("small_lists", run(ex, s, dv, pairs, 96, 300, (0, 1), (0, 1), n_mp=n_mp, exits=False), pairs, n_mp=n_mp)
    # a count below 0 or above mp_capacity is clamped
    got = run(ex, s, dv, pairs, 96, 300, (0, 1), (0, 1), n_mp=[150, -5, 150])
    assert_equals_walk("small_lists", got, pairs, n_mp=[150, 0, 150])
    dv = upload(s, 96, 150)
    assert_equals_walk("small_lists", run(ex, s, dv, pairs, 96, 150, (0, 1), (0, 1), n_mp=[4000, 150, 1 << 30]), pairs)


@pytest.mark.gpu
def test_gpu_a_second_handle_with_twelve_levels_of_1_1():
    ex8, ex12 = extractor(), extractor((1.1, 12))
    s = T.get("small_12")
    dv = upload(s, 96, 150)
    pairs = [(0, 0), (1, 0), (2, 0)]
    assert_equals_walk("small_12", run(ex12, s, dv, pairs, 96, 150, (0, 1), (0, 0)), pairs)
    s8 = T.get("small")
    assert_equals_walk("small", run(ex8, s8, upload(s8, 96, 150), pairs, 96, 150, (0, 1), (0, 0)), pairs)      # the first handle keeps its own table
    with pytest.raises(X.OrbxError) as e:                                                                       # nlevels mismatch
        run(ex12, s, dv, pairs, 96, 150, (0, 1), (0, 0), nlevels=8)
    assert e.value.code == -2


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["edge", "edge_12"])
def test_gpu_edge_scenes(name):
    """the planted probes: the truncated bounds, z = +-0, the early returns, the tie, th_low, level - 1 = -1, a right winner at NLeft + i"""
    s = T.get(name)
    ex = extractor(s["setting"])
    n = len(s["lists"][0]["world"]); cap = max(len(e["kps"]) for e in s["kfs"][0]["eyes"])
    dv = upload(s, cap, n)
    for opt in (dict(), dict(reproj_check=False, eyes=1), T.RETURNS):
        assert_equals_walk(name, run(ex, s, dv, [(0, 0)], cap, n, (0, 1), (0, 0), **opt), [(0, 0)], **opt)


@pytest.mark.gpu
def test_gpu_non_integer_image_bounds_and_differing_cameras():
    """bounds4 truncated for IsInImage and the window, untruncated for the grid inverses; and the right eye projects with its own camera: with
    the cameras swapped the device follows the walk of the swapped rig, which is another result"""
    s = T.get("small_frac")
    ex = extractor()
    pairs = [(0, 0), (1, 0), (2, 0)]
    assert_equals_walk("small_frac", run(ex, s, upload(s, 96, 150), pairs, 96, 150, (0, 1), (0, 0)), pairs)
    s = T.get("small")
    swapped = dict(s, cams=(s["cams"][1], s["cams"][0]))
    bi, bd, exits, nf = run(ex, swapped, upload(s, 96, 150), [(0, 0)], 96, 150, (0, 1), (0, 0), eyes=2)
    want = T.FW.search(s["kfs"][0], True, s["lists"][0], T.flags_for(s, 0, 150), s["tlr"], swapped["cams"], s["bounds"], s["tab"])
    assert np.array_equal(bi[0, 1], want["best_idx"]) and np.array_equal(bd[0, 1], want["best_dist"]) and np.array_equal(exits[0, 1], want["exit"])
    assert not np.array_equal(exits[0, 1], T.walk("small", 0, 0, True)["exit"]) or not np.array_equal(bd[0, 1], T.walk("small", 0, 0, True)["best_dist"])


@pytest.mark.gpu
def test_gpu_real_sizes_and_a_long_list():
    """the per-eye capacity of a 1200-feature handle: 1000 MapPoints x 4 rigs; 5000 MapPoints into one rig (40 blocks)"""
    ex = extractor(nfeatures=1200)
    cap = ex.capacity
    assert cap == 1302
    s = T.get("real")
    pairs = [(k, 0) for k in range(4)]
    got = run(ex, s, upload(s, cap, 1000), pairs, cap, 1000, (0, 1), (0, 0))
    assert_equals_walk("real", got, pairs)
    assert got[3][:, 0].sum() > 200 and got[3][:, 1].sum() > 200
    s = T.get("long")
    got = run(ex, s, upload(s, cap, 5000), [(0, 0)], cap, 5000, (0, 1), (0, 0))
    assert_equals_walk("long", got, [(0, 0)])
    assert got[3][0, 0] > 200 and got[3][0, 1] > 200


@pytest.mark.gpu
def test_gpu_argument_errors_are_rejected_before_any_launch():
    import torch
    ex = extractor()
    z = torch.zeros(8192, dtype=torch.int32, device="cuda")
    out, out2, out3 = (torch.full((64,), POISON, dtype=torch.int32, device="cuda") for _ in range(3))
    torch.cuda.synchronize()
    ex.profile(True)
    eye3 = np.concatenate([np.eye(3), np.zeros((3, 1))], axis=1).astype(f32)
    good = dict(n_pairs=1, kf=(0, 1), mp=(0, 0), d_mp_world=z, d_mp_normal=z, d_mp_dist=z, d_mp_desc=z, d_n_mp=None, mp_capacity=16, d_mp_flags=z,
                d_poses=z, tlr=eye3, cam_left=X.camera_kb8(*T.CAM_L), cam_right=X.camera_kb8(*T.CAM_R), d_kps=z, d_desc=z, d_n=z, capacity=16,
                d_grid_off=z, d_grid_idx=z, bounds=T.BOUNDS, d_best_idx=out, d_best_dist=out2, d_exit=None, d_n_fused=out3)
    bad = [dict(n_pairs=0), dict(n_pairs=-1), dict(n_pairs=65536), dict(kf=(-1, 1)), dict(mp=(-1, 0)), dict(n_pairs=3, kf=(1, -1)), dict(n_pairs=3, mp=(1, -1)),
           dict(capacity=0), dict(capacity=-3), dict(mp_capacity=0), dict(mp_capacity=-1), dict(th_low=-1), dict(nlevels=7), dict(nlevels=12),
           dict(bounds=np.array([0, 0, 0, 480], f32)), dict(bounds=np.array([0, 640, 5, 5], f32)), dict(bounds=None), dict(cam_left=None), dict(cam_right=None),
           dict(tlr=None), dict(eyes=0), dict(eyes=4), dict(eyes=-1), dict(eyes=7), dict(reproj_check=False, eyes=3), dict(reproj_check=False, eyes=2)]
    bad += [dict([(k, None)]) for k in ("d_mp_world", "d_mp_normal", "d_mp_dist", "d_mp_desc", "d_mp_flags", "d_poses", "d_kps", "d_desc", "d_n",
                                       "d_grid_off", "d_grid_idx", "d_best_idx", "d_best_dist", "d_n_fused")]
    for change in bad:
        with pytest.raises(X.OrbxError) as e:
            ex.fuse_two_eyes_device(**dict(good, **change))
        assert e.value.code == -2, change
    ex.synchronize()
    assert (out == POISON).all() and (out2 == POISON).all() and (out3 == POISON).all()
    assert sum(v[1] for v in ex.profile_read().values()) == 0      # nothing was launched
    ex.fuse_two_eyes_device(**good)                                # the unchanged call is accepted: n_out = 0, empty grids, flags 0
    ex.synchronize()
    assert (out[:32] == -1).all() and (out2[:32] == 256).all() and (out3[:2] == 0).all() and (out[32:] == POISON).all() and (out3[2:] == POISON).all()
    assert sum(v[1] for v in ex.profile_read().values()) == 1
    ex.fuse_two_eyes_device(**dict(good, reproj_check=False, eyes=1))      # the loop-closing form is accepted with the left eye alone
    ex.synchronize()
    assert sum(v[1] for v in ex.profile_read().values()) == 2
