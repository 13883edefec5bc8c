"""orbx_fuse_device against the sequential walk (tests/fuse_walk.py) on the scenes of tests/test_fuse.py: d_best_idx, d_best_dist, d_exit and
d_n_fused exactly, all mp_capacity entries of every pair written (the outputs are poisoned first).  tests/test_fuse.py (e) runs the kernel's
own source, compiled for the host, against the same walks on the same scenes."""
import numpy as np
import pytest

import extractorb_amd as X
import test_fuse as T
from fuse_walk import f32

POISON = -559038737
POISON8 = 0xA5


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda()


def upload(scene, cap, mp_cap):
    """the batch: frame f = keyframe f of the scene, list l = MapPoint list l"""
    kfs, lists = scene["kfs"], scene["lists"]
    B, NL = len(kfs), len(lists)
    kps = np.zeros((B, cap), X.KEYPOINT_DTYPE); desc = np.zeros((B, cap, 32), np.uint8); ur = np.full((B, cap), -1, f32)
    nout = np.zeros(B, np.int32); off = np.zeros((B, 64 * 48 + 1), np.int32); idx = np.zeros((B, cap), np.int32); poses = np.zeros((B, 12), f32)
    for f, k in enumerate(kfs):
        n = len(k["kps"])
        kps[f, :n] = k["kps"]; desc[f, :n] = k["desc"]; nout[f] = n; off[f] = k["grid_off"]; idx[f, :len(k["grid_idx"])] = k["grid_idx"]
        poses[f] = k["pose"].reshape(12)
        if k["ur"] is not None:
            ur[f, :n] = k["ur"]
    world = np.zeros((NL, mp_cap, 3), f32); normal = np.zeros((NL, mp_cap, 3), f32); dist = np.zeros((NL, mp_cap, 3), f32)
    mdesc = np.zeros((NL, mp_cap, 32), np.uint8)
    for l, m in enumerate(lists):
        n = len(m["world"])
        world[l, :n] = m["world"]; normal[l, :n] = m["normal"]; dist[l, :n] = m["dist"]; mdesc[l, :n] = m["desc"]
    return dict(kps=_dev(kps), desc=_dev(desc), ur=_dev(ur), nout=_dev(nout), off=_dev(off), idx=_dev(idx), poses=_dev(poses), world=_dev(world),
                normal=_dev(normal), dist=_dev(dist), mdesc=_dev(mdesc))


def run(ex, scene, dv, pairs, cap, mp_cap, kf, mp, n_mp=None, use_u_right=True, exits=True, **opt):
    """pairs: (keyframe, list) per pair - they fix the flags (T.flags_for) and must agree with kf / mp = (first, step)"""
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
    d_bi = torch.full((P, mp_cap), POISON, dtype=torch.int32, device="cuda"); d_bd = torch.full((P, mp_cap), POISON, dtype=torch.int32, device="cuda")
    d_ex = torch.full((P, mp_cap), POISON8, dtype=torch.uint8, device="cuda") if exits else None
    d_nf = torch.full((P,), POISON, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                            # torch's copies and fills have landed before the handle's stream runs
    ex.fuse_device(P, kf, mp, dv["world"], dv["normal"], dv["dist"], dv["mdesc"], d_nmp, mp_cap, d_fl, dv["poses"], dv["kps"],
                   dv["ur"] if use_u_right else None, dv["desc"], dv["nout"], cap, dv["off"], dv["idx"], scene["bounds"], X.camera(*scene["cam"]),
                   float(scene["mbf"]), d_bi, d_bd, d_ex, d_nf, **opt)
    ex.synchronize()
    return d_bi.cpu().numpy(), d_bd.cpu().numpy(), None if d_ex is None else d_ex.cpu().numpy(), d_nf.cpu().numpy()


def assert_equals_walk(name, got, pairs, n_mp=None, use_u_right=True, **opt):
    bi, bd, ex, nf = got
    s = T.get(name)
    for p, (k, l) in enumerate(pairs):
        n = len(s["lists"][l]["world"]) if n_mp is None else int(n_mp[l])
        want = T.walk(name, k, l, n_mp=None if n_mp is None else n, use_u_right=use_u_right, **opt)
        m = len(want["exit"])
        what = "%s pair %d %r" % (name, p, opt)
        print("%s: %d fused (walk %d), exits %s" % (what, int(nf[p]), want["n_fused"], np.bincount(want["exit"], minlength=8).tolist()))
        assert np.array_equal(bi[p, :m], want["best_idx"]) and np.array_equal(bd[p, :m], want["best_dist"]), what
        assert ex is None or np.array_equal(ex[p, :m], want["exit"]), what
        assert int(nf[p]) == want["n_fused"], what
        # past the list: written all the same, as flag exits
        assert (bi[p, m:] == -1).all() and (bd[p, m:] == 256).all() and (ex is None or (ex[p, m:] == 0).all()), what


def extractor(setting=(1.2, 8), nfeatures=1000):
    return X.ORBextractor(nfeatures, setting[0], setting[1])


@pytest.mark.gpu
@pytest.mark.parametrize("reproj_check", [True, False])
def test_gpu_one_list_into_three_keyframes(reproj_check):
    """capacity 96 x 150 MapPoints x 3 keyframes, mp_step = 0 (SearchInNeighbors' first half); mp_capacity 150 is no multiple of the block"""
    s = T.get("small")
    ex = extractor()
    dv = upload(s, 96, 150)
    pairs = [(0, 0), (1, 0), (2, 0)]
    got = run(ex, s, dv, pairs, 96, 150, (0, 1), (0, 0), reproj_check=reproj_check)
    assert_equals_walk("small", got, pairs, reproj_check=reproj_check)
    again = run(ex, s, dv, pairs, 96, 150, (0, 1), (0, 0), reproj_check=reproj_check)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


def check_gpu_on_seed(seed, **opt):
    """the body tools/fuzz_matchers.py runs with seeds outside the committed ones: a scene of this seed, one list into three keyframes"""
    s = T.random_scene(seed, 300, 400, 3)
    ex = extractor()
    bi, bd, exits, nf = run(ex, s, upload(s, 300, 400), [(0, 0), (1, 0), (2, 0)], 300, 400, (0, 1), (0, 0), **opt)
    for k in range(3):
        want = T.W.search(s["kfs"][k], s["lists"][0], T.flags_for(s, k, 400), s["cam"], s["bounds"], s["mbf"], s["tab"], **opt)
        assert np.array_equal(bi[k], want["best_idx"]) and np.array_equal(bd[k], want["best_dist"]) and np.array_equal(exits[k], want["exit"]), (seed, k)
        assert int(nf[k]) == want["n_fused"], (seed, k)


@pytest.mark.gpu
def test_gpu_the_soak_body_on_a_committed_seed():
    """check_gpu_on_seed as tools/fuzz_matchers.py calls it: the Sim3 mode with the wider window (th = 5)"""
    check_gpu_on_seed(21, reproj_check=False, th=5.0)


@pytest.mark.gpu
def test_gpu_one_list_per_keyframe_and_one_keyframe_for_all_lists():
    s = T.get("small_lists")
    ex = extractor()
    dv = upload(s, 96, 150)
    pairs = [(0, 0), (1, 1), (2, 2)]
    assert_equals_walk("small_lists", run(ex, s, dv, pairs, 96, 150, (0, 1), (0, 1)), pairs)
    # kf_step = 0: every list into keyframe 1; a keyframe and a list that are not the first
    pairs = [(1, 0), (1, 1), (1, 2)]
    bi, bd, exits, nf = run(ex, s, dv, pairs, 96, 150, (1, 0), (0, 1))
    for p, (k, l) in enumerate(pairs):
        mps = s["lists"][l]
        want = T.W.search(s["kfs"][k], mps, T.flags_for(s, k, 150), s["cam"], s["bounds"], s["mbf"], s["tab"])
        assert np.array_equal(bi[p], want["best_idx"]) and np.array_equal(bd[p], want["best_dist"]) and np.array_equal(exits[p], want["exit"])
        assert int(nf[p]) == want["n_fused"]
    pairs = [(2, 1), (2, 2)]
    bi, bd, exits, nf = run(ex, s, dv, pairs, 96, 150, (2, 0), (1, 1))
    for p, (k, l) in enumerate(pairs):
        want = T.W.search(s["kfs"][k], s["lists"][l], T.flags_for(s, k, 150), s["cam"], s["bounds"], s["mbf"], s["tab"])
        assert np.array_equal(bi[p], want["best_idx"]) and np.array_equal(exits[p], want["exit"]) and int(nf[p]) == want["n_fused"]


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
    # a count above mp_capacity or below 0 is clamped
    got = run(ex, s, dv, pairs, 96, 300, (0, 1), (0, 1), n_mp=[150, -5, 150])
    assert_equals_walk("small_lists", got, pairs, n_mp=[150, 0, 150])


@pytest.mark.gpu
def test_gpu_monocular_null_u_right_and_a_stereo_batch_read_as_monocular():
    s = T.get("small_mono")
    ex = extractor()
    dv = upload(s, 96, 150)
    pairs = [(0, 0), (1, 0), (2, 0)]
    assert_equals_walk("small_mono", run(ex, s, dv, pairs, 96, 150, (0, 1), (0, 0), use_u_right=False), pairs)
    assert_equals_walk("small_mono", run(ex, s, dv, pairs, 96, 150, (0, 1), (0, 0)), pairs)      # an all -1 array is the same as NULL
    s = T.get("small")
    dv = upload(s, 96, 150)
    assert_equals_walk("small", run(ex, s, dv, pairs, 96, 150, (0, 1), (0, 0), use_u_right=False), pairs, use_u_right=False)


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
@pytest.mark.parametrize("name", ["edge", "edge_12", "edge_frac"])
def test_gpu_edge_scenes(name):
    s = T.get(name)
    ex = extractor(s["setting"])
    n = len(s["lists"][0]["world"]); cap = len(s["kfs"][0]["kps"])
    dv = upload(s, cap, n)
    for opt in (dict(), dict(reproj_check=False), T.RETURNS):
        assert_equals_walk(name, run(ex, s, dv, [(0, 0)], cap, n, (0, 1), (0, 0), **opt), [(0, 0)], **opt)


@pytest.mark.gpu
def test_gpu_non_integer_image_bounds():
    """bounds4 of a distorted camera: truncated for IsInImage and the window, untruncated for the grid inverses"""
    s = T.get("small_frac")
    ex = extractor()
    pairs = [(0, 0), (1, 0), (2, 0)]
    assert_equals_walk("small_frac", run(ex, s, upload(s, 96, 150), pairs, 96, 150, (0, 1), (0, 0)), pairs)


@pytest.mark.gpu
def test_gpu_real_sizes_and_a_long_list():
    """capacity 1302: 1000 MapPoints x 4 keyframes; 5000 MapPoints into one keyframe (20 blocks)"""
    ex = extractor(nfeatures=1200)
    cap = ex.capacity
    assert cap == 1302
    s = T.get("real")
    pairs = [(k, 0) for k in range(4)]
    got = run(ex, s, upload(s, cap, 1000), pairs, cap, 1000, (0, 1), (0, 0))
    assert_equals_walk("real", got, pairs)
    assert got[3].sum() > 200
    s = T.get("long")
    got = run(ex, s, upload(s, cap, 5000), [(0, 0)], cap, 5000, (0, 1), (0, 0))
    assert_equals_walk("long", got, [(0, 0)])
    assert got[3][0] > 200


@pytest.mark.gpu
def test_gpu_argument_errors_are_rejected_before_any_launch():
    import torch
    ex = extractor()
    z = torch.zeros(8192, dtype=torch.int32, device="cuda")
    out, out2, out3 = (torch.full((64,), POISON, dtype=torch.int32, device="cuda") for _ in range(3))
    torch.cuda.synchronize()
    ex.profile(True)
    good = dict(n_pairs=1, kf=(0, 1), mp=(0, 0), d_mp_world=z, d_mp_normal=z, d_mp_dist=z, d_mp_desc=z, d_n_mp=None, mp_capacity=16, d_mp_flags=z,
                d_poses=z, d_kps_un=z, d_u_right=None, d_desc=z, d_n=z, capacity=16, d_grid_off=z, d_grid_idx=z, bounds=T.BOUNDS, cam=X.camera(*T.CAM),
                mbf=40.0, d_best_idx=out, d_best_dist=out2, d_exit=None, d_n_fused=out3)
    bad = [dict(n_pairs=0), dict(n_pairs=-1), dict(n_pairs=65536), dict(kf=(-1, 1)), dict(mp=(-1, 0)), dict(n_pairs=3, kf=(1, -1)), dict(n_pairs=3, mp=(1, -1)),
           dict(capacity=0), dict(capacity=-3), dict(mp_capacity=0), dict(mp_capacity=-1), dict(th_low=-1), dict(nlevels=7), dict(nlevels=12),
           dict(bounds=np.array([0, 0, 0, 480], f32)), dict(bounds=np.array([0, 640, 5, 5], f32)), dict(bounds=None), dict(cam=None)]
    bad += [dict([(k, None)]) for k in ("d_mp_world", "d_mp_normal", "d_mp_dist", "d_mp_desc", "d_mp_flags", "d_poses", "d_kps_un", "d_desc", "d_n",
                                       "d_grid_off", "d_grid_idx", "d_best_idx", "d_best_dist", "d_n_fused")]
    for change in bad:
        with pytest.raises(X.OrbxError) as e:
            ex.fuse_device(**dict(good, **change))
        assert e.value.code == -2, change
    ex.synchronize()
    assert (out == POISON).all() and (out2 == POISON).all() and (out3 == POISON).all()
    assert sum(v[1] for v in ex.profile_read().values()) == 0      # nothing was launched
    ex.fuse_device(**good)                                         # the unchanged call is accepted: n_out = 0, an empty grid, flags 0
    ex.synchronize()
    assert (out[:16] == -1).all() and (out2[:16] == 256).all() and int(out3[0]) == 0 and (out[16:] == POISON).all() and sum(v[1] for v in ex.profile_read().values()) == 1
