"""orbx_create_new_map_points_device and orbx_create_new_map_points_two_eyes_device on the GPU: byte-equal to the sequential walk
(tests/new_map_points_walk.py) on the crafted and edge scenes of tests/test_new_map_points.py at capacity 32 (per eye) with every output
pre-filled with poison, twice on one handle; chained behind the two triangulation searches on their own crafted scenes with no host copy in
between; the marks feeding the next search (n_pairs = 1 per neighbour) against the sequential walk over three neighbours, and the batched
call against the walk with frozen flags; at the real size (2024 one-camera, 1302 per eye; one keyframe against 4 neighbours, the match lists
taken from the searches) against the kernel's own source compiled for the host, which the CPU suite proves against the walk; the rejections;
the debug counters."""
import copy

import numpy as np
import pytest

import extractorb_amd as X
import new_map_points_scenes as SC
import new_map_points_walk as NW
import test_new_map_points as TN
import test_search_triangulation_two_eyes as T2
import triangulation_two_eyes_scenes as S2
import triangulation_two_eyes_walk as W2


def _one_camera_search_tests():
    """tests/test_search_triangulation.py asks the library for its tables while it is imported, which loads the library: imported here, from
    inside a test, so that torch has been asked for the GPU first (a process whose first HIP call is the library's leaves torch, and then the
    library, without a device)"""
    import test_search_triangulation
    return test_search_triangulation

f32 = np.float32


def _dev(a):
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda()


def extractor():
    return X.ORBextractor(1000, 1.2, 8)


def device_outputs(P, L, marks=True):
    import torch
    o = TN.outputs(dict(P=P, L=L, cap=0), marks)
    return dict((k, _dev(v)) for k, v in o.items())


def call(ex, s, d, o, n_pairs=None, kf1=None, kf2=None, pairs=None, n_matches=None, far_points=None, mark1="own", mark2="own"):
    """one call of the form's entry on device arrays d (SC.pack's, uploaded) and outputs o"""
    kf1, kf2 = kf1 or s["kf1"], kf2 or s["kf2"]
    P = d["P"] if n_pairs is None else n_pairs
    far = s["far_points"] if far_points is None else far_points
    m1 = o["mark1"] if isinstance(mark1, str) else mark1
    m2 = o["mark2"] if isinstance(mark2, str) else mark2
    pr = d["pairs"] if pairs is None else pairs
    nm = d["n_matches"] if n_matches is None else n_matches
    if s["two_eyes"]:
        ex.create_new_map_points_two_eyes_device(P, kf1, kf2, pr, nm, d["poses"], s["tlr"], X.camera_kb8(*s["cams"][0]), X.camera_kb8(*s["cams"][1]),
                                                 d["kps_un"], d["n_out"], d["cap"], o["exit"], o["x3d"], o["n_new"], m1, m2, far_points=far,
                                                 th_far_points=s["th_far"])
    else:
        ex.create_new_map_points_device(P, kf1, kf2, pr, nm, d["poses"], s["cams"], d["kps_un"], d["kps"], d["u_right"], d["depth"], d["n_out"], d["cap"],
                                        s["mb"], s["mbf"], o["exit"], o["x3d"], o["n_new"], m1, m2, far_points=far, th_far_points=s["th_far"])


def upload(s, **kw):
    h = SC.pack(s, **kw)
    return dict((k, _dev(v) if isinstance(v, np.ndarray) else v) for k, v in h.items())


def gpu_run(ex, s, marks=True, **kw):
    import torch
    d = upload(s, **kw)
    o = device_outputs(d["P"], d["L"], marks)
    torch.cuda.synchronize()                            # torch's copies and fills have landed before the handle's stream runs
    ex.new_map_points_count(True)
    call(ex, s, d, o)
    ex.synchronize()
    out = dict((k, None if v is None else v.cpu().numpy()) for k, v in o.items())
    out["stats"] = ex.new_map_points_stats()
    ex.new_map_points_count(False)
    return out


def same_outputs(a, b):
    return all((a[k] is None and b[k] is None) or (k == "stats" and a[k] == b[k]) or (k != "stats" and a[k].tobytes() == b[k].tobytes()) for k in a)


@pytest.mark.gpu
@pytest.mark.parametrize("two_eyes", [False, True])
def test_gpu_crafted_scene_equals_the_walk(two_eyes):
    ex = extractor()
    s = TN.scene(two_eyes, 1)
    o = gpu_run(ex, s)
    TN.assert_equals_walk(o, s, what="crafted")
    again = gpu_run(ex, s)
    assert same_outputs(o, again)
    print("SVD branches %d, UnprojectStereo branches %d" % o["stats"])
    TN.assert_equals_walk(gpu_run(ex, s, marks=False), s, what="no marks")


@pytest.mark.gpu
@pytest.mark.parametrize("two_eyes,name", [(False, "nan_pose"), (True, "nan_pose"), (False, "nan_parallax"), (True, "nan_parallax"), (False, "mono"),
                                           (True, "nleft_zero"), (False, "zero_dist"), (False, "empty"), (True, "empty"), (False, "past"), (True, "past")])
def test_gpu_edge_scenes_equal_the_walk(two_eyes, name):
    ex = extractor()
    base = TN.scene(two_eyes, 1)
    L = (2 if two_eyes else 1) * base["cap"]
    if name == "zero_dist":
        s = SC.zero_dist_scene()
        o = gpu_run(ex, s)
        assert o["exit"][0, 0] == NW.ZERO_DIST
    elif name == "empty":
        s = copy.deepcopy(base); s["pairs"] = [[], [], [], []]; s["kinds"] = [[], [], [], []]
        o = gpu_run(ex, s)
        assert (o["n_new"] == 0).all() and (o["exit"] == TN.POISON_EXIT).all()
        TN.assert_equals_walk(gpu_run(ex, s, n_matches=-3), s, what="negative")
    elif name == "past":                                                            # n_matches past the capacity: all L entries, poison pairs are bad indices
        s = copy.deepcopy(base)
        for p in range(4):
            pad = L - len(s["pairs"][p])
            s["pairs"][p] = list(s["pairs"][p]) + [(SC.POISON_PAIR, SC.POISON_PAIR)] * pad; s["kinds"][p] = list(s["kinds"][p]) + ["bad"] * pad
        o = gpu_run(ex, s, n_matches=L + 40)
    else:
        s = TN.scene(two_eyes, 1, name)
        o = gpu_run(ex, s)
    TN.assert_equals_walk(o, s, what=name)


# ---- chained behind the searches, nothing returns to the host in between ----
def one_camera_keyframes(searches, poses, rng):
    """test_search_triangulation's keyframes as the walk's: the pose, mvKeysUn = mvKeys = its keypoints, its mvuRight, and an mvDepth of this test's"""
    kfs = []
    for kf, (R, t) in zip([searches[0]["kf1"]] + [s["kf2"] for s in searches], poses):
        n = len(kf["kps"])
        depth = np.where(rng.random(n) < 0.1, -1.0, rng.uniform(4, 12, n)).astype(f32)
        kfs.append(dict(pose=np.hstack([R, np.asarray(t)[:, None]]).astype(f32), kps_un=kf["kps"], kps=kf["kps"], u_right=kf["ur"], depth=depth))
    return kfs


def one_camera_chain(ex, searches, kfs, cap, host=None):
    import torch
    T1 = _one_camera_search_tests()
    P = len(searches)
    dv = T1.pack([searches[0]["kf1"]] + [s["kf2"] for s in searches], cap)
    fl1 = np.zeros((P, cap), np.uint8); fl2 = np.zeros((P, cap), np.uint8)
    for p, s in enumerate(searches):
        fl1[p, :len(s["kf1"]["mp"])] = s["kf1"]["mp"]; fl2[p, :len(s["kf2"]["mp"])] = s["kf2"]["mp"]
    d_f = _dev(np.stack([s["F"].reshape(9) for s in searches]).astype(f32)); d_e = _dev(np.stack([s["ep"] for s in searches]).astype(f32))
    d_m = torch.full((P, cap), -7, dtype=torch.int32, device="cuda"); d_p = torch.full((P, cap, 2), -1, dtype=torch.int32, device="cuda")
    d_nm = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    d_fl1, d_fl2 = _dev(fl1), _dev(fl2)
    scene = dict(two_eyes=False, cap=cap, kfs=kfs, pairs=[[]] * P, kinds=[[]] * P, kf1=(0, 0), kf2=(1, 1), tlr=None, cams=SC.CAM, mb=SC.MB, mbf=SC.MBF,
                 far_points=True, th_far=11.0)
    d = upload(scene)
    o = device_outputs(P, cap)
    torch.cuda.synchronize()
    ex.search_for_triangulation_device(P, (0, 0), (1, 1), dv["fn"], dv["fi"], dv["nfeat"], d_fl1, d_fl2, dv["kps"], dv["ur"], dv["desc"], dv["nout"], cap,
                                       d_f, d_e, d_m, d_p, d_nm)
    call(ex, scene, d, o, pairs=d_p, n_matches=d_nm)                                 # the search's device output, as it is
    ex.synchronize()
    out = dict((k, v.cpu().numpy()) for k, v in o.items())
    n = d_nm.cpu().numpy(); pr = d_p.cpu().numpy()
    scene["pairs"] = [[tuple(r) for r in pr[p, :n[p]].tolist()] for p in range(P)]
    return scene, out


@pytest.mark.gpu
def test_gpu_chained_with_the_one_camera_search():
    T1 = _one_camera_search_tests()
    ex = X.ORBextractor(1200)
    s = T1.get("side")
    scene, out = one_camera_chain(ex, [s], one_camera_keyframes([s], T1.SIDE, np.random.default_rng(5)), T1.CAP_1200)
    assert scene["pairs"][0] == T1.walk(s)["pairs"] and len(scene["pairs"][0]) > 100          # the search's walk, then this entry's walk
    TN.assert_equals_walk(out, scene, w=SC.walk(scene), what="chained")
    h = np.bincount(out["exit"][0, :len(scene["pairs"][0])], minlength=14)
    print("one camera chained:", dict(zip(NW.EXIT_NAMES, h.tolist())))
    assert h[NW.TRIANGULATED] > 20 and h[NW.STEREO_1] + h[NW.STEREO_2] + h[NW.EMPTY_STEREO] > 0


def two_eyes_search(ex, s, pairs, kf2, d_fl1=None, n_pairs=None):
    """the two-camera search on a scene of triangulation_two_eyes_scenes; returns its device outputs (pairs, n_matches) and uploads.  Every
    tensor of the caller's, the outputs of the entry that follows included, has to exist BEFORE this call: the one synchronize is in here,
    and torch's allocator does not know the handle's stream (d keeps the search's own outputs alive for the same reason)."""
    import torch
    cap = s["cap"]
    d = dict((k, _dev(v)) for k, v in S2.pack(s, pairs, cap).items())
    P = len(pairs)
    m12 = torch.full((P, 2, cap), -7, dtype=torch.int32, device="cuda"); d_p = torch.full((P, 2 * cap, 2), -1, dtype=torch.int32, device="cuda")
    d_n = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ex.search_for_triangulation_two_eyes_device(P, (0, 0), kf2, d["fn"], d["fi"], d["nfeat"], d["fl1"] if d_fl1 is None else d_fl1, d["fl2"], d["poses"],
                                                s["tlr"], X.camera_kb8(*s["cams"][0]), X.camera_kb8(*s["cams"][1]), d["kps"], d["desc"], d["nout"], cap, m12,
                                                d_p, d_n)
    d["m12"] = m12
    return d, d_p, d_n


def as_new_points_scene(s, pairs_frames, lists):
    return dict(two_eyes=True, cap=s["cap"], kfs=s["kfs"], pairs=lists, kinds=[["search"] * len(l) for l in lists], kf1=(0, 0), kf2=(pairs_frames[0][1], 1),
                tlr=s["tlr"], cams=s["cams"], mb=0.0, mbf=0.0, far_points=True, th_far=3.4)


@pytest.mark.gpu
def test_gpu_chained_with_the_two_eyes_search():
    ex = extractor()
    s = T2.scene(T2.CRAFTED_SEED)
    frames = T2.LOCAL_MAPPING
    lists = [T2.walk(T2.CRAFTED_SEED, a, b)["pairs"] for a, b in frames]
    scene = as_new_points_scene(s, frames, lists)
    P, cap = len(frames), s["cap"]
    o = device_outputs(P, 2 * cap)
    d, d_p, d_n = two_eyes_search(ex, s, frames, (1, 1))
    nd = dict(poses=d["poses"], kps_un=d["kps"], n_out=d["nout"], cap=cap, P=P)
    call(ex, scene, nd, o, pairs=d_p, n_matches=d_n)
    ex.synchronize()
    out = dict((k, v.cpu().numpy()) for k, v in o.items())
    assert d_n.cpu().numpy().tolist() == [len(l) for l in lists]
    TN.assert_equals_walk(out, scene, w=SC.walk(scene), what="chained")
    h = np.bincount(np.concatenate([out["exit"][p, :len(l)] for p, l in enumerate(lists)]), minlength=14)
    print("two eyes chained:", dict(zip(NW.EXIT_NAMES, h.tolist())))
    assert h[NW.TRIANGULATED] > 10 and out["n_new"][2] == 0                          # (the third neighbour's pose holds a NaN)


@pytest.mark.gpu
def test_gpu_marks_feed_the_next_search():
    """the reference's walk over the neighbours: a keypoint of the current keyframe that received a MapPoint from neighbour i is skipped by
    the search of neighbour i + 1 (ORBmatcher.cc:1033-1039).  n_pairs = 1 per neighbour, d_mark1 = the flag row the next search reads."""
    import torch
    ex = extractor()
    s = T2.scene(T2.CRAFTED_SEED)
    cap, m = s["cap"], W2.libm_math()
    frames = T2.LOCAL_MAPPING[:2] + [(0, 1)]                                         # (the third neighbour of the scene has a NaN pose: the first again)
    # the sequential walk: keyframe 0's flags grow
    kf0 = copy.deepcopy(s["kfs"][0])
    want_lists, want = [], []
    for a, b in frames:
        found = W2.search_for_triangulation(m, kf0, s["kfs"][b], s["tlr"], s["cams"], s["sigma2"])["pairs"]
        r = NW.create_new_map_points(NW.Binary32(m), kf0, s["kfs"][b], found, s["cams"], SC.TAB, far_points=True, th_far=3.4, tlr=s["tlr"])
        for eye, i in r["mark1"]:
            kf0["eyes"][eye]["mp"][i] |= 1
        want_lists.append(found); want.append(r)
    assert sum(r["n_new"] for r in want) > 10 and len(want_lists[2]) < len(want_lists[0])      # the marks of neighbour 1 closed keypoints for its second visit
    d_fl1 = _dev(S2.pack(s, [(0, 1)], cap)["fl1"])                                   # keyframe 0's flag row, [1][2][cap]
    got = []
    for a, b in frames:
        o = device_outputs(1, 2 * cap)
        d, d_p, d_n = two_eyes_search(ex, s, [(a, b)], (b, 1), d_fl1=d_fl1)
        scene = as_new_points_scene(s, [(a, b)], [[]])
        call(ex, scene, dict(poses=d["poses"], kps_un=d["kps"], n_out=d["nout"], cap=cap, P=1), o, pairs=d_p, n_matches=d_n, mark1=d_fl1, mark2=None)
        got.append((d_p, d_n, o, d))
    ex.synchronize()
    for (d_p, d_n, o, _), lst, r in zip(got, want_lists, want):
        n = int(d_n.cpu().numpy()[0])
        assert [tuple(v) for v in d_p.cpu().numpy()[0, :n].tolist()] == lst
        assert o["exit"].cpu().numpy()[0, :n].tolist() == r["exit"] and int(o["n_new"].cpu().numpy()[0]) == r["n_new"]
    final = d_fl1.cpu().numpy().reshape(2, cap)
    for e in (0, 1):
        assert np.array_equal(final[e, :len(kf0["eyes"][e]["mp"])], kf0["eyes"][e]["mp"])
    # the batched call: every neighbour sees the flags of before
    lists = [T2.walk(T2.CRAFTED_SEED, a, b)["pairs"] for a, b in T2.LOCAL_MAPPING]
    scene = as_new_points_scene(s, T2.LOCAL_MAPPING, lists)
    o = device_outputs(3, 2 * cap)
    d, d_p, d_n = two_eyes_search(ex, s, T2.LOCAL_MAPPING, (1, 1))
    call(ex, scene, dict(poses=d["poses"], kps_un=d["kps"], n_out=d["nout"], cap=cap, P=3), o, pairs=d_p, n_matches=d_n)
    ex.synchronize()
    TN.assert_equals_walk(dict((k, v.cpu().numpy()) for k, v in o.items()), scene, w=SC.walk(scene), what="batched")


@pytest.mark.gpu
def test_gpu_marks_feed_the_next_one_camera_search():
    """the same walk over three neighbours for one-camera keyframes: the row orbx_search_for_triangulation_device reads as d_kf1_mp_flags
    ([p*capacity + i], here one row) is the d_mark1 of orbx_create_new_map_points_device; six launches in stream order, one synchronize"""
    import torch
    from triangulation_walk import search_for_triangulation
    T1 = _one_camera_search_tests()
    ex = X.ORBextractor(1000)
    cap = 448
    searches, kfs = real_size_one_camera(400, views=3)
    scene = dict(two_eyes=False, cap=cap, kfs=kfs, pairs=[[]] * 3, kinds=[[]] * 3, kf1=(0, 0), kf2=(1, 1), tlr=None, cams=SC.CAM, mb=SC.MB, mbf=SC.MBF,
                 far_points=True, th_far=11.0)
    # the sequential walk: keyframe 0's flags grow
    mp0 = searches[0]["kf1"]["mp"].copy()
    want_lists, want, before = [], [], int((mp0 & 1).sum())
    for i, sr in enumerate(searches):
        a, b = sr["kf1"], sr["kf2"]
        found = search_for_triangulation(a["fv"], b["fv"], mp0, b["mp"], a["kps"], b["kps"], a["ur"], b["ur"], a["desc"], b["desc"], sr["F"], sr["ep"],
                                         T1.SF, T1.SIG2)["pairs"]
        r = NW.create_new_map_points(NW.Binary32(), kfs[0], kfs[1 + i], found, SC.CAM, SC.TAB, SC.MB, SC.MBF, True, 11.0)
        for _, k in r["mark1"]:
            mp0[k] |= 1
        want_lists.append(found); want.append(r)
    frozen = [T1.walk(sr)["pairs"] for sr in searches]                                # every neighbour against the flags of before
    assert sum(r["n_new"] for r in want) > 20 and [len(l) for l in want_lists[1:]] != [len(l) for l in frozen[1:]]      # the marks closed keypoints
    dv = T1.pack([searches[0]["kf1"]] + [sr["kf2"] for sr in searches], cap)
    fl1 = np.zeros((1, cap), np.uint8); fl1[0, :len(mp0)] = searches[0]["kf1"]["mp"]
    fl2 = np.zeros((3, cap), np.uint8)
    for p, sr in enumerate(searches):
        fl2[p, :len(sr["kf2"]["mp"])] = sr["kf2"]["mp"]
    d_f = _dev(np.stack([sr["F"].reshape(9) for sr in searches]).astype(f32)); d_e = _dev(np.stack([sr["ep"] for sr in searches]).astype(f32))
    d_m = torch.full((3, cap), -7, dtype=torch.int32, device="cuda"); d_p = torch.full((3, cap, 2), -1, dtype=torch.int32, device="cuda")
    d_nm = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    d_fl1, d_fl2 = _dev(fl1), _dev(fl2)
    d = upload(scene)
    o = device_outputs(3, cap)
    torch.cuda.synchronize()
    for i in range(3):                                                               # n_pairs = 1 per neighbour; nothing returns to the host in between
        ex.search_for_triangulation_device(1, (0, 0), (1 + i, 0), dv["fn"], dv["fi"], dv["nfeat"], d_fl1, d_fl2[i], dv["kps"], dv["ur"], dv["desc"], dv["nout"],
                                           cap, d_f[i], d_e[i], d_m[i], d_p[i], d_nm[i:])
        oi = dict(exit=o["exit"][i], x3d=o["x3d"][i], n_new=o["n_new"][i:], mark1=None, mark2=None)
        call(ex, scene, d, oi, n_pairs=1, kf2=(1 + i, 0), pairs=d_p[i], n_matches=d_nm[i:], mark1=d_fl1, mark2=None)
    ex.synchronize()
    n = d_nm.cpu().numpy(); pr = d_p.cpu().numpy()
    assert [[tuple(v) for v in pr[i, :n[i]].tolist()] for i in range(3)] == want_lists
    scene["pairs"] = want_lists
    out = dict((k, v.cpu().numpy()) for k, v in o.items()); out["mark1"] = out["mark2"] = None
    TN.assert_equals_walk(out, scene, w=want, what="one camera, sequential")
    assert np.array_equal(d_fl1.cpu().numpy()[0, :len(mp0)], mp0) and int((mp0 & 1).sum()) > before


# ---- the real size, against the host-compiled kernel source ----
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return TN.build_host(tmp_path_factory.mktemp("nmpgpu"))


def real_size_one_camera(n=2000, views=4):
    """a tools/fuzz_matchers.py-style scene: one keyframe of n features and 4 neighbours that see the same world from poses of their own
    (tests/test_search_triangulation.py: world, view); returns the searches and the walk's keyframes"""
    T1 = _one_camera_search_tests()
    w = T1.world(31, n, n // 12)
    rng = np.random.default_rng(32)
    home = (T1.rot_y(0.0), np.zeros(3))
    shared = T1.view(w, home, 0.3, 0.0)
    poses, searches = [home], []
    for v in range(views):
        pose = (T1.rot_y(rng.uniform(-0.04, 0.04)), np.array([rng.choice([-1, 1]) * rng.uniform(0.3, 0.7), rng.uniform(-0.05, 0.05), rng.uniform(-0.1, 0.1)]))
        searches.append(T1.pair_of(shared, T1.view(w, pose, 0.5, rng.uniform(-20, 20), off_line=0.25, n_seen=n - 23 * v), *T1.fundamental(home, pose)))
        poses.append(pose)
    return searches, one_camera_keyframes(searches, poses, rng)


@pytest.mark.gpu
def test_gpu_real_size_one_camera_equals_the_host_compiled_kernel(host):
    """2024 keypoints (a 2000-feature extractor), one keyframe against 4 neighbours, the match lists taken from the search"""
    ex = X.ORBextractor(2000)
    cap = 2024                                                                      # the batch's capacity is the caller's: an argument of both entries
    searches, kfs = real_size_one_camera()
    scene, out = one_camera_chain(ex, searches, kfs, cap)
    n = [len(l) for l in scene["pairs"]]
    want = TN.host_run(host, scene)
    print("one camera, real size: matches %s, new points %s, SVD / stereo branches %s" % (n, out["n_new"].tolist(), want["stats"]))
    assert min(n) > 150 and out["n_new"].min() > 30
    for k in ("exit", "x3d", "n_new", "mark1", "mark2"):
        assert out[k].tobytes() == want[k].tobytes(), k


@pytest.mark.gpu
def test_gpu_real_size_two_eyes_equals_the_host_compiled_kernel(host):
    """1302 keypoints per eye, one keyframe against 4 neighbours (the scene of tests/test_search_triangulation_two_eyes_gpu.py)"""
    ex = extractor()
    s = S2.make(21, cap=1302, n_points=1500, rigs=5, nan_rig=-1, skew=0.02, nodes=300, dup=40, decoys=8)
    frames = [(0, b) for b in (1, 2, 3, 4)]
    o = device_outputs(4, 2 * 1302)
    d, d_p, d_n = two_eyes_search(ex, s, frames, (1, 1))
    scene = as_new_points_scene(s, frames, [[]] * 4)
    call(ex, scene, dict(poses=d["poses"], kps_un=d["kps"], n_out=d["nout"], cap=1302, P=4), o, pairs=d_p, n_matches=d_n)
    ex.synchronize()
    out = dict((k, v.cpu().numpy()) for k, v in o.items())
    n = d_n.cpu().numpy(); pr = d_p.cpu().numpy()
    scene["pairs"] = [[tuple(r) for r in pr[p, :n[p]].tolist()] for p in range(4)]
    want = TN.host_run(host, scene)
    print("two eyes, real size: matches %s, new points %s, SVD branches %d" % (n.tolist(), out["n_new"].tolist(), want["stats"][0]))
    assert n.min() > 300 and out["n_new"].min() > 100
    for k in ("exit", "x3d", "n_new", "mark1", "mark2"):
        assert out[k].tobytes() == want[k].tobytes(), k


@pytest.mark.gpu
def test_gpu_rejections():
    """ORBX_ERR_BAD_ARGUMENT (-2) before any launch: the outputs keep their poison"""
    import torch
    ex = extractor()
    for two_eyes in (False, True):
        s = TN.scene(two_eyes, 1)
        d = upload(s)
        o = device_outputs(d["P"], d["L"])
        torch.cuda.synchronize()
        if two_eyes:
            fn = ex.create_new_map_points_two_eyes_device
            good = dict(n_pairs=4, kf1=(0, 0), kf2=(0, 1), d_pairs=d["pairs"], d_n_matches=d["n_matches"], d_poses=d["poses"], tlr=s["tlr"],
                        cam_left=X.camera_kb8(*s["cams"][0]), cam_right=X.camera_kb8(*s["cams"][1]), d_kps=d["kps_un"], d_n=d["n_out"], capacity=d["cap"],
                        d_exit=o["exit"], d_x3d=o["x3d"], d_n_new=o["n_new"], d_mark1=o["mark1"], d_mark2=o["mark2"])
            nulls = ("d_pairs", "d_n_matches", "d_poses", "tlr", "cam_left", "cam_right", "d_kps", "d_n", "d_exit", "d_x3d", "d_n_new")
        else:
            fn = ex.create_new_map_points_device
            good = dict(n_pairs=4, kf1=(0, 0), kf2=(0, 1), d_pairs=d["pairs"], d_n_matches=d["n_matches"], d_poses=d["poses"], cam=s["cams"],
                        d_kps_un=d["kps_un"], d_kps=d["kps"], d_u_right=d["u_right"], d_depth=d["depth"], d_n=d["n_out"], capacity=d["cap"], mb=s["mb"],
                        mbf=s["mbf"], d_exit=o["exit"], d_x3d=o["x3d"], d_n_new=o["n_new"], d_mark1=o["mark1"], d_mark2=o["mark2"])
            nulls = ("d_pairs", "d_n_matches", "d_poses", "cam", "d_kps_un", "d_kps", "d_depth", "d_n", "d_exit", "d_x3d", "d_n_new")      # (d_kps / d_depth beside d_u_right)
        bad = [{k: None} for k in nulls]
        bad += [dict(n_pairs=0), dict(n_pairs=-1), dict(capacity=0), dict(capacity=-5), dict(kf1=(-1, 0)), dict(kf2=(0, -1)), dict(kf1=(0, -1)),
                dict(nlevels=7), dict(nlevels=9)]
        for change in bad:
            with pytest.raises(X.OrbxError) as e:
                fn(**dict(good, **change))
            assert e.value.code == -2, (two_eyes, change, e.value.code)
        ex.synchronize()
        assert (o["exit"].cpu().numpy() == TN.POISON_EXIT).all() and (o["x3d"].cpu().numpy() == TN.POISON_X).all()      # nothing was launched
        assert (o["n_new"].cpu().numpy() == TN.POISON_N).all() and (o["mark1"].cpu().numpy() == 0).all()
    assert X.load_library().orbx_debug_new_map_points_stats(None) == -2
