"""orbx_update_map_points_device and orbx_update_map_points_two_eyes_device against the sequential walk (tests/map_point_update_walk.py) on the
scenes of tests/map_point_update_scenes.py: capacity 32, a batch of 8 frames (4 rigs), both forms.  Every output and every table row is
poisoned first, every call runs twice on one handle with identical bytes, and everything - status, BestIdx, the median, the descriptor, the
normal and the three distances - is compared BYTE-EQUAL to the walk, with no tolerance.  tests/test_map_point_update.py runs the kernel's
statement, compiled for the host, against the same walks on the same scenes, and asserts where the crafted points end."""
import numpy as np
import pytest

import extractorb_amd as X
import fuse_walk
import map_point_update_scenes as SC
import map_point_update_walk as MW
import test_fuse as TF
import test_fuse_gpu as TG
import test_map_point_update as T

f32 = np.float32
POISON = -559038737
POISON8 = 0xEE


def _dev(a):
    import torch
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda()


def extractor():
    return X.ORBextractor(1000, 1.2, 8)


def call(ex, s, dv, what, out, **change):
    args = dict(n_points=len(s["obs_off"]) - 1, d_obs_off=dv["obs_off"], d_obs=dv["obs"], d_obs_flags=dv["flags"], d_ref=dv["ref"], d_slot=dv["slot"],
                d_mp_world=dv["world"], d_poses=dv["poses"], d_desc=dv["desc"], d_n=dv["n_out"], capacity=s["capacity"], d_mp_desc=out["mp_desc"],
                d_mp_normal=out["mp_normal"], d_mp_dist=out["mp_dist"], d_best=out["best"], d_best_median=out["best_median"], d_status=out["status"],
                what=what)
    if s["two_eyes"]:
        args.update(tlr=s["tlr"], n_rigs=len(s["poses"]), d_kps=dv["kps"])
        args.update(change)
        ex.update_map_points_two_eyes_device(**args)
    else:
        args.update(n_frames=len(s["poses"]), d_kps_un=dv["kps"])
        args.update(change)
        ex.update_map_points_device(**args)


def upload(s):
    return dict(obs_off=_dev(s["obs_off"].astype(np.int32)), obs=_dev(s["obs"].astype(np.int32)), flags=_dev(s["flags"]), ref=_dev(s["ref"].astype(np.int32)),
                slot=_dev(s["slot"]), world=_dev(s["world"].astype(f32)), poses=_dev(s["poses"].astype(f32)), kps=_dev(T.keypoints(s)),
                desc=_dev(s["desc"]), n_out=_dev(s["n_out"].astype(np.int32)))


def poisoned(s):
    import torch
    P, S = len(s["obs_off"]) - 1, len(s["world"])
    return dict(mp_desc=torch.full((S, 32), POISON8, dtype=torch.uint8, device="cuda"), mp_normal=torch.full((S, 3), MW.POISON_FLOAT, dtype=torch.float32, device="cuda"),
                mp_dist=torch.full((S, 3), MW.POISON_FLOAT, dtype=torch.float32, device="cuda"), best=torch.full((P,), POISON, dtype=torch.int32, device="cuda"),
                best_median=torch.full((P,), POISON, dtype=torch.int32, device="cuda"), status=torch.full((P,), POISON8, dtype=torch.uint8, device="cuda"))


def run(ex, s, what=3, dv=None):
    """one call from poisoned outputs and tables: the dict the walk returns"""
    import torch
    dv = dv or upload(s)
    out = poisoned(s)
    torch.cuda.synchronize()                            # torch's copies and fills have landed before the handle's stream runs
    call(ex, s, dv, what, out)
    ex.synchronize()
    return dict((k, v.cpu().numpy()) for k, v in out.items())


def run_twice(ex, s, what=3):
    dv = upload(s)
    got, again = run(ex, s, what, dv), run(ex, s, what, dv)
    assert all(got[k].tobytes() == again[k].tobytes() for k in got), "two calls on one handle differ"
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("two_eyes", [False, True])
def test_gpu_every_list_length_in_one_call(two_eyes):
    """0, 1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 129, 1024 and 1025 entries, short and long lists as neighbours; d_slot a permutation"""
    s = T.scene("lengths", two_eyes)
    got = run_twice(extractor(), s)
    T.same_bytes(got, T.walk(s), "lengths")
    n = np.diff(s["obs_off"])
    assert (got["status"][n == 1025] == MW.TOO_LONG).all() and (got["status"][n == 0] == MW.EMPTY).all() and (got["status"][n == 1024] == MW.OK).all()
    assert (got["mp_desc"][s["slot"][n == 1025]] == POISON8).all() and (got["mp_normal"][s["slot"][n == 0]] == MW.POISON_FLOAT).all()


@pytest.mark.gpu
@pytest.mark.parametrize("two_eyes", [False, True])
def test_gpu_crafted_points(two_eyes):
    """median ties (duplicates, an outlier among three, the best row last), bad keyframes (some, all), BAD_INDEX (frame -1, frame = frames,
    row = d_n_out[f], d_ref = -1, d_ref = N), octaves -1 and nlevels on the reference entry, and for two eyes a point seen by both eyes of
    a rig and one seen by right eyes only; d_slot NULL"""
    s = T.scene("crafted", two_eyes)
    got = run_twice(extractor(), s)
    w = T.walk(s)
    T.same_bytes(got, w, "crafted")
    name = s["names"]
    assert (got["best"][name["duplicates"]], got["best"][name["outlier"]], got["best"][name["best_last"]]) == (1, 0, 4)
    m = name["all_flagged"]
    assert got["status"][m] == MW.NO_DESCRIPTOR and (got["mp_desc"][m] == POISON8).all() and (got["mp_normal"][m] != MW.POISON_FLOAT).all()
    m = name["some_flagged"]                            # the normal still counts the flagged entries: it is the walk's, which counts five
    assert got["best"][m] == 0 and got["mp_normal"][m].tobytes() == w["mp_normal"][m].tobytes()
    for n in ("frame_minus_one", "frame_past", "row_past", "ref_minus_one", "ref_past"):
        m = name[n]
        assert got["status"][m] == MW.BAD_INDEX and (got["mp_desc"][m] == POISON8).all() and (got["mp_normal"][m] == MW.POISON_FLOAT).all() and \
            (got["mp_dist"][m] == MW.POISON_FLOAT).all(), n


@pytest.mark.gpu
@pytest.mark.parametrize("two_eyes", [False, True])
def test_gpu_null_flags(two_eyes):
    s = T.scene("no_flags", two_eyes)
    got = run_twice(extractor(), s)
    T.same_bytes(got, T.walk(s), "no_flags")
    assert got["status"][s["names"]["all_flagged"]] == MW.OK


@pytest.mark.gpu
@pytest.mark.parametrize("two_eyes", [False, True])
@pytest.mark.parametrize("what", [1, 2])
def test_gpu_one_half_leaves_the_other_halfs_rows_alone(two_eyes, what):
    ex = extractor()
    for name in ("lengths", "crafted"):
        s = T.scene(name, two_eyes)
        got = run_twice(ex, s, what)
        T.same_bytes(got, T.walk(s, what), "%s what=%d" % (name, what))
        if what == 1:
            assert (got["mp_normal"] == MW.POISON_FLOAT).all() and (got["mp_dist"] == MW.POISON_FLOAT).all() and (got["best"] >= 0).any()
        else:
            assert (got["mp_desc"] == POISON8).all() and (got["best"] == -1).all() and (got["mp_normal"] != MW.POISON_FLOAT).any()


@pytest.mark.gpu
@pytest.mark.parametrize("two_eyes", [False, True])
def test_gpu_a_strict_subset_of_the_table(two_eyes):
    s = T.scene("subset", two_eyes)
    got = run_twice(extractor(), s)
    T.same_bytes(got, T.walk(s), "subset")
    unnamed = np.setdiff1d(np.arange(len(s["world"])), s["slot"])
    assert len(unnamed) > 8
    assert (got["mp_desc"][unnamed] == POISON8).all() and (got["mp_normal"][unnamed] == MW.POISON_FLOAT).all() and (got["mp_dist"][unnamed] == MW.POISON_FLOAT).all()


def chain_scene(seed=31):
    """test_fuse.py's small scene (3 keyframes, capacity 96, a list of 150 MapPoints) with an observation list per MapPoint over its keyframes"""
    fs = TF.get("small")
    rng = np.random.default_rng(seed)
    cap, M = 96, len(fs["lists"][0]["world"])
    B = len(fs["kfs"])
    desc = np.zeros((B, cap, 32), np.uint8); octave = np.zeros((B, cap), np.int32)
    for f, k in enumerate(fs["kfs"]):
        desc[f, :len(k["kps"])] = k["desc"]; octave[f, :len(k["kps"])] = k["kps"]["octave"]
    b = dict(two_eyes=False, capacity=cap, nlevels=fs["tab"]["nlevels"], scale=fs["tab"]["scale"], tlr=None, poses=np.stack([k["pose"] for k in fs["kfs"]]),
             n_out=np.array([len(k["kps"]) for k in fs["kfs"]], np.int32), desc=desc, octave=octave)
    pts = []
    for i in range(M):                                  # where a keyframe holds a keypoint with (nearly) the MapPoint's descriptor, that is its observation
        near = [(int(fuse_walk.POPCOUNT[k["desc"] ^ fs["lists"][0]["desc"][i]].sum(axis=1).min()), f, int(fuse_walk.POPCOUNT[k["desc"] ^ fs["lists"][0]["desc"][i]].sum(axis=1).argmin()))
                for f, k in enumerate(fs["kfs"])]
        entries = [(f, j) for d, f, j in near if d <= 60]
        others = [f for f in range(B) if f not in [e[0] for e in entries]]
        if others and (not entries or rng.random() < 0.5):
            f = int(rng.choice(others))
            entries.append((f, int(rng.integers(len(fs["kfs"][f]["kps"])))))
        pts.append(dict(entries=sorted(entries), ref=0))
    s = SC.with_points(b, pts)
    s["world"] = fs["lists"][0]["world"].astype(f32)
    return fs, s


@pytest.mark.gpu
def test_gpu_update_then_fuse_with_no_host_copy_in_between():
    """the update writes d_mp_desc / d_mp_normal / d_mp_dist, orbx_fuse_device reads them in place: against the walk's update followed by
    fuse_walk.search on the walk's tables"""
    import torch
    fs, s = chain_scene()
    ex = extractor()
    w = T.walk(s)
    assert (w["status"] == MW.OK).all()
    dvf = TG.upload(fs, 96, 150)                        # the keyframes as Fuse takes them (and list 0's tables, which the update overwrites)
    dv = upload(s)
    P = len(s["world"])
    out = dict(mp_desc=dvf["mdesc"], mp_normal=dvf["normal"], mp_dist=dvf["dist"], best=torch.full((P,), POISON, dtype=torch.int32, device="cuda"),
               best_median=torch.full((P,), POISON, dtype=torch.int32, device="cuda"), status=torch.full((P,), POISON8, dtype=torch.uint8, device="cuda"))
    flags = np.stack([TF.flags_for(fs, k, P) for k in range(3)])
    d_fl = _dev(flags)
    d_bi, d_bd, d_nf = (torch.full(shape, POISON, dtype=torch.int32, device="cuda") for shape in ((3, P), (3, P), (3,)))
    d_ex = torch.full((3, P), POISON8, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    call(ex, s, dict(dv, world=dvf["world"], poses=dvf["poses"], desc=dvf["desc"], n_out=dvf["nout"], kps=dvf["kps"]), 3, out)
    ex.fuse_device(3, (0, 1), (0, 0), dvf["world"], dvf["normal"], dvf["dist"], dvf["mdesc"], None, P, d_fl, dvf["poses"], dvf["kps"], dvf["ur"], dvf["desc"],
                   dvf["nout"], 96, dvf["off"], dvf["idx"], fs["bounds"], X.camera(*fs["cam"]), float(fs["mbf"]), d_bi, d_bd, d_ex, d_nf)
    ex.synchronize()
    mps = dict(world=s["world"], normal=w["mp_normal"], dist=w["mp_dist"], desc=w["mp_desc"])
    fused = 0
    for k in range(3):
        want = fuse_walk.search(fs["kfs"][k], mps, flags[k], fs["cam"], fs["bounds"], fs["mbf"], fs["tab"])
        assert np.array_equal(d_bi[k].cpu().numpy(), want["best_idx"]) and np.array_equal(d_bd[k].cpu().numpy(), want["best_dist"]), k
        assert np.array_equal(d_ex[k].cpu().numpy(), want["exit"]) and int(d_nf[k]) == want["n_fused"], k
        fused += want["n_fused"]
        print("keyframe %d: exits %s" % (k, np.bincount(want["exit"], minlength=8).tolist()))
    assert fused > 20                                   # (a property of the scene: the updated tables let MapPoints through to their own keypoints)


class DeviceMap(fuse_walk.Map):
    """fuse_walk's map model with the survivor's ComputeDistinctiveDescriptors (MapPoint.cc:298) run by orbx_update_map_points_device: the
    keyframes' descriptors live on the device, the observation list of the one point goes up, 32 bytes come back"""

    @classmethod
    def of(cls, m, ex):
        import torch
        d = cls([], [])
        d.desc = [x.copy() for x in m.desc]; d.kf_desc = m.kf_desc
        d.obs = [dict(o) for o in m.obs]; d.bad = list(m.bad); d.slots = [list(x) for x in m.slots]; d.recomputed = set(m.recomputed)
        d.ex, d.cap, d.calls = ex, max(len(k) for k in m.kf_desc), 0
        desc = np.zeros((len(m.kf_desc), d.cap, 32), np.uint8)
        for f, k in enumerate(m.kf_desc):
            desc[f, :len(k)] = k
        d.d_desc, d.d_n = _dev(desc), _dev(np.array([len(k) for k in m.kf_desc], np.int32))
        d.zeros = torch.zeros(len(m.kf_desc) * max(d.cap * 7, 12), dtype=torch.float32, device="cuda")      # poses, keypoints, a position: not read for what = 1
        return d

    def compute_distinctive_descriptors(self, mp):
        import torch
        if self.bad[mp] or not self.obs[mp]:
            return
        obs = np.array(sorted(self.obs[mp].items()), np.int32)
        out = poisoned(dict(obs_off=[0, len(obs)], world=[0]))
        torch.cuda.synchronize()
        self.ex.update_map_points_device(1, _dev(np.array([0, len(obs)], np.int32)), _dev(obs), None, _dev(np.zeros(1, np.int32)), None, self.zeros, self.zeros,
                                         len(self.kf_desc), self.zeros, self.d_desc, self.d_n, self.cap, out["mp_desc"], out["mp_normal"], out["mp_dist"],
                                         out["best"], out["best_median"], out["status"], what=1)
        self.ex.synchronize()
        assert int(out["status"][0]) == MW.OK
        self.desc[mp] = out["mp_desc"][0].cpu().numpy()
        self.calls += 1


@pytest.mark.gpu
def test_gpu_replace_sequence_with_the_survivors_descriptors_from_the_device():
    """test_fuse.py's map model: the sequential Fuse over three keyframes, every Replace's survivor recomputed by the entry, ends in the map
    of the sequential reference"""
    s, m0, mp_list = TF.licence_scene(11)
    kw = dict(cam=s["cam"], bounds=s["bounds"], mbf=s["mbf"], tab=s["tab"])
    seq, dev = m0.copy(), DeviceMap.of(m0, extractor())
    for k, kf in enumerate(s["kfs"]):
        n_seq = fuse_walk.fuse_sequential(seq, k, kf, mp_list, s["lists"][0], **kw)
        assert fuse_walk.fuse_sequential(dev, k, kf, mp_list, s["lists"][0], **kw) == n_seq
    assert dev.state() == seq.state() and dev.calls > 5
    assert sum(a != b for a, b in zip(m0.state()[3], seq.state()[3])) > 3      # descriptors did change


@pytest.mark.gpu
@pytest.mark.parametrize("two_eyes", [False, True])
def test_gpu_working_size(two_eyes, tmp_path_factory):
    """2048 points over a batch of 32 frames at capacity 2024, a mean of about 6 entries and a tail into the hundreds, against the
    host-compiled header (which tests/test_map_point_update.py proves against the walk on this very scene)"""
    s = T.scene("working", two_eyes)
    host = T.build_host(tmp_path_factory.mktemp("mpuhost"))
    got = run_twice(extractor(), s)
    T.same_bytes(got, T.host_update(host, s), "working")
    assert (got["status"] == MW.OK).sum() > 1900


@pytest.mark.gpu
def test_gpu_argument_errors_are_rejected_before_any_launch():
    import torch
    ex = extractor()
    z = torch.zeros(8192, dtype=torch.int32, device="cuda")
    outs = [torch.full((64,), POISON, dtype=torch.int32, device="cuda") for _ in range(6)]
    torch.cuda.synchronize()
    ex.profile(True)
    common = dict(n_points=4, d_obs_off=z, d_obs=z, d_obs_flags=None, d_ref=z, d_slot=None, d_mp_world=z, d_poses=z, d_desc=z, d_n=z, capacity=16,
                  d_mp_desc=outs[0], d_mp_normal=outs[1], d_mp_dist=outs[2], d_best=outs[3], d_best_median=outs[4], d_status=outs[5])
    forms = [(ex.update_map_points_device, dict(common, n_frames=2, d_kps_un=z), ["d_kps_un"], [dict(n_frames=0), dict(n_frames=-1)]),
             (ex.update_map_points_two_eyes_device, dict(common, tlr=SC.TLR, n_rigs=1, d_kps=z), ["d_kps", "tlr"], [dict(n_rigs=0), dict(n_rigs=-2)])]
    for fn, good, own, own_bad in forms:
        bad = [dict(what=0), dict(what=4), dict(what=-1), dict(what=7), dict(nlevels=7), dict(nlevels=12), dict(n_points=-1), dict(capacity=0)] + own_bad
        bad += [dict([(k, None)]) for k in ["d_obs_off", "d_obs", "d_ref", "d_mp_world", "d_poses", "d_desc", "d_n", "d_mp_desc", "d_mp_normal", "d_mp_dist",
                                            "d_best", "d_best_median", "d_status"] + own]
        for change in bad:
            with pytest.raises(X.OrbxError) as e:
                fn(**dict(good, **change))
            assert e.value.code == -2, change
        fn(**dict(good, n_points=0))                    # nothing to do: accepted, nothing launched
    ex.synchronize()
    assert all((o == POISON).all() for o in outs)
    assert sum(v[1] for v in ex.profile_read().values()) == 0      # nothing was launched
    forms[0][0](**forms[0][1])                          # the unchanged call is accepted: four empty lists
    ex.synchronize()
    assert (outs[3][:4] == -1).all() and (outs[3][4:] == POISON).all() and (outs[0] == POISON).all()
    assert sum(v[1] for v in ex.profile_read().values()) == 1
