"""orbx_search_for_triangulation_two_eyes_device, orbx_kb8_unproject_device and orbx_kb8_triangulate_device on the GPU: byte-equal to the
sequential walk (tests/triangulation_two_eyes_walk.py) on the crafted and edge scenes of tests/test_search_triangulation_two_eyes.py at
capacity 32 per eye, a 9-node vocabulary and 3 pairs with kf1_step = 0 (the smallest shape with a node both eyes share and a candidate list
longer than 16); at one capacity just below and one just above the staging threshold; at the real size (1302 per eye, one keyframe against
4 neighbours) against the kernel's own source compiled for the host, which the CPU suite proves against the walk; the entry's rejections; the
two camera entries on 4096 elements against the header compiled for the host; the debug counter."""
import ctypes as C

import numpy as np
import pytest

import extractorb_amd as X
import test_kb8_unproject_math as M
import test_search_triangulation_two_eyes as T
import triangulation_two_eyes_scenes as S

f32 = np.float32
POISON = -559038737
ORBX_ERR_UNSUPPORTED = -8


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda()


def extractor():
    return X.ORBextractor(1000, 1.2, 8)


def run(ex, s, pairs, kf1, kf2, cap=None, **opt):
    import torch
    cap = cap or s["cap"]
    d = dict((k, _dev(v)) for k, v in S.pack(s, pairs, cap).items())
    P = len(pairs)
    m12 = torch.full((P, 2, cap), POISON, dtype=torch.int32, device="cuda"); out_pairs = torch.full((P, 2 * cap, 2), -7, dtype=torch.int32, device="cuda")
    n = torch.full((P,), POISON, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                            # torch's copies and fills have landed before the handle's stream runs
    ex.search_triangulation_two_eyes_count(True)
    ex.search_for_triangulation_two_eyes_device(P, kf1, kf2, d["fn"], d["fi"], d["nfeat"], d["fl1"], d["fl2"], d["poses"], s["tlr"],
                                                X.camera_kb8(*s["cams"][0]), X.camera_kb8(*s["cams"][1]), d["kps"], d["desc"], d["nout"], cap, m12,
                                                out_pairs, n, **opt)
    ex.synchronize()
    return m12.cpu().numpy(), out_pairs.cpu().numpy(), n.cpu().numpy(), ex.search_triangulation_two_eyes_stats()


def check_gpu_on_seed(seed, **opt):
    """tools/fuzz_matchers.py: a scene with descriptor families of this seed, one keyframe against three neighbours"""
    name = "f%d" % seed
    got = run(extractor(), T.scene(name), T.LOCAL_MAPPING, (0, 0), (1, 1), **opt)
    T.assert_equals_walk(name, got, T.LOCAL_MAPPING, **opt)


@pytest.mark.gpu
def test_gpu_crafted_scene_equals_the_walk():
    ex = extractor()
    s = T.scene(T.CRAFTED_SEED)
    got = run(ex, s, T.LOCAL_MAPPING, (0, 0), (1, 1))
    T.assert_equals_walk(T.CRAFTED_SEED, got, T.LOCAL_MAPPING)
    again = run(ex, s, T.LOCAL_MAPPING, (0, 0), (1, 1))
    assert all(np.array_equal(a, b) for a, b in zip(got[:3], again[:3])) and got[3] == again[3]
    # the rows rank by Hamming key first: fewer triangulations than candidates with dist <= th_low
    within = sum(T.walk(T.CRAFTED_SEED, a, b)["within"] for a, b in T.LOCAL_MAPPING)
    print("triangulations %d, candidates within th_low %d (walk %d)" % (got[3][0], got[3][1], within))
    assert got[3][1] == within and 0 < got[3][0] < within


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["empty_right_eye", "nleft_zero", "zero_w", "only_stereo", "coarse", "itself", "families"])
def test_gpu_edge_scenes_equal_the_walk(case):
    ex = extractor()
    name, pairs, kf2, opt = T.CRAFTED_SEED, T.LOCAL_MAPPING, (1, 1), {}
    if case in ("empty_right_eye", "nleft_zero", "zero_w"):
        name = "%d:%s" % (T.CRAFTED_SEED, case)
    elif case == "only_stereo":
        opt = dict(only_stereo=True)
    elif case == "coarse":
        opt = dict(coarse=True)
    elif case == "itself":
        pairs, kf2 = [(0, 0)], (0, 1)
    elif case == "families":
        name = T.RANDOM_SEEDS[0]
    got = run(ex, T.scene(name), pairs, (0, 0), kf2, **opt)
    T.assert_equals_walk(name, got, pairs, **opt)
    if case == "zero_w":                                                           # infinity flowed through and was accepted, on the GPU as in the walk
        T.assert_zero_fourth_component_reached(name)
        a, b = T.scene(name)["zero_w"]
        assert got[0][0, 0, a] == T.walk(name, 0, 1)["matches12"][a] >= 0
    if case in ("only_stereo", "coarse"):
        assert got[3][0] == 0                                                      # neither evaluates the geometry
    if case == "only_stereo":
        assert (got[2] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [1280, 1281])
def test_gpu_both_sides_of_the_staging_threshold(cap):
    """126 * capA + 1024 <= 163 328 holds for 1280 (keyframe 2's descriptors staged in LDS) and not for 1281 (read through L2)"""
    ex = extractor()
    got = run(ex, T.scene(T.CRAFTED_SEED), T.LOCAL_MAPPING[:2], (0, 0), (1, 1), cap=cap)
    T.assert_equals_walk(T.CRAFTED_SEED, got, T.LOCAL_MAPPING[:2])


@pytest.fixture(scope="module")
def tri_host(tmp_path_factory):
    return T.build_host(tmp_path_factory.mktemp("tri2gpu"))


@pytest.mark.gpu
def test_gpu_real_size_equals_the_host_compiled_kernel(tri_host):
    """1302 keypoints per eye, one keyframe against 4 neighbours, a 300-node vocabulary"""
    ex = extractor()
    s = S.make(21, cap=1302, n_points=1500, rigs=5, nan_rig=-1, skew=0.02, nodes=300, dup=40, decoys=8)
    pairs = [(0, b) for b in (1, 2, 3, 4)]
    assert min(len(e["kps"]) for kf in s["kfs"] for e in kf["eyes"]) > 900
    got = run(ex, s, pairs, (0, 0), (1, 1))
    want = T.host_search(tri_host, s, pairs, (0, 0), (1, 1))
    print("matches %s, triangulations %d of %d candidates within th_low (host, one lane per row: %d)" % (got[2].tolist(), got[3][0], got[3][1], want[3][0]))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2]) and np.array_equal(got[1], want[1])
    assert got[2].min() > 300 and got[3][1] == want[3][1]


@pytest.mark.gpu
def test_gpu_rejections():
    """ORBX_ERR_BAD_ARGUMENT (-2) / ORBX_ERR_UNSUPPORTED before any launch: the outputs keep their poison"""
    import torch
    ex = extractor()
    s = T.scene(T.CRAFTED_SEED)
    cap, P = s["cap"], 2
    d = dict((k, _dev(v)) for k, v in S.pack(s, T.LOCAL_MAPPING[:2], cap).items())
    m12 = torch.full((P, 2, cap), POISON, dtype=torch.int32, device="cuda"); out_pairs = torch.full((P, 2 * cap, 2), POISON, dtype=torch.int32, device="cuda")
    n = torch.full((P,), POISON, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    cams = (X.camera_kb8(*s["cams"][0]), X.camera_kb8(*s["cams"][1]))
    good = dict(n_pairs=P, kf1=(0, 0), kf2=(1, 1), d_feat_nodes=d["fn"], d_feat_idx=d["fi"], d_n_feat=d["nfeat"], d_kf1_mp_flags=d["fl1"],
                d_kf2_mp_flags=d["fl2"], d_poses=d["poses"], tlr=s["tlr"], cam_left=cams[0], cam_right=cams[1], d_kps=d["kps"], d_desc=d["desc"],
                d_n=d["nout"], capacity=cap, d_matches12=m12, d_pairs=out_pairs, d_n_matches=n)
    bad = []
    for k in ("d_feat_nodes", "d_feat_idx", "d_n_feat", "d_kf1_mp_flags", "d_kf2_mp_flags", "d_poses", "tlr", "cam_left", "cam_right", "d_kps", "d_desc",
              "d_n", "d_matches12", "d_pairs", "d_n_matches"):
        bad.append({k: None})
    bad += [dict(n_pairs=0), dict(capacity=0), dict(kf1=(-1, 0)), dict(kf2=(0, -1)), dict(kf1=(0, -1)), dict(nlevels=7), dict(nlevels=9)]
    for change in bad:
        with pytest.raises(X.OrbxError) as e:
            ex.search_for_triangulation_two_eyes_device(**dict(good, **change))
        assert e.value.code == -2, (change, e.value.code)
    for capacity in (2609, 100000):                                                # 62 * capA + 1024 > 163 328
        with pytest.raises(X.OrbxError) as e:
            ex.search_for_triangulation_two_eyes_device(**dict(good, capacity=capacity))
        assert e.value.code == ORBX_ERR_UNSUPPORTED and "LDS" in str(e.value), (e.value.code, str(e.value))
    z = torch.zeros(8, device="cuda")
    for call in (lambda: ex.kb8_unproject_device(0, z, cams[0], z), lambda: ex.kb8_unproject_device(4, None, cams[0], z),
                 lambda: ex.kb8_unproject_device(4, z, None, z), lambda: ex.kb8_unproject_device(4, z, cams[0], None),
                 lambda: ex.kb8_triangulate_device(0, z, z, cams[0], cams[1], np.eye(3, dtype=f32), np.zeros(3, f32), 1.0, 1.0, z, z),
                 lambda: ex.kb8_triangulate_device(2, z, None, cams[0], cams[1], np.eye(3, dtype=f32), np.zeros(3, f32), 1.0, 1.0, z, z),
                 lambda: ex.kb8_triangulate_device(2, z, z, cams[0], cams[1], None, np.zeros(3, f32), 1.0, 1.0, z, z),
                 lambda: ex.kb8_triangulate_device(2, z, z, cams[0], cams[1], np.eye(3, dtype=f32), np.zeros(3, f32), 1.0, 1.0, z, None)):
        with pytest.raises(X.OrbxError) as e:
            call()
        assert e.value.code == -2
    ex.synchronize()
    assert (m12.cpu().numpy() == POISON).all() and (out_pairs.cpu().numpy() == POISON).all() and (n.cpu().numpy() == POISON).all()      # nothing was launched
    assert X.load_library().orbx_search_for_triangulation_two_eyes_device(None, *([0] * 26)) == -2
    assert X.load_library().orbx_debug_search_triangulation_two_eyes_stats(None) == -2


@pytest.fixture(scope="module")
def kb8_host(tmp_path_factory):
    return M.build_kb8_unproject_host(tmp_path_factory.mktemp("kb8ugpu"))


@pytest.mark.gpu
def test_gpu_unproject_equals_the_host_compiled_header(kb8_host):
    """4096 pixels: the image and a margin, the principal point, far outside (theta_d clamps), NaN and infinity"""
    import torch
    ex = extractor()
    rng = np.random.default_rng(2)
    cam = S.CAMS[1]
    uv = rng.uniform(-100, 612, (4096, 2)).astype(f32)
    uv[0] = cam[2:4]; uv[1] = (1e6, -1e6); uv[2] = (np.nan, 3.0); uv[3] = (np.inf, 7.0); uv[4] = cam[2:4] + f32(1e-5)
    want = np.zeros((4096, 2), f32)
    kb8_host.kb8u_unproject(M.ptr(cam), 4096, M.ptr(uv), M.ptr(want))
    d_uv = _dev(uv); d_rays = torch.full((4096, 3), 7.0, device="cuda")
    torch.cuda.synchronize()
    ex.kb8_unproject_device(4096, d_uv, cam, d_rays)
    ex.synchronize()
    rays = d_rays.cpu().numpy()
    assert rays[:, :2].tobytes() == want.tobytes() or np.array_equal(rays[:, :2].view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)])
    assert np.array_equal(np.isnan(rays[:, :2]), np.isnan(want)) and (rays[:, 2] == 1.0).all()


@pytest.mark.gpu
def test_gpu_triangulate_equals_the_host_compiled_header(kb8_host):
    """4096 keypoint pairs of the crafted scene's keyframes 0 (left) and 1 (right): true partners, wrong pairs, NaN"""
    import torch
    ex = extractor()
    s = T.scene(T.CRAFTED_SEED)
    rng = np.random.default_rng(4)
    cam1, cam2 = S.CAMS
    R12, t12 = S.relative64(s["kfs"][0]["pose"], s["kfs"][1]["pose"], 0, 1)
    R12 = np.ascontiguousarray(R12, f32); t12 = np.ascontiguousarray(t12, f32)
    e1, e2 = s["kfs"][0]["eyes"][0], s["kfs"][1]["eyes"][1]
    n = 4096
    i1 = rng.integers(0, len(e1["kps"]), n); i2 = rng.integers(0, len(e2["kps"]), n)
    by_point = {id(f["p"]): j for j, f in enumerate(e2["feats"])}
    for a in range(n // 2):                                                        # half of them a keypoint and its point's keypoint in the other frame
        j = by_point.get(id(e1["feats"][i1[a]]["p"]))
        if j is not None:
            i2[a] = j
    kp1 = np.stack([e1["kps"]["x"][i1], e1["kps"]["y"][i1]], 1).astype(f32); kp2 = np.stack([e2["kps"]["x"][i2], e2["kps"]["y"][i2]], 1).astype(f32)
    kp1[n // 2:] += rng.uniform(-0.3, 0.3, (n - n // 2, 2)).astype(f32)           # (not all the same few values)
    kp2[-1] = np.nan
    z = np.zeros(n, f32); x = np.zeros((n, 3), f32); why = np.zeros(n, np.int32)
    kb8_host.kb8u_triangulate(M.ptr(cam1), M.ptr(cam2), M.ptr(R12), M.ptr(t12), 1.0, 1.44, n, M.ptr(kp1), M.ptr(kp2), M.ptr(z), M.ptr(x), M.ptr(why))
    assert (z > 0.0001).sum() > 200 and len(set(why.tolist())) >= 4, np.bincount(why).tolist()
    d_z = torch.full((n,), 7.0, device="cuda"); d_x = torch.full((n, 3), 7.0, device="cuda")
    d1, d2 = _dev(kp1), _dev(kp2)
    torch.cuda.synchronize()
    ex.kb8_triangulate_device(n, d1, d2, cam1, cam2, R12, t12, 1.0, 1.44, d_z, d_x)
    ex.synchronize()
    gz, gx = d_z.cpu().numpy(), d_x.cpu().numpy()
    fin = ~np.isnan(z)
    assert np.array_equal(np.isnan(gz), np.isnan(z)) and gz[fin].tobytes() == z[fin].tobytes()
    finx = ~np.isnan(x)
    assert np.array_equal(np.isnan(gx), np.isnan(x)) and gx[finx].tobytes() == x[finx].tobytes()


@pytest.mark.gpu
def test_gpu_zero_fourth_component_equals_the_host_compiled_header(kb8_host):
    """R12 = diag(1, 1, 0): vt.row(3) = (0, 0, 1, 0), x3D = (NaN, NaN, inf), the result inf (tests/test_kb8_unproject_math.py holds the
    header to the walk on the same pairs and shows that w == 0 occurred)"""
    import torch
    ex = extractor()
    cam1, cam2 = S.CAMS
    R12, t12, kp1, kp2 = M.zero_w_pairs()
    n = len(kp1)
    z = np.zeros(n, f32); x = np.zeros((n, 3), f32)
    kb8_host.kb8u_triangulate(M.ptr(cam1), M.ptr(cam2), M.ptr(R12), M.ptr(t12), 1.0, 1.0, n, M.ptr(kp1), M.ptr(kp2), M.ptr(z), M.ptr(x), None)
    assert np.isposinf(z[0]) and np.isposinf(x[0, 2])
    d_z = torch.full((n,), 7.0, device="cuda"); d_x = torch.full((n, 3), 7.0, device="cuda")
    d1, d2 = _dev(kp1), _dev(kp2)
    torch.cuda.synchronize()
    ex.kb8_triangulate_device(n, d1, d2, cam1, cam2, R12, t12, 1.0, 1.0, d_z, d_x)
    ex.synchronize()
    assert M.same_floats(d_z.cpu().numpy(), z) and M.same_floats(d_x.cpu().numpy(), x)
