"""The two-camera SearchForTriangulation without a GPU: extractorb_amd/csrc/k_triangulate_match_two_eyes.hip compiled for the host
(tests/cpp/triangulation_two_eyes_host_check.cpp: the kernel's own stage / slot / segment / row functions, a row being one lane) against the
sequential walk (tests/triangulation_two_eyes_walk.py) on the scenes of tests/triangulation_two_eyes_scenes.py, byte for byte:
  (a) random scenes with descriptor families (every feature of a node within TH_LOW of every other: hundreds of wrong pairs reach the
      geometry and land near every threshold);
  (b) a crafted scene in which every counter of the walk is above zero: rejections by parallax, z1, z2, error 1 and error 2, candidates
      dropped for a MapPoint, equal-distance replacements, all four eye combinations accepted, removals by the rotation histogram;
  (c) edge scenes: an empty right eye, NLeft = 0, a zero fourth component of the triangulated vector (infinity flows through and is
      accepted, as in the reference), nodes present in one eye only, only_stereo = 1 returning 0, coarse = 1, a keyframe against
      itself (identical rays in the left-left and right-right combinations), a NaN pose that ends with no match;
and an INDEPENDENT margin check: a float64 statement of the geometric test (np.linalg.svd, math.tan, math.atan2) gives the same accept /
reject as the binary32 walk on every candidate pair the walk tests, and finds no candidate within a factor 2 of a gate, within 2e-5 of 0.9998
in cosParallaxRays or with |z| below 1e-3 (a factor 10 of the 0.0001 limit).  The seeds below satisfy that.
Both host programs (this kernel's and the camera header's) run under -fsanitize=address,undefined as stand-alone programs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import triangulation_two_eyes_scenes as S
import triangulation_two_eyes_walk as W
from test_kb8_math import HOST_FLAGS, ROOT

f32 = np.float32
VP = C.c_void_p
RANDOM_SEEDS = ("f11", "f12")                 # descriptor families: hundreds of wrong pairs reach the geometry, near every threshold by chance
CRAFTED_SEED = 1
MARGIN_SEEDS = (1, 3, 4)
LOCAL_MAPPING = [(0, 1), (0, 2), (0, 3)]      # kf1_step = 0: one keyframe against three neighbours, the third with a NaN pose


def build_host(directory):
    so = os.path.join(str(directory), "libtri_two_eyes_host.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", *HOST_FLAGS, os.path.join(ROOT, "tests", "cpp", "triangulation_two_eyes_host_check.cpp"),
                           "-o", so])
    L = C.CDLL(so)
    L.tri_two_eyes_host.argtypes = [C.c_int] * 5 + [VP] * 11 + [C.c_int, VP] + [C.c_int] * 6 + [VP] * 4
    L.tri_two_eyes_relative.argtypes = [VP] * 3 + [C.c_int, VP]
    L.tri_two_eyes_lds_bytes.restype = C.c_long
    L.tri_two_eyes_lds_bytes.argtypes = [C.c_int, C.c_int]
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("tri2"))


_SCENES, _WALKS = {}, {}


def scene(name):
    """'seed', 'f' + seed (descriptor families) or 'seed:variant'"""
    if name not in _SCENES:
        seed, _, var = str(name).partition(":")
        _SCENES[name] = S.variant(scene(seed), var) if var else S.make(int(seed.lstrip("f")), families=seed.startswith("f"),
                                                                       decoys=0 if seed.startswith("f") else 6)
    return _SCENES[name]


def walk(name, a, b, trace=None, **opt):
    key = (name, a, b, tuple(sorted(opt.items())))
    if key not in _WALKS or trace is not None:
        s = scene(name)
        _WALKS[key] = W.search_for_triangulation(W.libm_math(), s["kfs"][a], s["kfs"][b], s["tlr"], s["cams"], s["sigma2"], trace=trace, **opt)
    return _WALKS[key]


def ptr(a):
    return a.ctypes.data_as(VP)


def host_search(host, s, pairs, kf1, kf2, stage=False, only_stereo=False, coarse=False, th_low=50, check_orientation=True, cap=None):
    cap = cap or s["cap"]
    d = S.pack(s, pairs, cap)
    P = len(pairs)
    m12 = np.full((P, 2, cap), -7, np.int32); out_pairs = np.full((P, 2 * cap, 2), -7, np.int32); n = np.full(P, -7, np.int32)
    stats = np.zeros(2, np.int32)
    cams = np.concatenate(s["cams"]).astype(f32)
    host.tri_two_eyes_host(P, kf1[0], kf1[1], kf2[0], kf2[1], ptr(d["fn"]), ptr(d["fi"]), ptr(d["nfeat"]), ptr(d["fl1"]), ptr(d["fl2"]), ptr(d["poses"]),
                           ptr(np.ascontiguousarray(s["tlr"], f32)), ptr(cams), ptr(d["kps"]), ptr(d["desc"]), ptr(d["nout"]), cap, ptr(s["sigma2"]), 8,
                           int(only_stereo), int(coarse), th_low, int(check_orientation), int(stage), ptr(m12), ptr(out_pairs), ptr(n), ptr(stats))
    return m12, out_pairs, n, stats


def assert_equals_walk(name, got, pairs, **opt):
    """d_matches12 per eye (all capacity entries written), d_pairs in stacked numbering, d_n_matches"""
    m12, out_pairs, n = got[:3]
    s = scene(name)
    for p, (a, b) in enumerate(pairs):
        want = walk(name, a, b, **opt)
        what = "%s pair %d (%d, %d) %r" % (name, p, a, b, opt)
        nl = len(s["kfs"][a]["eyes"][0]["kps"]); nr = len(s["kfs"][a]["eyes"][1]["kps"])
        assert m12[p, 0, :nl].tolist() == want["matches12"][:nl] and m12[p, 1, :nr].tolist() == want["matches12"][nl:], what
        assert (m12[p, 0, nl:] == -1).all() and (m12[p, 1, nr:] == -1).all(), what
        assert int(n[p]) == want["n"] == len(want["pairs"]), what
        assert [tuple(x) for x in out_pairs[p, :want["n"]].tolist()] == want["pairs"], what
        assert (out_pairs[p, want["n"]:] == -7).all(), what                       # entries from d_n_matches on are left as they were


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
@pytest.mark.parametrize("stage", [False, True])
def test_host_kernel_equals_the_walk_on_random_scenes(host, seed, stage):
    got = host_search(host, scene(seed), LOCAL_MAPPING, (0, 0), (1, 1), stage=stage)
    assert_equals_walk(seed, got, LOCAL_MAPPING)
    assert sum(walk(seed, a, b)["n"] for a, b in LOCAL_MAPPING[:2]) > 20


def test_the_crafted_scene_reaches_every_branch(host):
    pairs = LOCAL_MAPPING[:2]
    total = {}
    for a, b in pairs:
        w = walk(CRAFTED_SEED, a, b)
        for k in ("mp", "parallax", "z1", "z2", "error1", "error2", "equal", "removals", "tests", "within"):
            total[k] = total.get(k, 0) + w[k]
        total["combos"] = [x + y for x, y in zip(total.get("combos", [0] * 4), w["combos"])]
    print(total)
    assert all(total[k] > 0 for k in ("mp", "parallax", "z1", "z2", "error1", "error2", "equal", "removals")), total
    assert all(c > 0 for c in total["combos"]), total                              # left-left, left-right, right-left, right-right
    s = scene(CRAFTED_SEED)
    # a node both eyes of keyframe 2 hold with more than 16 candidates, and nodes only one eye holds
    fv = dict(W.stacked_feature_vector(s["kfs"][1]))
    assert max(len(v) for v in fv.values()) > 16
    left = set(s["kfs"][0]["eyes"][0]["fv"][0].tolist()); right = set(s["kfs"][0]["eyes"][1]["fv"][0].tolist())
    assert left - right and right - left
    for stage in (False, True):
        got = host_search(host, s, pairs, (0, 0), (1, 1), stage=stage)
        assert_equals_walk(CRAFTED_SEED, got, pairs)
    # the row ranks by Hamming key first: fewer triangulations than the walk's list-order scan, and than candidates within th_low
    assert 0 < got[3][0] < total["tests"] and got[3][0] < got[3][1] == total["within"], (got[3], total)


def assert_zero_fourth_component_reached(name):
    """the crafted pair of scene `name` (a ':zero_w' variant) is tested, its vt.row(3) has a zero fourth component, TriangulateMatches
    returns infinity on it and epipolarConstrain accepts it"""
    s = scene(name)
    a, b = s["zero_w"]
    trace = []
    walk(name, 0, 1, trace=trace)
    hit = [t for t in trace if t[0] == a and t[1] == b]
    assert len(hit) == 1 and hit[0][2] and np.isposinf(hit[0][3]), hit
    from fuse_two_eyes_walk import keyframe_rig
    R12, t12 = W.eye_relative(keyframe_rig(s["kfs"][0]["pose"], s["tlr"]), keyframe_rig(s["kfs"][1]["pose"], s["tlr"]), 0, 0)
    assert R12.tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 0]] and t12.tolist() == [0.5, 0, 0]
    k1, k2 = s["kfs"][0]["eyes"][0]["kps"][a], s["kfs"][1]["eyes"][0]["kps"][b]
    dbg = {}
    z, x3d, why = W.triangulate_matches(W.libm_math(), S.CAMS[0], S.CAMS[0], (k1["x"], k1["y"]), (k2["x"], k2["y"]), R12, t12, 1.0, 1.0, debug=dbg)
    assert [float(v) for v in dbg["vt"]] == [0, 0, 1, 0] and why == W.OK and np.isposinf(z)
    assert np.isnan(x3d[0]) and np.isnan(x3d[1]) and np.isposinf(x3d[2])


@pytest.mark.parametrize("case", ["empty_right_eye", "nleft_zero", "zero_w", "only_stereo", "coarse", "itself", "nan_pose", "no_orientation", "th_low_0"])
def test_edge_scenes(host, case):
    name, pairs, kf2, opt = CRAFTED_SEED, LOCAL_MAPPING[:2], (1, 1), {}
    if case in ("empty_right_eye", "nleft_zero", "zero_w"):
        name = "%d:%s" % (CRAFTED_SEED, case)
    elif case == "only_stereo":
        opt = dict(only_stereo=True)
    elif case == "coarse":
        opt = dict(coarse=True)
    elif case == "itself":
        pairs, kf2 = [(0, 0)], (0, 1)
    elif case == "nan_pose":
        pairs, kf2 = [(0, 3)], (3, 1)
    elif case == "no_orientation":
        opt = dict(check_orientation=False)
    elif case == "th_low_0":
        opt = dict(th_low=0)
    got = host_search(host, scene(name), pairs, (0, 0), kf2, **opt)
    assert_equals_walk(name, got, pairs, **opt)
    n = [walk(name, a, b, **opt)["n"] for a, b in pairs]
    if case == "zero_w":
        assert_zero_fourth_component_reached(name)
    if case in ("only_stereo", "nan_pose"):
        assert n == [0] * len(pairs)                                               # bStereo1 is false by construction; NaN > 0.0001f rejects
    elif case == "itself":
        w = walk(name, 0, 0)
        assert w["combos"][0] == 0 and w["combos"][3] == 0 and w["parallax"] > 20 and n[0] > 0      # identical rays: left-right and right-left only
    elif case == "coarse":
        assert walk(name, 0, 1, coarse=True)["tests"] == 0 and n[0] > walk(name, 0, 1)["n"]
    elif case != "th_low_0":
        assert min(n) > 0


@pytest.mark.parametrize("seed", MARGIN_SEEDS)
def test_float64_statement_agrees_with_margin(seed):
    """every candidate pair the binary32 walk tests: the float64 statement decides the same and no threshold is near"""
    s = scene(seed)
    tested = 0
    for a, b in LOCAL_MAPPING[:2] + [(0, 0)]:
        trace = []
        walk(seed, a, b, trace=trace)
        n1, n2 = len(s["kfs"][a]["eyes"][0]["kps"]), len(s["kfs"][b]["eyes"][0]["kps"])
        for idx1, idx2, ok, _z in trace:
            e1, e2 = int(idx1 >= n1), int(idx2 >= n2)
            k1 = s["kfs"][a]["eyes"][e1]["kps"][idx1 - e1 * n1]; k2 = s["kfs"][b]["eyes"][e2]["kps"][idx2 - e2 * n2]
            R12, t12 = S.relative64(s["kfs"][a]["pose"], s["kfs"][b]["pose"], e1, e2)
            ok64, margins = S.triangulate64(S.CAMS[e1], S.CAMS[e2], (k1["x"], k1["y"]), (k2["x"], k2["y"]), R12, t12,
                                            S.SIGMA2[k1["octave"]], S.SIGMA2[k2["octave"]])
            assert S.margins_hold(margins), (seed, a, b, idx1, idx2, margins)
            assert ok64 == ok, (seed, a, b, idx1, idx2, margins)
            tested += 1
    assert tested > 100


def test_relative_poses_as_the_walk(host):
    s = scene(CRAFTED_SEED)
    from fuse_two_eyes_walk import keyframe_rig
    from fuse_walk import gemm_row
    for b in (1, 2):
        rig1, rig2 = keyframe_rig(s["kfs"][0]["pose"], s["tlr"]), keyframe_rig(s["kfs"][b]["pose"], s["tlr"])
        for combo in range(4):
            R12, t12 = W.eye_relative(rig1, rig2, combo >> 1, combo & 1)
            t21 = np.array([gemm_row(R12.T[r], t12, -1.0) for r in range(3)], f32)
            out = np.zeros(12, f32)
            host.tri_two_eyes_relative(ptr(np.ascontiguousarray(s["kfs"][0]["pose"], f32)), ptr(np.ascontiguousarray(s["kfs"][b]["pose"], f32)),
                                       ptr(np.ascontiguousarray(s["tlr"], f32)), combo, ptr(out))
            assert out[:9].tobytes() == R12.tobytes() and out[9:].tobytes() == t21.tobytes(), (b, combo)


def test_the_scenes_level_table_is_the_handles():
    import extractorb_amd as X
    assert S.SIGMA2.tobytes() == X.compute_tables(1000, 1.2, 8)["level_sigma2"].tobytes()


def test_lds_formula(host):
    """62 bytes per slot of the per-eye capacity rounded up to 16, 126 staged, + 1024, against 163 328"""
    budget = 160 * 1024 - 512
    assert host.tri_two_eyes_lds_bytes(1302, 0) == 62 * 1312 + 1024 <= budget          # 2 x 1302 keypoints fit unstaged
    assert host.tri_two_eyes_lds_bytes(1302, 1) > budget
    assert host.tri_two_eyes_lds_bytes(2608, 0) <= budget < host.tri_two_eyes_lds_bytes(2609, 0)
    assert host.tri_two_eyes_lds_bytes(1280, 1) <= budget < host.tri_two_eyes_lds_bytes(1281, 1)


@pytest.mark.parametrize("source,define", [("triangulation_two_eyes_host_check.cpp", "TRI_TWO_EYES_HOST_MAIN"),
                                           ("kb8_unproject_host_check.cpp", "KB8_UNPROJECT_HOST_MAIN")])
def test_host_programs_run_clean_under_the_sanitizers(tmp_path, source, define):
    exe = str(tmp_path / "prog")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-D" + define, *HOST_FLAGS,
                           os.path.join(ROOT, "tests", "cpp", source), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and "runtime error" not in out.stdout and "AddressSanitizer" not in out.stdout, out.stdout[-3000:]
