"""ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) for two-camera frames (reference src/ORBmatcher.cc:1961-2177,
CurrentFrame.Nleft != -1; caller Tracking::TrackWithMotionModel) and KannalaBrandt8::project (src/CameraModels/KannalaBrandt8.cpp:28-44).
CPU: the checker (tests/last_frame_two_eyes_walk.py) pinned by the one-eye oracle on its left half and by the device headers compiled for
the host; the crafted scenes, each asserted to reach what it was built for; the front half as a sanitized stand-alone program; the C
surface.  GPU: orbx_kb8_project_device, orbx_project_last_frame_two_eyes_device and orbx_search_last_frame_two_eyes_device against the
host-compiled header and the walk, byte for byte, each case twice over poisoned outputs."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import extractorb_amd as X
import helpers
import last_frame_two_eyes_scenes as S
import last_frame_two_eyes_walk as W
import oracle_lib as O
from test_kb8_math import HOST_FLAGS, ROOT, build_kb8_host

f32 = np.float32
CAP_1200 = 1302                # orbx_max_keypoints() of a 1200-feature extractor (asserted on the GPU)
LDS_LIMIT = 160 * 1024 - 512
_cache = {}


def lds_bytes(capacity):
    """the bound the header documents: 96 * ((capacity + 3) & ~3) + 12 * capacity + 12 496 <= 163 328"""
    return 96 * ((capacity + 3) & ~3) + 12 * capacity + 12496


class HostParams(C.Structure):      # == ProjectTwoEyesParams of extractorb_amd/csrc/orbx_params.hpp
    _fields_ = [("cam", C.c_float * 8), ("minX", C.c_float), ("maxX", C.c_float), ("minY", C.c_float), ("maxY", C.c_float),
                ("scale", C.c_float * 16), ("trl", C.c_float * 12), ("mb", C.c_float), ("th", C.c_float), ("mono", C.c_int),
                ("capacity", C.c_int), ("lastFirst", C.c_int), ("lastStep", C.c_int), ("curFirst", C.c_int), ("curStep", C.c_int)]


@pytest.fixture(scope="module")
def kb8(tmp_path_factory):
    return build_kb8_host(tmp_path_factory.mktemp("kb8"))


@pytest.fixture(scope="module")
def front_host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("l2e") / "liblast_two_eyes_host.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", *HOST_FLAGS, os.path.join(ROOT, "tests", "cpp", "last_two_eyes_host_check.cpp"), "-o", so])
    L = C.CDLL(so)
    assert L.last_two_eyes_host_params_size() == C.sizeof(HostParams)
    offsets = (C.c_int * len(HostParams._fields_))()
    assert L.last_two_eyes_host_params_offsets(offsets, len(offsets)) == len(offsets)      # field by field, in the struct's own order
    assert list(offsets) == [getattr(HostParams, name).offset for name, _ in HostParams._fields_]
    return L


def libm():
    return _cache.setdefault("libm", W.libm_math())


# ---------------------------------------------------------------- the front-half cases ----------------------------------------------------------------
def front_cases():
    """name -> (rigs, poses, [(last rig, current rig)], capacity, mono), shared by the CPU and the GPU tests"""
    if "front" not in _cache:
        rigs, poses, pairs = S.crafted_front_half(5)
        full = S.full_front_half(600)
        mv, mp = _moving()
        _cache["front"] = {
            "crafted": (rigs, poses, [(l, 0) for l, _ in pairs], 5, False),
            "crafted_mono": (rigs, poses, [(l, 0) for l, _ in pairs], 5, True),
            "full": (full[0], full[1], [(1, 0)], 600, False),
            "moving": (mv, mp, [(0, 1), (1, 2)], _moving_capacity(), False),
        }
    return _cache["front"]


def _moving():
    return _cache.setdefault("moving", S.moving_rigs(1, n_rigs=3))


def _moving_capacity():
    return max(len(E["k"]) for rig in _moving()[0] for E in rig) + 3


def front_walk(name, m=None, tag="libm"):
    key = ("front_walk", name, tag)
    if key not in _cache:
        rigs, poses, pairs, cap, mono = front_cases()[name]
        _cache[key] = [S.walk_front_half(m or libm(), rigs, poses, l, c, cap, mono) for l, c in pairs]
    return _cache[key]


def test_crafted_last_rig_meets_every_exit_in_each_eye_half_under_each_level_form():
    rigs, poses, pairs = S.crafted_front_half(5)
    walks = front_walk("crafted")
    assert len(pairs) == 12 and all(len(E["k"]) <= 5 for rig in rigs for E in rig)
    seen = {}
    for (last, form), (q, ex, got_form) in zip(pairs, walks):
        assert got_form == form
        for e in (0, 1):
            for j in range(e * 5, e * 5 + len(rigs[last][e]["k"])):
                seen.setdefault((form, e), set()).add(int(ex[j]))
                if ex[j] == W.EXIT_REQUEST:
                    octave = int(rigs[last][e]["k"]["octave"][j - e * 5])
                    want = dict(forward=(octave, -1), backward=(0, octave), neither=(octave - 1, octave + 1))[form]
                    assert (int(q[j, 0]["min_level"]), int(q[j, 0]["max_level"])) == want == (int(q[j, 1]["min_level"]), int(q[j, 1]["max_level"]))
                    assert q[j, 0]["flags"] == q[j, 1]["flags"] and q[j, 0]["flags"] & 1
                    assert (q[j, 1]["u"], q[j, 1]["v"]) != (q[j, 0]["u"], q[j, 0]["v"])          # mTrl moves the right projection
    for form in ("forward", "backward", "neither"):
        for e in (0, 1):
            assert seen[(form, e)] == set(range(8)), (form, e, seen[(form, e)])
    # the thresholds: consecutive crafted points are adjacent floats of one coordinate on the two sides of the comparison
    pts = S.crafted_points()
    for a in range(3, 13, 2):
        d = sorted(abs(S.ordered_bits(u) - S.ordered_bits(v)) for u, v in zip(pts[a][0], pts[a + 1][0]))
        assert d == [0, 0, 1]
        assert (S.exit_of(libm(), pts[a][0]) == W.EXIT_REQUEST) != (S.exit_of(libm(), pts[a + 1][0]) == W.EXIT_REQUEST)
    # bMono overrides the level forms
    for (last, form), (q, ex, got_form) in zip(pairs, front_walk("crafted_mono")):
        assert got_form == "neither"


def test_walk_with_libm_equals_walk_with_the_host_compiled_header(kb8):
    hm = W.header_math(kb8)
    requests = 0
    for name in front_cases():
        for (q, ex, form), (q2, ex2, form2) in zip(front_walk(name), front_walk(name, hm, "header")):
            assert q.tobytes() == q2.tobytes() and np.array_equal(ex, ex2) and form == form2, name
            requests += int((ex == W.EXIT_REQUEST).sum())
    assert requests > 1000


def host_front_half(lib, name):
    rigs, poses, pairs, cap, mono = front_cases()[name]
    k, n, fl, w = S.front_half_arrays(rigs, cap)
    out = []
    for last, cur in pairs:
        p = HostParams()
        p.cam[:] = S.CAM.tolist(); p.minX, p.maxX, p.minY, p.maxY = [float(b) for b in S.BOUNDS]
        sc = S.scales()
        p.scale[:] = [float(sc[min(l, len(sc) - 1)]) for l in range(16)]
        p.trl[:] = S.TRL.reshape(-1).tolist()
        p.mb, p.th, p.mono, p.capacity, p.lastFirst, p.lastStep, p.curFirst, p.curStep = S.MB, S.TH, int(mono), cap, last, 0, cur, 0
        q = np.zeros((2 * cap, 2), O.PROJ_QUERY_DTYPE); ex = np.zeros(2 * cap, np.int32)
        lib.last_two_eyes_host(k.ctypes.data_as(C.c_void_p), n.ctypes.data_as(C.c_void_p), fl.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p),
                               np.ascontiguousarray(poses).ctypes.data_as(C.c_void_p), C.byref(p), 1, q.ctypes.data_as(C.c_void_p),
                               ex.ctypes.data_as(C.c_void_p))
        out.append((q, ex))
    return out


def test_front_half_compiled_for_the_host_equals_the_walk(front_host):
    merged = {W.EXIT_NO_MAPPOINT: 0, W.EXIT_OUTLIER: 0, W.EXIT_NEG_DEPTH: 1, W.EXIT_LEFT_OF: 2, W.EXIT_RIGHT_OF: 2, W.EXIT_ABOVE: 2, W.EXIT_BELOW: 2,
              W.EXIT_REQUEST: 3, -1: 0}
    for name in front_cases():
        for (q, ex), (wq, wex, _) in zip(host_front_half(front_host, name), front_walk(name)):
            assert q.tobytes() == wq.tobytes(), name
            assert ex.tolist() == [merged[int(v)] for v in wex], name


def test_front_half_stays_inside_its_arrays_as_a_sanitized_host_program(tmp_path):
    """the per-request front half as a stand-alone program under AddressSanitizer + UBSan: exact-size buffers, counts outside [0, capacity],
    coordinates that are 0, infinite and NaN"""
    exe = str(tmp_path / "last_two_eyes_host_check")
    subprocess.check_call(["g++", "-O1", "-g", "-DLAST_TWO_EYES_HOST_MAIN", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", *HOST_FLAGS,
                           os.path.join(ROOT, "tests", "cpp", "last_two_eyes_host_check.cpp"), "-o", exe])
    out = subprocess.check_output([exe], text=True)
    assert out.count("trial") == 6 and out.strip().endswith("clean") and "inconsistent" not in out


# ---------------------------------------------------------------- the search cases ----------------------------------------------------------------
@pytest.mark.parametrize("seed,orientation", [(1, True), (2, False), (3, True), (4, False)])
def test_walk_left_half_equals_the_one_eye_oracle(seed, orientation):
    """every R request off, the requests given: the walk's L half is the one-eye frame-to-frame search on the raw keypoints and mGrid"""
    rng = np.random.default_rng(seed)
    s = S.random_requests(rng, nl=500, nr=300, nq=600, clusters=6 if seed > 2 else 0)
    s["q"][:, 1]["flags"] = 0
    got = S.walk_search(s, orientation)
    L = s["left"]
    nm, m, o = O.search_by_projection(s["q"][:, 0], s["qd"], L["k"], L["d"], L["off"], L["idx"], s["bounds"], None, s["occ"][0], False, 0.9,
                                      orientation, 100)
    assert got["n"] == nm and got["matches"][0] == m.tolist() and got["occupied"][0] == o.tolist()
    assert got["matches"][1] == [-1] * len(s["right"]["k"]) and got["occupied"][1] == s["occ"][1].tolist()
    assert nm > 100 and (not orientation or got["dropped"] > 0)


def without(s, eye_index):
    """the scene with every request of one eye off"""
    t = dict(s, q=s["q"].copy())
    t["q"][:, eye_index]["flags"] &= ~1
    return t


def assert_consequence(name, s, got):
    """what each crafted scene was built for, asserted on the walk's result"""
    acc = got["accepted"].tolist()
    if name == "closure_chain":
        assert acc == [[0, 1], [1, 2], [2, 0], [-1, 3]] and got["closure_changed"] == 6 and got["n"] == 7
    elif name == "overwritten":
        assert acc == [[0, 0], [0, 0], [-1, -1]] and got["matches"] == [[1], [1]] and got["n"] == 4
    elif name == "ties":
        assert acc == [[2, 1]]                              # the last / the second keypoint: first in the traversal, not in the index
    elif name == "empty_left_suppresses_right":
        assert got["suppressed"] == 1 and acc == [[-1, -1], [1, 1]] and got["n"] == 2
        assert S.walk_search(without(s, 0))["accepted"].tolist() == [[-1, 0], [-1, 1]]      # alone, the suppressed R matches
    elif name == "left_above_th_high":
        assert acc == [[-1, 0], [-1, 1]] and got["suppressed"] == 0 and got["n"] == 2
    elif name == "right_off_grid":
        assert acc == [[0, -1], [-1, -1]] and got["n"] == 1
    elif name == "two_bins_one_dropped":
        assert got["bins"][0] == 26 and got["bins"][5] == 1 and got["maxima"] == (0, -1, -1) and got["dropped"] == 1
        assert acc[0] == [0, 0] and acc[13] == [0, -1] and got["matches"][0][0] == -1 and got["n"] == 26
    elif name == "joint_histogram":
        assert got["maxima"] == (3, 0, 1) and got["n"] == 26
        left, right = S.walk_search(without(s, 1)), S.walk_search(without(s, 0))
        assert left["maxima"] == (0, 1, 2) and right["maxima"] == (3, 4, -1) and left["n"] + right["n"] == 29 != got["n"]
    else:
        raise AssertionError(name)


CRAFTED = ["closure_chain", "overwritten", "ties", "empty_left_suppresses_right", "left_above_th_high", "right_off_grid", "two_bins_one_dropped",
           "joint_histogram"]


@pytest.mark.parametrize("name", CRAFTED)
def test_walk_on_crafted_scenes(name):
    s = S.crafted_scenes()[name]
    assert_consequence(name, s, S.walk_search(s))


def chained(last, cur):
    key = ("chained", last, cur)
    if key not in _cache:
        rigs, poses = _moving()
        s, ex = S.chained_scene(libm(), rigs, poses, last, cur, _moving_capacity())
        _cache[key] = (s, ex, S.walk_search(s))
    return _cache[key]


def test_chained_scene_is_not_too_easy():
    rigs, _ = _moving()
    assert 280 <= len(rigs[1][0]["k"]) <= 320
    for last, cur in ((0, 1), (1, 2)):
        s, ex, got = chained(last, cur)
        asked = int((s["q"][:, 0]["flags"] & 1).sum())
        taken = int((got["accepted"] >= 0).any(1).sum())
        assert asked > 300 and 3 * taken >= asked and got["closure_changed"] >= 1, (asked, taken, got["closure_changed"])


def test_entries_are_declared_documented_exported_and_check_their_arguments():
    names = ["orbx_kb8_project_device", "orbx_project_last_frame_two_eyes_device", "orbx_search_last_frame_two_eyes_device",
             "orbx_debug_last_frame_two_eyes_stats"]
    L = X.load_library()
    text = open(X.orbextractor._HEADER).read()
    for n in names:
        assert n in X.header_symbols() and hasattr(L, n)
        pos = text.index("int %s(" % n)
        assert "/*" in text[:pos] and len(text[text.rindex("/*", 0, pos):pos]) > 150, n
    doc = text[text.rindex("/*", 0, text.index("int orbx_search_last_frame_two_eyes_device(")):text.index("int orbx_search_last_frame_two_eyes_device(")]
    assert "ORBX_ERR_UNSUPPORTED" in doc and ":2024" in doc and "96 * ((capacity + 3) & ~3) + 12 * capacity + 12 496" in doc
    assert "typedef struct orbx_camera_kb8 { float fx, fy, cx, cy, k1, k2, k3, k4; } orbx_camera_kb8;" in text
    z = C.c_void_p(16)             # never dereferenced: the handle is checked first
    b = np.array([0, 512, 0, 512], f32).ctypes.data_as(C.c_void_p)
    assert L.orbx_kb8_project_device(None, 4, z, z, z) == -2
    assert L.orbx_project_last_frame_two_eyes_device(None, 1, 0, 1, 1, 1, z, z, 16, z, z, z, z, z, b, C.c_float(0.1), C.c_float(7), 0, z) == -2
    assert L.orbx_search_last_frame_two_eyes_device(None, 1, 0, 1, z, z, z, z, z, 16, z, z, b, None, 100, 1, z, z) == -2
    assert L.orbx_debug_last_frame_two_eyes_stats(None) == -2
    assert np.array_equal(X.camera_kb8(1, 2, 3, 4, 5, 6, 7, 8), np.arange(1, 9, dtype=f32))
    assert LDS_LIMIT == helpers.entry_lds_budget()
    assert max(c for c in range(1, 3000) if lds_bytes(c) <= LDS_LIMIT) >= CAP_1200          # the required envelope


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def structured_points():
    """a few thousand points: every pair of a coordinate list that holds 0, both signs, tiny, huge and ordinary values (z <= 0, x = y = 0
    and huge / tiny ratios among them), plus the atanf thresholds as exact ratios"""
    vals = np.array([0.0, -0.0, 1.0, -1.0, 0.3, -2.5, 7.0, 1e-30, -1e-30, 1e-38, 1e30, -1e30, 3e38, 123.456, -0.001], f32)
    pts = [(x, y, z) for x in vals for y in vals for z in vals]
    for t in (7 / 16, 11 / 16, 19 / 16, 39 / 16, 2.0 ** 25, 2.0 ** -29):
        for d in (-1, 0, 1):
            r = (np.array(t, f32).view(np.int32) + d).view(f32)
            pts += [(r, 0.0, 1.0), (0.0, -r, 1.0), (r * f32(2), 0.0, -2.0), (1.0, r, 1.0), (-2.0, r * f32(2), 3.0)]
    rng = np.random.default_rng(9)
    pts += [tuple(v) for v in rng.uniform(-10, 10, (600, 3)).astype(f32)]
    return np.array(pts, f32)


@pytest.mark.gpu
def test_gpu_kb8_project_equals_the_host_compiled_header(kb8):
    import torch
    xyz = structured_points()
    n = len(xyz)
    assert 3000 < n < 6000 and (xyz[:, 2] <= 0).sum() > 500 and ((xyz[:, 0] == 0) & (xyz[:, 1] == 0)).sum() > 10
    want = np.zeros((n, 2), f32)
    kb8.kb8_project(S.CAM.ctypes.data_as(C.c_void_p), n, xyz.ctypes.data_as(C.c_void_p), want.ctypes.data_as(C.c_void_p))
    assert np.isfinite(want).all()
    ex = X.ORBextractor(1000)
    d_xyz = _dev(xyz)
    runs = []
    for _ in range(2):
        d_uv = torch.full((n, 2), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ex.kb8_project_device(n, d_xyz, S.CAM, d_uv)
        ex.synchronize()
        runs.append(d_uv.cpu().numpy())
    assert runs[0].tobytes() == runs[1].tobytes()
    bad = np.nonzero((runs[0].view(np.uint32) != want.view(np.uint32)).any(1))[0]
    assert len(bad) == 0, (xyz[bad[:5]], runs[0][bad[:5]], want[bad[:5]])
    for change in (dict(n=0), dict(d_xyz=None), dict(cam=None), dict(d_uv=None)):
        with pytest.raises(X.OrbxError) as e:
            ex.kb8_project_device(**dict(dict(n=n, d_xyz=d_xyz, cam=S.CAM, d_uv=d_xyz), **change))
        assert e.value.code == -2


def run_front_half(ex, name):
    """the device front half over the pairs of a case, one call per (last, current) pair list: twice over poison"""
    import torch
    rigs, poses, pairs, cap, mono = front_cases()[name]
    k, n, fl, w = S.front_half_arrays(rigs, cap)
    d_k, d_n, d_fl, d_w, d_p = _dev(k.view(np.uint8)), _dev(n), _dev(fl), _dev(w), _dev(poses)
    P = len(pairs)
    last_first, cur_first = pairs[0]
    last_step = pairs[1][0] - pairs[0][0] if P > 1 else 1
    cur_step = pairs[1][1] - pairs[0][1] if P > 1 else 1
    assert all(p == (last_first + i * last_step, cur_first + i * cur_step) for i, p in enumerate(pairs))
    runs = []
    for _ in range(2):
        d_q = torch.full((P, 2 * cap, 2, 32), 0xA5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ex.project_last_frame_two_eyes_device(P, (last_first, last_step), (cur_first, cur_step), d_k, d_n, cap, d_fl, d_w, d_p, S.TRL, S.CAM,
                                              S.BOUNDS, S.MB, S.TH, mono, d_q)
        ex.synchronize()
        runs.append(d_q.cpu().numpy())
    assert runs[0].tobytes() == runs[1].tobytes()
    return runs[0].reshape(P, -1).view(O.PROJ_QUERY_DTYPE).reshape(P, 2 * cap, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["crafted", "crafted_mono", "full", "moving"])
def test_gpu_front_half_equals_the_walk(name):
    """capacity 5 (twelve pairs: every exit in each eye half under the three level forms, and under bMono), capacity 600 with both eye
    halves full (1200 requests), and two pairs of a stream of three rigs with steps (0, 1, 1, 1)"""
    q = run_front_half(X.ORBextractor(1200), name)
    walks = front_walk(name)
    if name == "moving":
        assert front_cases()[name][2] == [(0, 1), (1, 2)]
    for p, (wq, wex, _) in enumerate(walks):
        bad = np.nonzero((np.ascontiguousarray(q[p]).view(np.uint8).reshape(len(wq), 64) != wq.view(np.uint8).reshape(len(wq), 64)).any(1))[0]
        assert len(bad) == 0, (name, p, bad[:5], q[p][bad[:3]], wq[bad[:3]], wex[bad[:3]])
    assert sum(int((wex == W.EXIT_REQUEST).sum()) for _, wex, _ in walks) >= (400 if name in ("full", "moving") else 40)


def search_arrays(scenes, cap, cur=(0, 1)):
    """scenes -> the arrays of the C entry: pair q is rig cur[0] + q * cur[1], device frames 2 * rig (left eye) and 2 * rig + 1 (right eye);
    2 * cap requests per pair; requests, request descriptors and occupancy are indexed by the pair.  Rigs no pair names hold another
    scene's eyes, so that a kernel that confused the pair with the rig would find keypoints there and match them."""
    P = len(scenes)
    rigs = cur[0] + (P - 1) * cur[1] + 1
    k = np.zeros((2 * rigs, cap), O.KEYPOINT_DTYPE); d = np.zeros((2 * rigs, cap, 32), np.uint8); n = np.zeros(2 * rigs, np.int32)
    off = np.zeros((2 * rigs, 64 * 48 + 1), np.int32); idx = np.zeros((2 * rigs, cap), np.int32)
    q = np.zeros((P, 2 * cap, 2), O.PROJ_QUERY_DTYPE); qd = np.zeros((P, 2 * cap, 32), np.uint8); occ = np.zeros((P, 2, cap), np.uint8)

    def put(rig, s):
        for e, E in enumerate((s["left"], s["right"])):
            f, m = 2 * rig + e, len(E["k"])
            k[f], d[f], idx[f] = 0, 0, 0
            k[f, :m], d[f, :m], n[f], off[f] = E["k"], E["d"], m, E["off"]
            idx[f, :len(E["idx"])] = E["idx"]
    for r in range(rigs):
        put(r, scenes[(r + 1) % P])
    for p, s in enumerate(scenes):
        put(cur[0] + p * cur[1], s)
        if s["occ"] is not None:
            for e, E in enumerate((s["left"], s["right"])):
                occ[p, e, :len(E["k"])] = s["occ"][e]
        q[p, :len(s["q"])] = s["q"]; qd[p, :len(s["q"])] = s["qd"]
    return k, d, n, off, idx, q, qd, occ


def run_search(ex, scenes, cap, orientation=True, with_occ=True, d_q=None, cur=(0, 1)):
    """twice over poisoned outputs; d_q: requests already on the device (the front half's); cur: (first, step) of the pairs' rigs"""
    import torch
    P = len(scenes)
    k, d, n, off, idx, q, qd, occ = search_arrays(scenes, cap, cur)
    dv = [_dev(k.view(np.uint8)), _dev(d), _dev(n), _dev(off), _dev(idx)]
    d_q = _dev(q.view(np.uint8)) if d_q is None else d_q
    d_qd = _dev(qd)
    runs = []
    for _ in range(2):
        d_occ = _dev(occ) if with_occ else None
        d_m = torch.full((P, 2, cap), -7, dtype=torch.int32, device="cuda"); d_nm = torch.full((P,), -7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ex.search_last_frame_two_eyes_device(P, cur, d_q, d_qd, dv[0], dv[1], dv[2], cap, dv[3], dv[4], scenes[0]["bounds"], d_occ, orientation,
                                             d_m, d_nm)
        ex.synchronize()
        runs.append((d_m.cpu().numpy(), d_occ.cpu().numpy() if with_occ else None, d_nm.cpu().numpy()))
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][2].tobytes() == runs[1][2].tobytes()
    assert not with_occ or runs[0][1].tobytes() == runs[1][1].tobytes()
    return runs[0]


def assert_equal_to_walk(scenes, wants, m, occ, nm):
    for p, (s, want) in enumerate(zip(scenes, wants)):
        assert int(nm[p]) == want["n"], "pair %d" % p
        for e, E in enumerate((s["left"], s["right"])):
            n = len(E["k"])
            assert m[p, e, :n].tolist() == want["matches"][e], "pair %d eye %d" % (p, e)
            assert (m[p, e, n:] == -1).all()
            if occ is not None:
                assert occ[p, e, :n].tolist() == want["occupied"][e], "pair %d eye %d" % (p, e)


def stats():
    out = (C.c_int * 4)()
    assert X.load_library().orbx_debug_last_frame_two_eyes_stats(out) == 0
    return list(out)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CRAFTED)
def test_gpu_crafted_scenes(name):
    s = S.crafted_scenes()[name]
    want = S.walk_search(s)
    assert_consequence(name, s, want)
    cap = 37 if name == "joint_histogram" else 17
    m, occ, nm = run_search(X.ORBextractor(1000), [s], cap, with_occ=s["occ"] is not None)
    assert_equal_to_walk([s], [want], m, occ, nm)
    if name == "closure_chain":
        assert stats()[0] >= 4                              # a chain of four requests takes the fixed point four rounds and one to see it settle


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["no_right_eye", "no_left_eye", "occupied_null", "occupied_given", "crowded", "no_orientation"])
def test_gpu_random_requests_equal_the_walk(shape):
    rng = np.random.default_rng(21)
    kw = dict(no_right_eye=dict(nr=0), no_left_eye=dict(nl=0), crowded=dict(clusters=5, nq=500, obs_share=1.0, occ_share=0.03)).get(shape, {})
    scenes = [S.random_requests(rng, **kw) for _ in range(2)]
    occ_given, orientation = shape != "occupied_null", shape != "no_orientation"
    wants = [S.walk_search(s, orientation, occ_given) for s in scenes]
    if shape == "no_left_eye":
        for s, w in zip(scenes, wants):                      # Nleft = 0: every L's area result is empty, so only an R whose L is off runs
            assert w["suppressed"] > 100 and not (w["accepted"][:, 0] >= 0).any()
            assert not ((w["accepted"][:, 1] >= 0) & ((s["q"][:, 0]["flags"] & 1) != 0)).any()
    elif shape == "no_right_eye":
        assert all(w["n"] > 50 and not (w["accepted"][:, 1] >= 0).any() for w in wants)
    else:
        assert all(w["n"] > 100 and (w["accepted"][:, 1] >= 0).sum() > 50 and w["closure_changed"] > 0 for w in wants)
    if shape == "crowded":
        assert min(w["closure_changed"] for w in wants) > 50
    cur = {"occupied_given": (1, 2), "crowded": (2, 1)}.get(shape, (0, 1))      # rigs 1 and 3 / 2 and 3: outputs stay indexed by the pair
    m, occ, nm = run_search(X.ORBextractor(1000), scenes, 333, orientation, occ_given, cur=cur)
    assert_equal_to_walk(scenes, wants, m, occ, nm)
    if shape == "crowded":
        assert stats()[0] > 6


@pytest.mark.gpu
def test_gpu_front_half_and_search_chained_on_a_moving_rig():
    """three rigs of ~300 keypoints per eye, steps (0, 1, 1, 1): the device's own requests feed the device's search"""
    import torch
    ex = X.ORBextractor(1200)
    cap = _moving_capacity()
    scenes, wants = [], []
    for last, cur in ((0, 1), (1, 2)):
        s, exits, want = chained(last, cur)
        asked, taken = int((s["q"][:, 0]["flags"] & 1).sum()), int((want["accepted"] >= 0).any(1).sum())
        assert 3 * taken >= asked > 300 and want["closure_changed"] >= 1
        scenes.append(s); wants.append(want)
    q = run_front_half(ex, "moving")
    assert q.tobytes() == np.stack([s["q"] for s in scenes]).tobytes()
    # rig r + 1 is the current rig of pair r, as in the front half: the search's rigs are 1 and 2 (first 1, step 1), its outputs pairs 0 and 1
    m, occ, nm = run_search(ex, scenes, cap, with_occ=False, d_q=_dev(q.view(np.uint8)), cur=(1, 1))
    assert_equal_to_walk(scenes, wants, m, None, nm)


@pytest.mark.gpu
def test_gpu_size_bound_both_sides():
    import torch
    ex = X.ORBextractor(1200)
    assert ex.capacity == CAP_1200
    cap = max(c for c in range(1, 3000) if lds_bytes(c) <= LDS_LIMIT)
    assert lds_bytes(cap + 1) > LDS_LIMIT and cap >= CAP_1200
    rng = np.random.default_rng(51)
    s = S.random_requests(rng, nl=400, nr=380, nq=500)
    want = S.walk_search(s)
    for c in (cap, CAP_1200):                               # the largest accepted size and the 1200-feature extractor's run
        m, occ, nm = run_search(ex, [s], c)
        assert_equal_to_walk([s], [want], m, occ, nm)
    k, d, n, off, idx, q, qd, occ = search_arrays([s], cap + 1)
    d_m = torch.full((1, 2, cap + 1), -7, dtype=torch.int32, device="cuda"); d_nm = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    d_occ = _dev(occ)
    torch.cuda.synchronize()
    with pytest.raises(X.OrbxError) as e:                   # the first refused one
        ex.search_last_frame_two_eyes_device(1, (0, 1), _dev(q.view(np.uint8)), _dev(qd), _dev(k.view(np.uint8)), _dev(d), _dev(n), cap + 1, _dev(off),
                                             _dev(idx), S.BOUNDS, d_occ, True, d_m, d_nm)
    assert e.value.code == -8
    ex.synchronize()
    assert (d_m == -7).all() and (d_nm == -7).all() and np.array_equal(d_occ.cpu().numpy(), occ)      # the poison is still there


@pytest.mark.gpu
def test_gpu_argument_errors_are_rejected_before_any_launch():
    import torch
    ex = X.ORBextractor(1000)
    z = torch.zeros(8192, dtype=torch.int32, device="cuda")
    nm = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    good = dict(n_pairs=1, cur=(0, 1), d_queries=z, d_query_desc=z, d_kps=z, d_desc=z, d_n=z, capacity=16, d_grid_off=z, d_grid_idx=z, bounds=S.BOUNDS,
                d_occupied=None, check_orientation=True, d_matches=z, d_n_matches=nm, max_distance=100)
    bad = [dict(n_pairs=0), dict(cur=(-1, 1)), dict(cur=(0, -1)), dict(capacity=0), dict(max_distance=-1), dict(bounds=np.array([10, 10, 0, 480], f32)),
           dict(bounds=np.array([0, 640, 5, 1], f32)), dict(bounds=None), dict(d_queries=None), dict(d_query_desc=None), dict(d_kps=None),
           dict(d_desc=None), dict(d_n=None), dict(d_grid_off=None), dict(d_grid_idx=None), dict(d_matches=None), dict(d_n_matches=None)]
    for change in bad:
        with pytest.raises(X.OrbxError) as e:
            ex.search_last_frame_two_eyes_device(**dict(good, **change))
        assert e.value.code == -2, change
    front = dict(n_pairs=1, last=(0, 1), cur=(1, 1), d_kps=z, d_n=z, capacity=16, d_mp_flags=z, d_world=z, d_poses=z, trl=S.TRL, cam=S.CAM, bounds=S.BOUNDS,
                 mb=0.1, th=7.0, mono=False, d_queries=nm)
    for change in [dict(n_pairs=0), dict(last=(-1, 1)), dict(cur=(1, -1)), dict(capacity=0), dict(trl=None), dict(cam=None), dict(bounds=None),
                   dict(bounds=np.array([3, 3, 0, 1], f32)), dict(d_kps=None), dict(d_n=None), dict(d_mp_flags=None), dict(d_world=None),
                   dict(d_poses=None), dict(d_queries=None)]:
        with pytest.raises(X.OrbxError) as e:
            ex.project_last_frame_two_eyes_device(**dict(front, **change))
        assert e.value.code == -2, change
    ex.synchronize()
    assert (nm == -7).all()                                 # nothing ran
