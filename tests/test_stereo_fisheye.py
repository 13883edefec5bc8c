"""Frame::ComputeStereoFishEyeMatches without a GPU: extractorb_amd/csrc/k_stereo_fisheye.hip compiled for the host
(tests/cpp/stereo_fisheye_host_check.cpp: the kernel's own chunk scan, ratio test and geometry, a row at a time) against the sequential
walk (tests/stereo_fisheye_walk.py) on the scenes of tests/stereo_fisheye_scenes.py, byte for byte:
  (a) the crafted scene at capacity 32 per eye, 20 x 18 lapping rows behind 5 / 7 mono rows, 3 rigs, rig_step 1 and 0;
  (b) the tie rules of the 2-NN: the minimum at two right indices ([0] is the first, the row is rejected), the second-best at two, d0 = d1 = 0;
  (c) the ratio test on the edge pairs (6,10) (7,10) (13,20) (14,20) (69,99) (70,100) (179,256) (0,1), each a rig of two right lapping rows;
  (d) two left rows choosing one right row: both accepted (right_to_left is the larger), the larger failing the geometry (the smaller),
      both failing (-1), every left_to_right standing on its own;
  (e) every exit of TriangulateMatches reached, from the walk's trace, and a NaN transform rejecting every row;
  (f) kSfChunk + 1 right lapping rows with the best and the second candidate on either side of the chunk boundary, in both orders, and a tie
      across it;
  (g) octaves outside [0, nlevels);
the mono clamps; the 257 x 257 enumeration of the three forms of the ratio test; and an INDEPENDENT margin check: the float64 statement of
tests/triangulation_two_eyes_scenes.py (np.linalg.svd, math.tan, math.atan2) decides every pair the walk triangulates as the walk does,
clear of every threshold, and its depth agrees with the binary32 one within DEPTH_RTOL.  The host program runs under
-fsanitize=address,undefined as a stand-alone program."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import extractorb_amd as X
import stereo_fisheye_scenes as SC
import stereo_fisheye_walk as SW
import triangulation_two_eyes_walk as W
from test_kb8_math import HOST_FLAGS, ROOT
from test_kb8_unproject_math import same_floats

f32 = np.float32
VP = C.c_void_p
POISON = -559038737
CRAFTED_SEED = 1
RATIO_EDGES = ((6, 10), (7, 10), (13, 20), (14, 20), (69, 99), (70, 100), (179, 256), (0, 1))
# The binary32 depth against the float64 one.  Each ray component carries about a dozen binary32 roundings (the Newton steps end below
# 1e-6 in theta with a quadratically smaller error, tanf and the divisions are correctly rounded): at most ~1e-6 relative.  The depth of a
# point is baseline / parallax angle, so a ray error e moves it by about 2 e / parallax relative; the smallest parallax of an accepted pair is
# 0.1 m / 3.5 m = 0.029, which gives 7e-5.  The null vector adds 3.4e-8 / sigma_3 (docs/history/r18_two_eyes_triangulation.md), below 1e-5
# here.  Rounded up to 2e-4.
DEPTH_RTOL = 2e-4


def build_host(directory):
    so = os.path.join(str(directory), "libstereo_fisheye_host.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", *HOST_FLAGS, os.path.join(ROOT, "tests", "cpp", "stereo_fisheye_host_check.cpp"), "-o", so])
    L = C.CDLL(so)
    L.stereo_fisheye_host.argtypes = [C.c_int] * 3 + [VP] * 4 + [C.c_int] + [VP] * 3 + [C.c_int] + [VP] * 7
    L.stereo_fisheye_ratio.argtypes = [C.c_int, C.c_int]
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("sfhost"))


def ptr(a):
    return a.ctypes.data_as(VP)


_SCENES, _WALKS = {}, {}


def scene(seed):
    if seed not in _SCENES:
        _SCENES[seed] = SC.make(seed)
    return _SCENES[seed]


def walk(rig, tlr=SC.TLR, trace=None):
    """the walk of a rig, computed once (the rig object is the key)"""
    key = (id(rig), np.asarray(tlr, f32).tobytes())
    if key not in _WALKS or trace is not None:
        _WALKS[key] = (rig, SW.compute_stereo_fisheye_matches(W.libm_math(), rig["left"], rig["right"], rig["mono"][0], rig["mono"][1], tlr, SC.CAMS,
                                                              SC.SIGMA2, trace=trace))
    return _WALKS[key][1]


def outputs(B, n_rigs, cap):
    return dict(l2r=np.full((B, cap), POISON, np.int32), r2l=np.full((B, cap), POISON, np.int32), depth=np.full((B, cap), -7.0, f32),
                x3d=np.full((B, cap, 3), -7.0, f32), n=np.full(n_rigs, POISON, np.int32), nd=np.full(n_rigs, POISON, np.int32))


def host_run(host, rigs, cap, first=0, step=1, n_rigs=None, tlr=SC.TLR, desc_matches=True):
    d = SC.pack(rigs, cap)
    n_rigs = len(rigs) if n_rigs is None else n_rigs
    o = outputs(2 * len(rigs), n_rigs, cap)
    calls = np.zeros(1, np.int32)
    host.stereo_fisheye_host(n_rigs, first, step, ptr(d["kps"]), ptr(d["desc"]), ptr(d["nout"]), ptr(d["mono"]), cap,
                             ptr(np.ascontiguousarray(tlr, f32)), ptr(np.concatenate(SC.CAMS).astype(f32)), ptr(SC.SIGMA2), 8, ptr(o["l2r"]),
                             ptr(o["r2l"]), ptr(o["depth"]), ptr(o["x3d"]), ptr(o["n"]), ptr(o["nd"]) if desc_matches else None, ptr(calls))
    o["calls"] = int(calls[0])
    return o


def assert_equals_walk(o, rigs, first=0, step=1, n_rigs=None, tlr=SC.TLR, what=""):
    """all five arrays and both counters: the rows of every rig the call names hold the walk's result in all capacity entries, every other
    row (the other eye's, a rig the call does not name) still holds the poison"""
    n_rigs = len(rigs) if n_rigs is None else n_rigs
    named = set()
    for q in range(n_rigs):
        r = first + q * step
        named.add(r)
        w = walk(rigs[r], tlr)
        nl, nr = len(w["left_to_right"]), len(w["right_to_left"])
        tag = "%s rig %d (q %d)" % (what, r, q)
        assert o["l2r"][2 * r, :nl].tolist() == w["left_to_right"] and (o["l2r"][2 * r, nl:] == -1).all(), tag
        assert o["r2l"][2 * r + 1, :nr].tolist() == w["right_to_left"] and (o["r2l"][2 * r + 1, nr:] == -1).all(), tag
        assert same_floats(o["depth"][2 * r, :nl], w["depth"]) and (o["depth"][2 * r, nl:] == -1.0).all(), tag
        assert same_floats(o["x3d"][2 * r, :nl], w["x3d"]) and (o["x3d"][2 * r, nl:] == 0.0).all(), tag
        assert int(o["n"][q]) == w["n"], (tag, int(o["n"][q]), w["n"])
        if (o["nd"] != POISON).any():
            assert int(o["nd"][q]) == w["desc"], (tag, int(o["nd"][q]), w["desc"])
    for r in range(len(rigs)):
        for f in (2 * r, 2 * r + 1):
            if not (r in named and f == 2 * r):                                      # not a left eye the call names
                assert (o["l2r"][f] == POISON).all() and (o["depth"][f] == -7.0).all() and (o["x3d"][f] == -7.0).all(), (what, f)
            if not (r in named and f == 2 * r + 1):
                assert (o["r2l"][f] == POISON).all(), (what, f)
    if "calls" in o:
        assert o["calls"] == sum(walk(rigs[first + q * step], tlr)["desc"] for q in range(n_rigs)), what


# ---- the rigs of (b) .. (g), built once and shared with the GPU tests ----
def _rng(k):
    return np.random.default_rng(1000 + k)


def tie_rigs():
    """(b): [0] minimum at two indices, the observation first; [1] the same, the observation second; [2] the second-best at two; [3] d0 = d1 = 0"""
    return [SC.edge_rig(_rng(0), [(5, True), (5, False), (40, False)]), SC.edge_rig(_rng(1), [(5, False), (5, True), (40, False)]),
            SC.edge_rig(_rng(2), [(20, False), (5, True), (20, False)]), SC.edge_rig(_rng(3), [(0, True), (0, False)])]


def ratio_rigs():
    """(c): two right lapping rows, the second candidate in front of the observation"""
    return [SC.edge_rig(_rng(10 + k), [(d1, False), (d0, True)]) for k, (d0, d1) in enumerate(RATIO_EDGES)]


def shared_rigs():
    """(d): [0] both left rows accepted; [1] the larger left row 40 px off; [2] both choose a right row that is not the observation"""
    return [SC.edge_rig(_rng(20), [(3, True), (60, False)], lefts=2), SC.edge_rig(_rng(21), [(3, True), (60, False)], lefts=2, left_shift=(40.0, 25.0)),
            SC.edge_rig(_rng(22), [(3, False), (60, False)], lefts=2)]


def octave_rigs():
    """(g)"""
    return [SC.edge_rig(_rng(30), [(4, True), (50, False)], left_octave=11, right_octave=-3), SC.edge_rig(_rng(31), [(50, False), (4, True)], left_octave=-1, right_octave=8)]


def straddle_rigs(chunk):
    """(f): best | second = last row of chunk 0 | first row of chunk 1, the reverse, and the minimum on both sides in either order"""
    return [SC.straddle_rig(_rng(40), chunk, chunk - 1, chunk), SC.straddle_rig(_rng(41), chunk, chunk, chunk - 1),
            SC.straddle_rig(_rng(42), chunk, chunk - 1, chunk, tie=True), SC.straddle_rig(_rng(43), chunk, chunk, chunk - 1, tie=True)]


_RIGS = {}


def rigs_of(name, chunk=None):
    if name not in _RIGS:
        _RIGS[name] = {"tie": tie_rigs, "ratio": ratio_rigs, "shared": shared_rigs, "octave": octave_rigs}[name]() if name != "straddle" else straddle_rigs(chunk)
    return _RIGS[name]


def check_rules(name, chunk=None):
    """what each group of rigs is built to show, asserted on the WALK (the host kernel and the GPU are then held to the walk)"""
    rigs = rigs_of(name, chunk)
    ws = [walk(r) for r in rigs]
    if name == "tie":
        assert [w["knn"][0] for w in ws] == [[(5, 0), (5, 1)], [(5, 0), (5, 1)], [(5, 1), (20, 0)], [(0, 0), (0, 1)]]
        assert [(w["desc"], w["n"]) for w in ws] == [(0, 0), (0, 0), (1, 1), (0, 0)]
        assert ws[2]["left_to_right"][rigs[2]["mono"][0]] == rigs[2]["mono"][1] + 1
    elif name == "ratio":
        for (d0, d1), w in zip(RATIO_EDGES, ws):
            assert w["knn"][0] == [(d0, 1), (d1, 0)]
            assert (w["desc"], w["n"]) == ((1, 1) if 10 * d0 < 7 * d1 else (0, 0)), (d0, d1)
        assert [w["desc"] for w in ws] == [1, 0, 1, 0, 1, 0, 1, 1]
    elif name == "shared":
        for k, (w, want_l2r, want_back) in enumerate(zip(ws, ((0, 0), (0, -1), (-1, -1)), (1, 0, -1))):
            ml, mr = rigs[k]["mono"]
            assert w["desc"] == 2 and w["left_to_right"][ml:] == [mr + v if v >= 0 else -1 for v in want_l2r], k
            assert w["right_to_left"][mr] == (ml + want_back if want_back >= 0 else -1), k
    elif name == "octave":
        assert [(w["desc"], w["n"]) for w in ws] == [(1, 1), (1, 1)]
    elif name == "straddle":
        mr = rigs[0]["mono"][1]
        assert [w["knn"][0] for w in ws] == [[(5, chunk - 1), (20, chunk)], [(5, chunk), (20, chunk - 1)], [(5, chunk - 1), (5, chunk)], [(5, chunk - 1), (5, chunk)]]
        assert [w["left_to_right"][rigs[0]["mono"][0]] for w in ws] == [mr + chunk - 1, mr + chunk, -1, -1]
        assert all(w["n"] == len(w["knn"]) - (k >= 2) for k, w in enumerate(ws))      # the rows on the chunks' first rows match too


def test_crafted_scene_step_one_and_zero(host):
    s = scene(CRAFTED_SEED)
    for rig in s["rigs"]:
        assert (len(rig["left"]["kps"]) - rig["mono"][0], len(rig["right"]["kps"]) - rig["mono"][1]) == (20, 18) and rig["mono"] == (5, 7)
        w = walk(rig)
        kinds = dict((i, k) for k, i, _ in rig["plan"])
        assert w["n"] == 12 and w["desc"] == 18                                      # 10 true pairs + 2 shared; the two ratio rows never reach the geometry
        assert all((w["left_to_right"][i] >= 0) == (kinds[i] in ("true", "shared")) for i in kinds)
        assert all(w["left_to_right"][i] == j for k, i, j in rig["plan"] if k in ("true", "shared"))
        for k, i, j in rig["plan"]:                                                  # of the two left rows on a right row the larger stays
            if k == "shared":
                assert w["right_to_left"][j] == max(i2 for _, i2, j2 in rig["plan"] if j2 == j)
        assert max(w["left_to_right"]) >= rig["mono"][1] and (np.array(w["left_to_right"][:5]) == -1).all()
    assert_equals_walk(host_run(host, s["rigs"], s["cap"]), s["rigs"], what="step 1")
    assert_equals_walk(host_run(host, s["rigs"], s["cap"], first=1, step=0, n_rigs=3), s["rigs"], first=1, step=0, n_rigs=3, what="step 0")
    assert_equals_walk(host_run(host, s["rigs"], s["cap"], first=2, step=-1, n_rigs=2), s["rigs"], first=2, step=-1, n_rigs=2, what="step -1")
    o = host_run(host, s["rigs"], s["cap"], desc_matches=False)                      # d_n_desc_matches = NULL
    assert (o["nd"] == POISON).all()
    assert_equals_walk(o, s["rigs"], what="no desc counter")


@pytest.mark.parametrize("name", ["tie", "ratio", "shared", "octave"])
def test_rules(host, name):
    check_rules(name)
    rigs = rigs_of(name)
    assert_equals_walk(host_run(host, rigs, 32), rigs, what=name)


def test_chunk_boundary(host):
    chunk = host.stereo_fisheye_chunk()
    check_rules("straddle", chunk)
    rigs = rigs_of("straddle", chunk)
    assert all(len(r["right"]["kps"]) - r["mono"][1] == chunk + 1 for r in rigs)
    assert_equals_walk(host_run(host, rigs, chunk + 8), rigs, what="straddle")


def test_every_exit_is_reached_and_a_nan_transform_rejects(host):
    s = scene(CRAFTED_SEED)
    trace = []
    walk(s["rigs"][0], trace=trace)
    assert set(t[4] for t in trace) == {"ok", "parallax", "z1", "z2", "error1", "error2"}
    kinds = dict((i, k) for k, i, _ in s["rigs"][0]["plan"])
    assert all(kinds[t[0]] == t[4] for t in trace if t[4] not in ("ok", "parallax")) and all(kinds[t[0]] == "far" for t in trace if t[4] == "parallax")
    nan = SC.TLR.copy(); nan[1, 3] = np.nan
    w = walk(s["rigs"][0], nan)
    assert w["n"] == 0 and w["desc"] == 18 and max(w["left_to_right"]) == -1 and max(w["right_to_left"]) == -1
    assert_equals_walk(host_run(host, s["rigs"], s["cap"], tlr=nan), s["rigs"], tlr=nan, what="NaN transform")


@pytest.mark.parametrize("mono,n_out", [((-3, 100), None), ((100, -3), None), ((25, 25), None), ((5, 24), None), ((5, 7), (40, 40))])
def test_mono_and_counts_are_clamped(host, mono, n_out):
    """mono outside [0, N] is clamped into it, N into [0, capacity]; one right lapping row matches nothing"""
    import copy
    rig = copy.deepcopy(scene(CRAFTED_SEED)["rigs"][1])
    rig["mono"] = mono
    want = copy.deepcopy(rig)
    if n_out:                                                                        # the rows up to the capacity are keypoints too (zeros here)
        rig["n_out"] = n_out
        for e in ("left", "right"):
            pad = 32 - len(want[e]["kps"])
            want[e] = dict(kps=np.concatenate([want[e]["kps"], np.zeros(pad, X.KEYPOINT_DTYPE)]), desc=np.concatenate([want[e]["desc"], np.zeros((pad, 32), np.uint8)]))
    o = host_run(host, [rig], 32)
    assert_equals_walk(o, [want], what=str((mono, n_out)))
    if mono in ((100, -3), (25, 25), (5, 24), (-3, 100)):
        assert int(o["n"][0]) == 0 and int(o["nd"][0]) == 0


def test_the_three_forms_of_the_ratio_test(host):
    """(float)d0 < (float)d1 * 0.7 in double (the reference), its binary32 product, and the kernel's 10 * d0 < 7 * d1 on all 257 x 257 pairs"""
    d0, d1 = np.meshgrid(np.arange(257), np.arange(257), indexing="ij")
    in_double = d0.astype(f32).astype(np.float64) < d1.astype(f32).astype(np.float64) * 0.7
    in_float = d0.astype(f32) < (d1.astype(f32) * f32(0.7)).astype(f32)
    integer = 10 * d0 < 7 * d1
    assert np.array_equal(in_double, integer) and np.array_equal(in_float, integer)
    assert not integer[np.arange(257), np.arange(257)].any()                         # equal distances never pass, 0 < 0 included
    kernel = np.array([[host.stereo_fisheye_ratio(a, b) for b in range(257)] for a in range(257)], bool)
    assert np.array_equal(kernel, integer)
    assert all(SW.ratio_passes(a, b) == bool(integer[a, b]) for a, b in RATIO_EDGES + ((0, 0), (256, 256), (179, 255)))


@pytest.mark.parametrize("seed", SC.MARGIN_SEEDS)
def test_float64_statement_agrees_with_margin(seed):
    s = scene(seed)
    tested, worst = 0, 0.0
    for rig in s["rigs"]:
        trace = []
        walk(rig, trace=trace)
        holds, st = SC.margin_ok(rig, trace)
        assert holds, seed
        for (i, j, ok, z, why), (ok64, z64, why64) in zip(trace, st):
            assert ok == ok64 and (why == why64 or ok), (seed, i, j, why, why64)
            if ok:
                worst = max(worst, abs(float(z) - z64) / z64)
            tested += 1
    print("seed %d: %d pairs, worst relative depth difference %.3g" % (seed, tested, worst))
    assert tested >= 50 and worst <= DEPTH_RTOL


def test_the_scenes_level_table_is_the_handles():
    assert SC.SIGMA2.tobytes() == X.compute_tables(1000, 1.2, 8)["level_sigma2"].tobytes()


def test_the_entry_is_declared_and_nothing_calls_it_unbuilt():
    assert "orbx_stereo_fisheye_match_device" in X.header_symbols() and "orbx_debug_stereo_fisheye_stats" in X.header_symbols()
    assert hasattr(X.ORBextractor, "stereo_fisheye_match_device") and hasattr(X.ORBextractor, "stereo_fisheye_stats")
    text = open(os.path.join(ROOT, "include", "orbx.h")).read()
    for sentence in re.split(r"(?<=[.;])\s", text):
        assert not ("ComputeStereoFishEyeMatches" in sentence and re.search(r"not\s+(\*\s*)?built", sentence)), sentence
    # the search that reads the two match arrays names the entry that writes them
    doc = text[text.index("d_left_to_right[fL*capacity + i]"):]
    assert "orbx_stereo_fisheye_match_device" in doc[:400]


def test_host_program_runs_clean_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "prog")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DSTEREO_FISHEYE_HOST_MAIN", *HOST_FLAGS,
                           os.path.join(ROOT, "tests", "cpp", "stereo_fisheye_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert out.returncode == 0 and "runtime error" not in out.stdout and "AddressSanitizer" not in out.stdout, out.stdout[-3000:]
