"""MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth without a GPU: extractorb_amd/csrc/k_map_point_update.hpp - the
statement of k_map_point_update.hip - compiled for the host (tests/cpp/map_point_update_host_check.cpp) against the sequential walk
(tests/map_point_update_walk.py) on the scenes of tests/map_point_update_scenes.py, byte for byte, for both rig kinds:
  (a) the descriptor half of the walk against fuse_walk's independent compute_distinctive_descriptors on random maps; int(0.5*(N-1)) ==
      (N-1)//2 up to the bound; the counting form of the median against the sorted form on every row of those maps;
  (b) the header against the Binary32 walk on every scene of the GPU tests, for what = 1, 2, 3 and the three forms of d_slot;
  (c) the Float64 walk: the same status and best everywhere, normal and distances within a bound derived here;
  (d) the semantics the header lists, on the crafted points; the stand-alone sanitizer program; the declarations."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import extractorb_amd as X
import fuse_walk
import map_point_update_scenes as SC
import map_point_update_walk as MW
from test_kb8_math import HOST_FLAGS, ROOT

f32 = np.float32
VP = C.c_void_p
U = 2.0 ** -24      # the unit roundoff of binary32


def build_host(directory):
    so = os.path.join(str(directory), "libmap_point_update_host.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", *HOST_FLAGS, os.path.join(ROOT, "tests", "cpp", "map_point_update_host_check.cpp"), "-o", so])
    L = C.CDLL(so)
    L.mpu_host.argtypes = [C.c_int, C.c_int] + [VP] * 8 + [C.c_int, VP, VP, VP, C.c_int, VP, C.c_int, C.c_int] + [VP] * 6
    L.mpu_host.restype = None
    return L


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host(tmp_path_factory.mktemp("mpuhost"))


def ptr(a):
    return None if a is None else a.ctypes.data_as(VP)


def keypoints(s):
    k = np.zeros(s["octave"].shape, X.KEYPOINT_DTYPE)
    k["octave"] = s["octave"]
    return k


def host_update(L, s, what=3):
    """mpu_host on a scene, from poisoned tables and outputs: the dict map_point_update_walk.update returns"""
    P = len(s["obs_off"]) - 1
    out = MW.tables(s)
    best = np.full(P, -559038737, np.int32); best_median = best.copy(); status = np.full(P, 0xEE, np.uint8)
    hold = [np.ascontiguousarray(s["obs_off"], np.int32), np.ascontiguousarray(s["obs"], np.int32), s["flags"], np.ascontiguousarray(s["ref"], np.int32),
            s["slot"], np.ascontiguousarray(s["world"], f32), np.ascontiguousarray(s["poses"], f32), None if s["tlr"] is None else np.ascontiguousarray(s["tlr"], f32),
            keypoints(s), np.ascontiguousarray(s["desc"]), np.ascontiguousarray(s["n_out"], np.int32), np.ascontiguousarray(s["scale"], f32)]
    L.mpu_host(int(s["two_eyes"]), P, ptr(hold[0]), ptr(hold[1]), ptr(hold[2]), ptr(hold[3]), ptr(hold[4]), ptr(hold[5]), ptr(hold[6]), ptr(hold[7]),
               len(s["n_out"]), ptr(hold[8]), ptr(hold[9]), ptr(hold[10]), s["capacity"], ptr(hold[11]), s["nlevels"], what, ptr(out["mp_desc"]),
               ptr(out["mp_normal"]), ptr(out["mp_dist"]), ptr(best), ptr(best_median), ptr(status))
    out.update(best=best, best_median=best_median, status=status)
    return out


def same_bytes(got, want, what=""):
    for k in ("status", "best", "best_median", "mp_desc", "mp_normal", "mp_dist"):
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k)
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero((a.reshape(len(a), -1).view(np.uint8) != b.reshape(len(b), -1).view(np.uint8)).any(axis=1))
            raise AssertionError("%s: %s differs in rows %s: got %s, want %s" % (what, k, bad[:8], a[bad[:3]], b[bad[:3]]))


_SCENES, _WALKS = {}, {}


def scene(name, two_eyes):
    """the scenes of the GPU tests, each built once"""
    key = (name, two_eyes)
    if key not in _SCENES:
        if name == "lengths":          # d_slot: a permutation
            b, pts = SC.lengths(two_eyes)
            _SCENES[key] = SC.with_points(b, pts, slot=np.random.default_rng(8).permutation(len(pts)).tolist())
        elif name == "subset":         # d_slot: a strict subset of a larger table
            b, pts = SC.lengths(two_eyes)
            keep = [m for m in range(len(pts)) if m % 3 != 1]
            _SCENES[key] = SC.with_points(b, [pts[m] for m in keep], n_slots=len(pts) + 4, slot=[m + 2 for m in keep])
        elif name == "crafted":        # d_slot NULL
            _SCENES[key] = SC.with_points(*SC.crafted(two_eyes))
        elif name == "no_flags":       # d_obs_flags NULL
            _SCENES[key] = SC.with_points(*SC.crafted(two_eyes), no_flags=True)
        elif name == "working":
            _SCENES[key] = SC.working(two_eyes)
    return _SCENES[key]


def walk(s, what=3, kind=MW.Binary32):
    """a walk of a scene, computed once and left unchanged"""
    key = (id(s), what, kind)
    if key not in _WALKS:
        _WALKS[key] = (s, MW.update(kind(), s, what))
    return _WALKS[key][1]


# ---- (a) the descriptor half against an independent statement ----
def random_map(rng, n_kf, rows, n_points, max_obs):
    kf_desc = [rng.integers(0, 256, (rows, 32)).astype(np.uint8) for _ in range(n_kf)]
    for d in kf_desc:                                   # near-duplicates, so that medians tie
        d[1] = d[0]; d[2] = SC.flip(d[0], [5]); d[3] = d[0]
    m = fuse_walk.Map([np.zeros(32, np.uint8)] * n_points, kf_desc)
    for p in range(n_points):
        for kf in rng.choice(n_kf, int(rng.integers(1, max_obs + 1)), replace=False):
            m.add(p, int(kf), int(rng.integers(0, 6 if p % 2 else rows)))
    return m


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_descriptor_half_equals_the_map_models_statement(seed):
    rng = np.random.default_rng(seed)
    m = random_map(rng, 12, 24, 60, 12)
    rows_checked = 0
    for p in range(60):
        ds = np.stack([m.kf_desc[kf][idx] for kf, idx in sorted(m.obs[p].items())])
        m.compute_distinctive_descriptors(p)
        b, med = MW.distinctive(ds)
        assert ds[b].tobytes() == m.desc[p].tobytes()
        D = MW.hamming_matrix(ds)
        assert D[0, 0] == 0 and (D == D.T).all()
        for row in D:                                   # the counting form of the median against the sorted form, on every row
            assert MW.median_by_count(row) == MW.median_sorted(row)
            rows_checked += 1
        assert med == min(MW.median_sorted(r) for r in D)
    assert rows_checked > 200


def test_the_median_rank_is_an_integer_division():
    for n in range(1, MW.MAX_OBSERVATIONS + 2):
        assert int(0.5 * (n - 1)) == (n - 1) // 2
    assert MW.median_by_count(np.array([0])) == 0 and MW.median_by_count(np.array([0, 200])) == 0 and MW.median_by_count(np.array([256, 256, 0])) == 256


# ---- (b) the header against the walk ----
@pytest.mark.parametrize("two_eyes", [False, True])
@pytest.mark.parametrize("name", ["lengths", "subset", "crafted", "no_flags"])
@pytest.mark.parametrize("what", [1, 2, 3])
def test_header_equals_the_walk(host, name, two_eyes, what):
    s = scene(name, two_eyes)
    same_bytes(host_update(host, s, what), walk(s, what), "%s two_eyes=%d what=%d" % (name, two_eyes, what))


@pytest.mark.parametrize("two_eyes", [False, True])
def test_header_equals_the_walk_at_working_size(host, two_eyes):
    s = scene("working", two_eyes)
    w = walk(s)
    same_bytes(host_update(host, s), w, "working two_eyes=%d" % two_eyes)
    n = np.diff(s["obs_off"])
    assert 5 < n.mean() < 9 and n.max() > 200 and (w["status"] == MW.OK).sum() > 1900


# ---- (c) the float64 kind ----
def float64_bounds(s, m, w64):
    """What binary32 may cost listed point m against the float64 kind, per component of the normal and per distance, from the roundings of
    the statement (u = 2^-24, every rounding at its worst sign; (1 + 1e-3) covers the products of two errors).
    One entry: Ow is rounded once per element (u |Ow_c|) and so is the difference (u |d_c|): the vector moves by at most u (|Ow| + |d|), its
    direction by at most twice that over |d|; (float)(1/norm) and the product add u each on a component of at most 1.
    The sum: every step rounds a partial sum of at most N, N steps: u N N; it is divided by N.  The quotient (float)(1/N) and the product: 2 u.
    The distances: dist = (float)norm moves by the vector's u (|Ow| + |d|) and rounds once; each product or quotient after it adds u."""
    off0, n = int(s["obs_off"][m]), int(s["obs_off"][m + 1] - s["obs_off"][m])
    slot = m if s["slot"] is None else int(s["slot"][m])
    pos = s["world"][slot].astype(np.float64)
    cen = MW.centres(MW.Float64(), s)
    eps = 0.0
    for f in s["obs"][off0:off0 + n, 0]:
        d = np.linalg.norm(pos - cen[f])
        eps += 2 * U * (np.linalg.norm(cen[f]) + d) / d + 2 * U
    normal = (eps / n + U * n * n / n + 2 * U) * (1 + 1e-3)
    rf = int(s["obs"][off0 + int(s["ref"][m]), 0])
    left = rf & ~1 if s["two_eyes"] else rf
    d = np.linalg.norm(pos - cen[left])
    min_inv, max_inv, max_d = (float(x) for x in w64["mp_dist"][slot])
    scale = max_d / d
    e_dist = U * (np.linalg.norm(cen[left]) + d) + U * d
    e_max = scale * e_dist + U * max_d
    e_min = e_max / float(s["scale"][-1]) + U * (min_inv / 0.8)
    return normal, np.array([0.8 * e_min + U * min_inv, 1.2 * e_max + U * max_inv, e_max]) * (1 + 1e-3)


@pytest.mark.parametrize("two_eyes", [False, True])
@pytest.mark.parametrize("name", ["lengths", "crafted", "working"])
def test_float64_kind_decides_the_same_within_the_derived_bound(name, two_eyes):
    s = scene(name, two_eyes)
    w32, w64 = walk(s), walk(s, 3, MW.Float64)
    assert (w32["status"] == w64["status"]).all() and (w32["best"] == w64["best"]).all() and (w32["best_median"] == w64["best_median"]).all()
    assert (w32["mp_desc"] == w64["mp_desc"]).all()
    worst = 0.0
    for m in np.flatnonzero((w32["status"] == MW.OK) | (w32["status"] == MW.NO_DESCRIPTOR)):
        slot = m if s["slot"] is None else int(s["slot"][m])
        bn, bd = float64_bounds(s, m, w64)
        en = np.abs(w32["mp_normal"][slot].astype(np.float64) - w64["mp_normal"][slot]).max()
        ed = np.abs(w32["mp_dist"][slot].astype(np.float64) - w64["mp_dist"][slot]) / bd
        worst = max(worst, en / bn, ed.max())
        assert en <= bn and (ed <= 1).all(), (m, en, bn, ed)
    print("%s two_eyes=%d: worst fraction of the bound %.3f" % (name, two_eyes, worst))
    assert worst > 0.0


# ---- (d) the semantics, on the crafted points ----
@pytest.mark.parametrize("two_eyes", [False, True])
def test_crafted_points_end_where_they_were_built_for(two_eyes):
    s = scene("crafted", two_eyes)
    w, name = walk(s), s["names"]
    st = lambda n: int(w["status"][name[n]])
    F = SC.FRAMES - 1
    assert (w["best"][name["duplicates"]], w["best_median"][name["duplicates"]]) == (1, 0)          # three rows share median 0: the first of them
    assert (w["best"][name["outlier"]], w["best_median"][name["outlier"]]) == (0, 3)
    assert (w["best"][name["best_last"]], w["best_median"][name["best_last"]]) == (4, 40)             # the best row is the last
    assert w["mp_desc"][name["best_last"]].tobytes() == s["desc"][F, 0].tobytes()
    # the flagged hub and spoke are out of the selection (positions count the three others) ...
    assert (w["best"][name["some_flagged"]], w["best_median"][name["some_flagged"]]) == (0, 80)
    assert w["mp_desc"][name["some_flagged"]].tobytes() == s["desc"][F, 1].tobytes()
    # ... but the normal counts all five: without the flagged entries it is another vector
    q = dict(s); m = name["some_flagged"]
    keep = [o for o in range(len(s["obs"])) if not (s["obs_off"][m] <= o < s["obs_off"][m + 1] and s["flags"][o])]
    q["obs"], q["flags"] = s["obs"][keep], s["flags"][keep]
    q["obs_off"] = np.concatenate([s["obs_off"][:m + 1], s["obs_off"][m + 1:] - 2]).astype(np.int32)
    q["ref"] = s["ref"].copy(); q["ref"][m] = 0
    assert MW.update(MW.Binary32(), q, 2)["mp_normal"][m].tobytes() != w["mp_normal"][m].tobytes()
    assert st("all_flagged") == MW.NO_DESCRIPTOR
    assert (w["mp_desc"][name["all_flagged"]] == MW.POISON_BYTE).all() and (w["mp_normal"][name["all_flagged"]] != MW.POISON_FLOAT).all()
    for n in ("frame_minus_one", "frame_past", "row_past", "ref_minus_one", "ref_past", "flagged_bad_row"):
        assert st(n) == MW.BAD_INDEX, n
        assert (w["mp_desc"][name[n]] == MW.POISON_BYTE).all() and (w["mp_normal"][name[n]] == MW.POISON_FLOAT).all() and (w["mp_dist"][name[n]] == MW.POISON_FLOAT).all()
    assert w["best_median"][name["single"]] == 0 and w["best_median"][name["pair"]] == 0 and w["best"][name["pair"]] == 0
    # the clamp: octave -1 scales as level 0, octave nlevels as the last level
    for n, level in (("octave_minus_one", 0), ("octave_nlevels", s["nlevels"] - 1), ("octave_last", s["nlevels"] - 1), ("octave_zero", 0)):
        d = w["mp_dist"][name[n]]
        pos = s["world"][name[n]]
        m = name[n]
        rf = int(s["obs"][s["obs_off"][m] + s["ref"][m], 0])
        cen = MW.centres(MW.Binary32(), s)[rf & ~1 if two_eyes else rf]
        dist = f32(MW.norm64([f32(pos[c] - cen[c]) for c in range(3)]))
        assert d[2] == f32(dist * s["scale"][level]), n
    if two_eyes:
        m = name["right_only"]
        assert (s["obs"][s["obs_off"][m]:s["obs_off"][m + 1], 0] & 1).all()
        rf = int(s["obs"][s["obs_off"][m] + s["ref"][m], 0])
        cen = MW.centres(MW.Binary32(), s)
        lvl = int(s["octave"][rf, s["obs"][s["obs_off"][m] + s["ref"][m], 1]])
        dist_of = lambda c: f32(f32(MW.norm64([f32(s["world"][m][k] - c[k]) for k in range(3)])) * s["scale"][lvl])
        assert w["mp_dist"][m][2] == dist_of(cen[rf - 1]) and dist_of(cen[rf - 1]) != dist_of(cen[rf])      # the LEFT centre, and it shows
        m = name["both_eyes"]
        e = s["obs"][s["obs_off"][m]:s["obs_off"][m + 1]]
        assert (e[1, 0], e[2, 0]) == (2, 3)                                                                  # left, then right, of rig 1


def test_lengths_scene_covers_every_path():
    s = scene("lengths", False)
    n = np.diff(s["obs_off"])
    assert set(n) >= {0, 1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 129, 1024, 1025} and len(n) > 16
    w = walk(s)
    assert (w["status"][n == 1025] == MW.TOO_LONG).all() and (w["status"][n == 0] == MW.EMPTY).all()
    assert (w["status"][(n > 0) & (n <= 1024)] != MW.TOO_LONG).all()
    short, long_ = n <= 16, n > 64
    assert (short[:-1] & long_[1:]).any() and (long_[:-1] & short[1:]).any()      # short and long lists are neighbours


def test_sanitizer_program(tmp_path):
    """the stand-alone program of tests/cpp/map_point_update_host_check.cpp under AddressSanitizer and UBSan: wild frames, rows, reference
    entries, offsets and slots on exact-size heap blocks"""
    exe = str(tmp_path / "map_point_update_host_check")
    subprocess.check_call(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-DMAP_POINT_UPDATE_HOST_MAIN", *HOST_FLAGS,
                           os.path.join(ROOT, "tests", "cpp", "map_point_update_host_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "every access inside its arrays" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


def test_declarations():
    header = open(os.path.join(ROOT, "include", "orbx.h")).read()
    assert int(re.search(r"#define ORBX_MAX_OBSERVATIONS (\d+)", header).group(1)) == MW.MAX_OBSERVATIONS
    hpp = open(os.path.join(ROOT, "extractorb_amd", "csrc", "k_map_point_update.hpp")).read()
    assert int(re.search(r"kMpuMaxObservations = (\d+)", hpp).group(1)) == MW.MAX_OBSERVATIONS
    enum = re.search(r"enum orbx_map_point_update \{(.*?)\};", header, re.S).group(1)
    names = re.findall(r"ORBX_MAP_POINT_([A-Z_]+) = (\d+)", enum)
    assert [(n.lower(), int(v)) for n, v in names] == list(zip(MW.STATUS_NAMES, range(5)))
    for sym in ("orbx_update_map_points_device", "orbx_update_map_points_two_eyes_device"):
        assert sym in X.header_symbols()
    assert hasattr(X.ORBextractor, "update_map_points_device") and hasattr(X.ORBextractor, "update_map_points_two_eyes_device")
