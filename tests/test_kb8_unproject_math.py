"""extractorb_amd/csrc/k_camera_kb8_unproject.hpp compiled for the host (tests/cpp/kb8_unproject_host_check.cpp behind tests/cpp/host_shim):
  * tanf32 against the host libm's tanf: every float of [-pi/2 - 1, pi/2 + 1] (the clamped theta_d after the Newton steps, plus slack) and a
    structured set outside it (the neighbourhoods of n * pi/2 on both sides of 120, where the reduction changes, every exponent, the
    thresholds, zeros, infinities, NaN, 2^22 raw bit patterns); kb8Unproject against a plain statement of KannalaBrandt8::unproject
    (reference src/CameraModels/KannalaBrandt8.cpp:103-130) that calls libm, on 10^7 pseudo-random pixels, the principal point among them.
    Equality of bytes (two NaN results count as equal).  The header restates glibc 2.35's algorithms: on another glibc a mismatch skips with
    that reason, on 2.35 it fails (tests/test_kb8_math.py's rule);
  * nullVector4 (the project's definition of vt.row(3) of cv::SVD::compute: a one-sided Jacobi in binary32) against numpy on 10^5 matrices
    built as KannalaBrandt8::Triangulate builds them from KB8 scenes: small and wide parallax, a point near infinity, identical rays.  The
    measure is the residual |A v| / |v|; the floor is the float64 sigma4; the yardstick is numpy's BINARY32 np.linalg.svd on the same
    matrices, an independent binary32 SVD: the Jacobi residual's worst excess over sigma4 may be at most 4 times numpy's worst excess;
  * the Python walk's unproject / null_vector4 / triangulate_matches (tests/triangulation_two_eyes_walk.py) byte-equal to the header's.
MEASURED (numpy's LAPACK sgesdd), 10^5 matrices: worst excess of the Jacobi residual over sigma4 3.44e-08, of numpy's binary32 SVD 2.58e-08
(ratio 1.34; without the routine's correction step 1.29e-07, ratio 5.0); docs/history/r18_two_eyes_triangulation.md."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import triangulation_two_eyes_scenes as S
import triangulation_two_eyes_walk as W
from test_kb8_math import HOST_FLAGS, ROOT, settle

f32 = np.float32
VP = C.c_void_p


def build_kb8_unproject_host(directory):
    """tests/cpp/kb8_unproject_host_check.cpp as a shared library (also used by the GPU tests)"""
    so = os.path.join(str(directory), "libkb8_unproject_host.so")
    subprocess.check_call(["g++", "-O2", "-fPIC", "-shared", *HOST_FLAGS, os.path.join(ROOT, "tests", "cpp", "kb8_unproject_host_check.cpp"), "-o", so])
    L = C.CDLL(so)
    for name in ("kb8u_check_tan_range", "kb8u_check_tan_structured", "kb8u_check_unproject"):
        getattr(L, name).restype = C.c_long
    L.kb8u_check_tan_range.argtypes = [C.c_int]
    L.kb8u_check_tan_structured.argtypes = [C.POINTER(C.c_long)]
    L.kb8u_check_unproject.argtypes = [C.c_long, C.c_ulonglong]
    L.kb8u_unproject.argtypes = [VP, C.c_int, VP, VP]
    L.kb8u_unproject_libm.argtypes = [VP, C.c_int, VP, VP]
    L.kb8u_null_vector.argtypes = [C.c_int, VP, VP]
    L.kb8u_triangulate.argtypes = [VP, VP, VP, VP, C.c_float, C.c_float, C.c_int, VP, VP, VP, VP, VP]
    L.kb8u_jacobi_sweeps.restype = C.c_int
    L.kb8u_jacobi_eps.restype = C.c_float
    return L


def ptr(a):
    return a.ctypes.data_as(VP)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_kb8_unproject_host(tmp_path_factory.mktemp("kb8u"))


@pytest.mark.parametrize("negative", [1, 0])
def test_tan_on_every_float_of_the_unprojection_range(host, negative):
    settle(host.kb8u_check_tan_range(negative), "tanf32 on every float of %s" % ("[-pi/2 - 1, -0]" if negative else "[0, pi/2 + 1]"))


def test_tan_on_the_structured_set(host):
    parts = (C.c_long * 3)()
    bad = host.kb8u_check_tan_structured(parts)
    assert parts[0] > 5_000_000 and parts[1] > 2_500 and parts[2] > 4_000_000      # neighbourhoods and grid, thresholds and exponents, specials and bit patterns
    settle(bad, "tanf32, structured set")


def test_unprojection_against_the_plain_statement(host):
    settle(host.kb8u_check_unproject(10_000_000, 1), "kb8Unproject on 10^7 pixels")


def test_the_principal_point_unprojects_along_the_axis(host):
    cam = S.CAMS[0]
    uv = np.array([cam[2], cam[3]], f32); ray = np.zeros(2, f32)
    host.kb8u_unproject(ptr(cam), 1, ptr(uv), ptr(ray))
    assert ray.tobytes() == np.zeros(2, f32).tobytes()                  # theta_d = 0: scale = 1, the ray is (0, 0, 1)


def triangulation_matrices(n, seed):
    """A of KannalaBrandt8::Triangulate (:428-431) for n KB8 scenes in binary32: a point seen from two poses; a quarter each with wide
    parallax, small parallax (baseline 1e-3 of the depth), the point near infinity, identical rays (no baseline, no rotation)"""
    rng = np.random.default_rng(seed)
    A = np.zeros((n, 4, 4), f32)
    for i in range(n):
        kind = i % 4
        z = rng.uniform(1.5, 8.0) * (1e4 if kind == 2 else 1.0)
        P = np.array([rng.uniform(-0.7, 0.7) * z, rng.uniform(-0.7, 0.7) * z, z])
        R21 = S.rodrigues(rng.uniform(-0.2, 0.2, 3)) if kind != 3 else np.eye(3)
        t21 = rng.uniform(-0.5, 0.5, 3) * (1e-3 * z if kind == 1 else 0.0 if kind == 3 else 1.0)
        P2 = R21 @ P + t21
        noise = rng.uniform(-1e-3, 1e-3, 4) if kind != 3 else np.zeros(4)
        p1 = P[:2] / P[2] + noise[:2]; p2 = P2[:2] / P2[2] + noise[2:]
        T2 = np.hstack([R21, t21[:, None]]).astype(f32)
        T1 = np.eye(3, 4, dtype=f32)
        for r, (p, T, k) in enumerate(((f32(p1[0]), T1, 0), (f32(p1[1]), T1, 1), (f32(p2[0]), T2, 0), (f32(p2[1]), T2, 1))):
            A[i, r] = (p * T[2]).astype(f32) - T[k]
    return A


def test_null_vector_against_numpy(host):
    n = 100_000
    A = triangulation_matrices(n, 3)
    v = np.zeros((n, 4), f32)
    host.kb8u_null_vector(n, ptr(A), ptr(v))
    A64 = A.astype(np.float64)
    sigma4 = np.linalg.svd(A64, compute_uv=False)[:, 3]
    v32 = np.linalg.svd(A)[2][:, 3, :]                                  # numpy's binary32 SVD (LAPACK sgesdd)
    assert v32.dtype == f32

    def residual(vec):
        vec = vec.astype(np.float64)
        return np.linalg.norm(np.einsum("nij,nj->ni", A64, vec), axis=1) / np.linalg.norm(vec, axis=1)

    jacobi, lapack = residual(v) - sigma4, residual(v32) - sigma4
    print("worst excess over sigma4: Jacobi %.3g, numpy binary32 SVD %.3g, ratio %.3g" % (jacobi.max(), lapack.max(), jacobi.max() / lapack.max()))
    for kind, name in enumerate(("wide parallax", "small parallax", "near infinity", "identical rays")):
        print("  %-15s Jacobi %.3g numpy %.3g" % (name, jacobi[kind::4].max(), lapack[kind::4].max()))
    assert np.isfinite(v).all()
    assert jacobi.max() <= 4 * lapack.max()


def test_the_walk_states_the_header(host):
    """the Python statements of tests/triangulation_two_eyes_walk.py, over libm, give the bytes of the header's routines"""
    assert host.kb8u_jacobi_sweeps() == W.JACOBI_SWEEPS and f32(host.kb8u_jacobi_eps()) == W.JACOBI_EPS
    m = W.libm_math()
    rng = np.random.default_rng(5)
    cam1, cam2 = S.CAMS
    uv = rng.uniform(0, 512, (300, 2)).astype(f32); uv[0] = cam1[2:4]
    rays = np.zeros((300, 2), f32)
    host.kb8u_unproject(ptr(cam1), 300, ptr(uv), ptr(rays))
    mine = np.array([W.unproject(m, cam1, u, v) for u, v in uv], f32)
    if mine.tobytes() != rays.tobytes():
        settle(int((mine != rays).sum()), "the walk's unproject against the header's")
    A = triangulation_matrices(400, 9)
    v = np.zeros((400, 4), f32)
    host.kb8u_null_vector(400, ptr(A), ptr(v))
    assert np.array([W.null_vector4(m, a) for a in A], f32).tobytes() == v.tobytes()
    # TriangulateMatches on pairs of a scene: true pairs, wrong pairs, far points
    s = S.make(1)
    R12, t12 = S.relative64(s["kfs"][0]["pose"], s["kfs"][1]["pose"], 0, 1)
    R12 = R12.astype(f32); t12 = t12.astype(f32)
    k1, k2 = s["kfs"][0]["eyes"][0]["kps"], s["kfs"][1]["eyes"][1]["kps"]
    n = min(len(k1), len(k2)) * 4
    i1 = rng.integers(0, len(k1), n); i2 = rng.integers(0, len(k2), n)
    by_point = {id(f["p"]): j for j, f in enumerate(s["kfs"][1]["eyes"][1]["feats"])}
    for a, f in enumerate(s["kfs"][0]["eyes"][0]["feats"]):            # the true partners first
        if id(f["p"]) in by_point and a < n:
            i1[a], i2[a] = a, by_point[id(f["p"])]
    kp1 = np.stack([k1["x"][i1], k1["y"][i1]], 1).astype(f32); kp2 = np.stack([k2["x"][i2], k2["y"][i2]], 1).astype(f32)
    z = np.zeros(n, f32); x = np.zeros((n, 3), f32); why = np.zeros(n, np.int32)
    host.kb8u_triangulate(ptr(cam1), ptr(cam2), ptr(R12), ptr(t12), 1.0, 1.44, n, ptr(kp1), ptr(kp2), ptr(z), ptr(x), ptr(why))
    want = [W.triangulate_matches(m, cam1, cam2, kp1[i], kp2[i], R12, t12, 1.0, 1.44) for i in range(n)]
    assert (z > 0.0001).sum() >= 5 and len(set(why.tolist())) >= 4, (int((z > 0.0001).sum()), np.bincount(why).tolist())
    same = np.array([w[0] for w in want], f32).tobytes() == z.tobytes() and np.array([w[1] for w in want], f32).tobytes() == x.tobytes() \
        and [w[2] for w in want] == why.tolist()
    if not same:
        settle(1, "the walk's triangulate_matches against the header's")


def zero_w_pairs():
    """R12 = diag(1, 1, 0), t12 = (0.5, 0, 0) and keypoint pairs: [0] both on their principal points (both rays (0, 0, 1): R12*r2 is the zero
    vector, cosParallaxRays NaN, column 2 of A zero: vt.row(3) = (0, 0, 1, 0), x3D = (NaN, NaN, inf), the result inf); then kp1 on the
    principal point against other kp2 (cos = 0: column 2 of A is zero again), and ordinary pairs under the degenerate pose"""
    cam1, cam2 = S.CAMS
    rng = np.random.default_rng(8)
    kp1 = np.tile(cam1[2:4], (8, 1)).astype(f32); kp2 = rng.uniform(100, 400, (8, 2)).astype(f32)
    kp2[0] = cam2[2:4]
    kp1[4:] = rng.uniform(100, 400, (4, 2)).astype(f32)
    return np.diag([1, 1, 0]).astype(f32), np.array([0.5, 0, 0], f32), kp1, kp2


def same_floats(a, b):
    """bytes equal, two NaNs counting as equal (0 / 0 has the sign the hardware gives it)"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return np.array_equal(np.isnan(a), np.isnan(b)) and a[~np.isnan(a)].tobytes() == b[~np.isnan(b)].tobytes()


def test_a_zero_fourth_component_flows_through(host):
    """the reference's outcome: infinity / NaN flow through, every <= and > on them is false, the result inf is accepted"""
    m = W.libm_math()
    cam1, cam2 = S.CAMS
    R12, t12, kp1, kp2 = zero_w_pairs()
    n = len(kp1)
    z = np.zeros(n, f32); x = np.zeros((n, 3), f32); why = np.zeros(n, np.int32)
    host.kb8u_triangulate(ptr(cam1), ptr(cam2), ptr(R12), ptr(t12), 1.0, 1.0, n, ptr(kp1), ptr(kp2), ptr(z), ptr(x), ptr(why))
    dbg = [{} for _ in range(n)]
    want = [W.triangulate_matches(m, cam1, cam2, kp1[i], kp2[i], R12, t12, 1.0, 1.0, debug=dbg[i]) for i in range(n)]
    assert [float(v) for v in dbg[0]["vt"]] == [0, 0, 1, 0]                     # w == 0 occurred
    assert np.isposinf(z[0]) and z[0] > f32(0.0001) and why[0] == W.OK and np.isnan(x[0, 0]) and np.isnan(x[0, 1]) and np.isposinf(x[0, 2])
    assert sum(1 for d in dbg if "vt" in d and float(d["vt"][3]) == 0) >= 4
    assert same_floats(z, [w[0] for w in want]) and same_floats(x, [w[1] for w in want]) and why.tolist() == [w[2] for w in want]
