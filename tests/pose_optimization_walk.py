"""The checker of orbx_optimize_pose_device: a sequential restatement in numpy binary64 of Optimizer::PoseOptimization (reference
src/Optimizer.cc:854-1168) with the g2o pieces under it - OptimizationAlgorithmLevenberg::solve, SparseOptimizer::optimize and
initializeOptimization(0), BaseUnaryEdge::constructQuadraticForm, RobustKernelHuber, SE3Quat (exp, the product, map), the three edge types
and the Eigen overloads of Pinhole / KannalaBrandt8 project and projectJac.  It is written as the reference's LOOPS: four rounds from the
initial pose, ten iterations, ten trials, the level flags.  What is Eigen's (the quaternion, the 6x6 solve, the order of the sums) is the
project's definition, stated in extractorb_amd/csrc/k_pose_optimization.hpp; this file states the same definitions a second time.

The edges of a pass are evaluated as numpy arrays - an elementwise binary64 operation rounds as the scalar one does - and summed in the
DECLARED order: SLOTS slots, slot s adds the active edges s, s + SLOTS, .. in ascending index onto 0.0, then the balanced tree (slot_sum).
`order="sequential"` replaces that by g2o's own edge-by-edge sum, `solver="numpy"` the Cholesky by numpy.linalg.solve, `math=LIBM_MATH`
the header's sin / cos / atan2 by libm: the float64 statement of tests/test_pose_optimization.py (d).

A problem is a dict: eyes, model, model2, cam[8], cam2[8], mbf, Trl[12], inv_sigma2[16], n [eyes], kps [eyes][cap] (x, y, octave),
u_right [cap] or None, matches [eyes][cap], world [M, 3], pose[12], flags [eyes][cap] uint8 (in/out), nlevels.  solve() returns a dict of
the result row's fields plus pose (12 floats or None), flags and a trace for the tests."""
import numpy as np

import sim3_solver_walk as SW

f32, f64 = np.float32, np.float64
STATUS = ("ALL_ROUNDS", "FEW_EDGES", "TOO_FEW", "BAD_ARGUMENT")
ALL_ROUNDS, FEW_EDGES, TOO_FEW, BAD_ARGUMENT = range(4)
SLOTS, SUMS = 256, 28
DBL_MAX = f64(1.7976931348623157e308)
CHI2_MONO, CHI2_STEREO = f32(5.991), f32(7.815)
DELTA_MONO, DELTA_STEREO = f64(f32(np.sqrt(f64(5.991)))), f64(f32(np.sqrt(f64(7.815))))
HEADER_MATH, LIBM_MATH = SW.HEADER_MATH, SW.LIBM_MATH
UPPER = [(r, c) for r in range(6) for c in range(r, 6)]


# ---- the sums -----------------------------------------------------------------------------------------------------------------------------
def slot_sum(terms, active):
    """terms [K, N], active [K] bool: the declared order"""
    terms = np.asarray(terms, f64)
    K, N = terms.shape
    acc = np.zeros((SLOTS, N), f64)
    with np.errstate(all="ignore"):
        for base in range(0, K, SLOTS):
            chunk = np.zeros((SLOTS, N), f64)
            on = np.zeros(SLOTS, bool)
            m = min(SLOTS, K - base)
            chunk[:m] = terms[base:base + m]
            on[:m] = active[base:base + m]
            acc = np.where(on[:, None], acc + np.where(on[:, None], chunk, 0.0), acc)
        idx = np.arange(SLOTS)
        stride = 1
        while stride < SLOTS:
            acc = acc + acc[idx ^ stride]
            stride *= 2
    return acc[0].copy()


def sequential_sum(terms, active):
    """g2o's own order: edge by edge onto 0.0"""
    terms = np.asarray(terms, f64)
    acc = np.zeros(terms.shape[1], f64)
    with np.errstate(all="ignore"):
        for k in np.nonzero(active)[0]:
            acc = acc + terms[k]
    return acc


# ---- Eigen's quaternion and g2o's SE3Quat (q = x, y, z, w) -------------------------------------------------------------------------------
def normalize(q):
    q = [f64(v) for v in q]
    if q[3] < 0:
        q = [-v for v in q]
    n = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return [v / n for v in q]


def quat_from_matrix(R):
    R = [f64(v) for v in np.asarray(R, f64).reshape(9)]
    t = (R[0] + R[4]) + R[8]
    if t > 0:
        t = np.sqrt(t + f64(1.0))
        w = f64(0.5) * t
        t = f64(0.5) / t
        return [(R[7] - R[5]) * t, (R[2] - R[6]) * t, (R[3] - R[1]) * t, w]
    i = 0
    if R[4] > R[0]:
        i = 1
    if R[8] > R[4 * i]:
        i = 2
    j = (i + 1) % 3
    k = (j + 1) % 3
    t = np.sqrt(((R[4 * i] - R[4 * j]) - R[4 * k]) + f64(1.0))
    q = [None] * 4
    q[i] = f64(0.5) * t
    t = f64(0.5) / t
    q[3] = (R[3 * k + j] - R[3 * j + k]) * t
    q[j] = (R[3 * j + i] + R[3 * i + j]) * t
    q[k] = (R[3 * k + i] + R[3 * i + k]) * t
    return q


def rot_matrix(q):
    x, y, z, w = q
    two = f64(2.0)
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * w, ty * w, tz * w, tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    one = f64(1.0)
    return [one - (tyy + tzz), txy - twz, txz + twy, txy + twz, one - (txx + tzz), tyz - twx, txz - twy, tyz + twx, one - (txx + tyy)]


def rotate(q, v):
    """q * v; v = three scalars or three arrays"""
    uv = [q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]]
    uv = [a + a for a in uv]
    c = [q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]]
    return [(v[k] + q[3] * uv[k]) + c[k] for k in range(3)]


def se3_map(T, X):
    r = rotate(T[0], X)
    return [r[k] + T[1][k] for k in range(3)]


def se3_mul(A, B):
    r = rotate(A[0], B[1])
    a, b = A[0], B[0]
    w = ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2]
    x = ((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1]
    y = ((a[3] * b[1] + a[1] * b[3]) + a[2] * b[0]) - a[0] * b[2]
    z = ((a[3] * b[2] + a[2] * b[3]) + a[0] * b[1]) - a[1] * b[0]
    return (normalize([x, y, z, w]), [A[1][k] + r[k] for k in range(3)])


def se3_from_float(T12):
    T = np.asarray(T12, f32).reshape(3, 4).astype(f64)
    return (normalize(quat_from_matrix(T[:, :3])), [f64(T[r, 3]) for r in range(3)])


def canon32(x):
    x = f32(x)
    return np.frombuffer(np.uint32(0x7fc00000).tobytes(), f32)[0] if np.isnan(x) else x


def canon64(x):
    x = f64(x)
    return f64(f32(np.frombuffer(np.uint32(0x7fc00000).tobytes(), f32)[0])) if np.isnan(x) else x


def se3_to_float(T):
    R = rot_matrix(T[0])
    out = np.zeros(12, f32)
    with np.errstate(all="ignore"):
        for r in range(3):
            for c in range(3):
                out[4 * r + c] = canon32(R[3 * r + c])
            out[4 * r + 3] = canon32(T[1][r])
    return out


def mat3(A, B):
    return [(A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c] for r in range(3) for c in range(3)]


def se3_exp(x, m=HEADER_MATH):
    x = [f64(v) for v in x]
    zero, one = f64(0.0), f64(1.0)
    theta = np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])
    Om = [zero, -x[2], x[1], x[2], zero, -x[0], -x[1], x[0], zero]
    Om2 = mat3(Om, Om)
    I = [one if k % 4 == 0 else zero for k in range(9)]
    if theta < 0.00001:
        R = [(I[k] + Om[k]) + Om2[k] for k in range(9)]
        V = list(R)
    else:
        s, c = m["sincos"](theta)
        th2 = theta * theta
        a, b, d = s / theta, (one - c) / th2, (theta - s) / (th2 * theta)
        R = [(I[k] + a * Om[k]) + b * Om2[k] for k in range(9)]
        V = [(I[k] + b * Om[k]) + d * Om2[k] for k in range(9)]
    q = normalize(quat_from_matrix(R))
    return (q, [(V[3 * r] * x[3] + V[3 * r + 1] * x[4]) + V[3 * r + 2] * x[5] for r in range(3)])


# ---- the cameras: X = three arrays ----------------------------------------------------------------------------------------------------------
def _each(fn, *arrays):
    return np.array([fn(*[a[i] for a in arrays]) for i in range(len(arrays[0]))], f64).reshape(len(arrays[0]), -1)


def project(model, k, X, m=HEADER_MATH):
    k = [f32(v) for v in k]
    if not model:
        return [f64(k[0]) * X[0] / X[2] + f64(k[2]), f64(k[1]) * X[1] / X[2] + f64(k[3])]
    kb = SW.kb8_math()
    x2y2 = X[0] * X[0] + X[1] * X[1]
    theta = _each(lambda a, z: f64(kb["atan2f"](kb["sqrtf"](f32(a)), f32(z))), x2y2, X[2])[:, 0]
    psi = _each(lambda y, x: f64(kb["atan2f"](f32(y), f32(x))), X[1], X[0])[:, 0]
    t2 = theta * theta
    t3 = theta * t2
    t5 = t3 * t2
    t7 = t5 * t2
    t9 = t7 * t2
    r = (((theta + f64(k[4]) * t3) + f64(k[5]) * t5) + f64(k[6]) * t7) + f64(k[7]) * t9

    def sc(p):
        s, c = m["sincos"](abs(p))
        return (-s if p < 0 else s, c)
    scv = _each(sc, psi)
    return [(f64(k[0]) * r) * scv[:, 1] + f64(k[2]), (f64(k[1]) * r) * scv[:, 0] + f64(k[3])]


def project_jac(model, k, X, m=HEADER_MATH):
    """J[6] row-major 2x3, each an array"""
    k = [f32(v) for v in k]
    zero = np.zeros_like(X[0])
    if not model:
        zz = X[2] * X[2]
        return [f64(k[0]) / X[2], zero, f64(-k[0]) * X[0] / zz, zero, f64(k[1]) / X[2], f64(-k[1]) * X[1] / zz]
    x2, y2, z2 = X[0] * X[0], X[1] * X[1], X[2] * X[2]
    r2 = x2 + y2
    r = np.sqrt(r2)
    r3 = r2 * r
    theta = _each(lambda a, b: m["atan2"](a, b), r, X[2])[:, 0]
    t2 = theta * theta
    t3 = t2 * theta
    t4 = t2 * t2
    t5 = t4 * theta
    t6 = t2 * t4
    t7 = t6 * theta
    t8 = t4 * t4
    t9 = t8 * theta
    f = (((theta + t3 * f64(k[4])) + t5 * f64(k[5])) + t7 * f64(k[6])) + t9 * f64(k[7])
    fd = (((f64(1.0) + f64(f32(3.0) * k[4]) * t2) + f64(f32(5.0) * k[5]) * t4) + f64(f32(7.0) * k[6]) * t6) + f64(f32(9.0) * k[7]) * t8
    den = r2 * (r2 + z2)
    fz = fd * X[2]
    cross = (fz * X[1]) * X[0] / den - (f * X[1]) * X[0] / r3
    return [f64(k[0]) * (fz * x2 / den + f * y2 / r3), f64(k[0]) * cross, (f64(-k[0]) * fd) * X[0] / (r2 + z2),
            f64(k[1]) * cross, f64(k[1]) * (fz * y2 / den + f * x2 / r3), (f64(-k[1]) * fd) * X[1] / (r2 + z2)]


def chain(J, X):
    """(-J) * SE3deriv(X): A[r][c], every product"""
    zero, one = np.zeros_like(X[0]), np.ones_like(X[0])
    D = [zero, X[2], -X[1], one, zero, zero, -X[2], zero, X[0], zero, one, zero, X[1], -X[0], zero, zero, zero, one]
    return [[((-J[3 * r]) * D[c] + (-J[3 * r + 1]) * D[6 + c]) + (-J[3 * r + 2]) * D[12 + c] for c in range(6)] for r in range(2)]


# ---- the edges of a problem -------------------------------------------------------------------------------------------------------------
class Edges:
    """the edges in index order k = eye * cap + i: kind (0 none, 1 mono, 2 stereo, 3 right), obs [K, 3], X [K, 3], w [K]"""

    def __init__(self, pb):
        cap, eyes = pb["cap"], pb["eyes"]
        K = cap * eyes
        self.K, self.cap = K, cap
        self.kind = np.zeros(K, np.int32)
        self.obs, self.X, self.w = np.zeros((K, 3), f64), np.zeros((K, 3), f64), np.zeros(K, f64)
        for eye in range(eyes):
            for i in range(pb["n"][eye]):
                mi = int(pb["matches"][eye][i])
                if mi < 0:
                    continue
                k = eye * cap + i
                kp = pb["kps"][eye][i]
                self.obs[k, 0], self.obs[k, 1] = f64(f32(kp["x"])), f64(f32(kp["y"]))
                self.w[k] = f64(f32(pb["inv_sigma2"][int(kp["octave"])]))
                self.X[k] = np.asarray(pb["world"][mi], f32).astype(f64)
                self.kind[k] = 3 if eye else 1
                if eyes == 1 and pb["u_right"] is not None:
                    ur = f32(pb["u_right"][i])
                    if not ur < 0:
                        self.kind[k] = 2
                        self.obs[k, 2] = f64(ur)


def errors(pb, ed, T, m):
    """computeError of every edge at the estimate T: e [K, 3], chi2 [K], we [K, 3] (information * e)"""
    K = ed.K
    e = np.zeros((K, 3), f64)
    dim = np.where(ed.kind == 2, 3, 2)
    cam = [f64(f32(v)) for v in pb["cam"]]
    with np.errstate(all="ignore"):
        for kind in (1, 2, 3):
            sel = np.nonzero(ed.kind == kind)[0]
            if not len(sel):
                continue
            X = [ed.X[sel, c] for c in range(3)]
            if kind == 2:
                Xc = se3_map(T, X)
                invz = (f64(1.0) / Xc[2]).astype(f32).astype(f64)
                u = ((Xc[0] * invz) * cam[0]) + cam[2]
                v = ((Xc[1] * invz) * cam[1]) + cam[3]
                e[sel, 0], e[sel, 1], e[sel, 2] = ed.obs[sel, 0] - u, ed.obs[sel, 1] - v, ed.obs[sel, 2] - (u - f64(f32(pb["mbf"])) * invz)
                continue
            if kind == 3:
                Xc = se3_map(se3_mul(se3_from_float(pb["Trl"]), T), X)
                uv = project(pb["model2"], pb["cam2"], Xc, m)
            else:
                Xc = se3_map(T, X)
                uv = project(pb["model"], pb["cam"], Xc, m)
            e[sel, 0], e[sel, 1] = ed.obs[sel, 0] - uv[0], ed.obs[sel, 1] - uv[1]
        w, z = ed.w, f64(0.0)
        we = np.zeros((K, 3), f64)
        two = dim == 2
        we2 = [w * e[:, 0] + z * e[:, 1], z * e[:, 0] + w * e[:, 1]]
        we3 = [(w * e[:, 0] + z * e[:, 1]) + z * e[:, 2], (z * e[:, 0] + w * e[:, 1]) + z * e[:, 2], (z * e[:, 0] + z * e[:, 1]) + w * e[:, 2]]
        we[:, 0], we[:, 1], we[:, 2] = np.where(two, we2[0], we3[0]), np.where(two, we2[1], we3[1]), np.where(two, 0.0, we3[2])
        chi2 = np.where(two, e[:, 0] * we[:, 0] + e[:, 1] * we[:, 1], (e[:, 0] * we[:, 0] + e[:, 1] * we[:, 1]) + e[:, 2] * we[:, 2])
    return e, chi2, we


def robust(ed, huber, chi2):
    """rho[0], rho[1] per edge"""
    with np.errstate(all="ignore"):
        if not huber:
            return chi2.copy(), np.ones_like(chi2)
        delta = np.where(ed.kind == 2, DELTA_STEREO, DELTA_MONO)
        dsqr = delta * delta
        sq = np.sqrt(chi2)
        inl = chi2 <= dsqr
        return np.where(inl, chi2, (f64(2.0) * sq) * delta - dsqr), np.where(inl, f64(1.0), delta / sq)


def jacobians(pb, ed, T, m):
    """linearizeOplus of every edge: A [K, 3, 6]"""
    A = np.zeros((ed.K, 3, 6), f64)
    with np.errstate(all="ignore"):
        for kind in (1, 2, 3):
            sel = np.nonzero(ed.kind == kind)[0]
            if not len(sel):
                continue
            Xl = se3_map(T, [ed.X[sel, c] for c in range(3)])
            if kind == 2:
                x, y = Xl[0], Xl[1]
                invz = f64(1.0) / Xl[2]
                invz2 = invz * invz
                fx, fy, bf = f64(f32(pb["cam"][0])), f64(f32(pb["cam"][1])), f64(f32(pb["mbf"]))
                one = f64(1.0)
                nil = np.zeros_like(x)
                rows = [[((x * y) * invz2) * fx, (-(one + (x * x) * invz2)) * fx, (y * invz) * fx, (-invz) * fx, nil, (x * invz2) * fx],
                        [(one + (y * y) * invz2) * fy, ((-x * y) * invz2) * fy, ((-x) * invz) * fy, nil, (-invz) * fy, (y * invz2) * fy]]
                rows.append([rows[0][0] - (bf * y) * invz2, rows[0][1] + (bf * x) * invz2, rows[0][2], rows[0][3], nil, rows[0][5] - bf * invz2])
            elif kind == 3:
                Trl = se3_from_float(pb["Trl"])
                Rrl = rot_matrix(Trl[0])
                Xr = se3_map(Trl, Xl)
                J = project_jac(pb["model2"], pb["cam2"], Xr, m)
                M = [((-J[3 * r]) * Rrl[c] + (-J[3 * r + 1]) * Rrl[3 + c]) + (-J[3 * r + 2]) * Rrl[6 + c] for r in range(2) for c in range(3)]
                rows = chain([-v for v in M], Xl)
            else:
                rows = chain(project_jac(pb["model"], pb["cam"], Xl, m), Xl)
            for r in range(len(rows)):
                for c in range(6):
                    A[sel, r, c] = rows[r][c]
    return A


def system_terms(ed, A, we, rho0, rho1):
    """the 28 terms of every edge: chi2, H's upper triangle row by row, g (b = -sum g)"""
    terms = np.zeros((ed.K, SUMS), f64)
    three = ed.kind == 2
    with np.errstate(all="ignore"):
        terms[:, 0] = rho0
        w = rho1 * ed.w
        for at, (r, c) in enumerate(UPPER):
            h = (A[:, 0, r] * w) * A[:, 0, c] + (A[:, 1, r] * w) * A[:, 1, c]
            terms[:, 1 + at] = np.where(three, h + (A[:, 2, r] * w) * A[:, 2, c], h)
        for j in range(6):
            g = A[:, 0, j] * we[:, 0] + A[:, 1, j] * we[:, 1]
            terms[:, 22 + j] = rho1 * np.where(three, g + A[:, 2, j] * we[:, 2], g)
    return terms


# ---- the 6x6 solve ----------------------------------------------------------------------------------------------------------------------
def solve6(Hu, lam, b, x):
    """(H + lambda I) x = b by Cholesky; returns (ok, x): a pivot that is not > 0 leaves x as it was"""
    L = [[f64(0.0)] * 6 for _ in range(6)]
    for at, (r, c) in enumerate(UPPER):
        L[c][r] = Hu[at] + (lam if r == c else f64(0.0))
    ok = True
    with np.errstate(all="ignore"):
        for j in range(6):
            d = L[j][j]
            for k in range(j):
                d = d - L[j][k] * L[j][k]
            if not d > 0:
                ok = False
            d = np.sqrt(d)
            L[j][j] = d
            for i in range(j + 1, 6):
                s = L[i][j]
                for k in range(j):
                    s = s - L[i][k] * L[j][k]
                L[i][j] = s / d
        if not ok:
            return False, list(x)
        y = [None] * 6
        for i in range(6):
            s = b[i]
            for k in range(i):
                s = s - L[i][k] * y[k]
            y[i] = s / L[i][i]
        out = [None] * 6
        for i in range(5, -1, -1):
            s = y[i]
            for k in range(i + 1, 6):
                s = s - L[k][i] * out[k]
            out[i] = s / L[i][i]
    return True, out


def solve6_numpy(Hu, lam, b, x):
    H = np.zeros((6, 6), f64)
    for at, (r, c) in enumerate(UPPER):
        H[r, c] = H[c, r] = Hu[at]
    H = H + np.eye(6) * lam
    if not np.all(np.isfinite(H)):
        return False, list(x)
    try:
        np.linalg.cholesky(H)
    except np.linalg.LinAlgError:
        return False, list(x)
    return True, [f64(v) for v in np.linalg.solve(H, np.asarray(b, f64))]


# ---- the function -----------------------------------------------------------------------------------------------------------------------
def solve(pb, math=HEADER_MATH, order="slots", solver="cholesky", observe=None, perturb=None):
    """Everything from :856 to :1167.  pb["flags"] is updated in place as mvbOutlier is.  observe(name, **values): the float64 statement's
    margins (test (d)); perturb(sums, terms, active) -> sums: that test's derivation of its bound."""
    plain = slot_sum if order == "slots" else sequential_sum
    summer = plain if perturb is None else (lambda terms, active: perturb(plain(terms, active), np.asarray(terms, f64), active))
    solver = solve6 if solver == "cholesky" else solve6_numpy
    see = observe or (lambda *a, **k: None)
    cap, eyes, m = pb["cap"], pb["eyes"], math
    res = dict(status=BAD_ARGUMENT, n_initial=0, n_bad=0, n_inliers=0, rounds=0, empty_rounds=0, its=[0] * 4, trials=[0] * 4,
               lam=[f64(0.0)] * 4, chi2=[f64(0.0)] * 4, pose=None, trace=[])
    bad = bool(pb["model"] & ~1) or (eyes == 2 and bool(pb["model2"] & ~1))
    bad = bad or any(pb["n"][e] < 0 or pb["n"][e] > cap for e in range(eyes))
    if not bad:
        for eye in range(eyes):
            for i in range(pb["n"][eye]):
                mi = int(pb["matches"][eye][i])
                if mi < -1 or mi >= len(pb["world"]):
                    bad = True
                elif mi >= 0:
                    o = int(pb["kps"][eye][i]["octave"])
                    if o < 0 or o >= pb["nlevels"]:
                        bad = True
                    else:
                        res["n_initial"] += 1
    if bad:
        res["n_initial"] = 0
        return res
    ed = Edges(pb)
    flags = np.zeros(ed.K, bool)                                  # mvbOutlier[i] = false (:908 ..): the level flags between the rounds
    exists = ed.kind != 0

    def store():
        for eye in range(eyes):
            for i in range(pb["n"][eye]):
                if ed.kind[eye * cap + i]:
                    pb["flags"][eye][i] = 1 if flags[eye * cap + i] else 0
    store()
    if res["n_initial"] < 3:                                        # :1050
        res["status"] = TOO_FEW
        return res
    T0 = se3_from_float(pb["pose"])
    T = T0
    with np.errstate(all="ignore"):
        for rnd in range(4):
            huber = rnd < 3                                         # setRobustKernel(0) follows round 2's classification
            T = T0                                                  # :1063: mTcw is not written before :1163
            err_T = T0
            active = exists & ~flags
            res["rounds"] = rnd + 1
            trace = dict(round=rnd, rejected_last=False, small_theta=0, terminate=None, accepted=0)
            if not active.any():                                    # no index mapping: optimize returns -1
                res["its"][rnd] = -1
                res["empty_rounds"] |= 1 << rnd
            else:
                lam, ni, n_bad_lm, cj, trials = f64(0.0), f64(2.0), 0, 0, 0
                x = [f64(0.0)] * 6
                current = f64(0.0)
                for it in range(10):
                    e, chi2, we = errors(pb, ed, T, m)
                    rho0, rho1 = robust(ed, huber, chi2)
                    S = summer(system_terms(ed, jacobians(pb, ed, T, m), we, rho0, rho1), active)
                    current = S[0]
                    ini = current
                    Hu, b = [S[1 + k] for k in range(21)], [-S[22 + k] for k in range(6)]
                    if it == 0:
                        max_d, at = f64(0.0), 0
                        for j in range(6):
                            h = abs(Hu[at])
                            max_d = max_d if h < max_d else h
                            at += 6 - j
                        lam, ni, n_bad_lm = f64(1e-5) * max_d, f64(2.0), 0
                    rho, qmax = f64(0.0), 0
                    while True:
                        backup = T
                        ok2, x = solver(Hu, lam, b, x)
                        if float(np.sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2])) < 0.00001:
                            trace["small_theta"] += 1
                        T = se3_mul(se3_exp(x, m), T)
                        err_T = T
                        _, chi2t, _ = errors(pb, ed, T, m)
                        temp = summer(robust(ed, huber, chi2t)[0][:, None], active)[0]
                        if not ok2:
                            temp = DBL_MAX
                        rho = current - temp
                        scale = f64(0.0)
                        for j in range(6):
                            scale = scale + x[j] * (lam * x[j] + b[j])
                        scale = scale + f64(1e-3)
                        rho = rho / scale
                        see("rho", value=rho, current=current, temp=temp)
                        if rho > 0 and np.isfinite(temp):
                            t = f64(2.0) * rho - f64(1.0)
                            alpha = f64(1.0) - (t * t) * t
                            hi, lo = f64(2.0) / f64(3.0), f64(1.0) / f64(3.0)
                            alpha = hi if hi < alpha else alpha
                            lam = lam * (alpha if lo < alpha else lo)
                            ni = f64(2.0)
                            current = temp
                            trace["rejected_last"] = False
                            trace["accepted"] += 1
                        else:
                            lam = lam * ni
                            ni = ni * f64(2.0)
                            T = backup
                            trace["rejected_last"] = True
                        qmax += 1
                        if not (rho < 0 and qmax < 10):
                            break
                    trials += qmax
                    cj += 1
                    if qmax == 10 or rho == 0:
                        trace["terminate"] = "trials" if qmax == 10 else "rho"
                        break
                    see("nbad", lhs=(ini - current) * f64(1e3), rhs=ini)
                    if (ini - current) * f64(1e3) < ini:
                        n_bad_lm += 1
                    else:
                        n_bad_lm = 0
                    if n_bad_lm >= 3:
                        trace["terminate"] = "nbad"
                        break
                res["its"][rnd], res["trials"][rnd], res["lam"][rnd], res["chi2"][rnd] = cj, trials, canon64(lam), canon64(current)
            # the classification
            _, chi_fresh, _ = errors(pb, ed, T, m)
            _, chi_stale, _ = errors(pb, ed, err_T, m)
            chi = np.where(flags, chi_fresh, chi_stale).astype(f32)
            thr = np.where(ed.kind == 2, CHI2_STEREO, CHI2_MONO)
            see("chi2", values=np.where(flags, chi_fresh, chi_stale)[exists], thresholds=thr[exists].astype(f64))
            trace["fresh_flags"] = (exists & (chi_fresh.astype(f32) > thr))
            flags = exists & (chi > thr)
            trace["flags"] = flags.copy()
            res["n_bad"] = int(flags.sum())
            res["trace"].append(trace)
            if res["n_initial"] < 10:                               # :1155
                break
    store()
    res["status"] = ALL_ROUNDS if res["rounds"] == 4 else FEW_EDGES
    res["n_inliers"] = res["n_initial"] - res["n_bad"]
    res["pose"] = se3_to_float(T)
    res["T"] = T
    return res
