"""extractorb_amd/csrc/k_small_math.hpp is the only statement of the draw without replacement (TwoViewReconstruction's sets of 8, Sim3Solver's of
3) and of the canonical quiet NaN, and k_small_svd.hpp's jacobiPair<N> the only statement of the one-sided Jacobi pair rotation (nullVector4,
topEigenvector4, svd3).  Here they are called directly: tests/cpp/small_math_check.cpp is the two headers compiled for the host behind
tests/cpp/host_shim (as a sanitized stand-alone program), and every answer is compared with an independent statement below - the reference's
vector with its swap-and-pop for the draw, float32 steps with the angle formulas as an if / else for the pair, the bit patterns for the NaN.
No GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
RAND_MAX = 2 ** 31 - 1
QUIET_NAN = 0x7FC00000
JACOBI_EPS = f32(2.0 ** -22)      # kJacobiEps


def bits(x):
    return struct.unpack("<I", struct.pack("<f", float(x)))[0]


def from_bits(u):
    return f32(struct.unpack("<f", struct.pack("<I", u))[0])


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("small_math") / "small_math_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "tests", "cpp"), "-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"),
                           "-I" + os.path.join(ROOT, "extractorb_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "small_math_check.cpp"), "-o", exe])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [line.split() for line in out]
    return run


# ---- the draw without replacement -----------------------------------------------------------------------------------------------------------
def draw(k, n, raw):
    """the reference's loop (TwoViewReconstruction.cc:83-95, Sim3Solver.cc:251-262) on a real list"""
    avail = list(range(n))
    out = []
    for j in range(k):
        randi = int((float(raw[j]) / 2147483648.0) * len(avail))      # DUtils::Random::RandomInt(0, size - 1)
        randi = max(0, min(randi, len(avail) - 1))
        out.append(avail[randi])
        avail[randi] = avail[-1]
        avail.pop()
    return out


def raw_for(randi, size):
    """a raw rand() value that RandomInt turns into randi of `size`"""
    r = -(-randi * 2 ** 31 // size)
    assert int((r / 2147483648.0) * size) == randi
    return r


def test_draw_statement_on_worked_examples():
    assert draw(3, 3, [0, 0, 0]) == [0, 2, 1]                        # slot 0 every time: 0, then the displaced last, then what displaced that
    assert draw(3, 3, [RAND_MAX] * 3) == [2, 1, 0]                   # the last slot every time
    assert draw(3, 10, [0, RAND_MAX, 0]) == [0, 8, 9]                # the first draw put 9 into slot 0
    assert draw(8, 8, [0] * 8) == [0, 7, 6, 5, 4, 3, 2, 1]


@pytest.mark.parametrize("k", [3, 8])
def test_draw_set(ask, k):
    cases = []
    for n in (k, k + 1, 2 * k, 300, 100000):                         # N == K: the last draw has one slot left
        cases += [(n, [0] * k), (n, [RAND_MAX] * k), (n, [RAND_MAX // 2] * k),                    # repeated values
                  (n, [0, RAND_MAX] * (k // 2) + [0] * (k % 2)), (n, [RAND_MAX, 0] * (k // 2) + [RAND_MAX] * (k % 2)),
                  (n, [raw_for(min(1, n - 1 - j), n - j) for j in range(k)]),                      # slot 1 (or the last) again and again
                  (n, [raw_for(n - 1 - j, n - j) if j % 2 else raw_for(0, n - j) for j in range(k)]),
                  (n, [raw_for(0, n - j) if j < k - 1 else raw_for(n - k, n - j) for j in range(k)])]      # the last draw reads the slot every earlier one displaced
    rng = np.random.default_rng(30 + k)
    for _ in range(200):
        n = int(rng.choice([k, k + 1, k + 2, 12, 60, 300]))
        cases.append((n, rng.integers(0, 2 ** 31, k).tolist()))
        cases.append((n, [raw_for(int(rng.integers(0, min(3, n - j))), n - j) for j in range(k)]))      # few slots, many collisions
    got = ask(["D %d %d %s" % (k, n, " ".join(map(str, raw))) for n, raw in cases])
    for (n, raw), g in zip(cases, got):
        want = draw(k, n, raw)
        assert [int(t) for t in g] == want, (n, raw)
        assert len(set(want)) == k and all(0 <= i < n for i in want)


# ---- the Jacobi pair ------------------------------------------------------------------------------------------------------------------------
def jacobi_pair(ai, aj, vi, vj):
    """one pair of a sweep in float32 steps, the angle as the if / else nullVector4 was first written with.  Returns rotated and the columns"""
    ai, aj, vi, vj = ([f32(x) for x in col] for col in (ai, aj, vi, vj))
    a = b = p = f32(0.0)
    with np.errstate(all="ignore"):
        for x0, x1 in zip(ai, aj):
            a = a + x0 * x0
            b = b + x1 * x1
            p = p + x0 * x1
        if not (abs(p) > JACOBI_EPS * np.sqrt(a * b)):               # (a NaN never rotates)
            return False, ai + aj + vi + vj
        p = p * f32(2.0)
        beta = a - b
        gamma = np.sqrt(p * p + beta * beta)
        if beta < 0:
            delta = (gamma - beta) * f32(0.5)
            s = np.sqrt(delta / gamma)
            c = p / ((gamma * s) * f32(2.0))
        else:
            c = np.sqrt((gamma + beta) / (gamma * f32(2.0)))
            s = p / ((gamma * c) * f32(2.0))
        rot = lambda u, w: ([c * x0 + s * x1 for x0, x1 in zip(u, w)], [c * x1 - s * x0 for x0, x1 in zip(u, w)])      # noqa: E731
        ni, nj = rot(ai, aj)
        wi, wj = rot(vi, vj)
    return True, ni + nj + wi + wj


def pair_cases(n):
    rng = np.random.default_rng(40 + n)
    unit = lambda k: [1.0 if t == k else 0.0 for t in range(n)]      # noqa: E731
    nan, inf = float("nan"), float("inf")
    cases = {
        "rotates, beta > 0": ([3.0, 1.0, 0.5, 0.25][:n], [1.0, 2.0, -0.5, 0.125][:n], unit(0), unit(1)),
        "rotates, beta < 0": ([1.0, 2.0, -0.5, 0.125][:n], [3.0, 1.0, 0.5, 0.25][:n], unit(0), unit(1)),
        "rotates, beta == 0": ([1.0, 2.0, 0.0, 0.0][:n], [2.0, 1.0, 0.0, 0.0][:n], unit(1), unit(2)),
        "rotates, negative p": ([1.0, -2.0, 0.5, 0.0][:n], [0.5, 3.0, 0.25, 0.0][:n], unit(0), unit(2)),
        "orthogonal: p == 0": ([1.0, 0.0, 0.0, 0.0][:n], [0.0, 2.0, 0.0, 0.0][:n], unit(0), unit(1)),
        "below kJacobiEps": ([1.0, 2.0 ** -24, 0.0, 0.0][:n], [0.0, 1.0, 0.0, 0.0][:n], unit(0), unit(1)),          # |p| = 2^-24 < 2^-22 * 1
        "exactly at kJacobiEps": ([1.0, 2.0 ** -22, 0.0, 0.0][:n], [0.0, 1.0, 0.0, 0.0][:n], unit(0), unit(1)),     # > is strict: no rotation
        "just above kJacobiEps": ([1.0, 2.0 ** -21, 0.0, 0.0][:n], [0.0, 1.0, 0.0, 0.0][:n], unit(0), unit(1)),
        "a zero column": ([0.0] * n, [1.0, 2.0, 3.0, 4.0][:n], unit(0), unit(1)),
        "both zero": ([0.0] * n, [0.0] * n, unit(0), unit(1)),
        "a NaN column": ([nan, 1.0, 2.0, 3.0][:n], [1.0, 2.0, 3.0, 4.0][:n], unit(0), unit(1)),
        "a NaN in the other": ([1.0, 2.0, 3.0, 4.0][:n], [1.0, nan, 3.0, 4.0][:n], unit(0), unit(1)),
        "an infinite column": ([inf, 1.0, 2.0, 3.0][:n], [1.0, 2.0, 3.0, 4.0][:n], unit(0), unit(1)),
        "a rotated V": ([0.3, -1.7, 2.2, 0.9][:n], [1.1, 0.4, -0.6, 2.5][:n], [0.6, 0.8, 0.0, 0.0][:n], [-0.8, 0.6, 0.0, 0.0][:n]),
    }
    for t in range(60):
        scale = 10.0 ** rng.integers(-6, 7)
        cases["random %d" % t] = tuple((rng.standard_normal(n) * (scale if c < 2 else 1.0)).astype(f32).tolist() for c in range(4))
    for t in range(20):                                              # nearly parallel and nearly orthogonal pairs
        x = rng.standard_normal(n).astype(f32)
        y = (x + f32(10.0 ** -rng.integers(1, 8)) * rng.standard_normal(n).astype(f32)) if t % 2 else rng.standard_normal(n).astype(f32) * f32(1e-7)
        cases["close %d" % t] = (x.tolist(), y.astype(f32).tolist(), unit(0), unit(1))
    return cases


@pytest.mark.parametrize("n", [3, 4])
def test_jacobi_pair(ask, n):
    cases = pair_cases(n)
    got = ask(["J %d %s" % (n, " ".join("%08x" % bits(f32(x)) for col in c for x in col)) for c in cases.values()])
    rotated = {}
    for (name, c), g in zip(cases.items(), got):
        want_rot, want = jacobi_pair(*c)
        rotated[name] = want_rot
        assert int(g[0]) == int(want_rot), name
        have = [int(t, 16) for t in g[1:]]
        if want_rot:
            assert have == [bits(x) for x in want], name
        else:                                                        # nothing is written: the input's own bits, a NaN's payload included
            assert have == [bits(f32(x)) for col in c for x in col], name
    assert rotated["rotates, beta > 0"] and rotated["rotates, beta < 0"] and rotated["rotates, beta == 0"] and rotated["just above kJacobiEps"]
    assert not rotated["below kJacobiEps"] and not rotated["exactly at kJacobiEps"] and not rotated["orthogonal: p == 0"]
    assert not rotated["a NaN column"] and not rotated["a NaN in the other"] and not rotated["both zero"] and not rotated["an infinite column"]


# ---- the canonical NaN ------------------------------------------------------------------------------------------------------------------------
def test_canonical_nan(ask):
    nans = [0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FC00001, 0x7FA00000]      # quiet, negative, signalling, payloads
    others = [0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x3F800000, 0x00000001, 0x807FFFFF, 0x7F7FFFFF]     # zeros, infinities, 1, subnormals, FLT_MAX
    got = ask(["C %08x" % u for u in nans + others])
    for u, g in zip(nans + others, got):
        assert int(g[1], 16) == QUIET_NAN
        assert int(g[0], 16) == (QUIET_NAN if u in nans else u), hex(u)
        assert np.isnan(from_bits(u)) == (u in nans)
    quiet64 = struct.unpack("<Q", struct.pack("<d", float(from_bits(QUIET_NAN))))[0]      # the float widened: 0x7ff8000000000000
    assert quiet64 == 0x7FF8000000000000
    nans64 = [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF, 0x7FF4000000000000]
    others64 = [0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x3FF0000000000000, 0x0000000000000001, 0x7FEFFFFFFFFFFFFF]
    got = ask(["E %016x" % u for u in nans64 + others64])
    for u, g in zip(nans64 + others64, got):
        assert int(g[0], 16) == (quiet64 if u in nans64 else u), hex(u)
