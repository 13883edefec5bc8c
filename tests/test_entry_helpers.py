"""extractorb_amd/csrc/orbx_entry.hpp is the one statement of what the C entry points of orbx_rows.cpp share: the two index-walk rules, the
empty-bounds test, the LDS budget, the distance clamp, the fills of the kernels' parameter blocks (grid, bounds, cameras, PredictScale's
breakpoints), the four padding rules of the level tables and the all-or-nothing regrow of a set of buffers.  Here they are called directly:
tests/cpp/entry_check.cpp is the header compiled for the host behind tests/cpp/host_shim (a sanitized stand-alone program), and every answer is
compared with an independent statement below.  Floats are compared as bit patterns.  No GPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

import extractorb_amd as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
GRID_COLS, GRID_ROWS, MAX_LEVELS = 64, 48, 16
LDS_BUDGET = 160 * 1024 - 512
INT_MAX = 2 ** 31 - 1


def bits(x):
    return "%08x" % struct.unpack("<I", struct.pack("<f", float(f32(x))))[0]


def words(values):
    return " ".join(bits(v) for v in values)


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("entry") / "entry_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"),
                           "-I" + os.path.join(ROOT, "extractorb_amd", "csrc"), "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "entry_check.cpp"), "-o", exe])

    def run(lines):
        done = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert done.returncode == 0, done.stderr[-2000:]      # a leak, a double free or an overflow ends the program with the sanitizer's report
        out = done.stdout.splitlines()
        assert len(out) == len(lines)
        return [line.split() for line in out]
    return run


def test_constants(ask):
    assert ask(["K"]) == [[str(LDS_BUDGET), str(150 * 1024), str(MAX_LEVELS)]]
    assert ask(["L %d" % LDS_BUDGET, "L %d" % (LDS_BUDGET + 1), "L 0", "L %d" % 2 ** 40]) == [["1"], ["0"], ["1"], ["0"]]
    assert ask(["C %d" % d for d in (0, 254, 255, 256, INT_MAX)]) == [["0"], ["254"], ["255"], ["255"], ["255"]]


def test_walk_rules(ask):
    cases = [(first, step, n) for first in (-1, 0, 5) for step in (-3, -1, 0, 2) for n in (1, 2, 4)]
    cases.append((INT_MAX, INT_MAX, 65535))      # 2^31-1 + 65534 * (2^31-1) is far past int: the sum must be made in 64 bits
    cases.append((INT_MAX, -INT_MAX, 65535))     # ... and far below zero
    got = ask(["P %d %d %d" % c for c in cases])
    for (first, step, n), g in zip(cases, got):
        walk = first < 0 or first + (n - 1) * step < 0      # Python's integers do not wrap
        assert g == [str(int(walk)), str(int(first < 0 or step < 0))], (first, step, n)
    # the two rules differ exactly where a negative step never takes an index below zero
    assert ask(["P 5 -1 4", "P 5 -3 2", "P 5 -3 4", "P 0 -1 1", "P 0 -1 2"]) == [["0", "1"], ["0", "1"], ["1", "1"], ["0", "1"], ["1", "1"]]
    assert got[-2] == ["0", "0"] and got[-1] == ["1", "1"]


def test_empty_bounds(ask):
    nan = float("nan")
    cases = {(0, 640, 0, 480): 0, (-12.7, 655.3, -9.4, 489.9): 0, (5, 5, 0, 480): 1, (0, 640, 7, 7): 1, (640, 0, 0, 480): 1, (0, 640, 480, 0): 1,
             (nan, 640, 0, 480): 1, (0, nan, 0, 480): 1, (0, 640, nan, 480): 1, (0, 640, 0, nan): 1}
    got = ask(["E " + words(b) for b in cases])
    assert [int(g[0]) for g in got] == list(cases.values())


BOUNDS = [(0.0, 640.0, 0.0, 480.0), (-12.7, 655.3, -9.4, 489.9), (-0.5, 639.5, -0.25, 479.75), (-1.5, 0.5, -2.999, 0.999)]


def trunc_bits(x):
    """truncf as bits: toward zero, the sign kept (truncf(-0.5f) is -0.0f)"""
    x = f32(x)
    t = f32(np.trunc(x))
    return bits(np.copysign(t, x))


def test_grid_and_bounds_fills(ask):
    got = ask(["G " + words(b) for b in BOUNDS])
    for b, g in zip(BOUNDS, got):
        w_inv = f32(GRID_COLS) / (f32(b[1]) - f32(b[0]))
        h_inv = f32(GRID_ROWS) / (f32(b[3]) - f32(b[2]))
        assert g == [bits(b[0]), bits(b[2]), bits(w_inv), bits(h_inv), bits(w_inv), bits(h_inv)], b
    assert got[0][2:4] == [bits(0.1), bits(0.1)]      # 64 / 640 and 48 / 480 in float32
    got = ask(["B " + words(b) for b in BOUNDS])
    for b, g in zip(BOUNDS, got):
        assert g[:4] == [bits(v) for v in b], b
        assert g[4:] == [trunc_bits(v) for v in b], b
    assert got[2][4:] == ["80000000", bits(639.0), "80000000", bits(479.0)]      # -0.0f, not +0.0f
    assert got[1][4:] == [bits(-12.0), bits(655.0), bits(-9.0), bits(489.0)]


def test_camera_fills(ask):
    c = (458.654, 457.296, 367.215, 248.375, -0.28340811, 0.07395907, 0.00019359, 1.76187114e-05, 0.5)
    got = ask(["Q " + words(c)])[0]
    assert got[:4] == [bits(v) for v in c[:4]] and got[4:] == [bits(v) for v in c[:8]]


def scale_tables(scale_factor, nlevels):
    """orbx_compute_tables' scale, 1 / scale, scale^2 and 1 / scale^2 (ORBextractor.cc:419-437): the factor is a double that holds the float
    argument, every element is rounded to float32; kMaxLevels long, zero past nlevels as the handle holds them"""
    sf = float(f32(scale_factor))
    scale = np.zeros(MAX_LEVELS, f32); sigma2 = scale.copy(); inv = scale.copy(); inv2 = scale.copy()
    scale[0] = sigma2[0] = 1.0
    for i in range(1, nlevels):
        scale[i] = f32(float(scale[i - 1]) * sf)
        sigma2[i] = scale[i] * scale[i]
    for i in range(nlevels):
        inv[i] = f32(1.0) / scale[i]
        inv2[i] = f32(1.0) / sigma2[i]
    return scale, inv, sigma2, inv2


@pytest.mark.parametrize("nlevels", [1, 8, 16])
def test_level_table_rules(ask, nlevels):
    tables = scale_tables(1.2, nlevels) + scale_tables(2.0, nlevels)[:1]
    lib = X.compute_tables(1000, 1.2, nlevels)      # the restated formula is the library's
    for mine, theirs in zip(tables, ("scale_factors", "inv_scale_factors", "level_sigma2", "inv_level_sigma2")):
        assert mine[:nlevels].tobytes() == lib[theirs].tobytes() and not mine[nlevels:].any()
    for src in tables:
        want = {1: [src[l] if l < nlevels else f32(1.0) for l in range(MAX_LEVELS)],               # stereo
                2: [src[l] if l < nlevels else src[nlevels - 1] for l in range(MAX_LEVELS)],       # the two project_last entries
                3: list(src),                                                                      # triangulation: the handle's table as it is
                4: [src[l] if l < nlevels else f32(0.0) for l in range(MAX_LEVELS)]}               # Fuse, Sim3, frustum: a zeroed block keeps its zeros
        got = ask(["T %d %d %s" % (rule, nlevels, words(src)) for rule in want])
        for rule, g in zip(want, got):
            assert g == [bits(v) for v in want[rule]], (rule, nlevels)
    # rule 3 copies what lies past nlevels too, whatever it is; rule 4 does not look at it
    junk = [f32(100 + l) for l in range(MAX_LEVELS)]
    got = ask(["T 3 %d %s" % (nlevels, words(junk)), "T 4 %d %s" % (nlevels, words(junk))])
    assert got[0] == [bits(v) for v in junk]
    assert got[1] == [bits(junk[l] if l < nlevels else 0.0) for l in range(MAX_LEVELS)]


@pytest.mark.parametrize("nlevels", [1, 2, 8])
def test_fill_breaks(ask, nlevels):
    src = [f32(1.1 * 1.2 ** l) for l in range(MAX_LEVELS)]
    got = ask(["R %d %s" % (nlevels, words(src))])[0]
    assert got == [bits(src[l] if l < nlevels - 1 else 0.0) for l in range(MAX_LEVELS)]
    assert all(g == "00000000" for g in got[max(nlevels - 1, 0):])


def test_regrow(ask):
    sizes = (40, 4096, 8)
    got = ask(["W %d %d %d %d" % ((k,) + sizes) for k in (0, 1, 2, 3)])
    # no failure: three live buffers of the asked sizes, every old buffer freed once
    assert got[0] == ["1", "3", "3", "1", "1", "1"] + [str(s) for s in sizes]
    # the k-th allocation fails: nothing is held, nothing is live, every old buffer was freed exactly once (the sanitizer ends the program
    # on a second free or a leak, which the fixture turns into a failure)
    for k in (1, 2, 3):
        assert got[k] == ["0", "0", "0", "1", "1", "1", "-1", "-1", "-1"], k


def test_the_library_is_built_with_this_header():
    make = open(os.path.join(ROOT, "extractorb_amd", "csrc", "Makefile")).read()
    hdr = [line for line in make.splitlines() if line.startswith("HDR =")][0]
    assert "orbx_entry.hpp" in hdr.split()
    assert '#include "orbx_entry.hpp"' in open(os.path.join(ROOT, "extractorb_amd", "csrc", "orbx_internal.hpp")).read()
