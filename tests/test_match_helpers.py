"""extractorb_amd/csrc/k_match_helpers.hpp is the only statement of four lines of the reference that every matcher kernel uses: ComputeThreeMaxima
(ORBmatcher.cc:2303-2344), the rotation-histogram bin (:773-783), GetFeaturesInArea's cell window (Frame.cc:666-688) and the sorted best-key
list; k_keyframe_project.hpp on top of it is the only statement of KeyFrame::GetFeaturesInArea's visit (KeyFrame.cc:794-811) with the clamps
that keep a corrupt grid inside its frame.  Here they are called directly: tests/cpp/match_helpers_check.cpp is the header compiled for the host behind tests/cpp/host_shim (as a
sanitized stand-alone program), and every answer is compared with an independent statement below - sorting for the maxima and the list, exact
rational rounding for the bin, float32 steps spelled out for the window.  No GPU."""
import math
import os
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
HISTO_LENGTH, GRID_COLS, GRID_ROWS = 30, 64, 48
EMPTY = 0x7FFFFFFF


def hexf(x):
    return "%08x" % struct.unpack("<I", struct.pack("<f", float(f32(x))))[0]


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("match_helpers") / "match_helpers_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "tests", "cpp", "host_shim"), "-I" + os.path.join(ROOT, "extractorb_amd", "csrc"),
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "match_helpers_check.cpp"), "-o", exe])

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return [[int(t) for t in line.split()] for line in out]
    return run


# ---- ComputeThreeMaxima ------------------------------------------------------------------------------------------------------------------
def three_maxima(hist):
    """the three fullest non-empty bins, a lower bin before a higher one of the same size; the second and third go if below a tenth of the first"""
    order = [i for i in sorted(range(len(hist)), key=lambda i: (-hist[i], i)) if hist[i] > 0][:3]
    ind = order + [-1] * (3 - len(order))
    size = [hist[i] if i >= 0 else 0 for i in ind]
    tenth = f32(0.1) * f32(size[0])
    if f32(size[1]) < tenth:
        ind[1] = ind[2] = -1
    elif f32(size[2]) < tenth:
        ind[2] = -1
    return ind


def histogram(**bins):
    h = [0] * HISTO_LENGTH
    for k, v in bins.items():
        h[int(k[1:])] = v
    return h


MAXIMA_CASES = {
    "all zero": histogram(),
    "single bin": histogram(b17=9),
    "single bin 0": histogram(b0=1),
    "single last bin": histogram(b29=4),
    "all equal": [7] * HISTO_LENGTH,                                  # strict '>': bins 0, 1, 2
    "two equal then larger": histogram(b3=5, b9=5, b20=6),            # 20 first, then 3 before 9
    "equal second and third": histogram(b2=40, b11=8, b25=8),
    "three equal and a fourth": histogram(b4=6, b5=6, b6=6, b7=6),
    "descending run": list(range(HISTO_LENGTH, 0, -1)),
    "ascending run": list(range(1, HISTO_LENGTH + 1)),                # every bin shifts the ranks
    "second exactly a tenth": histogram(b1=30, b8=3, b9=3),           # 0.1f * 30 rounds to 3.0f: 3 < 3 is false, both stay
    "second just below a tenth": histogram(b1=30, b8=2, b9=2),        # both go
    "second just above a tenth": histogram(b1=30, b8=4, b9=2),        # the second stays, the third goes
    "third exactly a tenth": histogram(b1=50, b8=20, b9=5),
    "third just below a tenth": histogram(b1=50, b8=20, b9=4),
    "third just above a tenth": histogram(b1=50, b8=20, b9=6),
    "a tenth that float32 rounds": histogram(b0=1000003, b1=100000, b2=100001),      # 0.1f * 1000003.0f = 100000.3 in float32
    "a tenth of seven": histogram(b5=7, b6=1),                        # 0.1f * 7 = 0.70000005: 1 stays
    "a tenth of ten": histogram(b5=10, b6=1, b7=0),                   # 0.1f * 10 rounds to 1.0f: 1 stays
    "a tenth of eleven": histogram(b5=11, b6=1),                      # 1.1: 1 goes
}


def test_three_maxima_statement_on_worked_examples():
    assert three_maxima(MAXIMA_CASES["all zero"]) == [-1, -1, -1]
    assert three_maxima(MAXIMA_CASES["all equal"]) == [0, 1, 2]
    assert three_maxima(MAXIMA_CASES["two equal then larger"]) == [20, 3, 9]
    assert three_maxima(MAXIMA_CASES["second exactly a tenth"]) == [1, 8, 9]
    assert three_maxima(MAXIMA_CASES["second just below a tenth"]) == [1, -1, -1]
    assert three_maxima(MAXIMA_CASES["second just above a tenth"]) == [1, 8, -1]
    assert three_maxima(MAXIMA_CASES["a tenth of eleven"]) == [5, -1, -1]


def test_compute_three_maxima(ask):
    rng = np.random.default_rng(11)
    cases = list(MAXIMA_CASES.values())
    cases += [rng.integers(0, 4, HISTO_LENGTH).tolist() for _ in range(40)]                     # many ties
    cases += [(rng.integers(0, 200, HISTO_LENGTH) * (rng.random(HISTO_LENGTH) < 0.3)).tolist() for _ in range(40)]      # sparse
    got = ask(["M " + " ".join(map(str, h)) for h in cases])
    for h, g in zip(cases, got):
        assert g == three_maxima(h), h


# ---- the rotation bin ----------------------------------------------------------------------------------------------------------------------
def rotation_bin(a1, a2):
    rot = f32(a1) - f32(a2)
    if rot < 0:
        rot = rot + f32(360.0)
    x = Fraction(float(rot * (f32(1.0) / f32(HISTO_LENGTH))))       # the float32 product, exactly
    b = int(math.floor(abs(x) + Fraction(1, 2))) * (1 if x >= 0 else -1)      # roundf: halves away from zero
    return 0 if b == HISTO_LENGTH else b


def test_rotation_bin(ask):
    below = float(np.nextafter(f32(360.0), f32(0.0)))
    pairs = [(0.0, 0.0), (123.5, 123.5), (359.9, 359.9),                                      # a difference of exactly 0
             (below, 0.0), (359.99, 0.0), (354.9, 0.0), (345.0, 0.0),                          # just below 360: round(rot / 30) = 12, the last bin angles in [0, 360) reach
             (0.0, below), (0.0, 1e-3), (10.0, 200.0), (1.0, 359.0), (0.0, 360.0),             # negative differences: + 360 once
             (15.0, 0.0), (45.0, 0.0), (75.0, 0.0), (105.0, 0.0), (0.0, 345.0), (0.0, 315.0),  # .5 ties of roundf
             (885.0, 0.0), (899.0, 0.0), (900.0, 0.0), (914.0, 0.0), (540.0, -360.0),          # 29.5 <= rot / 30 < 30.5: bin 30 wraps to 0 (angles outside [0, 360))
             (884.0, 0.0), (916.0, 0.0), (-400.0, 0.0)]                                        # ... and its neighbours, which the helper leaves alone
    for t in range(1, 13):      # around every tie, one float32 step each side
        tie = f32(30.0 * t - 15.0)
        pairs += [(float(np.nextafter(tie, f32(0))), 0.0), (float(np.nextafter(tie, f32(1e9))), 0.0)]
    rng = np.random.default_rng(5)
    pairs += [tuple(rng.uniform(0, 360, 2)) for _ in range(200)]
    got = ask(["B %s %s" % (hexf(a), hexf(b)) for a, b in pairs])
    for (a, b), g in zip(pairs, got):
        assert g == [rotation_bin(a, b)], (a, b)
    assert rotation_bin(0.0, 0.0) == 0 and rotation_bin(below, 0.0) == 12 and rotation_bin(15.0, 0.0) == 1 and rotation_bin(900.0, 0.0) == 0
    assert rotation_bin(884.0, 0.0) == 29 and rotation_bin(916.0, 0.0) == 31 and rotation_bin(0.0, 345.0) == 1


# ---- GetFeaturesInArea's cell window -------------------------------------------------------------------------------------------------------
def cell_window(u, v, r, min_x, min_y, w_inv, h_inv):
    u, v, r, min_x, min_y, w_inv, h_inv = map(f32, (u, v, r, min_x, min_y, w_inv, h_inv))
    lo_x = max(0, int(math.floor(((u - min_x) - r) * w_inv)))
    hi_x = min(GRID_COLS - 1, int(math.ceil(((u - min_x) + r) * w_inv)))
    lo_y = max(0, int(math.floor(((v - min_y) - r) * h_inv)))
    hi_y = min(GRID_ROWS - 1, int(math.ceil(((v - min_y) + r) * h_inv)))
    inside = not (lo_x >= GRID_COLS or hi_x < 0 or lo_y >= GRID_ROWS or hi_y < 0 or lo_x > hi_x or lo_y > hi_y)
    return [int(inside), lo_x, hi_x, lo_y, hi_y]


def test_cell_window(ask):
    # two frames: cells of exactly 8 x 8 px from the origin (every product exact), and undistorted bounds of a 640 x 480 image
    exact = (0.0, 0.0, 0.125, 0.125)
    b = (f32(-13.7), f32(-9.2), f32(661.4), f32(494.6))
    real = (b[0], b[1], f32(GRID_COLS) / (b[2] - b[0]), f32(GRID_ROWS) / (b[3] - b[1]))
    cases = []
    for fr, (w, h) in ((exact, (512.0, 384.0)), (real, (675.1, 503.8))):
        x0, y0 = float(fr[0]), float(fr[1])
        cases += [(x0 - 50, y0 + 100, 10, *fr), (x0 + w + 50, y0 + 100, 10, *fr), (x0 + 100, y0 - 50, 10, *fr), (x0 + 100, y0 + h + 50, 10, *fr),   # left, right, above, below
                  (x0 - 10, y0 + 100, 10, *fr), (x0 + w + 10, y0 + 100, 10, *fr), (x0 + 100, y0 - 10, 10, *fr), (x0 + 100, y0 + h + 10, 10, *fr),   # touching the grid from outside
                  (x0 - 5, y0 - 5, 10, *fr), (x0 + w + 5, y0 + h + 5, 10, *fr),                                                                  # overlapping a corner
                  (x0 + 88, y0 + 168, 8, *fr), (x0 + 80, y0 + 160, 16, *fr), (x0 + 96, y0 + 96, 0, *fr),                                         # exactly on cell edges (exact frame)
                  (x0 + 504, y0 + 376, 8, *fr), (x0 + 8, y0 + 8, 8, *fr), (x0, y0, 0, *fr), (x0 + w, y0 + h, 0, *fr),
                  (x0 + 300, y0 + 200, 2000, *fr), (x0 - 900, y0 + 200, 2000, *fr), (x0 + 300, y0 + 200, 1e6, *fr),                              # a radius larger than the image
                  (x0 + 300, y0 + 200, -3, *fr), (x0 + 300, y0 + 200, -300, *fr)]                                                                # a negative radius: empty
    rng = np.random.default_rng(9)
    for _ in range(200):
        fr = exact if rng.random() < 0.5 else real
        cases.append((rng.uniform(-100, 800), rng.uniform(-100, 600), rng.choice([0.5, 3, 7.2, 15, 40, 120]), *fr))
    got = ask(["W " + " ".join(hexf(x) for x in c) for c in cases])
    for c, g in zip(cases, got):
        assert g == cell_window(*c), c
    assert cell_window(88, 168, 8, *exact) == [1, 10, 12, 20, 22]        # (88 - 8) / 8 = 10 and (88 + 8) / 8 = 12 exactly: floor and ceil keep them
    assert cell_window(-50, 100, 10, *exact)[0] == 0 and cell_window(562, 100, 10, *exact)[0] == 0
    assert cell_window(300, 200, 2000, *exact) == [1, 0, GRID_COLS - 1, 0, GRID_ROWS - 1]
    assert {tuple(g[:1]) for g in got} == {(0,), (1,)}


# ---- the sorted key list -------------------------------------------------------------------------------------------------------------------
def top_keys(n, keys):
    return (sorted(keys) + [EMPTY] * n)[:n]


def test_sorted_insert(ask):
    key = lambda dist, slot: (dist << 16) | slot      # noqa: E731
    cases = []
    for n in (2, 4):
        cases += [(n, []), (n, [key(40, 7)]),
                  (n, [key(33, s) for s in range(10, 20)]),                                   # equal distances, ascending slots: the first n stay, in order
                  (n, [key(50, 3), key(33, 10), key(33, 11), key(20, 90), key(33, 12), key(33, 13), key(20, 91)]),
                  (n, [key(d, 100 - d) for d in range(60, 0, -1)]),                           # every key displaces the whole list
                  (n, [key(d, d) for d in range(1, 60)]),                                     # only the first n enter
                  (n, [key(256, 0xFFFF), key(0, 0), key(255, 0xFFFE)])]
    rng = np.random.default_rng(2)
    for _ in range(60):
        n = int(rng.choice([2, 4]))
        slots = rng.permutation(500)[:int(rng.integers(0, 30))]
        cases.append((n, [key(int(rng.integers(0, 6)) * 10, int(s)) for s in np.sort(slots)]))      # few distinct distances, slots ascending as in a scan
    got = ask(["I %d %d %s" % (n, len(k), " ".join(map(str, k))) for n, k in cases])
    for (n, k), g in zip(cases, got):
        assert g == top_keys(n, k), (n, k)
    assert top_keys(2, [key(33, s) for s in range(10, 20)]) == [key(33, 10), key(33, 11)]


# ---- DescriptorDistance --------------------------------------------------------------------------------------------------------------------
def test_hamming_256(ask):
    rng = np.random.default_rng(4)
    pairs = [(np.zeros(8, np.uint32), np.zeros(8, np.uint32)), (np.zeros(8, np.uint32), np.full(8, 0xFFFFFFFF, np.uint32))]
    pairs += [(np.uint32(1) << np.arange(8, dtype=np.uint32) * 4, np.zeros(8, np.uint32))]      # one bit in every word
    pairs += [(rng.integers(0, 2 ** 32, 8, dtype=np.uint64).astype(np.uint32), rng.integers(0, 2 ** 32, 8, dtype=np.uint64).astype(np.uint32)) for _ in range(50)]
    got = ask(["H " + " ".join("%x" % int(w) for w in np.concatenate([a, b])) for a, b in pairs])
    for (a, b), g in zip(pairs, got):
        assert g == [sum(bin(int(x) ^ int(y)).count("1") for x, y in zip(a, b))]
    assert got[1] == [256] and got[2] == [8]


# ---- KeyFrame::GetFeaturesInArea's visit ---------------------------------------------------------------------------------------------------
GRID_CELLS = GRID_COLS * GRID_ROWS
CELL_PX = 10.0      # this test's own frame: 640 x 480 px from the origin in cells of 10 x 10 px


class Grid:
    """A hand-made keyframe: keypoints (x, y, octave) pushed into the cell they lie in, in list order, as KeyFrame's constructor does, and the
    tables the kernels read of it - the cells' CSR offsets (cell = ix * GRID_ROWS + iy) and the slot -> keypoint table - with room for
    `capacity` keypoints and not one entry more."""

    def __init__(self, kps, capacity):
        self.kps, self.capacity, self.n_out = list(kps), capacity, len(kps)
        self.cells = [[] for _ in range(GRID_CELLS)]
        for i, (x, y, _) in enumerate(self.kps):
            self.cells[int(x // CELL_PX) * GRID_ROWS + int(y // CELL_PX)].append(i)
        self.off, self.gi = [0], []
        for c in self.cells:
            self.gi += c
            self.off.append(len(self.gi))
        self.gi += [0] * (capacity - len(self.gi))

    def features_in_area(self, u, v, r, win):
        """KeyFrame.cc:794-811 on the cells themselves: ix outer, iy inner, push order inside a cell, both coordinates strictly inside r"""
        out = []
        for ix in range(win[0], win[1] + 1):
            for iy in range(win[2], win[3] + 1):
                for i in self.cells[ix * GRID_ROWS + iy]:
                    if abs(f32(self.kps[i][0]) - f32(u)) < f32(r) and abs(f32(self.kps[i][1]) - f32(v)) < f32(r):
                        out.append(i)
        return out


def visit_by_brute_force(g, u, v, r, win):
    """What the visit may read of tables that need not be a grid at all: only slots below nIn (the grid's total, cut to the frame's count, cut to
    the capacity), for every column those between its two offsets AS THEY STAND (a decreasing pair holds none), every index pulled into the frame."""
    n = max(0, min(g.n_out, g.capacity))
    n_in = max(0, min(g.off[GRID_CELLS], n))
    seen = []
    for ix in range(win[0], win[1] + 1):
        if win[2] > win[3]:
            break
        for s in range(n_in):
            if g.off[ix * GRID_ROWS + win[2]] <= s < g.off[ix * GRID_ROWS + win[3] + 1]:
                i = min(max(g.gi[s], 0), g.capacity - 1)
                x, y = (g.kps[i][:2] if i < len(g.kps) else (0.0, 0.0))
                if abs(f32(x) - f32(u)) < f32(r) and abs(f32(y) - f32(v)) < f32(r):
                    seen += [s, i]
    return [int(bool(seen)), n_in, len(seen) // 2] + seen


VISIT_KEYPOINTS = [(205.0, 33.0, 0), (57.5, 71.0, 1), (228.0, 38.0, 2), (52.0, 78.0, 0), (100.0, 100.0, 3), (108.0, 100.0, 1),      # 5: exactly r = 8 right of 4
                   (107.5, 92.5, 0), (100.0, 92.0, 2), (201.0, 36.0, 1), (224.0, 31.0, 0), (635.0, 475.0, 4), (3.0, 2.0, 0)]       # 7: exactly r above 4
WHOLE = (0, GRID_COLS - 1, 0, GRID_ROWS - 1)


def visit_line(g, u, v, r, win, frames=2, f=1):
    """frame f of `frames` is g; the others are empty keyframes whose tables say so"""
    n_out, off, gi, kps = [], [], [], []
    for k in range(frames):
        n_out.append(g.n_out if k == f else 0)
        off += g.off if k == f else [0] * (GRID_CELLS + 1)
        gi += g.gi if k == f else [0] * g.capacity
        mine = g.kps + [(0.0, 0.0, 0)] * (g.capacity - len(g.kps))
        kps += mine if k == f else [(0.0, 0.0, 0)] * g.capacity
    assert len(gi) == frames * g.capacity and len(off) == frames * (GRID_CELLS + 1)
    return "V %d %d %d %s %s %s %s %s %s %s 0 %d %d %d %d" % (frames, f, g.capacity, " ".join(map(str, n_out)), " ".join(map(str, off)), " ".join(map(str, gi)),
                                                              " ".join("%s %s %d" % (hexf(x), hexf(y), o) for x, y, o in kps), hexf(u), hexf(v), hexf(r), *win)


def test_keyframe_visit(ask):
    cap = len(VISIT_KEYPOINTS)
    good = Grid(VISIT_KEYPOINTS, cap)
    cases = {}
    cases["one cell"] = (good, 55.0, 75.0, 30.0, (5, 5, 7, 7))
    cases["one empty cell"] = (good, 305.0, 205.0, 30.0, (30, 30, 20, 20))
    cases["all cells"] = (good, 320.0, 240.0, 1000.0, WHOLE)
    cases["all cells, small radius"] = (good, 104.0, 96.0, 6.0, WHOLE)
    cases["minCY above maxCY"] = (good, 55.0, 75.0, 30.0, (5, 5, 9, 6))
    cases["minCX above maxCX"] = (good, 55.0, 75.0, 30.0, (6, 5, 7, 7))
    cases["empty column between two full"] = (good, 215.0, 35.0, 30.0, (20, 22, 3, 3))
    cases["exactly r away"] = (good, 100.0, 100.0, 8.0, (9, 11, 8, 11))
    cases["one float above r"] = (good, 100.0, 100.0, float(np.nextafter(f32(8.0), f32(9.0))), (9, 11, 8, 11))
    corrupt = {}
    for name, n_out in (("nOut above capacity", cap + 5), ("nOut below 0", -3), ("nOut below the grid's total", 8)):
        g = Grid(VISIT_KEYPOINTS, cap)
        g.n_out = n_out
        corrupt[name] = (g, 320.0, 240.0, 1000.0, WHOLE)
    g = Grid(VISIT_KEYPOINTS[:8], 8)                     # the offsets speak of 20 slots, the tables have 8
    g.off = [o + 12 * (c > 600) for c, o in enumerate(g.off)]
    corrupt["total above N"] = (g, 320.0, 240.0, 1000.0, WHOLE)
    g = Grid(VISIT_KEYPOINTS, cap)
    g.off = [o + 100000 for o in g.off]
    corrupt["every offset far above N"] = (g, 320.0, 240.0, 1000.0, WHOLE)
    g = Grid(VISIT_KEYPOINTS, cap)
    g.off = [-o for o in g.off]
    g.off[GRID_CELLS] = cap
    corrupt["negative offsets"] = (g, 320.0, 240.0, 1000.0, WHOLE)
    g = Grid(VISIT_KEYPOINTS, cap)
    g.off = [cap - o for o in g.off[:GRID_CELLS]] + [cap]      # decreasing throughout: only a window turned round finds a range (slots 9 .. 10) in it
    corrupt["minCY above maxCY, offsets decreasing"] = (g, 320.0, 240.0, 1000.0, (5, 5, 9, 6))
    g = Grid(VISIT_KEYPOINTS, cap)
    g.off[20 * GRID_ROWS + 3],g.off[20 * GRID_ROWS + 4] = g.off[20 * GRID_ROWS + 4], g.off[20 * GRID_ROWS + 3]      # column 20's cell: 2 slots, backwards
    corrupt["decreasing pair"] = (g, 215.0, 35.0, 30.0, (20, 22, 3, 3))
    for name, bad in (("gi of -1", -1), ("gi of capacity", cap), ("gi far outside", 1 << 30)):
        g = Grid(VISIT_KEYPOINTS, cap)
        g.gi[g.off[10 * GRID_ROWS + 10]] = bad           # the slot of keypoint 4
        corrupt[name] = (g, 320.0, 240.0, 1000.0, WHOLE)
    got = ask([visit_line(*c) for c in list(cases.values()) + list(corrupt.values())])
    for (name, c), out in zip(list(cases.items()) + list(corrupt.items()), got):
        assert out == visit_by_brute_force(*c), name
    # on a grid that is one, the brute force is GetFeaturesInArea itself
    for name, (g, u, v, r, win) in cases.items():
        want = g.features_in_area(u, v, r, win)
        assert visit_by_brute_force(g, u, v, r, win)[4::2] == want and visit_by_brute_force(g, u, v, r, win)[0] == int(bool(want)), name
    answer = dict(zip(list(cases) + list(corrupt), got))
    assert answer["one cell"][3:] == [good.off[5 * GRID_ROWS + 7], 1, good.off[5 * GRID_ROWS + 7] + 1, 3]
    assert answer["one empty cell"] == [0, cap, 0] and answer["minCY above maxCY"] == [0, cap, 0] and answer["minCX above maxCX"] == [0, cap, 0]
    assert answer["all cells"][4::2] == [11, 1, 3, 6, 7, 4, 5, 0, 8, 2, 9, 10]                   # column by column, rows inside (6, 7 lie above 4, 5), push order in a cell
    assert answer["empty column between two full"][4::2] == [0, 8, 2, 9]
    assert answer["exactly r away"][4::2] == [6, 4] and answer["one float above r"][4::2] == [6, 7, 4, 5]      # 5 and 7 are exactly 8 px from (100, 100)
    assert answer["nOut above capacity"] == answer["all cells"] and answer["nOut below 0"] == [0, 0, 0]
    assert answer["nOut below the grid's total"][1:3] == [8, 8] and answer["total above N"][1:3] == [8, 8]
    assert answer["every offset far above N"] == [0, cap, 0] and answer["decreasing pair"][4::2] == [2, 9]
    assert answer["minCY above maxCY, offsets decreasing"] == [0, cap, 0]
    assert answer["gi of -1"][4::2].count(0) == 2 and 4 not in answer["gi of -1"][4::2]
    assert answer["gi of capacity"][4::2].count(cap - 1) == 2 and answer["gi far outside"] == answer["gi of capacity"]
    # a second copy of the same keyframe in frame 0 of one: the frame index only moves the pointers
    assert ask([visit_line(*cases["all cells"], frames=1, f=0)])[0] == answer["all cells"]
