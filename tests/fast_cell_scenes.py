"""Crafted scenes for the FAST cells (extractorb_amd/csrc/k_fast.hip, k_fast_body.hpp), an independent statement of what a level's cells
return, a mirror of the cell list of makeFrameGeom with what the kernels derive per cell, and device helpers.
tests/test_fast_cell_edges.py runs them; docs/history/r29_fast_cell_edges.md has the tables.

The statement is written from the reference's lines (ORBextractor.cc:777-864) and the definition of FAST-9/16 with cornerScore and a strict
3x3 non-maximum suppression, in numpy and Python integers:

  S(p)       the largest c for which 9 contiguous ring pixels (wrapping 15 -> 0) are all >= v + c, or all <= v - c; 0 if there is none
  corner(t)  S(p) > t;  cornerScore = S(p) - 1 (the largest threshold at which p is still a corner) = the key's response
  cv::FAST   on a w x h ROI evaluates x in [3, w - 3), y in [3, h - 3), nothing if w < 7 or h < 7; the score buffer holds cornerScore at
             corners and 0 elsewhere; a corner is kept if its score is greater than all eight neighbours'; raster order

Coordinates: a probe is given in RECTANGLE coordinates (image - 16, the coordinates of vToDistributeKeys)."""
import numpy as np

EDGE = 19                      # EDGE_THRESHOLD (:72)
MINB = EDGE - 3                # minBorderX / minBorderY (:781-782)
BG = 100
RING = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3))
NEIGHBOURS_8 = tuple((dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy)
NEIGHBOURS_4 = ((0, -1), (-1, 0), (1, 0), (0, 1))

ARC_MUTANTS = ("arc_8", "arc_10", "arc_no_wrap", "bright_only", "dark_only", "score_over_all_arcs_min")      # these change S itself
MUTANTS = ("fast_ge",) + ARC_MUTANTS + ("nms_ge", "nms_4", "nms_across_cells", "no_retry", "retry_before_nms", "retry_per_level", "response_is_score",
                           "interior_from_2", "interior_to_max_minus_2", "cell_floor", "cell_w_35", "order_level_raster", "order_column_major",
                           "nms_sees_sub_threshold", "skip_x_minus3")
# oracle/orb_oracle.cpp `enum Mutation` numbers of the mutations the oracle also carries
ORACLE_MUTATION = {"fast_ge": 5, "nms_ge": 6, "nms_across_cells": 7, "no_retry": 8, "skip_x_minus3": 9, "cell_w_35": 14}

_score_cache = {}


def score_map(img, variant=None):
    """S of every pixel whose ring lies inside img (0 elsewhere)"""
    key = (img.shape, hash(img.tobytes()), variant)
    if key in _score_cache:
        return _score_cache[key]
    a = img.astype(np.int16)
    H, W = a.shape
    S = np.zeros((H, W), np.int16)
    if H >= 7 and W >= 7:
        v = a[3:H - 3, 3:W - 3]
        d = np.stack([a[3 + dy:H - 3 + dy, 3 + dx:W - 3 + dx] - v for dx, dy in RING])      # ring pixel k minus the centre
        n = {"arc_8": 8, "arc_10": 10}.get(variant, 9)
        starts = range(16 - n + 1) if variant == "arc_no_wrap" else range(16)
        over_arcs = np.minimum if variant == "score_over_all_arcs_min" else np.maximum
        best = np.zeros_like(v)
        for sign in (+1, -1):             # +1: the arc is brighter than the centre, -1: darker
            if (variant == "bright_only" and sign < 0) or (variant == "dark_only" and sign > 0):
                continue
            pol = None
            for k in starts:
                arc = (sign * d[[(k + j) % 16 for j in range(n)]]).min(axis=0)
                pol = arc if pol is None else over_arcs(pol, arc)
            best = np.maximum(best, pol)
        S[3:H - 3, 3:W - 3] = best
    if len(_score_cache) > 400:
        _score_cache.clear()
    _score_cache[key] = S
    return S


def _fast(S, x0, y0, x1, y1, t, mutant):
    """cv::FAST(img(y0:y1, x0:x1), keys, t, true) given the level's S: [(x, y, cornerScore)] in ROI coordinates, raster order; and whether any
    evaluated pixel was a corner before the suppression"""
    w, h = x1 - x0, y1 - y0
    if w < 7 or h < 7:
        return [], False
    lo = 2 if mutant == "interior_from_2" else 3
    hi = 2 if mutant == "interior_to_max_minus_2" else 3
    s = S[y0 + lo:y1 - hi, x0 + lo:x1 - hi].astype(np.int32)
    corner = s >= t if mutant == "fast_ge" else s > t
    buf = np.zeros((h + 2, w + 2), np.int32)                                                  # the ROI with a one-pixel frame of zeros
    inner = buf[1 + lo:1 + h - hi, 1 + lo:1 + w - hi]
    inner[...] = np.maximum(s - 1, 0) if mutant == "nms_sees_sub_threshold" else np.where(corner, s - 1, 0)
    keep = corner.copy()
    for dx, dy in (NEIGHBOURS_4 if mutant == "nms_4" else NEIGHBOURS_8):
        other = buf[1 + lo + dy:1 + h - hi + dy, 1 + lo + dx:1 + w - hi + dx]
        keep &= (inner >= other) if mutant == "nms_ge" else (inner > other)
    ys, xs = np.nonzero(keep)
    return [(int(x) + lo, int(y) + lo, int(inner[y, x])) for y, x in zip(ys, xs)], bool(corner.any())


def statement(level_image, ini, mn, mutant=None):
    """The candidates of one level in the reference's order [(x, y, response)] (rectangle coordinates), and per cell in the order visited
    dict(i, j, count, th, first): th = the threshold of the call that gave the cell's keys (the last one made, if it has none), first = the
    index of its first key in the list"""
    assert mutant is None or mutant in MUTANTS, mutant
    img = np.asarray(level_image)
    S = score_map(img, mutant if mutant in ARC_MUTANTS else None)
    rows, cols = img.shape
    minBX = minBY = MINB
    maxBX, maxBY = cols - EDGE + 3, rows - EDGE + 3                                            # :783-784
    width, height = maxBX - minBX, maxBY - minBY
    W = 35 if mutant == "cell_w_35" else 30                                                    # :777
    nCols, nRows = width // W, height // W                                                     # :792-793
    if nCols < 1 or nRows < 1:
        return [], []
    wCell, hCell = (width // nCols, height // nRows) if mutant == "cell_floor" else (-(-width // nCols), -(-height // nRows))      # :794-795
    grid = []
    for i in range(nRows):
        iniY = minBY + i * hCell
        maxY = iniY + hCell + 6
        if iniY >= maxBY - 3:
            continue
        maxY = min(maxY, maxBY)
        for j in range(nCols):
            iniX = minBX + j * wCell
            maxX = iniX + wCell + 6
            if iniX >= maxBX - (3 if mutant == "skip_x_minus3" else 6):
                continue
            maxX = min(maxX, maxBX)
            grid.append((i, j, iniX, iniY, maxX, maxY))
    if mutant == "order_column_major":
        grid.sort(key=lambda c: (c[1], c[0]))
    whole = {}
    if mutant == "nms_across_cells":      # one call over the rectangle per threshold; a cell takes the keys inside its own evaluated pixels
        whole = {t: _fast(S, minBX, minBY, maxBX, maxBY, t, mutant)[0] for t in (ini, mn)}

    def call(c, t):
        i, j, x0, y0, x1, y1 = c
        if mutant == "nms_across_cells":
            if x1 - x0 < 7 or y1 - y0 < 7:
                return [], False
            ax, ay = x0 - minBX, y0 - minBY
            keys = [(x - ax, y - ay, s) for x, y, s in whole[t] if ax + 3 <= x < ax + (x1 - x0) - 3 and ay + 3 <= y < ay + (y1 - y0) - 3]
            return keys, bool(keys)
        return _fast(S, x0, y0, x1, y1, t, mutant)

    first = [call(c, ini) for c in grid]
    level_empty = not any(keys for keys, _ in first)
    out, cells = [], []
    for c, (keys, any_corner) in zip(grid, first):
        th = ini
        retry = not keys                                                                       # :835
        if mutant == "no_retry" or (mutant == "retry_before_nms" and any_corner) or (mutant == "retry_per_level" and not level_empty):
            retry = False
        if retry:
            keys, th = call(c, mn)[0], mn
        i, j = c[0], c[1]
        cells.append(dict(i=i, j=j, count=len(keys), th=th, first=len(out)))
        bonus = 1 if mutant == "response_is_score" else 0
        out += [(x + j * wCell, y + i * hCell, s + bonus) for x, y, s in keys]                 # :857-858
    if mutant == "order_level_raster":
        out.sort(key=lambda k: (k[1], k[0]))
    return out, cells


def as_tuples(keypoints):
    """an array of the oracle's or the library's candidates as the statement's tuples; the constant fields are checked here"""
    k = np.asarray(keypoints)
    assert (k["size"] == 7).all() and (k["angle"] == -1).all() and (k["octave"] == 0).all() and (k["class_id"] == -1).all()
    return [(int(x), int(y), int(r)) for x, y, r in zip(k["x"], k["y"], k["response"])]


def kept_map(cands, cells):
    """(x, y) -> (response, threshold of its cell)"""
    out = {}
    bounds = [c["first"] for c in cells] + [len(cands)]
    for c, a, b in zip(cells, bounds, bounds[1:]):
        for x, y, r in cands[a:b]:
            assert (x, y) not in out
            out[(x, y)] = (r, c["th"])
    return out


# ---------------------------------------------------- the library's cell list, mirrored ----------------------------------------------------
K_PAD_L, TILE_SHIFT = 32, 1      # orbx_device.hpp: kPadL, kFastTileShift


def cell_geometry(rows, cols):
    """makeFrameGeom's cells of a level of rows x cols (orbx_geometry.hpp) with what k_fast / k_fast_wide derive for each: cw, ch (evaluated
    columns and rows), nq (dword items per row), gsh (byte misalignment of the staged ROI), last (valid bytes of a row's last dword),
    sx64 / sx256 (64 % nq, 256 % nq: 0 = a lane keeps its item column), items.  None: the geometry is refused."""
    rectW, rectH = cols - EDGE + 3 - MINB, rows - EDGE + 3 - MINB
    nCols, nRows = rectW // 30, rectH // 30
    if nCols < 1 or nRows < 1:
        return None
    wCell, hCell = -(-rectW // nCols), -(-rectH // nRows)
    if wCell > 63 or hCell > 63:
        return None
    out = []
    for i in range(nRows):
        y0 = MINB + i * hCell
        if y0 >= rectH + MINB - 3:
            continue
        y1 = min(y0 + hCell + 6, rectH + MINB)
        for j in range(nCols):
            x0 = MINB + j * wCell
            if x0 >= rectW + MINB - 6:
                continue
            x1 = min(x0 + wCell + 6, rectW + MINB)
            if x1 - x0 < 7 or y1 - y0 < 7:
                continue
            cw, ch = x1 - x0 - 6, y1 - y0 - 6
            q0, q1 = (TILE_SHIFT + 3) >> 2, (TILE_SHIFT + 2 + cw) >> 2
            nq = q1 - q0 + 1
            out.append(dict(i=i, j=j, x0=x0, y0=y0, roiW=x1 - x0, roiH=y1 - y0, cw=cw, ch=ch, nq=nq, gsh=(K_PAD_L + x0 - 1) & 3,
                            first=TILE_SHIFT + 3 - 4 * q0, last=min(4, TILE_SHIFT + 3 + cw - 4 * q1), sx64=64 % nq, sx256=256 % nq, items=nq * ch,
                            shiftX=j * wCell, shiftY=i * hCell, cap=((cw + 1) // 2) * ((ch + 1) // 2)))
    return dict(rectW=rectW, rectH=rectH, nCols=nCols, nRows=nRows, wCell=wCell, hCell=hCell, cells=out,
                tile="48x45" if max(c["roiW"] for c in out) <= 45 and max(c["roiH"] for c in out) <= 45 else "72x69")


def _axis_path(v, b0, b1):      # orbx_device.hpp: octAxisPath (DivideNode's decisions along one axis, ORBextractor.cc:488-489, :520)
    path = 0
    for _ in range(5):
        c = b0 + ((b1 - b0 + 1) >> 1)
        bit = 0 if v < c else 1
        path = 2 * path + bit
        if bit:
            b0 = c
        else:
            b1 = c
    return path


def leaf_branches(rows, cols):
    """which branch of nLeafLocal every cell of a rows x cols level takes in each kernel (k_fast_body.hpp, k_fast.hip): "lds" (the leaf cells
    the cell touches fit the kernel's LDS table), "l2" (key by key) or "off" (the level has more than 7 roots: no leaf tables).
    -> {"k_fast": set, "k_fast_wide": set}"""
    f32 = np.float32
    g = cell_geometry(rows, cols)
    nIni = int(np.floor(f32(g["rectW"]) / f32(g["rectH"]) + f32(0.5)))
    if nIni > 7:
        return {"k_fast": {"off"}, "k_fast_wide": {"off"}}
    hX = f32(g["rectW"]) / f32(nIni)
    def xcode(x):
        r = min(int(f32(x) / hX), nIni - 1)
        return (r << 5) | _axis_path(x, int(hX * f32(r)), int(hX * f32(r + 1)))
    caps = {"k_fast": (48 * 42 if g["tile"] == "48x45" else 72 * 66) // 8, "k_fast_wide": 48 * 45 // 8}
    out = {"k_fast": set(), "k_fast_wide": set()}
    for c in g["cells"]:
        nxl = xcode(min(c["shiftX"] + 3 + c["cw"] - 1, g["rectW"] - 1)) - xcode(c["shiftX"] + 3) + 1
        nyl = _axis_path(min(c["shiftY"] + 3 + c["ch"] - 1, g["rectH"] - 1), 0, g["rectH"]) - _axis_path(c["shiftY"] + 3, 0, g["rectH"]) + 1
        for k, cap in caps.items():
            out[k].add("lds" if nxl * nyl <= cap else "l2")
    if g["tile"] != "48x45":
        out["k_fast_wide"] = set()
    return out


# ------------------------------------------------------------------ scenes ------------------------------------------------------------------
class Canvas:
    """a flat frame with planted probes; expect() records what the scene's own text says about a probe under a parameter set"""

    def __init__(self, name, rows, cols, params=((20, 7),), bg=BG, nlevels=1, what=""):
        self.name, self.params, self.nlevels, self.what = name, tuple(params), nlevels, what
        self.img = np.full((rows, cols), bg, np.uint8)
        self.probes = []

    def put(self, rx, ry, value):
        y, x = ry + MINB, rx + MINB
        assert 0 <= y < self.img.shape[0] and 0 <= x < self.img.shape[1] and 0 <= value <= 255, (self.name, rx, ry, value)
        self.img[y, x] = value

    def dot(self, rx, ry, c, **expect):
        """one pixel c above (below) its surroundings: all sixteen ring pixels differ by |c|, S = |c|"""
        self.put(rx, ry, int(self.img[ry + MINB, rx + MINB]) + c)
        if expect:
            self.expect(rx, ry, **expect)

    def arc(self, rx, ry, start, contrasts, **expect):
        """ring pixels start, start + 1, ... of (rx, ry) differ from the centre by contrasts[i]"""
        v = int(self.img[ry + MINB, rx + MINB])
        for i, c in enumerate(contrasts):
            dx, dy = RING[(start + i) % 16]
            self.put(rx + dx, ry + dy, v + c)
        if expect:
            self.expect(rx, ry, **expect)

    def expect(self, rx, ry, kept, resp=None, th=None, params=None, why=""):
        for p in (self.params if params is None else params):
            self.probes.append(dict(x=rx, y=ry, params=tuple(p), kept=kept, resp=resp, th=th, why=why))

    def scene(self, **more):
        return dict(name=self.name, img=self.img, params=self.params, nlevels=self.nlevels, probes=self.probes, what=self.what, **more)


def threshold_steps():
    """63 x 152: four cells of 30 (the last clipped to 24 evaluated columns), dots of contrast 7, 8, ..., 22 of both signs.
    Cell 0: 8 ... 20 and two 7s - everything above 7 comes back from the retry.  Cell 1: one 21 among 8s and 20s - the 21 alone.
    Cell 2: only 7s - nothing.  Cell 3: -21 and 22 among weaker ones.  With the thresholds 7 / 20 (ini < min) the first call keeps
    everything above 7."""
    c = Canvas("threshold_steps", 63, 152, params=((20, 7), (7, 20)), what=threshold_steps.__doc__)
    plan = {0: [8, -8, 20, -20, 9, -15, 7, -7, 12, -19, 16, -10], 1: [20, 21, 8, -8, -20, 8, -8, 7],      # (a 20 in front of the 21: a kernel that emits
            2: [7, -7, 7, -7, 7, -7], 3: [20, -21, 22, -8]}                                                  # S >= 20 beside a count of S > 20 shows it first)
    for j, contrasts in plan.items():
        slots = [(30 * j + x, y) for y in (5, 13, 21) for x in ((5, 13, 21, 29) if j < 3 else (5, 13, 21))]
        has_ini = any(abs(k) > 20 for k in contrasts)
        for (x, y), k in zip(slots, contrasts):
            c.dot(x, y, k)
            s = abs(k)
            if has_ini:
                c.expect(x, y, kept=s > 20, resp=s - 1, th=20, params=[(20, 7)])
            else:
                c.expect(x, y, kept=s > 7, resp=s - 1, th=7, params=[(20, 7)])
            c.expect(x, y, kept=s > 7, resp=s - 1, th=7, params=[(7, 20)])
    return c.scene(counts={(20, 7): [10, 1, 0, 2], (7, 20): [10, 7, 0, 4]})


def arc_positions():
    """122 x 182 (5 x 3 cells of 30): for each of the 16 arc starts and both polarities a 9-arc of contrast 30 (a corner, response 29) and an
    8-arc (none); graded arcs 21 ... 29 in three orders (S = 21); longer arcs whose S is that of their best 9-sub-arc.  The probes stand 9
    apart in x and y: every x mod 4, odd and even rows."""
    c = Canvas("arc_positions", 122, 182, what=arc_positions.__doc__)
    slots = [(6 + 9 * a, 7 + 9 * b) for b in range(9) for a in range(16)]
    at = iter(slots)
    for pol in (1, -1):
        for start in range(16):
            x, y = next(at); c.arc(x, y, start, [30 * pol] * 9, kept=True, resp=29, th=20, why="9-arc at %d" % start)
            x, y = next(at); c.arc(x, y, start, [30 * pol] * 8, kept=False, why="8-arc at %d" % start)
    graded = (list(range(21, 30)), list(range(29, 20, -1)), [25, 29, 21, 27, 23, 28, 22, 26, 24])
    longer = (([21] + [30] * 9, 30), ([25, 24] + [30] * 9 + [23], 30), ([30] * 5 + [21] + [30] * 10, 30), ([21] + [30] * 7 + [22] + [30] * 7, 22),
              ([30] * 5 + [22] + [30] * 5, 22), ([40] * 16, 40), ([30, 21] * 8, 21))
    for pol in (1, -1):
        for n, g in enumerate(graded):
            x, y = next(at); c.arc(x, y, (3, 12, 15)[n], [k * pol for k in g], kept=True, resp=20, th=20, why="graded")
        for n, (arc, s) in enumerate(longer):
            x, y = next(at); c.arc(x, y, (0, 11, 5, 14, 9, 0, 3)[n], [k * pol for k in arc], kept=True, resp=s - 1, th=20, why="%d-arc" % len(arc))
    xs, ys = [s[0] for s in slots[:84]], [s[1] for s in slots[:84]]
    assert {x % 4 for x in xs} == {0, 1, 2, 3} and {y % 2 for y in ys} == {0, 1}
    return c.scene()


def extremes():
    """62 x 92 (two cells): the left half 0 with one pixel of 255, the right half 255 with one pixel of 0 (S = 255, response 254), and weak
    dots (10, 15 on the black half, 12 on the white one).  Thresholds 20 / 7; 254 / 253, under which only the two extremes are corners;
    20 / 20; and 7 / 20 (ini < min), where the first call already returns the weak dots."""
    c = Canvas("extremes", 62, 92, params=((20, 7), (254, 253), (20, 20), (7, 20)), what=extremes.__doc__)
    c.img[:, :MINB + 30] = 0
    c.img[:, MINB + 30:] = 255
    c.dot(15, 12, 255); c.dot(45, 14, -255)
    weak = ((8, 20, 10), (22, 22, 15), (50, 6, -12))
    for x, y, k in weak:
        c.dot(x, y, k)
    for p in c.params:
        c.expect(15, 12, kept=True, resp=254, th=p[0], params=[p]); c.expect(45, 14, kept=True, resp=254, th=p[0], params=[p])
        for x, y, k in weak:
            c.expect(x, y, kept=p == (7, 20), resp=abs(k) - 1, th=7, params=[p])
    return c.scene()


DIRECTIONS = NEIGHBOURS_8


def nms_ties():
    """92 x 152 (4 x 2 cells of 30): equal dots adjacent in each of the 8 directions (both go), 30 beside 25 in each direction (the 30 stays),
    equal dots 2 apart (both stay), the chains 25 < 30 > 27 along x and y, a 2 x 2 plateau (all go); then pairs astride the cell boundaries
    x = 32 | 33, 62 | 63, 92 | 93 and y = 32 | 33 - equal, unequal, diagonal - and a 2 x 2 plateau on the corner of four cells: all stay."""
    c = Canvas("nms_ties", 92, 152, what=nms_ties.__doc__)
    slots = iter([(30 * j + dx, y) for y in (10, 22, 40, 50) for j in range(4) for dx in (10, 22)])
    for dx, dy in DIRECTIONS:
        x, y = next(slots)
        c.dot(x, y, 30, kept=False, why="equal pair"); c.dot(x + dx, y + dy, 30, kept=False, why="equal pair")
    for dx, dy in DIRECTIONS:
        x, y = next(slots)
        c.dot(x, y, 30, kept=True, resp=29, th=20, why="greater"); c.dot(x + dx, y + dy, 25, kept=False, why="lesser")
    for dx, dy in ((2, 0), (2, 2)):
        x, y = next(slots)
        c.dot(x - 1, y - 1, 30, kept=True, resp=29, th=20); c.dot(x - 1 + dx, y - 1 + dy, 30, kept=True, resp=29, th=20)
    for dx, dy in ((1, 0), (0, 1)):
        x, y = next(slots)
        c.dot(x - dx, y - dy, 25, kept=False); c.dot(x, y, 30, kept=True, resp=29, th=20); c.dot(x + dx, y + dy, 27, kept=False)
    x, y = next(slots)
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        c.dot(x + dx, y + dy, 30, kept=False, why="plateau")
    stay = dict(kept=True, th=20)
    c.dot(32, 16, 30, resp=29, **stay); c.dot(33, 16, 30, resp=29, **stay)             # equal, astride x
    c.dot(62, 16, 25, resp=24, **stay); c.dot(63, 16, 30, resp=29, **stay)             # unequal
    c.dot(92, 16, 30, resp=29, **stay); c.dot(93, 17, 30, resp=29, **stay)             # diagonal
    c.dot(16, 32, 30, resp=29, **stay); c.dot(16, 33, 30, resp=29, **stay)             # equal, astride y
    c.dot(46, 32, 25, resp=24, **stay); c.dot(46, 33, 30, resp=29, **stay)
    c.dot(76, 32, 30, resp=29, **stay); c.dot(77, 33, 30, resp=29, **stay)
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        c.dot(92 + dx, 32 + dy, 30, resp=29, why="plateau on four cells", **stay)
    return c.scene()


def plateau_forces_retry():
    """62 x 92 (two cells).  Cell 0: two equal adjacent dots of 30 (above iniThFAST, both suppressed) and one dot of 10: the first call
    returns nothing, the retry the weak dot alone (response 9).  Cell 1: the same and a dot of 25, which the first call returns alone."""
    c = Canvas("plateau_forces_retry", 62, 92, what=plateau_forces_retry.__doc__)
    c.dot(10, 10, 30, kept=False); c.dot(11, 10, 30, kept=False); c.dot(20, 18, 10, kept=True, resp=9, th=7)
    c.dot(40, 10, 30, kept=False); c.dot(41, 10, 30, kept=False); c.dot(50, 18, 10, kept=False); c.dot(45, 22, 25, kept=True, resp=24, th=20)
    return c.scene(counts={(20, 7): [1, 1]})


CELL_EDGE_SHAPES = [(62, w) for w in (62, 63, 64, 65, 67, 68, 69, 70, 153, 154, 155, 156)] + [(93, w) for w in (63, 69, 154, 156)]


def cell_edges(rows, cols):
    """a dot of 30 on the first and last evaluated column and row of every cell (kept, response 29); dots 1 px outside the evaluated pixels
    and 1 px outside the rectangle on each of the four sides (never kept)"""
    c = Canvas("cell_edges_%dx%d" % (rows, cols), rows, cols, what=cell_edges.__doc__)
    g = cell_geometry(rows, cols)
    yes = dict(kept=True, resp=29, th=20)
    for k in g["cells"]:
        xf, yf = k["x0"] - MINB + 3, k["y0"] - MINB + 3
        xl, yl = xf + k["cw"] - 1, yf + k["ch"] - 1
        assert k["cw"] >= 22 and k["ch"] >= 24
        c.dot(xf, yf + 6, 30, **yes); c.dot(xl, yf + 13, 30, **yes); c.dot(xf + 6, yf, 30, **yes); c.dot(xf + 13, yl, 30, **yes)
    W, H = g["rectW"], g["rectH"]
    for x, y in ((2, 23), (W - 3, 23), (23, 2), (23, H - 3), (-1, 13), (W, 13), (13, -1), (13, H)):
        c.dot(x, y, 30, kept=False, why="outside")
    return c.scene(outside=8)


def lattice(name, rows, cols, graded=False, nlevels=1, contrast=30, what="", skew=False):
    """dots on the lattice spanned by (5, 0) and (0, 2) - skew: (5, 0) and (2, 3), whose dots stand on odd and even rows alike -: no dot lies
    on another's ring or beside it, so every evaluated dot is kept"""
    c = Canvas(name, rows, cols, nlevels=nlevels, what=what or lattice.__doc__)
    for b in range(0, rows // (3 if skew else 2) + 1):
        for a in range(-rows, cols // 5 + 1):
            x, y = (5 * a + 2 * b, 3 * b) if skew else (5 * a, 2 * b)
            if 0 <= x < cols and 0 <= y < rows:
                c.img[y, x] = BG + (12 + 4 * ((a + 3 * b) % 5) if graded else contrast)
    return c.scene()


def skipped_cells():
    """63 x 813: 26 cell columns of 31, the last of which the reference skips (iniX = 791 >= maxBorderX - 6).  Dots on the columns 776 ... 780
    of the rectangle: 776 and 777 are the last evaluated columns of cell column 24, nobody evaluates 778 ... 780."""
    c = Canvas("skipped_cells", 63, 813, what=skipped_cells.__doc__)
    for n, x in enumerate((776, 777, 778, 779, 780)):
        c.dot(x, 5 + 4 * n, 30, kept=x <= 777, resp=29, th=20)
    for x in (3, 40, 400, 747, 760):
        c.dot(x, 14, 30, kept=True, resp=29, th=20)
    return c.scene()


def big():
    """62 x 4200: one level beyond 4096 px (two-dword candidates), 135 evaluated cell columns of 31, the last 8 columns wide.  Dots at both ends
    and on either side of x = 4095 of the rectangle; one cell of weak dots only (the retry)."""
    c = Canvas("big", 62, 4200, what=big.__doc__)
    for n, x in enumerate((3, 4, 40, 2000, 4090, 4095, 4096, 4097, 4100, 4157, 4164)):
        c.dot(x, 4 + 4 * (n % 5), 30 + n, kept=True, resp=29 + n, th=20)
    c.dot(2, 20, 30, kept=False); c.dot(4165, 22, 30, kept=False)
    c.dot(1000, 10, 9, kept=True, resp=8, th=7); c.dot(1008, 12, -8, kept=True, resp=7, th=7); c.dot(1012, 20, 7, kept=False)
    return c.scene()


def crafted_scenes():
    out = [threshold_steps(), arc_positions(), extremes(), nms_ties(), plateau_forces_retry()]
    out += [cell_edges(r, w) for r, w in CELL_EDGE_SHAPES]
    out += [lattice("dense_63x84", 63, 84), lattice("dense_63x152", 63, 152), lattice("dense_graded_63x84", 63, 84, graded=True),
            lattice("dense_graded_63x152", 63, 152, graded=True), lattice("dense_104x104", 104, 104), lattice("dense_106x108", 106, 108, skew=True), lattice("dense_skew_63x84", 63, 84, skew=True),
            lattice("dense_skew_graded_63x152", 63, 152, graded=True, skew=True), lattice("dense_graded_110x110", 110, 110, graded=True),
            skipped_cells(), big(), lattice("levels_3", 90, 120, nlevels=3, contrast=90)]
    return out


SWEEP_SHAPES = [(62, w) for w in range(62, 92)] + [(h, 62) for h in (70, 77, 78, 91)] + [(80, 68), (91, 91)]


def sweep_scenes():
    """the graded lattice on every one-column frame width 62 ... 91 (ROIs 30 ... 59 px wide: every width either tile holds for one cell), some
    heights up to 91 and the 8-item cell under the large tile (80 x 68).  Statement, oracle and device only: no mutant runs over these."""
    return [lattice("sweep_%dx%d" % (r, w), r, w, graded=True) for r, w in SWEEP_SHAPES]


def flat(rows, cols):
    return Canvas("flat_%dx%d" % (rows, cols), rows, cols).scene()


def corners_outside_only(rows, cols):
    """the outside dots of cell_edges alone: corners in the image, none where a cell evaluates"""
    c = Canvas("outside_only_%dx%d" % (rows, cols), rows, cols)
    g = cell_geometry(rows, cols)
    W, H = g["rectW"], g["rectH"]
    for x, y in ((2, 23), (W - 3, 23), (23, 2), (23, H - 3), (-1, 13), (W, 13), (13, -1), (13, H), (-10, -10), (W + 8, H + 8)):
        c.dot(x, y, 60, kept=False)
    return c.scene()


# ------------------------------------------------------------ oracle and device ------------------------------------------------------------
NF = 500
_oracle_cache = {}


def oracle(img, nlevels, ini, mn, mutation=0):
    """dict(result = (mono, keypoints, descriptors), levels = the level images, candidates, level_keys) of the oracle; computed once"""
    import oracle_lib as O
    key = (img.shape, hash(img.tobytes()), nlevels, ini, mn, mutation)
    if key not in _oracle_cache:
        o = O.Oracle(NF, 1.2, nlevels, ini, mn)
        o.set_mutation(mutation)
        res = o.extract(img)
        _oracle_cache[key] = dict(result=res, levels=[o.level(l) for l in range(nlevels)], candidates=[o.candidates(l) for l in range(nlevels)],
                                  level_keys=[o.level_keypoints(l).copy() for l in range(nlevels)])
    return _oracle_cache[key]


SWITCH_SETS = {
    "default": {},
    "wide0": {"ORBX_FAST_WIDE": "0"},
    "wide1": {"ORBX_FAST_WIDE": "1"},
    "leaf0": {"ORBX_LEAF_FRAMES": "0"},
    "nofuse": {"ORBX_FUSE_SMALL": "0"},
    "wide0_nofuse": {"ORBX_FAST_WIDE": "0", "ORBX_FUSE_SMALL": "0"},
    "wide0_leaf0": {"ORBX_FAST_WIDE": "0", "ORBX_LEAF_FRAMES": "0"},
}


def plan_line(rows, cols, nlevels, switches, B=1, max_batch=1):
    """the case line of tests/cpp/batch_plan_check.cpp for a whole extraction of B frames under a switch set"""
    e = lambda k, d: int(switches.get(k, d))
    tok = dict(rows=rows, cols=cols, nf=NF, nlevels=nlevels, sf=1.2, maxB=max_batch, numCUs=256, fastWide=e("ORBX_FAST_WIDE", -1),
               fuseSmall=e("ORBX_FUSE_SMALL", 1), leafFrames=max(0, min(e("ORBX_LEAF_FRAMES", 128), max_batch)), B=B, stages=3)
    return " ".join("%s=%s" % kv for kv in tok.items())


def expected_form(rows, cols, nlevels, switches, B=1):
    """what the launch policy gives these small calls (orbx_batch_plan.hpp: planBack, blurRidesWithFast), stated from the mirror for one level:
    (kernel, tile, blur carried, big build, leaf tables)"""
    g = cell_geometry(rows, cols)
    is_big = max(rows, cols) > 4096
    fits = g["tile"] == "48x45"
    wide_switch = int(switches.get("ORBX_FAST_WIDE", -1))
    wide = not is_big and (wide_switch > 0 or (wide_switch < 0 and len(g["cells"]) * B <= 4 * 256))
    carry = int(switches.get("ORBX_FUSE_SMALL", 1)) != 0 and fits and not is_big
    leaf = int(switches.get("ORBX_LEAF_FRAMES", 128)) > 0 and not is_big
    return ("k_fast_wide" if wide and fits else "k_fast", g["tile"], carry, is_big, leaf)


class Device:
    """handles by (shape, levels, thresholds, batch) for one switch set: the environment is read when a handle is created"""

    def __init__(self, X):
        self.X, self.handles = X, {}

    def handle(self, rows, cols, nlevels, ini, mn, max_batch=1):
        key = (rows, cols, nlevels, ini, mn, max_batch)
        if key not in self.handles:
            self.handles[key] = self.X.ORBextractor(NF, 1.2, nlevels, ini, mn, max_width=cols, max_height=rows, max_batch=max_batch)
        return self.handles[key]

    def fast_kernel(self, ex):
        return ex._L.orbx_profile_kernel_name_of(ex._h, 3).decode()      # profile slot 3: FAST (include/orbx.h)


def check_frame(ex, out, frame, img, nlevels, ini, mn, what):
    """frame `frame` of the last call: the candidates of every level IN ORDER against the statement on the oracle's level images, then the
    whole result and the per-level keypoints against the oracle"""
    from helpers import assert_same_result
    want = oracle(img, nlevels, ini, mn)
    for l in range(nlevels):
        cands, _ = statement(want["levels"][l], ini, mn)
        got = as_tuples(ex.debug_candidates(l, frame))
        assert got == cands, "%s level %d: candidates differ from the statement (%d vs %d); first at %s" % (
            what, l, len(got), len(cands), next((i for i, (a, b) in enumerate(zip(got, cands)) if a != b), min(len(got), len(cands))))
    assert_same_result(out[:3], want["result"], what)
    assert [len(a) for a in out[3]] == [len(a) for a in want["level_keys"]], what
    assert all(a.tobytes() == b.tobytes() for a, b in zip(out[3], want["level_keys"])), "%s: per-level keypoints" % what
