"""The FAST cells' survivor list as raw words and its one pass (k_fast_body.hpp: the NMS trips' entry, pass 3) on crafted cells.

An entry of the list is the kept pixel PAIR's score register with the coordinates in the bytes the scores leave free; the pass over the list
takes the kept pixel as the strictly larger half, counts and emits in one trip at iniThFAST and, where that kept nothing, in a second trip at
minThFAST.  What can go wrong is a matter of single cells, so every cell of these one-level frames is one case:

  positions   kept dots of 30 at x mod 4 = 0, 1, 2, 3 (pair A / pair B, low / high half), the other pixel of the pair scoring 29; a dot of
              255; dots on x = 0, y = 0, the last column and the last row
  weak        the same pairs at 9 | 8 and one at 8 | 7 (S = minThFAST + 1): nothing above iniThFAST, everything comes from the second trip
  n0 ... n128 cells whose list has exactly 0 (dots of 7 only), 1, 63 (all <= iniThFAST: second trip), 64 (all above), 65 (only the LAST
              above iniThFAST) and 128 entries (every other one above): the pass walks the list 64 entries at a time
  segcap      a dot on every even (x, y) of the cell, 21 lower per column away from the middle one: every dot is a corner of S >= 21 and
              there are exactly ceil(cw/2) * ceil(ch/2) of them, the size of the cell's segment

All frames are 0 with dots of the value they are to score: a lone dot's ring is 0, so S = its value.  Dots of one case stand on the pool
(4a, 2b), (4a + 2, 2b + 1) or further apart: no dot on another's ring, no two 8-adjacent but the pairs.  The tent of `segcap` has four dots on
every dot's ring; its scores come from the statement like everything else here.

Frames: 62 x 153 (cells of 31 x 24: 8 items per row, a lane keeps its item column; the last cell 22 wide: 6 items, lanes re-dealt every trip),
62 x 163 (33 x 24: 9 items), 62 x 150 (40 x 24, 32 x 24: the 72 x 69 tile, byte form), 62 x 4200 (two-dword candidates), 77 x 77 (one cell of
39 x 39, the largest of the 48 x 45 tile) and 91 x 91 (one cell of 53 x 53).  The 72 x 69 tile would hold a cell of 63 x 63, but no frame
has one: a level's cells are ceil(W / floor(W / 30)) wide, 59 at most (W = 59: one cell column), and a cell clipped by the rectangle on
both sides evaluates W - 6 = 53 columns; with two columns or more a cell is 45 wide at most.  53 x 53 is the largest cell there is.

CPU: the frames hold every case (from the statement and its score map).  GPU: every frame alone and the frames of a shape as one batch,
candidates in order against the statement and results against the oracle, over poisoned buffers and polluted LDS."""
import functools

import numpy as np
import pytest

import extractorb_amd as X
import fast_cell_scenes as S

INI, MN = 20, 7
CASES = ("positions", "weak", "n0", "n1", "n63", "n64", "n65", "n128", "segcap")
COUNTS = {"n0": 0, "n1": 1, "n63": 63, "n64": 64, "n65": 65, "n128": 128}
WIDTHS = (153, 163, 150)                      # 62-row frames: every case on each
BIG_W = 4200
BIG_CASES = {0: "positions", 1: "weak", 2: "segcap", 4: "n65", 5: "n128", 6: "n0"}      # the first cells of the wide frame (3: empty, beside the tent)
# switch set -> (kernel, blur's lanes carried) for the frames that fit the 48 x 45 tile; the others run k_fast without the blur's lanes
FORMS = {"wide0": ("k_fast", True), "wide0_nofuse": ("k_fast", False)}


def pool(cw, ch):
    return [(x, y) for y in range(ch) for x in range(0 if y % 2 == 0 else 2, cw, 4)]


def _value(case, n, i):
    """score of entry i of a cell of n entries"""
    weak, strong = 8 + (5 * i) % 13, 21 + (37 * i) % 235      # 8 .. 20, 21 .. 255
    if case == "n63":
        return weak
    if case == "n65":
        return 30 if i == n - 1 else weak
    if case == "n128":
        return strong if i % 2 else weak
    return strong


def plant(c, cell, case):
    """the dots of one case in one cell of Canvas c (rectangle coordinates)"""
    xf, yf, cw, ch = cell["x0"] - S.MINB + 3, cell["y0"] - S.MINB + 3, cell["cw"], cell["ch"]
    assert cw >= 22 and ch >= 24, cell
    dot = lambda x, y, v: c.put(xf + x, yf + y, v)
    if case in ("positions", "weak"):
        hi, lo = (30, 29) if case == "positions" else (9, 8)
        for y, kept, other in ((4, 4, 5), (8, 13, 12), (12, 18, 19), (16, 7, 6)):      # kept at x mod 4 = 0, 1, 2, 3
            dot(kept, y, hi); dot(other, y, lo)
        if case == "positions":
            dot(16, 20, 255)
            dot(0, 0, 40); dot(cw - 1, 2, 41); dot(9, ch - 1, 42); dot(cw - 1, ch - 1, 43)
        else:
            dot(10, 20, 8); dot(11, 20, 7)
    elif case == "n0":
        for x, y in pool(cw, ch)[3:40:7]:
            dot(x, y, 7)
    elif case == "segcap":
        mid = ((cw + 1) // 2) // 2
        for y in range(0, ch, 2):
            for a in range((cw + 1) // 2):
                dot(2 * a, y, 230 - 21 * abs(a - mid))
    else:
        n = COUNTS[case]
        for i, (x, y) in enumerate(pool(cw, ch)[:n]):
            dot(x, y, _value(case, n, i))


@functools.lru_cache(maxsize=None)
def scenes():
    """[dict(name, img, cases = {cell index: case})]"""
    out = []
    for w in WIDTHS:
        cells = S.cell_geometry(62, w)["cells"]
        order = list(CASES) + ["weak", "n63", "n65"]      # (12 slots on four cells a frame; three cells a frame at 150: 9 slots)
        for k in range(0, len(CASES), len(cells)):
            c = S.Canvas("raw_62x%d_%d" % (w, k // len(cells)), 62, w, bg=0)
            plan = {i: order[k + i] for i in range(len(cells)) if k + i < len(order)}
            for i, case in plan.items():
                plant(c, cells[i], case)
            out.append(dict(name=c.name, img=c.img, cases=plan))
    c = S.Canvas("raw_big", 62, BIG_W, bg=0)
    cells = S.cell_geometry(62, BIG_W)["cells"]
    plan = dict(BIG_CASES)
    plan.update({len(cells) - 2: "positions", len(cells) - 3: "n65"})      # beyond x = 4096
    for i, case in plan.items():
        plant(c, cells[i], case)
    out.append(dict(name=c.name, img=c.img, cases=plan))
    for side in (77, 91):       # one cell: the largest each tile meets
        c = S.Canvas("raw_%dx%d" % (side, side), side, side, bg=0)
        n = side - 32 - 6
        for x, y, v in ((0, 0, 30), (n - 1, 4, 31), (4, n - 1, 32), (n - 1, n - 1, 33), (0, 20, 25), (20, 0, 26), (21, 9, 9), (20, 9, 8)):
            c.put(3 + x, 3 + y, v)
        out.append(dict(name=c.name, img=c.img, cases={0: "corners"}))
    return out


def cell_view(s):
    """per cell of scene s: dict(case, tile, cw, ch, cap, entries = the minThFAST list [(x, y, S)] in interior coordinates, raster order,
    keys = what the statement returns for the cell [(x, y, response)], th, other = S of the other pixel of each entry's pair)"""
    rows, cols = s["img"].shape
    g = S.cell_geometry(rows, cols)
    smap = S.score_map(s["img"])
    cands, per_cell = S.statement(s["img"], INI, MN)
    assert len(per_cell) == len(g["cells"])
    bounds = [c["first"] for c in per_cell] + [len(cands)]
    out = []
    for i, (cell, pc) in enumerate(zip(g["cells"], per_cell)):
        x0, y0 = cell["x0"], cell["y0"]
        listed = S._fast(smap, x0, y0, x0 + cell["roiW"], y0 + cell["roiH"], MN, None)[0]
        entries = [(x - 3, y - 3, r + 1) for x, y, r in listed]
        keys = [(x - cell["shiftX"] - 3, y - cell["shiftY"] - 3, r) for x, y, r in cands[bounds[i]:bounds[i + 1]]]
        other = [int(smap[y0 + 3 + y, x0 + 3 + (x ^ 1)]) if (x ^ 1) < cell["cw"] else 0 for x, y, _ in entries]
        out.append(dict(case=s["cases"].get(i), tile=g["tile"], cw=cell["cw"], ch=cell["ch"], cap=cell["cap"], nq=cell["nq"], entries=entries,
                        keys=keys, th=pc["th"], other=other))
    return out


def test_the_frames_hold_every_case():
    tiles = ("48x45", "72x69")
    seen = {t: set() for t in tiles}
    margin = {t: set() for t in tiles}            # (x mod 4 of a kept pixel whose pair's other pixel scores exactly one less, final threshold)
    for s in scenes():
        for v in cell_view(s):
            t, case, E = v["tile"], v["case"], v["entries"]
            above = [e for e in E if e[2] > INI]
            kept = {(x, y): r for x, y, r in v["keys"]}
            assert all(0 <= x < v["cw"] and 0 <= y < v["ch"] for x, y in kept)
            assert len(kept) == (len(above) if above else len(E)) and v["th"] == (INI if above else MN)
            for (x, y, sc), o in zip(E, v["other"]):
                if (x, y) in kept and o == sc - 1:
                    margin[t].add((x & 3, v["th"]))
            if case is None:
                continue
            if case in COUNTS:
                assert len(E) == COUNTS[case], (s["name"], case, len(E))
            if case in ("weak", "n63"):              # the second trip
                assert E and not above and v["th"] == MN and len(kept) == len(E)
            if case == "weak":
                assert sorted(kept.values()) == [7, 8, 8, 8, 8]                       # S = minThFAST + 1 among them
            if case == "n65":                        # only the last entry above iniThFAST
                assert above == [E[-1]] and list(kept) == [E[-1][:2]]
            if case == "n64":
                assert len(above) == 64
            if case == "n128":
                assert len(above) == 64 and len(kept) == 64
            if case == "n0":
                assert not E and not kept
            if case == "segcap":
                assert len(kept) == v["cap"] == len(E) > 128 and v["th"] == INI
            if case == "positions":
                assert 254 in kept.values()
                assert {(0, 0), (v["cw"] - 1, 2), (9, v["ch"] - 1), (v["cw"] - 1, v["ch"] - 1)} <= set(kept)
            if case == "corners":
                n = v["cw"]
                assert v["cw"] == v["ch"] == {"48x45": 39, "72x69": 53}[t] and v["nq"] == {"48x45": 10, "72x69": 14}[t]
                assert {(0, 0), (n - 1, 4), (4, n - 1), (n - 1, n - 1), (0, 20), (20, 0)} <= set(kept)
            seen[t].add(case)
    for t in tiles:
        assert seen[t] == set(CASES) | {"corners"}, (t, sorted(set(CASES) - seen[t]))
        assert margin[t] >= {(p, th) for p in range(4) for th in (INI, MN)}, (t, sorted(margin[t]))
    big = next(s for s in scenes() if s["name"] == "raw_big")
    xs = [x for x, _, _ in S.statement(big["img"], INI, MN)[0]]
    assert min(xs) < 64 and max(xs) > 4096
    # the item widths: a lane keeps its item column (8 items) and is re-dealt every trip (6, 7, 9, 10 items)
    assert {c["nq"] for w in WIDTHS for c in S.cell_geometry(62, w)["cells"]} == {6, 7, 8, 9, 10}
    assert [S.cell_geometry(62, w)["tile"] for w in WIDTHS] == ["48x45", "48x45", "72x69"]
    # a small batch keeps the leaf tables, and cells of its frames take the second trip
    for w in WIDTHS:
        assert S.expected_form(62, w, 1, S.SWITCH_SETS["wide0"], B=3)[4] and "off" not in S.leaf_branches(62, w)["k_fast"]
        assert sum(v["case"] in ("weak", "n63") for s in scenes() if s["img"].shape == (62, w) for v in cell_view(s)) >= 2


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
def _device(switches, monkeypatch):
    for k, v in S.SWITCH_SETS[switches].items():
        monkeypatch.setenv(k, v)
    X.debug_set_option("poison", 0xA5)
    X.debug_set_option("lds_pollute", 0xC3)
    return S.Device(X)


def _check_form(dev, ex, shape, switches, B=1):
    kernel, tile, carry, big, leaf = S.expected_form(shape[0], shape[1], 1, S.SWITCH_SETS[switches], B)
    assert kernel == "k_fast" and tile == S.cell_geometry(*shape)["tile"] and big == (shape[1] > 4096)
    assert carry == (FORMS[switches][1] and tile == "48x45" and not big)
    assert dev.fast_kernel(ex) == kernel, (shape, switches, dev.fast_kernel(ex))
    assert (ex.last_forms()[2] == 1) == carry, (shape, switches, ex.last_forms())


@pytest.mark.gpu
@pytest.mark.parametrize("switches", list(FORMS))
def test_gpu_frames_one_by_one(switches, monkeypatch):
    dev = _device(switches, monkeypatch)
    wrong = []
    for s in scenes():
        rows, cols = s["img"].shape
        ex = dev.handle(rows, cols, 1, INI, MN)
        out = ex(s["img"])
        _check_form(dev, ex, (rows, cols), switches)
        try:
            S.check_frame(ex, out, 0, s["img"], 1, INI, MN, "%s %s" % (s["name"], switches))
        except AssertionError as e:
            wrong.append(str(e).splitlines()[0][:200])
    assert not wrong, "%d frames differ:\n%s" % (len(wrong), "\n".join(wrong))


@pytest.mark.gpu
@pytest.mark.parametrize("switches", list(FORMS))
def test_gpu_frames_as_one_batch_per_shape(switches, monkeypatch):
    """small batches carry the leaf tables: a cell whose first trip keeps nothing must leave them as they were"""
    dev = _device(switches, monkeypatch)
    for w in WIDTHS:
        group = [s for s in scenes() if s["img"].shape == (62, w)]
        frames = np.stack([s["img"] for s in group])
        ex = dev.handle(62, w, 1, INI, MN, max_batch=len(group))
        for rep in range(2):
            out = ex.extract_batch(frames)
            _check_form(dev, ex, (62, w), switches, B=len(group))
            for f, s in enumerate(group):
                S.check_frame(ex, out[f], f, frames[f], 1, INI, MN, "%s, frame %d of a batch, call %d, %s" % (s["name"], f, rep, switches))
