"""The FAST cells' score tile and its suppression pass (k_fast_body.hpp: ScoreTile, nmsNeighbourMax, clearScoreApron) on dense noise.

The crafted scenes of tests/fast_cell_scenes.py place their probes far apart; what the suppression pass does with a neighbour in EVERY
direction at EVERY position of a pixel inside its four-pixel item, and with scores just outside the interior on every side of a cell, needs
dense scores.  Frames: frames 0-5 of the noise stream at 62 rows (the smallest frame) and 153 ... 156 columns (every byte misalignment of
the staged ROI, every width of a row's last item), ANDed with 0xF0 so that equal scores are common.  24 frames.

CPU: the frame set reaches every case it exists for (counted from the statement's score map and the mirror of the cell list).
GPU: the frames, one by one and as one batch per width, and the one-column sweep widths 62 ... 77 (the 48 x 45 tile at 6 ... 10 items per row:
the lanes re-dealt every trip), candidates in order against the statement and the whole result against the oracle, over poisoned buffers and
polluted LDS, under the switch sets that select k_fast<48,45> with and without the blur's lanes and k_fast_wide."""
import functools

import numpy as np
import pytest

import extractorb_amd as X
import fast_cell_scenes as S
from extractorb_amd import synth

INI, MN = 20, 7
ROWS, WIDTHS, PER_WIDTH = 62, (153, 154, 155, 156), 6
# switch set -> the kernel it selects for these one-level frames: (kernel, blur's lanes carried)
FORMS = {"wide0": ("k_fast", True), "wide0_nofuse": ("k_fast", False), "default": ("k_fast_wide", True)}
SWEEP_WIDTHS = tuple(range(62, 78))


@functools.lru_cache(maxsize=None)
def frames_of(w):
    return np.stack([synth.frames("noise", f, 1, ROWS, w)[0] & 0xF0 for f in range(PER_WIDTH)])


def all_frames():
    return [(w, f, frames_of(w)[f]) for w in WIDTHS for f in range(PER_WIDTH)]


def reached_cases():
    """the cases of the module docstring that the frame set reaches.  A case counts only where the named neighbour alone decides: every other
    neighbour of the pixel scores less than the pixel."""
    greater, equal, sides = set(), set(), set()
    for w, f, img in all_frames():
        raw = S.score_map(img).astype(np.int32)
        for c in S.cell_geometry(ROWS, w)["cells"]:
            xf, yf, cw, ch = c["x0"] + 3, c["y0"] + 3, c["cw"], c["ch"]
            seen = np.zeros_like(raw)                                        # the scores as the cell's suppression sees them: 0 outside its interior
            seen[yf:yf + ch, xf:xf + cw] = raw[yf:yf + ch, xf:xf + cw]
            for y in range(yf, yf + ch):
                for x in range(xf, xf + cw):
                    s = raw[y, x]
                    if s <= MN:
                        continue
                    col = (x - xf) & 3
                    inside = {d: seen[y + d[1], x + d[0]] for d in S.DIRECTIONS}
                    outside = {d: raw[y + d[1], x + d[0]] for d in S.DIRECTIONS}
                    for d in S.DIRECTIONS:
                        if all(v < s for e, v in inside.items() if e != d):
                            if inside[d] > s:
                                greater.add((col, d))
                            if inside[d] == s:
                                equal.add((col, d))
                        # kept (every neighbour the cell sees is smaller), although the raw score of the neighbour d outside the interior is at least as high
                        out_d = not (xf <= x + d[0] < xf + cw and yf <= y + d[1] < yf + ch)
                        if out_d and outside[d] >= s and all(v < s for v in inside.values()):
                            if x == xf and d[0] == -1:
                                sides.add(("left", d[1]))
                            if x == xf + cw - 1 and d[0] == 1:
                                sides.add(("right", c["last"], d[1]))
                            if y == yf and d[1] == -1:
                                sides.add(("top", col))
                            if y == yf + ch - 1 and d[1] == 1:
                                sides.add(("bottom", col))
    return greater, equal, sides


def test_the_frames_reach_every_direction_at_every_item_column_and_every_cell_side():
    assert [c["last"] for w in WIDTHS for c in S.cell_geometry(ROWS, w)["cells"]] == [3, 3, 3, 2, 3, 3, 3, 3, 3, 3, 3, 4, 3, 3, 3, 1]
    assert all(c["sx64"] == 0 for c in S.cell_geometry(ROWS, 153)["cells"][:3]) and S.cell_geometry(ROWS, 153)["cells"][3]["sx64"] != 0
    assert all(S.cell_geometry(ROWS, w)["tile"] == "48x45" for w in WIDTHS + SWEEP_WIDTHS)
    greater, equal, sides = reached_cases()
    every = {(col, d) for col in range(4) for d in S.DIRECTIONS}
    assert len(every) == 32
    assert greater == every, sorted(every - greater)
    assert equal == every, sorted(every - equal)
    want = {("left", dy) for dy in (-1, 0, 1)} | {("right", last, dy) for last in (1, 2, 3, 4) for dy in (-1, 0, 1)} | \
           {(side, col) for side in ("top", "bottom") for col in range(4)}
    assert sides >= want, sorted(want - sides)


def test_the_sweep_widths_re_deal_the_lanes():
    nq = [S.cell_geometry(62, w)["cells"][0]["nq"] for w in SWEEP_WIDTHS]
    assert set(nq) == {6, 7, 8, 9, 10} and {S.cell_geometry(62, w)["cells"][0]["last"] for w in SWEEP_WIDTHS} == {1, 2, 3, 4}
    assert {64 % n for n in nq} >= {0, 1, 4} and all(len(S.cell_geometry(62, w)["cells"]) == 1 for w in SWEEP_WIDTHS)


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
def _device(switches, monkeypatch):
    for k, v in S.SWITCH_SETS[switches].items():
        monkeypatch.setenv(k, v)
    X.debug_set_option("poison", 0xA5)
    X.debug_set_option("lds_pollute", 0xC3)
    return S.Device(X)


def _check_form(dev, ex, switches):
    kernel, carry = FORMS[switches]
    assert dev.fast_kernel(ex) == kernel, (switches, dev.fast_kernel(ex))
    assert (ex.last_forms()[2] == 1) == carry, (switches, ex.last_forms())


@pytest.mark.gpu
@pytest.mark.parametrize("switches", list(FORMS))
def test_gpu_noise_frames_one_by_one(switches, monkeypatch):
    dev = _device(switches, monkeypatch)
    wrong = []
    for w, f, img in all_frames():
        ex = dev.handle(ROWS, w, 1, INI, MN)
        out = ex(img)
        _check_form(dev, ex, switches)
        assert S.expected_form(ROWS, w, 1, S.SWITCH_SETS[switches])[:3] == (FORMS[switches][0], "48x45", FORMS[switches][1])
        try:
            S.check_frame(ex, out, 0, img, 1, INI, MN, "noise %dx%d frame %d %s" % (ROWS, w, f, switches))
        except AssertionError as e:
            wrong.append(str(e).splitlines()[0][:200])
    assert not wrong, "%d frames differ:\n%s" % (len(wrong), "\n".join(wrong))


@pytest.mark.gpu
@pytest.mark.parametrize("switches", list(FORMS))
def test_gpu_noise_frames_as_one_batch_per_width(switches, monkeypatch):
    dev = _device(switches, monkeypatch)
    for w in WIDTHS:
        frames = frames_of(w)
        ex = dev.handle(ROWS, w, 1, INI, MN, max_batch=PER_WIDTH)
        out = ex.extract_batch(frames)
        assert dev.fast_kernel(ex) == FORMS[switches][0], (switches, dev.fast_kernel(ex))
        for f in range(PER_WIDTH):
            S.check_frame(ex, out[f], f, frames[f], 1, INI, MN, "noise %dx%d frame %d of a batch, %s" % (ROWS, w, f, switches))


@pytest.mark.gpu
@pytest.mark.parametrize("switches", list(FORMS))
def test_gpu_sweep_widths(switches, monkeypatch):
    dev = _device(switches, monkeypatch)
    scenes = {s["name"]: s for s in S.sweep_scenes()}
    for w in SWEEP_WIDTHS:
        s = scenes["sweep_62x%d" % w]
        for ini, mn in s["params"]:
            ex = dev.handle(62, w, s["nlevels"], ini, mn)
            out = ex(s["img"])
            _check_form(dev, ex, switches)
            S.check_frame(ex, out, 0, s["img"], s["nlevels"], ini, mn, "%s %s %s" % (s["name"], (ini, mn), switches))
