"""k_fast<48,45>'s score tile shares its LDS with the pixel tile (orbx_device.hpp: FastAlias).  CPU only.

The layout's constants and its own no-overlap statement (FastAlias::ok, asserted at compile time for every cell) are read from the header by a
small host program.  Independently of that statement, every (cw, ch) the 48 x 45 tile accepts is replayed here byte by byte from the passes'
own address arithmetic (k_fast_body.hpp: fastCell), trip by trip, with the lanes dealt as the kernel deals them:
  * no score row stored in a trip of the score pass touches a pixel byte that a later trip reads;
  * no list entry the NMS pass can have written after a trip (at most ceil(cw / 2) * ceil(rows visited / 2): no two survivors are
    8-adjacent) touches a score byte that a later trip reads;
  * the apron clear behind the score pass touches no stored score, its trim of every row's last item zeroes exactly the pixels past the
    interior (the score pass stores every item whole, without masks), and every byte the NMS pass reads was stored by the score pass or
    by the clear (the apron-only clear leaves nothing unset);
  * the list at its largest ends before the leaf tables, and everything stays inside the wave's region."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "extractorb_amd", "csrc")
TS, ROWS = 48, 45

PROGRAM = r"""
#include <cstdio>
#include "orbx_device.hpp"
int main() {
    using A = orbx::FastAlias<%d, %d>;
    std::printf("%%d %%d %%d %%d %%d %%d %%d %%d\n", A::kScoreStride, A::kScoreItem, A::kPixelOff, A::kWaveBytes, A::kLeafCap, A::kLeafOff, A::kMaxInterior, orbx::kFastTileShift);
    for (int cw = 1; cw <= A::kMaxInterior; cw++)
        for (int ch = 1; ch <= A::kMaxInterior; ch++)
            if (!A::ok(cw, ch)) std::printf("bad %%d %%d\n", cw, ch);
    return 0;
}
""" % (TS, ROWS)


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    d = tmp_path_factory.mktemp("alias")
    src, exe = str(d / "alias.cpp"), str(d / "alias")
    open(src, "w").write(PROGRAM)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), src, "-o", exe])
    lines = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.splitlines()
    assert lines[1:] == [], lines[1:]                                       # FastAlias::ok holds for every cell
    keys = ("stride", "item", "pixel_off", "wave_bytes", "leaf_cap", "leaf_off", "max_interior", "shift")
    return dict(zip(keys, map(int, lines[0].split())))


def deal(nq, ch, wide_perm):
    """the (row, item) of every lane in every trip of a pass, as fastCell deals them: [trip][lane] -> (y, qi) or None once the lane is done"""
    recip = (65536 + nq - 1) // nq                                          # CellDesc::itemRecip
    sy = (64 * recip) >> 16
    sx = 64 - sy * nq
    assert sy == 64 // nq and sx == 64 % nq
    lanes = []
    for lane in range(64):
        y = (lane * recip) >> 16
        qi = lane - y * nq
        assert (y, qi) == divmod(lane, nq)
        if wide_perm and nq == 8:
            y = ((y & 3) << 1) | (y >> 2)
        lanes.append([y, qi])
    trips = (nq * ch + 63) >> 6
    out = []
    for t in range(trips):
        out.append([tuple(l) for l in lanes])
        for l in lanes:
            if sx == 0:
                l[0] += sy
            else:
                l[1] += sx; l[0] += sy
                if l[1] >= nq:
                    l[1] -= nq; l[0] += 1
    return out


def mark(mask, starts, length):
    idx = (np.asarray(starts, np.int64)[:, None] + np.arange(length)[None, :]).ravel()
    assert idx.size == 0 or (idx.min() >= 0 and idx.max() < mask.size), (idx.min(), idx.max())
    mask[idx] = True


def replay(L, cw, ch):
    q0, q1 = (L["shift"] + 3) >> 2, (L["shift"] + 2 + cw) >> 2
    nq = q1 - q0 + 1
    RS, IB, P, W = L["stride"], L["item"], L["pixel_off"], L["wave_bytes"]
    roiH = ch + 6
    assert P + TS * roiH <= W
    # ---- score pass ----
    trips = deal(nq, ch, wide_perm=True)
    reads, writes = [], []
    for lanes in trips:
        act = [(y, qi) for y, qi in lanes if y < ch]
        r, w = np.zeros(W, bool), np.zeros(W, bool)
        for d in range(7):
            mark(r, [P + (y + d) * TS + 4 * (q0 + qi) - 4 for y, qi in act], 12)      # L | C | R of tile row y + d
        mark(w, [(y + 1) * RS + IB * (q0 + qi) for y, qi in act], 8)
        reads.append(r); writes.append(w)
    assert sorted((y, qi) for lanes in trips for y, qi in lanes if y < ch) == [(y, qi) for y in range(ch) for qi in range(nq)]
    later = np.zeros(W, bool)
    for t in range(len(trips) - 1, -1, -1):
        assert not (writes[t] & later).any(), ("score pass", cw, ch, t)
        later |= reads[t]
    stored = np.logical_or.reduce(writes)
    # ---- the apron clear behind it (clearScoreApron<PAIR, TS, 2>) ----
    clear = np.zeros(W, bool)
    RD = RS // 8
    mark(clear, [(0 if t // RD == 0 else ch + t // RD) * RS + 8 * (t % RD) for t in range(3 * RD)], 8)
    mark(clear, [(t + 1) * RS + IB * q0 - 4 for t in range(ch)], 4)
    mark(clear, [(t + 1) * RS + IB * (q1 + 1) for t in range(ch)], 4)
    assert 3 * RD <= 64 and ch <= 64 and not (clear & stored).any(), ("clear", cw, ch)
    # ... which also trims the last item of every row to the interior (TRIM): the score pass stores every item whole
    valid = L["shift"] + 3 + cw - 4 * q1
    assert 1 <= valid <= 4
    trim = np.zeros(W, bool)
    if valid & 1:
        mark(trim, [(t + 1) * RS + IB * q1 + 2 * valid for t in range(ch)], 2)
    if valid <= 2:
        mark(trim, [(t + 1) * RS + IB * q1 + 4 for t in range(ch)], 4)
    outside = np.zeros(W, bool)                                              # the u16 of every stored pixel that lies past the interior
    mark(outside, [(t + 1) * RS + IB * q0 + 2 * x for t in range(ch) for x in range(cw, 4 * nq)], 2)
    assert (trim == outside).all() and not (trim & ~stored).any(), ("trim", cw, ch)
    # ---- NMS pass ----
    trips = deal(nq, ch, wide_perm=False)
    reads, list_end = [], []
    for lanes in trips:
        r = np.zeros(W, bool)
        for k in range(3):
            mark(r, [(min(y, ch) + k) * RS + IB * (q0 + qi) - 4 for y, qi in lanes], 16)      # P | A | B | N of score row y + k
        reads.append(r)
        visited = max(y for y, qi in lanes if y < ch) + 1
        list_end.append(4 * ((cw + 1) // 2) * ((visited + 1) // 2))
        assert not (r & ~(stored | clear)).any(), ("NMS reads a byte nothing has set", cw, ch)
    first_read = W
    for t in range(len(trips) - 1, -1, -1):
        assert list_end[t] <= first_read, ("list", cw, ch, t, list_end[t], first_read)
        first_read = min(first_read, int(np.flatnonzero(reads[t])[0]))
    assert list_end[-1] == 4 * ((cw + 1) // 2) * ((ch + 1) // 2) <= L["leaf_off"] and L["leaf_off"] + 8 * L["leaf_cap"] <= W


def test_the_layout_is_the_one_the_replay_is_about(layout):
    assert (layout["stride"], layout["item"], layout["shift"], layout["max_interior"]) == (2 * TS, 8, 1, ROWS - 6)
    assert layout["wave_bytes"] == layout["pixel_off"] + TS * ROWS == 4176 and layout["pixel_off"] % 16 == 0 and layout["leaf_cap"] == TS * (ROWS - 3) // 8
    assert 16 + 4 * layout["wave_bytes"] + 4 * 2 * 64 == 17232 <= 20480      # the workgroup: eight and more per CU by LDS


def test_no_store_touches_what_a_later_trip_reads(layout):
    for cw in range(1, layout["max_interior"] + 1):
        for ch in range(1, layout["max_interior"] + 1):
            replay(layout, cw, ch)


def test_the_replay_can_fail(layout):
    """the same replay refuses a pixel tile two pixel rows nearer to the score rows, for the largest cell"""
    with pytest.raises(AssertionError, match="score pass"):
        replay(dict(layout, pixel_off=layout["pixel_off"] - 2 * TS), layout["max_interior"], layout["max_interior"])
