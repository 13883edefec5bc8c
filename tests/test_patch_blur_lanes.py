"""k_describe<PB>'s patch blur, dealt so that every tile row's horizontal pass is made by one lane: a numpy model of the two lane tables of
k_describe_body.hpp (c_pbRun: the rows a lane stores, c_pbSrc: the tile rows a lane sums) and of the exchange between lanes (the first three
row pairs of lane l + 1 reach lane l by DPP row_shl:1, inside a row of 16 lanes), replayed on random tiles against a plain separable blur."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RMAX = [11, 15, 17, 18, 18, 18, 18, 16, 13, 6]          # test_tables.py derives these from the pattern
TAPS = np.array([18, 34, 49, 55, 49, 34, 18], dtype=np.int64)
PB_ROWS, PB_STRIDE, BLUR_ROWS, BLUR_STRIDE, PB_LDS = 43, 44, 37, 40, 3384
OWN, HALO = 12, 6                                      # tile rows a lane sums itself / receives from the next lane


def _table(name, digits):
    text = open(os.path.join(ROOT, "extractorb_amd", "csrc", "k_describe_body.hpp")).read()
    body = text[text.index("%s[32] = {" % name):]
    entries = [int(t, 16) for t in re.findall(r"0x[0-9a-fA-F]{%d}\b" % digits, body[:body.index("};")])]
    assert len(entries) == 32
    return entries


def _lanes():
    lanes = []
    for run, src in zip(_table("c_pbRun", 6), _table("c_pbSrc", 8)):
        off_a, off_b, split, k0 = src & 0x7ff, ((src >> 11) & 0xfff) - 1024, (src >> 23) & 15, src >> 27
        assert split % 2 == 0 and split <= OWN, "a row pair has one address"
        reads = [(off_a if i < split else off_b) + PB_STRIDE * i for i in range(OWN)]
        lanes.append(dict(g=run & 0xff, o0=(run >> 8) & 0xff, n=run >> 16, k0=k0, reads=reads))
    return lanes


def test_constants_match_the_header():
    text = open(os.path.join(ROOT, "extractorb_amd", "csrc", "k_describe_body.hpp")).read()
    for name, want in (("kPbStride", PB_STRIDE), ("kBlurStride", BLUR_STRIDE)):
        assert int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1)) == want
    assert "row_shl:1: lane l + 1's" in text          # the carrier of the halo: a DPP shift inside a row of 16 lanes


def test_every_needed_tile_row_has_exactly_one_producing_lane():
    lanes = _lanes()
    made = {}
    for l, ln in enumerate(lanes):
        for off in ln["reads"]:
            assert off >= 0 and off % 4 == 0 and off + 12 <= PB_LDS, "a read stays inside the keypoint's own LDS"
            row, col = divmod(off, PB_STRIDE)
            assert col % 4 == 0 and col // 4 < 10
            made.setdefault((col // 4, row), []).append(l)
    passes = sum(len(v) for v in made.values())
    needed = [(g, row) for g in range(10) for row in range(18 - RMAX[g], 24 + RMAX[g] + 1)]
    assert len(needed) == 370 and passes == 32 * OWN == 384          # (the runs of round 5 took 32 x 18 = 576 passes)
    for item in needed:
        assert len(made.get(item, [])) == 1, item


def test_every_consumed_row_comes_from_the_lane_itself_or_its_neighbour_in_the_same_dpp_row():
    """Lock step: every lane fills its six pairs first, the exchange follows, then the vertical pass - so a halo row is there when it is read
    if the NEXT lane sums it among its first six rows, and that lane lies in the same row of 16 lanes."""
    lanes = _lanes()
    for l, ln in enumerate(lanes):
        assert 1 <= ln["n"] <= OWN and 0 <= ln["k0"] and ln["k0"] + ln["n"] <= OWN
        window = list(ln["reads"])
        if ln["k0"] + ln["n"] + HALO > OWN:                       # the run reads rows of the halo
            assert l % 16 != 15, "the last lane of a DPP row has no lower neighbour"
            assert (l + 1) // 16 == l // 16
            window += lanes[l + 1]["reads"][:HALO]
        for r in range(ln["n"]):                                  # output row o0 + r of group g reads tile rows o0 + r .. o0 + r + 6 of group g
            for t in range(7):
                assert window[ln["k0"] + r + t] == (ln["o0"] + r + t) * PB_STRIDE + 4 * ln["g"], (l, r, t)
                assert ln["o0"] + r + t < PB_ROWS                 # (rows that are not staged reach no stored output)


def _hsums(buf, off):
    """hsums4: pixel j of the group reads bytes j + 1 .. j + 7 of the twelve at off"""
    s = buf[off:off + 12].astype(np.int64)
    return np.array([int((TAPS * s[j + 1:j + 8]).sum()) for j in range(4)], dtype=np.int64)


def _replay(buf):
    """the kernel's schedule on one keypoint's LDS bytes: returns the blurred tile (37 x 40) and which bytes were stored"""
    lanes = _lanes()
    pairs = []
    for ln in lanes:                                              # phase 1: six row pairs per lane, two u16 sums to a register
        p = []
        for k in range(OWN // 2):
            he, ho = _hsums(buf, ln["reads"][2 * k]), _hsums(buf, ln["reads"][2 * k + 1])
            assert he.max() <= 0xffff and ho.max() <= 0xffff
            p.append((ho << 16) | he)
        pairs.append(p)
    out = np.zeros((BLUR_ROWS, BLUR_STRIDE), dtype=np.uint8)
    stored = np.zeros((BLUR_ROWS, BLUR_STRIDE), dtype=bool)
    for l, ln in enumerate(lanes):                                # phase 2: row_shl:1 (0 where the row of 16 lanes ends), phase 3: the vertical pass
        halo = pairs[l + 1][:HALO // 2] if l % 16 != 15 else [np.zeros(4, dtype=np.int64)] * (HALO // 2)
        w = pairs[l] + list(halo)
        for k in range(ln["k0"], ln["k0"] + ln["n"]):
            t = k // 2
            lo = [w[t + i] & 0xffff for i in range(4)]
            hi = [w[t + i] >> 16 for i in range(4)]
            if k % 2 == 0:
                acc = 32768 + 18 * lo[0] + 34 * hi[0] + 49 * lo[1] + 55 * hi[1] + 49 * lo[2] + 34 * hi[2] + 18 * lo[3]
            else:
                acc = 32768 + 18 * hi[0] + 34 * lo[1] + 49 * hi[1] + 55 * lo[2] + 49 * hi[2] + 34 * lo[3] + 18 * hi[3]
            assert acc.max() < 1 << 32
            row = ln["o0"] + k - ln["k0"]
            cols = slice(4 * ln["g"], 4 * ln["g"] + 4)
            assert not stored[row, cols].any()
            out[row, cols] = np.minimum(acc >> 16, 255)
            stored[row, cols] = True
    return out, stored


def _plain(tile):
    """separable 7-tap blur: blurred row o, byte c <- tile rows o .. o + 6, tile bytes c + 1 .. c + 7"""
    t = tile.astype(np.int64)
    h = sum(TAPS[k] * t[:, 1 + k:1 + k + BLUR_STRIDE - 3] for k in range(7))      # tile bytes 1 .. 43 feed blurred bytes 0 .. 36
    v = sum(TAPS[k] * h[k:k + BLUR_ROWS] for k in range(7))
    return np.minimum((v + 32768) >> 16, 255).astype(np.uint8)


def test_replayed_schedule_equals_a_plain_separable_blur_on_the_disc():
    rng = np.random.default_rng(7)
    disc = np.zeros((BLUR_ROWS, BLUR_STRIDE), dtype=bool)
    for g in range(10):
        disc[18 - RMAX[g]:18 + RMAX[g] + 1, 4 * g:4 * g + 4] = True
    tiles = [rng.integers(0, 256, (PB_ROWS, PB_STRIDE), dtype=np.uint8) for _ in range(6)]
    tiles.append(np.full((PB_ROWS, PB_STRIDE), 255, dtype=np.uint8))                  # row sums of 65535, outputs that saturate at 257
    tiles.append((rng.integers(0, 2, (PB_ROWS, PB_STRIDE)) * 255).astype(np.uint8))
    for tile in tiles:
        buf = rng.integers(0, 256, PB_LDS, dtype=np.uint8)                            # whatever lies behind the tile
        buf[:PB_ROWS * PB_STRIDE] = tile.reshape(-1)
        out, stored = _replay(buf)
        assert np.array_equal(stored, disc)                                            # exactly the rows of c_pbRun, each once
        want = _plain(tile)
        assert want.shape == (BLUR_ROWS, BLUR_STRIDE - 3)
        assert np.array_equal(out[:, :37][disc[:, :37]], want[disc[:, :37]])
