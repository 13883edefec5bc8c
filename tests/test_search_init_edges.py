"""ORBmatcher::SearchForInitialization (reference src/ORBmatcher.cc:706-821) where k_search_init (extractorb_amd/csrc/k_match.hip) differs most from
the reference's loop: crafted scenes with many requests on one keypoint, long steal / second-choice chains, histogram ties and stolen votes, keypoints on
cell edges and requests outside the image, and the limit of the on-chip tables.  Keypoints, descriptors and grids are built in numpy (O.frame_finish) and
uploaded directly; the extractor is not used.

CPU: the oracle against the walk of tests/search_init_statement.py on every scene, the REACH of every scene asserted from the walk's exit codes and
counters, and the walk against synchronous_rounds (the kernel header's "parallel fixed point = sequential result", apart from the kernel).
GPU: orbx_search_for_initialization_device against the oracle, bit-exact (vnMatches12, vbPrevMatched bytes, nmatches).

A scene is a function of a seed and returns a dict: k1, d1, k2, d2 (raw keypoints and descriptors of the two frames), prev (vbPrevMatched, default: the
undistorted positions of frame 1), window, nnratio, check, cam.  window, nnratio, check and the image bounds are arguments of the CALL, not of a pair:
the GPU tests put all scenes that share them into one launch, one pair per scene."""
import functools
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import extractorb_amd as X
import search_init_statement as S
from test_search_init import PINHOLE, EUROC, random_frame, make_descriptor_pair

COLS, ROWS = 640, 480
SEED = 9
POISON = np.float32(-777.25)
SENTINEL = -99
ROOM = 160 * 1024 - 1024          # LDS bytes k_search_init's tables are sized for (initMatchSlotCapacity)
FIXED_LDS = (64 + 2 + 30 + 8) * 4 + 2 * 16 * 4 + 64      # colStart, hist, flags, the compaction counts, alignment slack
SLOT_BYTES = 32 + 8 + 2 + 2 + 4 + 4 * 2 + 2 + 4 + 4      # descriptor, position, cell, index, holder count, two holders | request index, two decisions


def slot_capacity(capacity):
    """initMatchSlotCapacity (k_match.hip), re-derived: level-0 keypoints of EITHER frame the tables hold"""
    fit = (ROOM - FIXED_LDS) // SLOT_BYTES
    return fit & ~3 if fit < capacity else (capacity + 3) & ~3


SLOT_LIMIT = slot_capacity(4096)


# ---------------------------------------------------------------- scenes ----------------------------------------------------------------
def keypoints(n, octave=0):
    k = np.zeros(n, O.KEYPOINT_DTYPE)
    k["size"], k["class_id"], k["octave"] = 31, -1, octave
    return k


def flipped(desc, bits):
    out = np.unpackbits(np.asarray(desc, np.uint8))
    out[np.asarray(bits, int)] ^= 1
    return np.packbits(out)


def scene(k1, d1, k2, d2, prev=None, window=100, nnratio=0.9, check=False, cam=None, **extra):
    return dict(k1=k1, d1=np.asarray(d1, np.uint8).reshape(-1, 32), k2=k2, d2=np.asarray(d2, np.uint8).reshape(-1, 32), prev=prev, window=window,
                nnratio=nnratio, check=check, cam=cam or PINHOLE, **extra)


def grouped(rng, groups, **params):
    """Every group is one keypoint of frame 2 (angle a2, a random descriptor, a random place) and requests (distance, a1) whose descriptors differ from
    it in exactly `distance` random bits and which sit within 3 px of it.  Groups are apart in descriptor space (random 256-bit strings: ~128 bits, far
    above TH_LOW), so they only meet in each other's candidate lists.  The requests of all groups are interleaved at random; inside a group their
    order is kept.  Returns the scene; scene["group_of"][i1], scene["slot_of"][g]."""
    G = len(groups)
    k2 = keypoints(G)
    k2["x"] = rng.uniform(30, COLS - 30, G).astype(np.float32); k2["y"] = rng.uniform(30, ROWS - 30, G).astype(np.float32)
    k2["angle"] = np.array([g.get("a2", 0.0) for g in groups], np.float32)
    d2 = rng.integers(0, 256, (G, 32), dtype=np.uint8)
    slot_of = rng.permutation(G)                                  # group g is keypoint slot_of[g] of frame 2
    k2o, d2o = k2.copy(), d2.copy()
    k2o[slot_of], d2o[slot_of] = k2, d2
    turn = rng.permutation(np.repeat(np.arange(G), [len(g["reqs"]) for g in groups]))
    at = [0] * G
    k1 = keypoints(len(turn)); d1 = np.zeros((len(turn), 32), np.uint8); group_of = np.zeros(len(turn), int)
    for i1, g in enumerate(turn):
        dist, a1 = groups[g]["reqs"][at[g]]; at[g] += 1
        k1["x"][i1] = k2["x"][g] + np.float32(rng.uniform(-3, 3)); k1["y"][i1] = k2["y"][g] + np.float32(rng.uniform(-3, 3))
        k1["angle"][i1] = a1
        d1[i1] = flipped(d2[g], rng.choice(256, dist, replace=False))
        group_of[i1] = g
    return scene(k1, d1, k2o, d2o, group_of=group_of, slot_of=slot_of, **params)


def ladder(seed, dists):
    """one keypoint of frame 2, len(dists) requests at the Hamming distances `dists` in index order"""
    return grouped(np.random.default_rng(seed), [dict(reqs=[(d, 0.0) for d in dists])])


def ladder_down(seed): return ladder(seed, range(39, -1, -1))
def ladder_up(seed): return ladder(seed + 1, range(40))
def equal(seed): return ladder(seed + 2, [7] * 40)


PAIR_ORDERS = ((9, 4), (4, 9))                                    # steal, no steal
TRIPLE_ORDERS = ((9, 6, 3), (3, 6, 9), (6, 3, 9), (6, 9, 3), (3, 9, 6), (9, 3, 6))


def pairs(seed):
    """10 keypoints wanted by exactly two requests (the kernel's holder list exactly full) and 12 wanted by exactly three (one more than it holds), in
    every order of the distances"""
    groups = [dict(reqs=[(d, 0.0) for d in o]) for o in PAIR_ORDERS * 5 + TRIPLE_ORDERS * 2]
    return grouped(np.random.default_rng(seed + 3), groups)


CASCADE = tuple(range(10)) + (11, 13, 15, 17, 19, 22, 25, 28, 32, 36, 41, 46)


def cascade(seed, dists=CASCADE, n_req=26, nnratio=0.9):
    """All requests carry one descriptor P; the keypoints of frame 2 differ from P by `dists` bits and lie at random places inside every request's window,
    so their grid order is a random permutation of the distance order.  Request j finds the j nearest already taken and takes the next."""
    rng = np.random.default_rng(seed + 4)
    P = rng.integers(0, 256, 32, dtype=np.uint8)
    n2 = len(dists)
    k2 = keypoints(n2)
    k2["x"] = rng.uniform(240, 400, n2).astype(np.float32); k2["y"] = rng.uniform(160, 320, n2).astype(np.float32)
    k2["angle"] = rng.uniform(0, 360, n2).astype(np.float32)
    d2 = np.stack([flipped(P, rng.choice(256, d, replace=False)) for d in dists])
    k1 = keypoints(n_req)
    k1["x"] = rng.uniform(315, 325, n_req).astype(np.float32); k1["y"] = rng.uniform(235, 245, n_req).astype(np.float32)
    return scene(k1, np.tile(P, (n_req, 1)), k2, d2, nnratio=nnratio)


def cascade_wide(seed): return cascade(seed + 1, tuple(range(51)), 60, 2.0)


def crowd(seed, cam=None):
    """5 to 8 clusters in the manner of test_search_projection.py::crowd_scene: the keypoints of frame 2 of a cluster lie within a few pixels and carry
    near-identical descriptors, the requests aim at the cluster centres.  A fifth of both frames is above level 0."""
    rng = np.random.default_rng(seed)
    clusters = int(rng.integers(5, 9))
    n2, n1 = int(rng.integers(150, 260)), int(rng.integers(200, 330))
    centres = np.stack([rng.uniform(60, COLS - 60, clusters), rng.uniform(60, ROWS - 60, clusters)], 1)
    proto = rng.integers(0, 256, (clusters, 32), dtype=np.uint8)
    spin = rng.uniform(0, 360, clusters)

    def frame(n, spread, max_flip, angle0):
        which = rng.integers(0, clusters, n)
        k = keypoints(n)
        k["x"] = (centres[which, 0] + rng.uniform(-spread, spread, n)).astype(np.float32)
        k["y"] = (centres[which, 1] + rng.uniform(-spread, spread, n)).astype(np.float32)
        k["octave"] = np.where(rng.random(n) < 0.8, 0, rng.integers(1, 4, n))
        k["angle"] = ((spin[which] + angle0 + rng.normal(0, 14, n)) % 360).astype(np.float32)
        d = np.stack([flipped(proto[c], rng.choice(256, int(rng.integers(0, max_flip + 1)), replace=False)) for c in which]) if n else np.zeros((0, 32), np.uint8)
        return k, d
    k2, d2 = frame(n2, 9, 30, 0.0)
    k1, d1 = frame(n1, 2, 3, 20.0)
    return scene(k1, d1, k2, d2, nnratio=float(rng.choice([0.9, 1.5])), check=True, cam=cam, clusters=clusters)


def euroc(seed): return crowd(seed, cam=EUROC)


def steal_then_hidden(seed, swapped=False):
    """A takes s at distance 10, B steals s at 5; C is at 7 to s (hidden: 5 <= 7) and at 20 to t and must take t.  A stays -1 and is not asked again:
    u, 30 bits from A, is free and would take it."""
    rng = np.random.default_rng(seed + 5)
    bits = rng.permutation(256)
    s = rng.integers(0, 256, 32, dtype=np.uint8)
    A, B, C = flipped(s, bits[:10]), flipped(s, bits[10:15]), flipped(s, bits[20:27])
    t, u = flipped(C, bits[30:50]), flipped(A, bits[60:90])
    k2 = keypoints(3); k2["x"] = (300, 310, 305); k2["y"] = (200, 215, 207)
    d2 = [s, t, u]
    if swapped:                                                   # u, t, s in index and grid order
        k2 = k2[::-1].copy(); d2 = d2[::-1]
    k1 = keypoints(3); k1["x"] = rng.uniform(295, 315, 3).astype(np.float32); k1["y"] = rng.uniform(195, 220, 3).astype(np.float32)
    return scene(k1, [A, B, C], k2, d2, expect={0: -1, 1: 2 if swapped else 0, 2: 1})


def slot_ties(seed):
    """eight requests, each with three keypoints of frame 2 at distance 4 (different bits) in different cells: the first in grid order wins (strict <
    at :748).  nnratio 2.0: under 0.9 a tie for the best distance always fails the ratio test."""
    rng = np.random.default_rng(seed + 12)
    k1 = keypoints(8); k1["x"] = rng.uniform(250, 390, 8).astype(np.float32); k1["y"] = rng.uniform(180, 300, 8).astype(np.float32)
    d1 = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    order = rng.permutation(24)
    k2 = keypoints(24); d2 = np.zeros((24, 32), np.uint8)
    for j, i2 in enumerate(order):
        g = j // 3
        k2["x"][i2] = k1["x"][g] + np.float32(rng.uniform(-60, 60)); k2["y"][i2] = k1["y"][g] + np.float32(rng.uniform(-60, 60))
        d2[i2] = flipped(d1[g], rng.choice(256, 4, replace=False))
    return scene(k1, d1, k2, d2, nnratio=2.0, group_of=np.arange(8), tied=[sorted(order[3 * g:3 * g + 3].tolist()) for g in range(8)])


def rot_for_bin(rng, b):
    """a rotation that falls into rotHist bin b = round(rot / 30), three degrees off the bin's edges: only bins 0..12 exist for rot in [0, 360)"""
    return float(rng.uniform(0.5, 12) if b == 0 else rng.uniform(348, 359) if b == 12 else 30 * b + rng.uniform(-12, 12))


def voting(rng, votes):
    """groups of `grouped`: votes = [(bin of the first request, its distance), ...] per keypoint of frame 2, angles chosen to place every vote"""
    groups = []
    for reqs in votes:
        a2 = float(np.float32(rng.uniform(0, 360)))
        groups.append(dict(a2=a2, reqs=[(dist, float(np.float32((a2 + rot_for_bin(rng, b)) % 360))) for b, dist in reqs]))
    return groups


def histogram(seed, sizes):
    """one exact match per vote: sizes = {bin: votes}"""
    rng = np.random.default_rng(seed + 6)
    return grouped(rng, voting(rng, [[(b, 0)] for b, n in sizes.items() for _ in range(n)]), check=True)


def stolen_votes(seed):
    """Surviving matches: bins 0, 1, 2, 3 hold 10, 6, 4, 3.  Five more requests vote for bin 3 and are then stolen from (by five of bin 0's): the
    reference counts them (rotHist is never cleaned, :773-783), so bin 3 has 8 votes, the top three are {0, 3, 1} and bin 2 is dropped; counting
    survivors only would keep {0, 1, 2} and drop bin 3."""
    rng = np.random.default_rng(seed + 7)
    votes = [[(3, 6), (0, 0)]] * 5 + [[(0, 0)]] * 5 + [[(1, 0)]] * 6 + [[(2, 0)]] * 4 + [[(3, 0)]] * 3
    return grouped(rng, voting(rng, votes), check=True)


def hist_ties_4(seed): return histogram(seed, {2: 5, 5: 5, 7: 5, 9: 5, 11: 2})
def hist_ties_3(seed): return histogram(seed + 1, {1: 2, 3: 4, 6: 4, 8: 4})
def hist_two_bins(seed): return histogram(seed + 2, {4: 3, 10: 3})
def hist_one_bin(seed): return histogram(seed + 3, {6: 4})
def hist_tenth_10_1(seed): return histogram(seed + 4, {0: 10, 2: 1})
def hist_tenth_11_1(seed): return histogram(seed + 5, {0: 11, 2: 1, 3: 1})
def hist_tenth_20_5_1(seed): return histogram(seed + 6, {1: 20, 2: 5, 3: 1})


HALVES = ((15.0, 0.0, 1), (45.0, 0.0, 2), (345.0, 0.0, 12), (359.99, 0.0, 12), (0.0, 15.0, 12), (10.0, 25.0, 12), (77.5, 77.5, 0), (0.0, 0.0, 0),
          (200.0, 185.0, 1), (14.99, 0.0, 0), (44.99, 0.0, 1), (100.0, 55.0, 2), (45.0, 0.0, 2), (15.0, 0.0, 1), (130.0, 20.0, 4), (75.0, 30.0, 2),
          (5.0, 20.0, 12))


def hist_halves(seed):
    """rot exactly on a bin's half (15, 45, 345), just below 360, a1 < a2 (the + 360 branch) and a1 == a2; HALVES = (a1, a2, bin).  Bins 12, 1 and 2
    are kept (5, 4, 4 votes), bins 0 and 4 (3 and 1) are dropped: a vote that lands in a neighbouring bin changes which matches survive."""
    rng = np.random.default_rng(seed + 8)
    return grouped(rng, [dict(a2=a2, reqs=[(0, a1)]) for a1, a2, _ in HALVES], check=True)


def cell_edges(seed):
    """Frame-2 keypoints exactly on x = 10 c + 5 and y = 10 r + 5 (the grid cells of a 640 x 480 PINHOLE frame are 10 x 10 and PosInGrid ROUNDS: these are
    the cell edges), in column 63 and row 47, and outside the grid (round(x / 10) = 64 or -1, round(y / 10) = 48 or -1); every one has a request with its
    exact descriptor on top of it.  Then eight keypoints with a request whose prev is exactly `window` away (strict <: excluded) or one ulp less."""
    rng = np.random.default_rng(seed + 9)
    spots, inside = [], []
    for c in (0, 7, 30, 31, 62, 63):                              # x = 635 rounds to column 64: not in the grid
        for r in (0, 11, 23, 46, 47):
            spots.append((10.0 * c + 5, 10.0 * r + 5)); inside.append(c < 63 and r < 47)
    for x, y, ok in ((634.9, 200.0, True), (629.5, 77.0, True), (300.0, 474.9, True), (111.0, 469.5, True), (634.9, 474.9, True), (636.0, 200.0, False),
                     (639.9, 100.0, False), (200.0, 476.0, False), (420.0, 479.9, False), (-6.0, 300.0, False), (-4.9, 310.0, True), (330.0, -5.1, False),
                     (340.0, -4.9, True), (0.0, 0.0, True)):
        spots.append((x, y)); inside.append(ok)
    n = len(spots)
    W = 100
    edge = [(-W, 0, False), (-W, 0, True), (W, 0, False), (W, 0, True), (0, -W, False), (0, -W, True), (0, W, False), (0, W, True)]      # (dx, dy, one ulp inwards)
    k2 = keypoints(n + len(edge))
    k2["x"][:n], k2["y"][:n] = np.array(spots, np.float32).T
    k2["x"][n:] = 256 + 8 * np.arange(len(edge)); k2["y"][n:] = 256 + np.arange(len(edge))      # powers of two nearby: prev = x -+ 100 is exact
    perm = rng.permutation(len(k2))
    k2 = k2[perm]
    d2 = rng.integers(0, 256, (len(k2), 32), dtype=np.uint8)
    k1 = k2.copy(); d1 = d2.copy()
    prev = np.stack([k1["x"], k1["y"]], 1).astype(np.float32)
    expect = {}
    for i, src in enumerate(perm):
        if src < n:
            expect[i] = i if inside[src] else -1
        else:
            dx, dy, ok = edge[src - n]
            at = np.array([k2["x"][i], k2["y"][i]], np.float32)
            prev[i] = at + np.array([dx, dy], np.float32)          # exact: |difference| = window, and `<` excludes it
            if ok:
                prev[i] = np.nextafter(prev[i], at)                # one ulp of prev nearer: the difference is exact again and below window
            expect[i] = i if ok else -1
    return scene(k1, d1, k2, d2, prev=prev, window=W, expect=expect)


def outside(seed, window=100):
    """prev left of, right of, above and below the image by more than `window` (the four early returns of GetFeaturesInArea) and by less than it"""
    rng = np.random.default_rng(seed + 10)
    k2 = keypoints(8)
    k2["x"] = (20, 620, 320, 330, 5, 635 - 1, 300, 310); k2["y"] = (240, 250, 20, 460, 5, 470, 200, 300)
    d2 = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    k1 = keypoints(12); d1 = rng.integers(0, 256, (12, 32), dtype=np.uint8)
    k1["x"], k1["y"] = rng.uniform(0, COLS, 12).astype(np.float32), rng.uniform(0, ROWS, 12).astype(np.float32)
    prev = np.array([(-50, 240), (690, 250), (320, -60), (330, 540), (-150, 240), (800, 250), (320, -150), (330, 700), (-101, -101), (745, 585),
                     (-1e6, 240), (320, 1e6)], np.float32)
    d1[:4] = d2[:4]; d1[4:8] = d2[:4]; d1[8], d1[9] = d2[4], d2[5]
    far = window > 900
    expect = {i: i for i in range(4)}
    expect.update({i: -1 for i in range(4, 12)})
    if window == 0:
        expect = {i: -1 for i in range(12)}
    if far:                                                       # everything but the last two sees the whole grid: the first holder of a descriptor keeps it
        expect = {0: 0, 1: 1, 2: 2, 3: 3, 4: -1, 5: -1, 6: -1, 7: -1, 8: 4, 9: 5, 10: -1, 11: -1}
    return scene(k1, d1, k2, d2, prev=prev, window=window, expect=expect)


def outside_1000(seed): return outside(seed, 1000)
def outside_0(seed): return outside(seed, 0)


def levels(seed, kind):
    """no level-0 keypoint in frame 1 / frame 2, empty frames, and octave-3 twins (same place, same descriptor, LOWER index) of otherwise perfect matches"""
    rng = np.random.default_rng(seed + 11)
    k1 = random_frame(rng, 40, level0_frac=0.6)
    d1, k2, d2 = make_descriptor_pair(rng, k1, 45)
    if kind == "no_f1": k1["octave"] = np.maximum(k1["octave"], 1)
    if kind == "no_f2": k2["octave"] = np.maximum(k2["octave"], 1)
    if kind == "n1_zero": k1, d1 = k1[:0], d1[:0]
    if kind == "n2_zero": k2, d2 = k2[:0], d2[:0]
    if kind == "twins":
        k1 = keypoints(15); k1["x"] = rng.uniform(50, 590, 15).astype(np.float32); k1["y"] = rng.uniform(50, 430, 15).astype(np.float32)
        d1 = rng.integers(0, 256, (15, 32), dtype=np.uint8)
        high = k1.copy(); high["octave"] = 3
        k1, d1 = np.concatenate([high, k1]), np.concatenate([d1, d1])
        k2, d2 = k1.copy(), d1.copy()
        return scene(k1, d1, k2, d2, expect={i: (-1 if i < 15 else i) for i in range(30)})
    return scene(k1, d1, k2, d2)


SCENES = dict(ladder_down=ladder_down, ladder_up=ladder_up, equal=equal, pairs=pairs, cascade=cascade, cascade_wide=cascade_wide, crowd_a=lambda s: crowd(s + 0),
              crowd_b=lambda s: crowd(s + 16), steal_then_hidden=steal_then_hidden, steal_then_hidden_swapped=lambda s: steal_then_hidden(s + 1, True),
              slot_ties=slot_ties, stolen_votes=stolen_votes, hist_ties_4=hist_ties_4, hist_ties_3=hist_ties_3, hist_two_bins=hist_two_bins, hist_one_bin=hist_one_bin,
              hist_tenth_10_1=hist_tenth_10_1, hist_tenth_11_1=hist_tenth_11_1, hist_tenth_20_5_1=hist_tenth_20_5_1, hist_halves=hist_halves,
              cell_edges=cell_edges, outside=outside, outside_1000=outside_1000, outside_0=outside_0,
              levels_no_f1=lambda s: levels(s, "no_f1"), levels_no_f2=lambda s: levels(s, "no_f2"), levels_n1_zero=lambda s: levels(s, "n1_zero"),
              levels_n2_zero=lambda s: levels(s, "n2_zero"), levels_twins=lambda s: levels(s, "twins"), euroc=lambda s: euroc(s + 2))
NAMES = tuple(SCENES)
RANDOM = [(1, True, 0.9, 100), (2, False, 0.9, 100), (3, True, 0.6, 40), (4, True, 1.5, 300)]      # test_search_init.py's brute-force parametrisation


def finished(s):
    """the Frame products of a scene: mvKeysUn of both frames, frame 2's mGrid, the bounds, prev"""
    cam = O.camera(**s["cam"])
    b = O.image_bounds(cam, COLS, ROWS)
    un1, off1, idx1 = O.frame_finish(cam, s["k1"], b)
    un2, off2, idx2 = O.frame_finish(cam, s["k2"], b)
    prev = np.stack([un1["x"], un1["y"]], 1).astype(np.float32) if s["prev"] is None else np.asarray(s["prev"], np.float32)
    inside2, pos2 = S.grid_tables(len(un2), idx2)
    return dict(s, un1=un1, off1=off1, idx1=idx1, un2=un2, off2=off2, idx2=idx2, bounds=b, prev=prev.reshape(len(un1), 2), inside2=inside2, pos2=pos2)


def build(name, seed=SEED):
    return finished(SCENES[name](seed))


@functools.lru_cache(maxsize=None)
def get(name):
    if name.startswith("random"):
        seed, check, nnratio, window = RANDOM[int(name[6:])]
        rng = np.random.default_rng(seed)
        k1 = random_frame(rng, 400, level0_frac=0.5)
        d1, k2, d2 = make_descriptor_pair(rng, k1, 450)
        return finished(scene(k1, d1, k2, d2, window=window, nnratio=nnratio, check=check))
    return build(name)


def oracle(s, prev=None):
    return O.search_for_initialization(s["un1"], s["d1"], s["un2"], s["d2"], s["off2"], s["idx2"], s["bounds"], s["prev"] if prev is None else prev,
                                       s["window"], s["nnratio"], s["check"])


def statement(s, check=None, bounds=True):
    return S.search_init_walk(s["un1"], s["d1"], s["un2"], s["d2"], s["inside2"], s["pos2"], s["prev"], s["window"], s["nnratio"],
                              s["check"] if check is None else check, s["bounds"] if bounds else None)


@functools.lru_cache(maxsize=None)
def walked(name):
    """(scene, statement, oracle) of a named scene"""
    s = get(name)
    return s, statement(s), oracle(s)


def reach_line(name, s, res):
    c = S.counts(res)
    return "%s: N1 %d, N2 %d, window %d, nnratio %.1f, check %d | %s | stolen %d, hist_dropped %d, second_choice %d, max_first_round_holders %d | %d matches" % (
        name, len(s["un1"]), len(s["un2"]), s["window"], s["nnratio"], s["check"], ", ".join("%s %d" % kv for kv in c.items() if kv[1]), res["stolen"],
        res["hist_dropped"], res["second_choice"], res["max_first_round_holders"], res["nmatches"])


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_oracle_equals_the_statement_on_every_scene(name):
    s, res, (n, m12, prev) = walked(name)
    print(reach_line(name, s, res))
    assert m12.tolist() == res["m12"] and n == res["nmatches"] == sum(m >= 0 for m in res["m12"])
    assert prev.tobytes() == res["prev"].tobytes()
    assert res["box_outside_cells"] == 0                          # the cell window cuts nothing from the box: the pure box test is the same statement
    assert statement(s, bounds=False)["m12"] == res["m12"]
    for i1, want in s.get("expect", {}).items():
        assert res["m12"][i1] == want, (name, i1)
    n2, m12b, prev2 = oracle(s, prev)                              # the second call of the GPU tests, with prev carried over
    res2 = S.search_init_walk(s["un1"], s["d1"], s["un2"], s["d2"], s["inside2"], s["pos2"], prev, s["window"], s["nnratio"], s["check"], s["bounds"])
    assert m12b.tolist() == res2["m12"] and n2 == res2["nmatches"] and prev2.tobytes() == res2["prev"].tobytes()


def exits(res, which=None):
    c = S.counts(res)
    return {k: v for k, v in c.items() if v} if which is None else c[which]


def test_contention_scenes_reach_what_they_are_named_for():
    s, r, _ = walked("ladder_down")
    assert exits(r) == {"ACCEPTED": 1, "ACCEPTED_STEALING": 39} and r["stolen"] == 39 and r["nmatches"] == 1 and r["m12"][39] == 0
    assert r["max_first_round_holders"] == 40                     # more holders than kAcc = 2: the kernel's scan over the decisions
    s, r, _ = walked("ladder_up")
    assert exits(r) == {"ACCEPTED": 1, "ALL_HIDDEN": 39} and r["m12"][0] == 0 and r["max_first_round_holders"] == 40
    s, r, _ = walked("equal")
    assert exits(r) == {"ACCEPTED": 1, "ALL_HIDDEN": 39} and r["m12"][0] == 0 and r["max_first_round_holders"] == 40
    assert len({s["d1"][i].tobytes() for i in range(40)}) == 40 and (S._distances(s["d1"], s["d2"]) == 7).all()
    s, r, _ = walked("pairs")
    assert r["first_round_holders"] == {2: 10, 3: 12}
    for g, order in enumerate(PAIR_ORDERS * 5 + TRIPLE_ORDERS * 2):      # the winner of a group: the first request that holds the smallest distance
        mine = np.flatnonzero(s["group_of"] == g)
        assert [r["m12"][i] for i in mine] == [int(s["slot_of"][g]) if d == min(order) else -1 for d in order]
    assert r["stolen"] == 5 * 1 + 2 * (2 + 0 + 1 + 1 + 0 + 1)
    s, r, _ = walked("steal_then_hidden")
    assert exits(r) == {"ACCEPTED": 2, "ACCEPTED_STEALING": 1} and r["stolen"] == 1 and r["second_choice"] == 1 and r["m12"] == [-1, 0, 1]
    assert r["prev"][0].tobytes() == s["prev"][0].tobytes()
    assert walked("steal_then_hidden_swapped")[1]["m12"] == [-1, 2, 1]
    s, r, _ = walked("slot_ties")
    assert exits(r) == {"ACCEPTED": 8} and r["m12"] == [min(s["tied"][g], key=lambda i2: s["pos2"][i2]) for g in s["group_of"]]
    assert sum(r["m12"][i1] != min(s["tied"][g]) for i1, g in enumerate(s["group_of"])) >= 2      # grid order, not index order, decides


def test_cascades_are_as_long_as_their_tables():
    for name, n_slots, n_req, rounds in (("cascade", 22, 26, 22), ("cascade_wide", 51, 60, 51)):
        s, r, _ = walked(name)
        order = np.argsort(s["pos2"])                              # keypoints of frame 2 in grid order
        assert len(s["idx2"]) == n_slots and order.tolist() != sorted(order.tolist()) and order.tolist() != sorted(order.tolist(), reverse=True)
        assert r["m12"] == list(range(n_slots)) + [-1] * (n_req - n_slots)      # request j takes keypoint j
        assert exits(r, "ACCEPTED") == n_slots and exits(r, "ALL_HIDDEN") + exits(r, "TH_LOW") == n_req - n_slots
        assert r["second_choice"] == n_slots - 1 and r["max_first_round_holders"] == n_req and r["stolen"] == 0
        assert S.synchronous_rounds(s["un1"], s["d1"], s["un2"], s["d2"], s["inside2"], s["pos2"], s["prev"], s["window"], s["nnratio"], s["bounds"])[1] >= rounds


@pytest.mark.parametrize("name", ["crowd_a", "crowd_b", "euroc"])
def test_crowds_steal_settle_for_second_choices_and_fill_one_keypoint_with_holders(name):
    s, r, _ = walked(name)
    assert 5 <= s["clusters"] <= 8
    assert r["stolen"] > 0 and r["second_choice"] > 20 and r["max_first_round_holders"] >= 3
    assert exits(r, "LEVEL") > 10 and r["nmatches"] > 10
    if name == "euroc":
        assert np.abs(s["bounds"] - np.round(s["bounds"])).min() > 1e-3 and (s["un2"]["x"] != s["k2"]["x"]).mean() > 0.9
    assert {walked("crowd_a")[0]["nnratio"], walked("crowd_b")[0]["nnratio"]} == {0.9, 1.5}


def test_histogram_scenes_place_their_votes():
    def sizes(r): return {b: n for b, n in enumerate(r["hist"]) if n}
    s, r, _ = walked("stolen_votes")
    assert sizes(r) == {0: 10, 1: 6, 2: 4, 3: 8} and r["stolen"] == 5 and r["kept_bins"] == [0, 3, 1] and r["hist_dropped"] == 4 and r["nmatches"] == 19
    survivors = [b for i, b in enumerate(r["bin"]) if b >= 0 and (np.array(statement(s, check=False)["m12"])[i] >= 0)]
    assert S.three_maxima([survivors.count(b) for b in range(30)]) == [0, 1, 2]      # counting the survivors only keeps another set
    for name, want_sizes, kept, dropped in (("hist_ties_4", {2: 5, 5: 5, 7: 5, 9: 5, 11: 2}, [2, 5, 7], 7), ("hist_ties_3", {1: 2, 3: 4, 6: 4, 8: 4}, [3, 6, 8], 2),
                                            ("hist_two_bins", {4: 3, 10: 3}, [4, 10, -1], 0), ("hist_one_bin", {6: 4}, [6, -1, -1], 0),
                                            ("hist_tenth_10_1", {0: 10, 2: 1}, [0, 2, -1], 0), ("hist_tenth_11_1", {0: 11, 2: 1, 3: 1}, [0, -1, -1], 2),
                                            ("hist_tenth_20_5_1", {1: 20, 2: 5, 3: 1}, [1, 2, -1], 1)):
        s, r, _ = walked(name)
        assert sizes(r) == want_sizes and r["kept_bins"] == kept and r["hist_dropped"] == dropped, name
        assert r["nmatches"] == sum(want_sizes.values()) - dropped
    s, r, _ = walked("hist_halves")
    for g, (a1, a2, b) in enumerate(HALVES):
        i1 = int(np.flatnonzero(s["group_of"] == g)[0])
        assert r["bin"][i1] == b, (a1, a2)
        assert (r["m12"][i1] >= 0) == (b in (12, 1, 2))
    assert sizes(r) == {0: 3, 1: 4, 2: 4, 4: 1, 12: 5} and r["kept_bins"] == [12, 1, 2] and r["hist_dropped"] == 4
    assert max(r["bin"]) == 12 and all(b <= 12 for b in r["bin"])      # round(rot / 30) of rot < 360: bins 13..29 stay empty


def test_geometry_scenes_reach_every_early_return_and_both_sides_of_the_window():
    s, r, _ = walked("cell_edges")
    assert sum(v >= 0 for v in s["expect"].values()) >= 30 and sum(v < 0 for v in s["expect"].values()) >= 20
    cells = np.searchsorted(s["off2"], np.arange(len(s["idx2"])), side="right") - 1      # the cell of every grid entry
    assert len(s["idx2"]) < len(s["un2"]) and 63 in cells // 48 and 47 in cells % 48 and 0 in cells // 48 and 0 in cells % 48
    assert exits(r, "ACCEPTED") == sum(v >= 0 for v in s["expect"].values()) and r["stolen"] == 0
    s, r, _ = walked("outside")
    assert r["early"][4:8].tolist() == [2, 1, 4, 3] and r["early"][8:].tolist() == [0, 1, 2, 3] and (r["early"][:4] == 0).all()      # (-101, -101): a cell window, an empty box
    assert (r["exit"][4:] == S.NO_CAND).all() and r["nmatches"] == 4
    s, r, _ = walked("outside_1000")
    assert (r["early"][:10] == 0).all() and r["nmatches"] == 6 and exits(r, "ALL_HIDDEN") + exits(r, "TH_LOW") == 4
    s, r, _ = walked("outside_0")
    assert exits(r) == {"NO_CAND": 12} and (r["early"][8:] > 0).all()
    assert exits(walked("levels_no_f1")[1]) == {"LEVEL": 40}
    assert exits(walked("levels_no_f2")[1]).keys() == {"LEVEL", "NO_CAND"} and walked("levels_no_f2")[1]["nmatches"] == 0
    assert len(walked("levels_n1_zero")[0]["un1"]) == 0 and len(walked("levels_n2_zero")[0]["un2"]) == 0
    assert exits(walked("levels_twins")[1]) == {"LEVEL": 15, "ACCEPTED": 15}


@pytest.mark.parametrize("name", NAMES + tuple("random%d" % i for i in range(len(RANDOM))))
def test_synchronous_rounds_settle_on_the_walk_within_requests_plus_one_rounds(name):
    """the only place where "the parallel fixed point is the sequential result" is tested apart from the kernel"""
    s = get(name)
    R = int((s["un1"]["octave"] <= 0).sum())
    dec, rounds = S.synchronous_rounds(s["un1"], s["d1"], s["un2"], s["d2"], s["inside2"], s["pos2"], s["prev"], s["window"], s["nnratio"], s["bounds"])
    assert rounds <= R + 1
    assert S.tables_of_decisions(dec) == statement(s, check=False)["m12"]


def test_slot_limit_is_derived_from_the_kernel_and_documented():
    src = open(os.path.join(os.path.dirname(X.orbextractor.__file__), "csrc", "k_match.hip")).read()
    assert "160LL * 1024 - 1024" in src and "(kGridCols + 2 + kHistoLength + 8) * sizeof(int) + 2 * kWaves * sizeof(int) + 64" in src
    # the two shared constants of that expression, where the kernels take them from
    csrc = os.path.dirname(os.path.join(os.path.dirname(X.orbextractor.__file__), "csrc", "k_match.hip"))
    assert "constexpr int kGridCols = 64, kGridRows = 48," in open(os.path.join(csrc, "orbx_device.hpp")).read()
    assert "constexpr int kHistoLength = 30;" in open(os.path.join(csrc, "k_match_helpers.hpp")).read()
    assert "constexpr int kThreads = 1024, kWaves = kThreads / 64;" in src
    per_slot = re.search(r"const long long sc = room / \(([0-9+* kAc]+)\);", src).group(1)
    assert "constexpr int kAcc = 2;" in src
    assert sum(int(np.prod([2 if f.strip() == "kAcc" else int(f) for f in term.split("*")])) for term in per_slot.split("+")) == SLOT_BYTES == 66
    assert FIXED_LDS == 608
    assert SLOT_LIMIT == 2456 and all(slot_capacity(c) == 2456 for c in (2458, 4096, 10000, 32767))
    assert slot_capacity(2456) == 2456 and slot_capacity(61) == 64 and slot_capacity(64) == 64 and slot_capacity(1024) == 1024
    # capacity 2457 alone gets a table of 2460 (its 2457 keypoints all fit): the byte count stays below the 160 KiB of a workgroup
    assert slot_capacity(2457) == 2460 and 2460 * SLOT_BYTES + FIXED_LDS <= 160 * 1024
    text = open(X.orbextractor._HEADER).read()
    pos = text.index("int orbx_search_for_initialization_device(")
    doc = text[text.rindex("/*", 0, pos):pos]
    assert "66 B" in doc and "2456" in doc and "either frame" in doc and "52 B" not in doc


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def upload(frames, cap):
    """frames: [(mvKeysUn, descriptors, grid offsets, grid indices)] -> the frame-major device arrays of the C ABI"""
    B = len(frames)
    un = np.zeros((B, cap), O.KEYPOINT_DTYPE); d = np.zeros((B, cap, 32), np.uint8)
    n = np.zeros(B, np.int32); off = np.zeros((B, 64 * 48 + 1), np.int32); idx = np.zeros((B, cap), np.int32)
    for f, (k, desc, o, i) in enumerate(frames):
        assert len(k) <= cap
        un[f, :len(k)], d[f, :len(k)], n[f], off[f] = k, desc, len(k), o
        idx[f, :len(i)] = i
    return dict(un=_dev(un.view(np.uint8)), d=_dev(d), n=_dev(n), off=_dev(off), idx=_dev(idx))


def launch_key(s):
    return (s["window"], s["nnratio"], s["check"], s["bounds"].tobytes())


def run_pairs(scenes, cap, what, frames=None, pair_frames=None, calls=2, overflow=()):
    """ONE launch over all `scenes` (one pair each; they share window, nnratio, check and bounds) with poisoned outputs, compared with the oracle;
    then the same launch again with prev carried over.  frames / pair_frames: frames shared between pairs (default: frames 2p and 2p + 1, steps 2)."""
    import torch
    P = len(scenes)
    s0 = scenes[0]
    assert len({launch_key(s) for s in scenes}) == 1
    if frames is None:
        frames = [fr for s in scenes for fr in ((s["un1"], s["d1"], s["off1"], s["idx1"]), (s["un2"], s["d2"], s["off2"], s["idx2"]))]
        pair_frames = ((0, 2), (1, 2))
    dev = upload(frames, cap)
    prev = np.full((P, cap, 2), POISON, np.float32)
    for p, s in enumerate(scenes):
        prev[p, :len(s["un1"])] = s["prev"]
    d_prev = _dev(prev)
    ex = X.ORBextractor(1000)
    want_prev = [s["prev"] for s in scenes]
    for call in range(calls):
        d_m12 = torch.full((P, cap), -7, dtype=torch.int32, device="cuda"); d_nm = torch.full((P,), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ex.search_for_initialization_device(P, pair_frames[0], pair_frames[1], dev["un"], dev["d"], dev["n"], cap, dev["off"], dev["idx"], s0["bounds"],
                                            d_prev, d_m12, d_nm, s0["window"], s0["nnratio"], s0["check"])
        ex.synchronize()
        m12, nm, got_prev = d_m12.cpu().numpy(), d_nm.cpu().numpy(), d_prev.cpu().numpy()
        for p, s in enumerate(scenes):
            n1 = len(s["un1"])
            tag = "%s, pair %d %s, capacity %d, call %d" % (what, p, s.get("name", ""), cap, call)
            if p in overflow:
                n_o, m_o, prev_o = -1, np.full(n1, -1, np.int32), want_prev[p]
            else:
                n_o, m_o, prev_o = oracle(s, want_prev[p])
            print("%s: N1 %d, N2 %d, %d matches" % (tag, n1, len(s["un2"]), n_o))
            assert int(nm[p]) == n_o, tag
            assert m12[p, :n1].tolist() == m_o.tolist(), tag
            assert got_prev[p, :n1].tobytes() == prev_o.tobytes(), tag
            assert (m12[p, n1:] == -7).all() and (got_prev[p, n1:] == POISON).all(), tag      # nothing written past N1
            want_prev[p] = prev_o


def launches(scenes):
    groups = {}
    for s in scenes:
        groups.setdefault(launch_key(s), []).append(s)
    return list(groups.values())


def named(names, seed=SEED):
    return [dict(get(n) if seed == SEED else build(n, seed), name=n) for n in names]


def size(s):
    return max(len(s["un1"]), len(s["un2"]), 1)


def test_named_scenes_share_a_few_launches_and_the_small_capacities_hold_most_of_them():
    groups = launches(named(NAMES))
    print([len(g) for g in groups])
    assert len(groups) <= 8 and sum(len(g) for g in groups) == len(NAMES) and max(len(g) for g in groups) >= 12
    assert {"ladder_down", "ladder_up", "equal", "stolen_votes", "hist_halves", "outside", "levels_twins"} <= {n for n in NAMES if size(get(n)) <= 40}
    small = [n for n in NAMES if size(get(n)) <= 61]
    assert len(small) >= 20 and {"ladder_down", "pairs", "cascade", "cascade_wide", "stolen_votes", "hist_ties_4", "outside", "levels_twins"} <= set(small)


@pytest.mark.gpu
def test_gpu_every_scene_in_one_launch_per_parameter_set_twice():
    for group in launches(named(NAMES)):
        run_pairs(group, max(size(s) for s in group) + 37, "named scenes")


@pytest.mark.gpu
@pytest.mark.parametrize("cap", [40, 61, 64, 1024])
def test_gpu_scenes_at_other_capacities(cap):
    """the tables hold (capacity + 3) & ~3 entries: 40 (the ladders' 40 requests fill it; the entry used to refuse every capacity below 61), 61 -> 64
    (padding), 64 (cascade_wide has 60 requests), 1024 (every scene)"""
    for group in launches([s for s in named(NAMES) if size(s) <= cap]):
        run_pairs(group, cap, "capacity")


@pytest.mark.gpu
def test_gpu_one_frame_1_against_many_frames_2():
    """frame1_step = 0: the crowd's frame 1 against its own frame 2, that frame 2 reversed, two other crowds' and an empty one; prev is per pair"""
    a = get("crowd_a")
    rev = dict(a, k2=a["k2"][::-1].copy(), d2=a["d2"][::-1].copy(), prev=None)
    others = [dict(a, k2=get(n)["k2"], d2=get(n)["d2"], prev=None) for n in ("crowd_b", "crowd_a")]
    others[1]["k2"] = others[1]["k2"].copy(); others[1]["k2"]["x"] += np.float32(7.5); others[1]["k2"]["y"] -= np.float32(3.25)
    empty = dict(a, k2=a["k2"][:0], d2=a["d2"][:0], prev=None)
    scenes = [a] + [finished(s) for s in (rev, others[0], others[1], empty)]
    frames = [(a["un1"], a["d1"], a["off1"], a["idx1"])] + [(s["un2"], s["d2"], s["off2"], s["idx2"]) for s in scenes]
    run_pairs(scenes, max(size(s) for s in scenes) + 5, "one frame 1", frames=frames, pair_frames=((0, 0), (1, 1)))


def limit_scene(n1_level0, n2_level0, cap, seed):
    """uniformly spread keypoints, random descriptors; a third of the smaller frame's level-0 keypoints have a partner 0..12 bits and a few pixels away"""
    rng = np.random.default_rng(seed)

    def frame(n0):
        n_other = min(300, cap - n0)                              # keypoints above level 0 beside them
        k = random_frame(rng, n0 + n_other, level0_frac=0.0)
        k["octave"][rng.permutation(n0 + n_other)[:n0]] = 0
        k["x"] *= np.float32(0.98); k["y"] *= np.float32(0.98)      # round(x / 10) <= 63 and round(y / 10) <= 47: every keypoint is in the grid
        return k, rng.integers(0, 256, (n0 + n_other, 32), dtype=np.uint8)
    (k1, d1), (k2, d2) = frame(n1_level0), frame(n2_level0)
    z1, z2 = np.flatnonzero(k1["octave"] == 0), np.flatnonzero(k2["octave"] == 0)
    m = min(len(z1), len(z2)) // 3
    for i, j in zip(rng.permutation(z1)[:m], rng.permutation(z2)[:m]):
        k2["x"][j] = np.clip(k1["x"][i] + np.float32(rng.uniform(-15, 15)), 0, COLS - 13); k2["y"][j] = np.clip(k1["y"][i] + np.float32(rng.uniform(-15, 15)), 0, ROWS - 10)
        k2["angle"][j] = np.float32((k1["angle"][i] + rng.normal(0, 6)) % 360)
        d2[j] = flipped(d1[i], rng.choice(256, int(rng.integers(0, 13)), replace=False))
    return finished(scene(k1, d1, k2, d2, window=30, check=True))


# (level-0 keypoints of frame 1, of frame 2, capacity); the last: capacity 2457 is the one value whose table is larger than SLOT_LIMIT (2460 entries, 162 968 B)
LIMIT_CASES = {"frame2_at_limit": (400, SLOT_LIMIT, 4096), "frame2_over": (400, SLOT_LIMIT + 1, 4096), "frame1_at_limit": (SLOT_LIMIT, 400, 4096),
               "frame1_over": (SLOT_LIMIT + 1, 400, 4096), "frame2_full_at_capacity_2457": (400, 2457, 2457)}


@functools.lru_cache(maxsize=None)
def limit_case(case):
    n1, n2, cap = LIMIT_CASES[case]
    return limit_scene(n1, n2, cap, seed=sum(map(ord, case))), max(n1, n2) > slot_capacity(cap)


@pytest.mark.parametrize("case", sorted(LIMIT_CASES))
def test_limit_scenes_have_the_level_0_counts_they_are_named_for(case):
    s, over = limit_case(case)
    n1, n2 = int((s["un1"]["octave"] == 0).sum()), int((s["un2"]["octave"][s["idx2"]] == 0).sum())
    assert (n1, n2) == LIMIT_CASES[case][:2] and over == ("over" in case) and max(len(s["un1"]), len(s["un2"])) <= LIMIT_CASES[case][2]
    assert len(s["idx2"]) == len(s["un2"])                        # every keypoint of frame 2 is in the grid: its level-0 count is the staged count
    assert oracle(s)[0] > 60                                      # the pair below or at the limit really matches


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(LIMIT_CASES))
def test_gpu_table_limit_in_either_frame(case):
    """exactly the limit: equal to the oracle; one more: d_n_matches = -1, an all -1 table, prev untouched, nothing past N1"""
    s, over = limit_case(case)
    run_pairs([s], LIMIT_CASES[case][2], case, overflow=(0,) if over else ())


@pytest.mark.gpu
def test_gpu_overflowing_pair_does_not_disturb_its_neighbours():
    over1, over2, fine = limit_case("frame2_over")[0], limit_case("frame1_over")[0], limit_case("frame2_at_limit")[0]
    small = dict(get("pairs"), window=30, check=True)
    run_pairs([small, over1, fine, over2, small], 4096, "overflow beside others", overflow=(1, 3))


def check_gpu_on_seed(seed):
    """the body tools/fuzz_matchers.py runs with seeds outside the committed one: every named scene of that seed, one launch per parameter set, twice"""
    scenes = named(NAMES, seed)
    for s in scenes:
        n, m12, prev = oracle(s)
        res = statement(s)
        assert m12.tolist() == res["m12"] and n == res["nmatches"] and prev.tobytes() == res["prev"].tobytes(), (seed, s["name"])
    for group in launches(scenes):
        run_pairs(group, max(size(s) for s in group) + int(seed % 5), "seed %d" % seed)
