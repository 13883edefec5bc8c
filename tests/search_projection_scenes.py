"""Crafted scenes of the one-camera projection search (tests/test_search_projection_edges.py, CPU and GPU), an independent statement of the
search with named single-rule mutants, and the helpers that put a batch of scenes on the device.

A scene is one current frame (keypoints, descriptors, mGrid, mvuRight, occupancy on entry) and the requests against it.  The image is 512 x 384
without distortion, so mnMinX = mnMinY = 0 and the grid cells are 8 x 8 pixels with mfGridElementWidthInv = mfGridElementHeightInv = 0.125:
every window bound of a scene with dyadic coordinates is exact.  Frame::PosInGrid rounds, so the keypoint at x sits in column round(x / 8)
(columns are centred on multiples of 8) and a keypoint with x >= 508 or y >= 380 is left out of the grid although it lies inside the image.

The statement is written from reference src/ORBmatcher.cc:44-135 (map-to-frame: best / second, level rule, mfNNratio), :1961-2177
(frame-to-frame: best only, rotation histogram), :2179-2300 (relocalisation: the caller's ORBdist), :2303-2344 (ComputeThreeMaxima) and
src/Frame.cc:655-724 (GetFeaturesInArea), on Python integers; floats appear only where the reference computes in binary32."""
import functools
import math

import numpy as np

import oracle_lib as O

f32 = np.float32
COLS, ROWS = 512, 384
GRID_COLS, GRID_ROWS, HISTO_LENGTH = 64, 48, 30
CAM = O.camera(256.0, 256.0, 256.0, 192.0)
TH_HIGH = 100

MUTANTS = ("maxdist_ge", "box_le", "stereo_ge", "uright_ge_zero", "ratio_double", "ratio_ge", "ratio_any_level", "last_tie", "second_tie_level",
           "closed_ignored", "no_obs_closes", "first_holder_wins", "round_half_even", "no_bin_wrap", "cut_gt", "cut_double", "maxima_ge",
           "drop_counts_keypoints", "level_check_always", "level_max_unguarded")


@functools.lru_cache(None)
def bounds():
    b = O.image_bounds(CAM, COLS, ROWS)
    assert b.tolist() == [0.0, COLS, 0.0, ROWS]
    b.setflags(write=False)
    return b


def up(v):
    return np.nextafter(f32(v), f32(np.inf))


def down(v):
    return np.nextafter(f32(v), f32(-np.inf))


# ---------------------------------------------------------------- the statement ----------------------------------------------------------------
def rotation_bin(angle1, angle2, mutant=None):
    """:2073-2078: rot = kpLF.angle - kpCF.angle in binary32, 360 added once if negative, round(rot * factor), 30 -> 0"""
    factor = f32(1.0) / f32(HISTO_LENGTH)
    rot = f32(angle1) - f32(angle2)
    if rot < 0.0:
        rot = f32(rot + f32(360.0))
    x = float(f32(rot * factor))                          # x + 0.5 below is exact in binary64
    b = round(x) if mutant == "round_half_even" else int(math.floor(x + 0.5))      # C round(): halves away from zero (x >= 0 here)
    if b == HISTO_LENGTH and mutant != "no_bin_wrap":
        b = 0
    return b


def three_maxima(sizes, mutant=None):
    """:2303-2344"""
    ge = mutant == "maxima_ge"
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if s > max1 or (ge and s >= max1):
            max3, max2, max1, ind3, ind2, ind1 = max2, max1, s, ind2, ind1, i
        elif s > max2 or (ge and s >= max2):
            max3, max2, ind3, ind2 = max2, s, ind2, i
        elif s > max3 or (ge and s >= max3):
            max3, ind3 = s, i
    cut = float(f32(0.1)) * max1 if mutant == "cut_double" else float(f32(0.1) * f32(max1))
    below = (lambda m: m <= cut) if mutant == "cut_gt" else (lambda m: m < cut)
    if below(max2):
        ind2 = ind3 = -1
    elif below(max3):
        ind3 = -1
    return ind1, ind2, ind3


def _cell(fn, v):
    """(int)floor(v) / (int)ceil(v); a request whose window is not finite has no cells at all (its box test fails for every keypoint anyway)"""
    return int(fn(v)) if math.isfinite(v) else None


def area(s, x, y, r, min_level, max_level, mutant=None):
    """Frame::GetFeaturesInArea (Frame.cc:655-724): keypoint indices in traversal order"""
    b = s["bounds"]
    mnx, mny = f32(b[0]), f32(b[2])
    winv, hinv = f32(GRID_COLS) / f32(b[1] - b[0]), f32(GRID_ROWS) / f32(b[3] - b[2])
    x, y, r = f32(x), f32(y), f32(r)
    lo = [_cell(math.floor, f32(f32(f32(c - m) - r) * inv)) for c, m, inv in ((x, mnx, winv), (y, mny, hinv))]
    hi = [_cell(math.ceil, f32(f32(f32(c - m) + r) * inv)) for c, m, inv in ((x, mnx, winv), (y, mny, hinv))]
    if None in lo or None in hi:
        return []
    x0, y0, x1, y1 = max(0, lo[0]), max(0, lo[1]), min(GRID_COLS - 1, hi[0]), min(GRID_ROWS - 1, hi[1])
    if x0 >= GRID_COLS or x1 < 0 or y0 >= GRID_ROWS or y1 < 0:
        return []
    check = min_level > 0 or max_level >= 0
    if mutant in ("level_check_always", "level_max_unguarded"):
        check = True
    un, off, idx = s["un"], s["off"], s["idx"]
    out = []
    for ix in range(x0, x1 + 1):
        for iy in range(y0, y1 + 1):
            c = ix * GRID_ROWS + iy
            for j in range(int(off[c]), int(off[c + 1])):
                k = int(idx[j])
                o = int(un["octave"][k])
                if check:
                    if o < min_level:
                        continue
                    if (max_level >= 0 or mutant == "level_max_unguarded") and o > max_level:
                        continue
                dx, dy = abs(f32(un["x"][k] - x)), abs(f32(un["y"][k] - y))
                if (dx <= r and dy <= r) if mutant == "box_le" else (dx < r and dy < r):
                    out.append(k)
    return out


def _bits(row):
    return int.from_bytes(bytes(bytearray(row)), "little")


def statement(s, ratio, check=True, stereo=None, mutant=None, trace=None, log=None):
    """The search of one scene: (nmatches, matches[N], occupied[N]).  ratio: the map-to-frame form (:44-135), else the frame-to-frame /
    relocalisation form.  trace (a list) receives one (request, [(distance, keypoint, closed at the decision)] of the static candidates,
    ascending by (distance, traversal position)) per active request; log (a dict) receives request -> the keypoint it was accepted at."""
    assert mutant is None or mutant in MUTANTS
    un, q = s["un"], s["q"]
    n = len(un)
    stereo = s["stereo"] if stereo is None else stereo
    ur = s["ur"] if stereo else None
    nn, th = f32(s["nnratio"]), int(s["max_distance"])
    d = [_bits(r) for r in s["d"]]
    qd = [_bits(r) for r in s["qd"]]
    occ = [int(v) for v in s["occ"]]
    entry = list(occ)
    m = [-1] * n
    nm = 0
    hist = [[] for _ in range(HISTO_LENGTH + 1)]
    for i in range(min(int(s.get("n_queries", len(q))), len(q))):
        fl = int(q["flags"][i])
        if not fl & 1:
            continue
        r = f32(q["radius"][i])
        cands = area(s, q["u"][i], q["v"][i], r, int(q["min_level"][i]), int(q["max_level"][i]), mutant)
        best, best2, lv, lv2, bi = 256, 256, -1, -1, -1
        seen = []
        for pos, k in enumerate(cands):
            if ur is not None and (ur[k] >= 0 if mutant == "uright_ge_zero" else ur[k] > 0):
                er = abs(f32(f32(q["ur"][i]) - ur[k]))
                if er >= r if mutant == "stereo_ge" else er > r:
                    continue
            dist = bin(qd[i] ^ d[k]).count("1")
            if not entry[k]:
                seen.append((dist, pos, k))
            if occ[k] and mutant != "closed_ignored":
                continue
            if dist < best or (mutant == "last_tie" and dist == best):
                best2, best, lv2, lv, bi = best, dist, lv, int(un["octave"][k]), k
            elif ratio and (dist < best2 or (mutant == "second_tie_level" and dist == best2)):
                lv2, best2 = int(un["octave"][k]), dist
        if trace is not None:
            trace.append((i, [(dist, k, bool(occ[k])) for dist, _, k in sorted(seen)]))
        if best < th if mutant == "maxdist_ge" else best <= th:
            if ratio and (lv == lv2 or mutant == "ratio_any_level"):
                if mutant == "ratio_double":
                    over = best > float(nn) * best2
                elif mutant == "ratio_ge":
                    over = f32(best) >= f32(nn * f32(best2))
                else:
                    over = f32(best) > f32(nn * f32(best2))
                if over:
                    continue
            if not (mutant == "first_holder_wins" and m[bi] >= 0):
                m[bi] = i
            occ[bi] = 1 if (fl & 2 or mutant == "no_obs_closes") else 0
            nm += 1
            if log is not None:
                log[i] = bi
            if not ratio and check:
                hist[rotation_bin(q["angle"][i], un["angle"][bi], mutant)].append(bi)
    if not ratio and check:
        keep = three_maxima([len(h) for h in hist[:HISTO_LENGTH]], mutant)
        gone = set()
        for b in range(HISTO_LENGTH + 1):
            if b in keep:
                continue
            for k in hist[b]:
                m[k] = -1
                occ[k] = 0
                nm -= 1
                gone.add(k)
        if mutant == "drop_counts_keypoints":
            nm += sum(len(hist[b]) for b in range(HISTO_LENGTH + 1) if b not in keep) - len(gone)
    return nm, m, occ


def oracle(s, ratio, check=True, stereo=None):
    stereo = s["stereo"] if stereo is None else stereo
    nq = min(int(s.get("n_queries", len(s["q"]))), len(s["q"]))
    nm, m, occ = O.search_by_projection(s["q"][:nq], s["qd"][:nq] if nq else np.zeros((1, 32), np.uint8), s["un"], s["d"], s["off"], s["idx"], s["bounds"],
                                        s["ur"] if stereo else None, s["occ"], ratio, s["nnratio"], check, s["max_distance"])
    return nm, m.tolist(), occ.tolist()


def rescans(s, ratio):
    """requests that k_search_proj<true> has to scan again: their list of the kTop = 4 smallest static keys is full, and closed keypoints
    leave fewer of it visible than the decision needs (one, or two in ratio mode)"""
    trace = []
    statement(s, ratio, trace=trace)
    out = []
    for i, keys in trace:
        top = keys[:4]
        if len(top) == 4 and sum(1 for _, _, closed in top if not closed) < (2 if ratio else 1):
            out.append(i)
    return out


def ratio_disagreements(nnratio):
    """distance pairs at which (float)b1 > nnratio * (float)b2 differs between binary32 and a double product: ([(b1, b2)], single, double)"""
    b = np.arange(257)
    nn = f32(nnratio)
    single = b[:, None].astype(f32) > (nn * b[None, :].astype(f32)).astype(f32)
    double = b[:, None].astype(np.float64) > float(nn) * b[None, :].astype(np.float64)
    return [(int(a), int(c)) for a, c in zip(*np.nonzero(single != double))], single, double


# ---------------------------------------------------------------- building scenes ----------------------------------------------------------------
class Builder:
    """keypoints and requests of one scene.  A "spot" is a place of its own on a 32-pixel lattice: requests of radius <= 16 at a spot see the
    keypoints of that spot (at offsets of 0 or 8 pixels) and no others."""

    def __init__(self, name, seed, modes=((False, True), (False, False), (True, False)), nnratio=0.9, max_distance=TH_HIGH, stereo=False):
        self.name, self.rng = name, np.random.default_rng(seed)
        self.kp, self.kd, self.kur, self.kocc, self.rq, self.rd = [], [], [], [], [], []
        self.params = dict(modes=tuple(modes), nnratio=nnratio, max_distance=max_distance, stereo=stereo)
        self.expect, self.nspots = {}, 0

    def spot(self):
        i = self.nspots
        self.nspots += 1
        assert i < 14 * 10
        return f32(32 * (1 + i % 14)), f32(32 * (1 + i // 14))

    def descriptor(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def keypoint(self, x, y, desc, octave=0, angle=0.0, ur=-1.0, occ=0):
        self.kp.append((f32(x), f32(y), octave, f32(angle)))
        self.kd.append(np.asarray(desc, np.uint8))
        self.kur.append(f32(ur))
        self.kocc.append(occ)
        return len(self.kp) - 1

    def request(self, u, v, r, desc, flags=3, levels=(-1, -1), angle=0.0, ur=0.0, expect=None):
        """expect: the keypoint this request is accepted at (None: nowhere) in every mode the scene runs in, if stated"""
        self.rq.append((f32(u), f32(v), f32(ur), f32(r), levels[0], levels[1], flags, f32(angle)))
        self.rd.append(np.asarray(desc, np.uint8))
        if expect is not None:
            self.expect[len(self.rq) - 1] = None if expect == "none" else expect
        return len(self.rq) - 1

    def build(self):
        k = np.zeros(len(self.kp), O.KEYPOINT_DTYPE)
        for i, (x, y, o, a) in enumerate(self.kp):
            k[i]["x"], k[i]["y"], k[i]["octave"], k[i]["angle"] = x, y, o, a
        k["size"], k["class_id"] = 31, -1
        un, off, idx = O.frame_finish(CAM, k, bounds())
        assert un.tobytes() == k.tobytes()                # no distortion: mvKeysUn = mvKeys
        q = np.zeros(len(self.rq), O.PROJ_QUERY_DTYPE)
        for i, row in enumerate(self.rq):
            q[i] = row
        s = dict(name=self.name, un=un, d=np.array(self.kd, np.uint8).reshape(-1, 32), off=off, idx=idx, bounds=bounds(), q=q,
                 qd=np.array(self.rd, np.uint8).reshape(-1, 32), ur=np.array(self.kur, f32), occ=np.array(self.kocc, np.uint8), expect=dict(self.expect))
        s.update(self.params)
        assert len(un) <= 300 and len(q) <= 400, self.name
        return s


def away(desc, n, start=0):
    """desc with bits start .. start + n - 1 flipped: exactly n bits away"""
    out = np.array(desc, np.uint8).copy()
    for bit in range(start, start + n):
        out[bit >> 3] ^= np.uint8(1 << (bit & 7))
    return out


def single(b, dist, expect, r=4.0, **kw):
    """a spot with one keypoint and one request `dist` bits from it"""
    x, y = b.spot()
    d = b.descriptor()
    kwk = dict((k, kw.pop(k)) for k in ("octave", "ur", "occ") if k in kw)
    kangle = kw.pop("kp_angle", 0.0)
    k = b.keypoint(x, y, d, angle=kangle, **kwk)
    return b.request(x, y, r, away(d, dist), expect=k if expect else "none", **kw), k


def th_high_boundary(maxd):
    b = Builder("th_high_boundary_%d" % maxd, 1, max_distance=maxd)
    for dist in (maxd - 1, maxd, maxd + 1):      # :2059 / :124 / :2246: bestDist <= TH_HIGH (ORBdist); every MapPoint closes (flags bit 1)
        single(b, dist, dist <= maxd)
    return b.build()


def box_boundary():
    """Frame.cc:717: fabs(distx) < factorX.  u = v = the spot, r = 8: a keypoint at exactly u + 8 lies in column (u + 8) / 8, the last one
    ceil((u + 8) * 0.125) visits, and is no candidate; one float nearer it is."""
    b = Builder("box_boundary", 2)
    for dx, dy in ((8, 0), (-8, 0), (0, 8), (0, -8)):
        for inside in (False, True):
            x, y = b.spot()
            kx, ky = f32(x + dx), f32(y + dy)
            if inside:
                kx = kx if dx == 0 else (down(kx) if dx > 0 else up(kx))
                ky = ky if dy == 0 else (down(ky) if dy > 0 else up(ky))
            d = b.descriptor()
            k = b.keypoint(kx, ky, d)
            b.request(x, y, 8.0, away(d, 7), expect=k if inside else "none")
    return b.build()


def stereo_column(stereo):
    """:68-73 / :2039-2046: a keypoint with mvuRight > 0 is skipped if fabs(ur - mvuRight) > radius.  Requests predict ur = 32, r = 8."""
    b = Builder("stereo_column" if stereo else "stereo_column_without_u_right", 3, stereo=stereo)
    for kur, kept in ((40.0, True), (up(40.0), False), (24.0, True), (down(24.0), False),       # |32 - mvuRight| = 8 exactly, and the next float
                      (0.0, True), (-0.0, True), (-1.0, True),                                  # no stereo observation: not tested (they are 32 away)
                      (np.finfo(f32).smallest_subnormal, False), (32.0, True), (1000.0, False)):
        x, y = b.spot()
        d = b.descriptor()
        k = b.keypoint(x, y, d, ur=kur)
        b.request(x, y, 8.0, away(d, 5), ur=32.0, expect=k if (kept or not stereo) else "none")
    return b.build()


def ratio_rounding(nnratio=0.9):
    """:126: bestDist > mfNNratio * bestDist2 is a binary32 product.  Every pair (b1, b2) with b1 <= 100 at which the double product decides
    otherwise, best and second on one level (accepted), (b1 + 1, b2) beside it (rejected), and both again on two levels (accepted)."""
    b = Builder("ratio_rounding_%g" % nnratio, 4, modes=((True, False),), nnratio=nnratio)
    pairs = [(b1, b2) for b1, b2 in ratio_disagreements(nnratio)[0] if b1 <= 100]
    for n, (b1, b2) in enumerate(pairs):
        for first, same in ((b1, True), (b1 + 1, True), (b1, False), (b1 + 1, False)):
            x, y = b.spot()
            d = b.descriptor()
            order = ((first, 2), (b2, 2 if same else 3))
            ks = [b.keypoint(x, y, away(d, dist), octave=o) for dist, o in (order if n % 2 == 0 else order[::-1])]
            best = ks[0] if n % 2 == 0 else ks[1]
            b.request(x, y, 4.0, d, expect=best if (first == b1 or not same) else "none")
    s = b.build()
    s["pairs"] = pairs
    return s


def second_level_ties():
    """:104-120: of two candidates with the second smallest distance the first in traversal order provides bestLevel2.  Best: 50 bits, level 2;
    A: 52 bits, level 2; B: 52 bits, level 3; 50 > 0.9 * 52, so the request is accepted only if B comes before A."""
    b = Builder("second_level_ties", 5, modes=((True, False),))
    for a_first in (True, False):
        for columns in (False, True):
            for best_pos in (0, 1, 2):
                x, y = b.spot()
                d = b.descriptor()
                tie = [("A", 52, 2), ("B", 52, 3)] if a_first else [("B", 52, 3), ("A", 52, 2)]
                trav = tie[:best_pos] + [("best", 50, 2)] + tie[best_pos:]      # traversal order
                if columns:      # one column per candidate, keypoint indices descending along the traversal
                    made = [(b.keypoint(x + 8 * (c - 1), y, away(d, dist), octave=o), nm) for c, (nm, dist, o) in reversed(list(enumerate(trav)))]
                else:            # one cell: traversal order is index order
                    made = [(b.keypoint(x, y, away(d, dist), octave=o), nm) for nm, dist, o in trav]
                best = [k for k, nm in made if nm == "best"][0]
                b.request(x, y, 12.0, d, expect="none" if a_first else best)
    return b.build()


def first_in_grid_order():
    """:104 / :2052: dist < bestDist is strict, so of equal best distances the first in GetFeaturesInArea's order (columns ascending, rows
    ascending inside a column, push_back order inside a cell) is taken.  The candidates lie on different levels: in ratio mode the tie is accepted."""
    b = Builder("first_in_grid_order", 6)
    ties = {}
    places = {"cell": ((0, 0), (0, 0), (0, 0)), "rows": ((0, -8), (0, 0), (0, 8)), "columns": ((-8, 0), (0, 0), (8, 0)),
              "diagonal": ((-8, 8), (0, -8), (8, 0)), "column_then_row": ((0, 8), (8, -8), (0, -8))}
    for name, offs in places.items():
        for n_tied in (2, 3):
            x, y = b.spot()
            d = b.descriptor()
            # traversal order of the offsets: column, then row, then index; indices are handed out against it where cells differ
            trav = sorted(range(3), key=lambda j: (offs[j][0], offs[j][1]))
            made = {}
            for j in (sorted(range(3), key=lambda j: (-offs[j][0], -offs[j][1])) if name != "cell" else range(3)):
                rank = trav.index(j) if name != "cell" else j
                dist = 40 if n_tied == 2 and rank == 0 else 30      # (two tied: the first in order is farther, the second and the third tie)
                made[rank] = b.keypoint(x + offs[j][0], y + offs[j][1], away(d, dist, start=16 * rank), octave=1 + rank)
            first = 0 if n_tied == 3 else 1
            ties[b.request(x, y, 12.0, d, expect=made[first])] = (name, made[first], [made[r] for r in range(first, 3)])
    s = b.build()
    s["ties"] = ties       # request -> (placement, expected keypoint, the keypoints with the best distance)
    return s


LEVEL_WINDOWS = ((-1, -1), (0, -1), (-1, 0), (0, 0), (3, -1), (0, 3), (2, 4), (5, 2), (7, 9), (6, -1), (1, 1))
LEVEL_DISTANCES = (12, 30, 20, 10, 25, 5, 35, 15)      # of the keypoint on octave 0 .. 7
LEVEL_EXPECT = (5, 5, 0, 0, 5, 3, 3, None, 7, 7, 1)    # octave of the nearest keypoint inside the window


def level_windows():
    """Frame.cc:690, :705-712: bCheckLevels = minLevel > 0 || maxLevel >= 0; octave < minLevel and (maxLevel >= 0 and octave > maxLevel) are out"""
    b = Builder("level_windows", 7)
    for lv, want in zip(LEVEL_WINDOWS, LEVEL_EXPECT):
        x, y = b.spot()
        d = b.descriptor()
        ks = [b.keypoint(x, y, away(d, dist, start=8 * o), octave=o) for o, dist in enumerate(LEVEL_DISTANCES)]
        b.request(x, y, 4.0, d, levels=lv, expect="none" if want is None else ks[want])
    return b.build()


CHAINS = {1: 3, 3: 5, 4: 6, 5: 7, 6: 5, 17: 19, 40: 32}      # requests -> keypoints of the cluster


def chain_cluster(b, n_kp, occ=()):
    """n_kp keypoints around (256, 192) in nine cells, keypoint j exactly j bits from the returned descriptor, levels alternating (so that in
    ratio mode the nearest and the second nearest open keypoint never share a level)"""
    d = b.descriptor()
    order = list(b.rng.permutation(n_kp))                  # indices are not in distance order
    ks = {}
    for j in order:
        ks[int(j)] = b.keypoint(256 + 8 * (int(j) % 3 - 1), 192 + 8 * ((int(j) // 3) % 3 - 1), away(d, int(j)), octave=2 + int(j) % 2, occ=int(j in occ))
    return d, [ks[j] for j in range(n_kp)]


def chains(k):
    """:64-66 / :2035-2037: k requests with one descriptor; every accepted one closes its keypoint, so request i takes the i-th nearest"""
    b = Builder("chains_%d" % k, 10 + k)
    d, ks = chain_cluster(b, CHAINS[k])
    for i in range(k):
        b.request(256.0, 192.0, 16.0, d, expect=ks[i] if i < len(ks) else "none")
    return b.build()


def chain_with_gaps():
    """the chain with requests that do not close (no observations: flags bit 1 clear), inactive requests, and a keypoint closed on entry"""
    b = Builder("chain_with_gaps", 8)
    d, ks = chain_cluster(b, 10, occ=(2,))
    R = lambda flags: b.request(256.0, 192.0, 16.0, d, flags=flags)
    # request: 0 closes 0 | 1 takes 1, open | 2 takes 1 over, closes | 3 inactive | 4: 2 is closed on entry: takes 3 | 5, 6 take 4, open | 7 closes 4
    #          8 inactive with bit 1 | 9 takes 5, open and stays its holder | 10 closes 6 ...
    for flags in (3, 1, 3, 0, 3, 1, 1, 3, 2, 1):
        R(flags)
    b.keypoint(64, 64, b.descriptor())                    # far from the cluster: untouched
    s = b.build()
    s["holders"] = {ks[0]: 0, ks[1]: 2, ks[2]: -1, ks[3]: 4, ks[4]: 7, ks[5]: 9}
    s["closed"] = [ks[0], ks[1], ks[2], ks[3], ks[4]]
    s["acceptances"] = 8
    return s


def planted_histogram(name, counts, seed):
    """single-candidate requests whose rotation falls in bin i for counts[i] of them (rot = 30 * i exactly)"""
    b = Builder(name, seed, modes=((False, True), (False, False)))
    for i, c in enumerate(counts):
        for _ in range(c):
            single(b, 3, True, angle=30.0 * i)
    if not counts:
        for _ in range(3):
            single(b, TH_HIGH + 1, False)
    return b.build()


HISTOGRAMS = {"hist_10_1_1": (10, 1, 1), "hist_11_1_1": (11, 1, 1), "hist_30_3_3": (30, 3, 3), "hist_four_tens": (10, 10, 10, 10),
              "hist_one_bin": (0, 0, 5), "hist_no_matches": ()}
HISTOGRAMS_KEPT = {"hist_10_1_1": 12, "hist_11_1_1": 11, "hist_30_3_3": 36, "hist_four_tens": 30, "hist_one_bin": 5, "hist_no_matches": 0}

# (request angle, keypoint angle, bin, times planted): round(rot / 30) with halves away from zero
BELOW_360 = down(360.0)
HALF_BELOW = f32(15.0)      # the largest angle difference whose product with factor lies below 0.5
while f32(HALF_BELOW * (f32(1.0) / f32(HISTO_LENGTH))) >= 0.5:
    HALF_BELOW = down(HALF_BELOW)
EDGE_ANGLES = ((0.0, 0.0, 0, 1), (-0.0, 0.0, 0, 1),        # rot = -0.0 is not < 0: no wrap, bin 0 (360 is not reached this way)
               (15.0, 0.0, 1, 3), (up(15.0), 0.0, 1, 1),                               # x = 0.5 exactly: bin 1, with halves to even bin 0
               (down(15.0), 0.0, 1, 1), (HALF_BELOW, 0.0, 0, 1),      # factor is a little above 1 / 30: the product still rounds onto 0.5 down to here
               (45.0, 0.0, 2, 1),                                                      # 1.5 -> 2 either way
               (75.0, 0.0, 3, 3), (100.0, 25.0, 3, 1),                                 # 2.5 -> 3, to even 2
               (345.0, 0.0, 12, 1), (10.0, 25.0, 12, 1),                               # 11.5 -> 12 either way; -15 wraps to 345
               (BELOW_360, 0.0, 12, 1), (0.0, 3e-5, 12, 1), (0.0, 1e-6, 12, 1))        # the last float below 360, met directly and by the wrap; 360 itself


def histogram_edges():
    """bins 1 (5 entries), 12 (5) and 3 (4) are kept, bins 0 (3) and 2 (1) are dropped: a match is kept or dropped by its bin"""
    b = Builder("histogram_edges", 9, modes=((False, True), (False, False)))
    for a1, a2, _, times in EDGE_ANGLES:
        for _ in range(times):
            single(b, 3, True, angle=a1, kp_angle=a2)
    s = b.build()
    s["expect"] = {}                                       # (with the orientation check the dropped bins' requests are not matched)
    return s


def holders_in_two_bins():
    """:2061 against :2166-2170: rotHist keeps one entry per ACCEPTANCE, the table one holder per keypoint.  Bins 0, 1, 2 (7, 5, 4 entries) are
    kept, every other bin is dropped.  X: taken by a request without observations in bin 3 (dropped), then by a closing one in bin 0.
    Y: the converse.  Z: taken twice by requests without observations, both in dropped bins, then by a closing request in bin 1."""
    b = Builder("holders_in_two_bins", 20, modes=((False, True), (False, False)))
    for i, c in enumerate((5, 4, 4)):
        for _ in range(c):
            single(b, 3, True, angle=30.0 * i)
    spots = {}
    for name, holders in (("X", ((1, 90.0), (3, 0.0))), ("Y", ((1, 0.0), (3, 120.0))), ("Z", ((1, 150.0), (1, 180.0), (3, 30.0)))):
        x, y = b.spot()
        d = b.descriptor()
        k = b.keypoint(x, y, d)
        spots[name] = (k, [b.request(x, y, 4.0, away(d, 2), flags=fl, angle=a) for fl, a in holders])
    s = b.build()
    s["spots"] = spots
    return s


def window_edges():
    """Frame.cc:666-688: windows outside the grid are empty, windows across its border are clipped; :717 with r = 0; keypoints outside mGrid"""
    b = Builder("window_edges", 21)
    d = [b.descriptor() for _ in range(12)]
    corner = b.keypoint(0.0, 0.0, d[0])                    # cell (0, 0)
    far = b.keypoint(506.0, 379.0, d[1])                   # cell (63, 47)
    left_out = [b.keypoint(510.0, 100.0, d[2]), b.keypoint(100.0, 381.0, d[3]), b.keypoint(-5.0, 200.0, d[4]), b.keypoint(200.0, -4.5, d[5])]
    mid = b.keypoint(256.0, 192.0, d[6])
    edge = [b.keypoint(3.0, 200.0, d[7]), b.keypoint(200.0, 3.0, d[8])]
    for u, v in ((-100.0, 192.0), (700.0, 192.0), (256.0, -100.0), (256.0, 600.0), (-9.0, 200.0), (200.0, -9.0)):      # outside on each side; r = 8
        b.request(u, v, 8.0, d[6], expect="none")
    b.request(-7.0, 200.0, 16.0, d[7], expect=edge[0])     # outside the image, the window reaches column 0 and 1
    b.request(200.0, -7.0, 16.0, d[8], expect=edge[1])
    b.request(2.0, 2.0, 8.0, away(d[0], 4), expect=corner)            # clipped to column 0 and row 0
    b.request(509.0, 381.0, 8.0, away(d[1], 4), flags=1, expect=far)  # clipped to column 63 and row 47 (no observations: stays open)
    b.request(256.0, 192.0, 0.0, d[6], expect="none")                 # r = 0: nothing is nearer than 0
    for k, (u, v) in zip(left_out, ((510.0, 100.0), (100.0, 381.0), (-5.0, 200.0), (200.0, -4.5))):
        b.request(u, v, 4.0, d[2 + left_out.index(k)], expect="none")      # its own keypoint is not in the grid
    b.request(256.0, 192.0, 1024.0, away(d[6], 9), expect=mid)        # the whole image
    b.request(100.0, 100.0, 2048.0, away(d[1], 6, start=100), flags=1, expect=far)
    s = b.build()
    s["left_out"] = left_out
    return s


def normal(name, seed):
    """an ordinary small scene: clusters of keypoints, requests that compete for them"""
    b = Builder(name, seed)
    for c in range(6):
        x, y = b.spot()
        d = b.descriptor()
        for j in range(5):
            b.keypoint(x + 8 * (j % 2), y, away(d, 3 * j, start=40 * (j % 3)), octave=1 + j % 3, occ=int(c == 2 and j == 0))
        for j in range(4):
            b.request(x + 1.0, y, 12.0, away(d, j, start=200), flags=3 if j != 1 else 1, levels=((-1, -1), (0, 3), (1, -1), (0, 2))[j])
    return b.build()


@functools.lru_cache(None)
def crafted_scenes():
    out = [th_high_boundary(100), th_high_boundary(64), box_boundary(), stereo_column(True), stereo_column(False), ratio_rounding(0.9),
           second_level_ties(), first_in_grid_order(), level_windows()]
    out += [chains(k) for k in CHAINS]
    out += [chain_with_gaps(), holders_in_two_bins(), histogram_edges()]
    out += [planted_histogram(n, c, 30 + i) for i, (n, c) in enumerate(HISTOGRAMS.items())]
    out += [window_edges(), normal("normal", 40)]
    return tuple(out)


def degenerate_pairs():
    """pairs of one batch: (scene, n_queries as the device sees it or None).  Every scene has the parameters of `normal`."""
    first, last = normal("normal_first", 41), normal("normal_last", 42)
    empty = Builder("no_keypoints", 43)
    empty.request(256.0, 192.0, 16.0, empty.descriptor())
    no_requests = dict(normal("no_requests", 44), n_queries=0)
    inactive = normal("all_inactive", 45)
    inactive["q"]["flags"] &= ~1
    closed = normal("all_closed", 46)
    closed["occ"][:] = 1
    return [first, empty.build(), no_requests, inactive, closed, last]


def groups(scenes):
    """launches: (ratio, check, nnratio, max_distance, stereo) -> scenes"""
    out = {}
    for s in scenes:
        for ratio, check in s["modes"]:
            out.setdefault((ratio, check, s["nnratio"], s["max_distance"], s["stereo"]), []).append(s)
    return out


# ---------------------------------------------------------------- capacities ----------------------------------------------------------------
LDS_BUDGET = 160 * 1024 - 512      # orbx_entry.hpp kLdsBudget
K_TOP = 4


def lds_bytes(capacity, query_capacity, top_list):
    """k_project.hip projSearchLdsBytes"""
    c = (capacity + 3) & ~3
    return c * (32 + 16 + 4 + 4 + 2 + 1 + 1 + 2) + (HISTO_LENGTH + 4) * 4 + (GRID_COLS * GRID_ROWS + 2) * 2 + query_capacity * (4 + 1 + (4 * K_TOP if top_list else 0)) + 64


def takes_top_list(capacity):
    return lds_bytes(capacity, capacity, True) <= LDS_BUDGET


def is_accepted(capacity):
    return capacity <= 32767 and lds_bytes(capacity, capacity, False) <= LDS_BUDGET


@functools.lru_cache(None)
def capacities():
    """1024, the last capacity with best-key lists, the first without, one without that is no multiple of 4, the largest accepted"""
    last_top = max(c for c in range(1, 4000) if takes_top_list(c))
    largest = max(c for c in range(1, 4000) if is_accepted(c))
    odd = next(c for c in range(last_top + 2, largest) if c % 4 == 3)
    return (1024, last_top, last_top + 1, odd, largest)


# ---------------------------------------------------------------- device ----------------------------------------------------------------
def run_device(ex, frames, requests, cur, desc_blocks, qdesc_blocks, n_pairs, cap, qcap, ratio, nnratio, check, max_distance, stereo, n_queries="array",
               bounds4=None):
    """frames: scenes whose frame goes to device frame f; requests: per pair a scene whose q / occ are the pair's; qdesc_blocks: the descriptor
    blocks as they lie in the buffer.  Outputs start as -7.  Returns (n_matches[P], matches[P, cap], occupied[P, cap])."""
    import torch
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    F = len(frames)
    un = np.zeros((F, cap), O.KEYPOINT_DTYPE); d = np.zeros((F, cap, 32), np.uint8); n = np.zeros(F, np.int32)
    off = np.zeros((F, GRID_COLS * GRID_ROWS + 1), np.int32); idx = np.zeros((F, cap), np.int32); ur = np.full((F, cap), -1.0, f32)
    for f, s in enumerate(frames):
        m = len(s["un"])
        un[f, :m], d[f, :m], n[f], off[f], ur[f, :m] = s["un"], s["d"], m, s["off"], s["ur"]
        idx[f, :len(s["idx"])] = s["idx"]
    q = np.zeros((n_pairs, qcap), O.PROJ_QUERY_DTYPE); nq = np.zeros(n_pairs, np.int32); occ = np.zeros((n_pairs, cap), np.uint8)
    for p, s in enumerate(requests):
        q[p, :len(s["q"])] = s["q"]
        nq[p] = s.get("n_queries_device", s.get("n_queries", len(s["q"])))
        occ[p, :len(s["occ"])] = s["occ"]
    qd = np.zeros((len(qdesc_blocks), qcap, 32), np.uint8)
    for k, blk in enumerate(qdesc_blocks):
        qd[k, :len(blk)] = blk
    d_occ = dev(occ)
    d_m = torch.full((n_pairs, cap), -7, dtype=torch.int32, device="cuda"); d_nm = torch.full((n_pairs,), -7, dtype=torch.int32, device="cuda")
    ex.search_by_projection_device(n_pairs, cur, dev(q.view(np.uint8)), dev(qd), desc_blocks, dev(nq) if n_queries == "array" else None, qcap,
                                   dev(un.view(np.uint8)), dev(d), dev(n), cap, dev(off), dev(idx), bounds() if bounds4 is None else bounds4,
                                   dev(ur) if stereo else None, d_occ, ratio, nnratio, check, d_m, d_nm, max_distance=max_distance)
    ex.synchronize()
    return d_nm.cpu().numpy(), d_m.cpu().numpy(), d_occ.cpu().numpy()


def run_scenes(ex, scenes, cap, key, n_queries="array"):
    """one pair per scene, frame p and descriptor block p"""
    ratio, check, nnratio, max_distance, stereo = key
    return run_device(ex, scenes, scenes, (0, 1), (0, 1), [s["qd"] for s in scenes], len(scenes), cap, cap, ratio, nnratio, check, max_distance, stereo,
                      n_queries)
