"""Crafted scenes for orbx_search_for_triangulation_device (one-camera SearchForTriangulation, reference src/ORBmatcher.cc:965-1206): tens of
features each, every probe a NAMED keyframe-1 feature whose outcome is planted, not read off the code under test.  No GPU here.

Exact geometry comes from the rectified matrix F12 = [[0,0,0],[0,0,-1],[0,1,0]]: the epipolar line of (x1, y1) is la = 0, lb = 1, lc = -y1,
so den = 1 and dsqr = fl((y2 - y1)^2); with y1 = 0 every dy is exact.  A scene is the dict tests/test_search_triangulation.py's walk, brute,
pack, run and assert_equals_walk take (kf1, kf2, F, ep) plus
  name, runs   the Run configurations it is searched under
  probes       name -> (keyframe-1 feature, expectation): an int (the keyframe-2 feature, -1 for none) or a function of the Run
  counters     name of a walk counter -> function of the Run giving its planted value (None: not planted under that Run)
  gpu          (optional) what the device is handed where that differs from what the walk is handed: raw octaves, a FeatureVector with
               entries whose index is at or above the frame's count beside buffers that hold rows there, stale counts."""
import collections

import numpy as np

import extractorb_amd as X
from triangulation_walk import POPCOUNT, epipolar_constrain

f32 = np.float32
INF = f32(np.inf)
TABLES = X.compute_tables(1200, 1.2, 8)
SF, SIG2 = TABLES["scale_factors"], TABLES["level_sigma2"]
RECT = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], f32)
FAR = np.array([-30000.0, -30000.0], f32)                 # an epipole no feature is near

Run = collections.namedtuple("Run", "ur only_stereo coarse th_low check_orientation", defaults=(True, False, False, 50, True))
DEFAULT = Run()
COARSE = Run(coarse=True)


def options(run):
    return dict(only_stereo=run.only_stereo, coarse=run.coarse, th_low=run.th_low, check_orientation=run.check_orientation)


def flip(d, bits, rng):
    d = d.copy()
    for b in rng.choice(256, bits, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def distance(a, b):
    return int(POPCOUNT[a ^ b].sum())


class Pair:
    """a keyframe pair under construction: a() adds a keyframe-1 feature, b() a keyframe-2 feature; the FeatureVector lists keep the order
    of the calls inside a node"""

    def __init__(self, name, runs=(DEFAULT,), F=RECT, ep=FAR, seed=0):
        self.name, self.runs, self.F, self.ep = name, tuple(runs), np.asarray(F, f32), np.asarray(ep, f32)
        self.rng = np.random.default_rng(1000 + seed)
        self.k = ([], []); self.fv = ([], [])
        self.probes, self.counters, self.node = {}, {}, 0

    def new_node(self):
        self.node += 7
        return self.node

    def desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def _add(self, side, node, desc, x, y, angle, octave, mp, ur, fv):
        self.k[side].append((f32(x), f32(y), f32(angle), int(octave), np.asarray(desc, np.uint8), int(mp), f32(ur)))
        i = len(self.k[side]) - 1
        if fv:
            self.fv[side].append((node, i))
        return i

    def a(self, node, desc, x=10.0, y=0.0, angle=0.0, octave=0, mp=0, ur=-1.0, fv=True):
        return self._add(0, node, desc, x, y, angle, octave, mp, ur, fv)

    def b(self, node, desc, x=10.0, y=0.0, angle=0.0, octave=0, mp=0, ur=-1.0, fv=True):
        return self._add(1, node, desc, x, y, angle, octave, mp, ur, fv)

    def probe(self, name, i1, expect):
        assert name not in self.probes
        self.probes[name] = (i1, expect)

    def keyframe(self, side):
        rows = self.k[side]
        kps = np.zeros(len(rows), X.KEYPOINT_DTYPE)
        kps["size"], kps["class_id"] = 31, -1
        for i, (x, y, angle, octave, _, _, _) in enumerate(rows):
            kps["x"][i], kps["y"][i], kps["angle"][i], kps["octave"][i] = x, y, angle, octave
        fv = self.fv[side]
        order = np.argsort(np.array([n for n, _ in fv], np.int64), kind="stable") if fv else []
        return dict(kps=kps, desc=np.array([r[4] for r in rows], np.uint8).reshape(-1, 32), mp=np.array([r[5] for r in rows], np.uint8),
                    ur=np.array([r[6] for r in rows], f32), fv=(np.array([fv[j][0] for j in order], np.uint32), np.array([fv[j][1] for j in order], np.uint32)))

    def done(self, **extra):
        return dict(name=self.name, runs=self.runs, kf1=self.keyframe(0), kf2=self.keyframe(1), F=self.F, ep=self.ep, probes=self.probes,
                    counters=self.counters, **extra)


def size(s):
    """the smallest capacity that holds what the device is handed"""
    g = s.get("gpu", {})
    return max(1, *(max(len(k["desc"]), len(k["fv"][0])) for k in (g.get("kf1", s["kf1"]), g.get("kf2", s["kf2"]))))


# ---------------------------------------------------------------- one candidate, planted facts ----------------------------------------------------------------
Facts = collections.namedtuple("Facts", "i2 dist gate inside ur1 ur2", defaults=(-1, 0, True, False, f32(-1), f32(-1)))


def single(c):
    """the outcome of a keyframe-1 feature whose node holds ONE candidate, from the planted facts about that candidate (ORBmatcher.cc:1041-1132
    in the order of the reference): a function of the Run"""
    def expect(run):
        st1, st2 = bool(run.ur and c.ur1 >= 0), bool(run.ur and c.ur2 >= 0)
        if run.only_stereo and not (st1 and st2):
            return -1
        if c.dist > run.th_low:
            return -1
        if not st1 and not st2 and c.inside:
            return -1
        if not run.coarse and not c.gate:
            return -1
        return c.i2
    return expect


def plant(p, name, facts=Facts(), y2=0.0, x2=10.0, octave=0, d1=None, d2=None, y1=0.0, x1=10.0):
    """one keyframe-1 feature and its one candidate, in a node of their own"""
    node = p.new_node()
    d1 = p.desc() if d1 is None else d1
    d2 = (flip(d1, facts.dist, p.rng) if facts.dist <= 255 else ~d1) if d2 is None else d2
    assert distance(d1, d2) == facts.dist
    i1 = p.a(node, d1, x=x1, y=y1, ur=facts.ur1)
    i2 = p.b(node, d2, x=x2, y=y2, octave=octave, ur=facts.ur2)
    p.probe(name, i1, single(facts._replace(i2=i2)))
    return i1, i2


# ---------------------------------------------------------------- the epipolar gate ----------------------------------------------------------------
def gate_pair(o):
    """(dy, its successor): the largest binary32 dy with (double)fl(dy * dy) < 3.84 * (double)sigma2[o], and the next value"""
    lim = 3.84 * float(SIG2[o])
    d = f32(np.sqrt(lim))
    while float(f32(d * d)) < lim:
        d = np.nextafter(d, INF)
    while not float(f32(d * d)) < lim:
        d = np.nextafter(d, f32(0))
    return d, np.nextafter(d, INF)


def gate_scene(name, F, seed):
    p = Pair(name, (DEFAULT, COARSE), F=F, seed=seed)
    n_out = 0
    for o in range(8):
        inside, outside = gate_pair(o)
        assert epipolar_constrain(10.0, 0.0, 10.0, inside, p.F, SIG2[o]) and not epipolar_constrain(10.0, 0.0, 10.0, outside, p.F, SIG2[o])
        assert epipolar_constrain(10.0, 0.0, 10.0, -inside, p.F, SIG2[o]) and not epipolar_constrain(10.0, 0.0, 10.0, -outside, p.F, SIG2[o])
        plant(p, "gate_o%d_in" % o, Facts(gate=True), y2=inside, octave=o)
        plant(p, "gate_o%d_out" % o, Facts(gate=False), y2=outside, octave=o)
        plant(p, "gate_o%d_in_neg" % o, Facts(gate=True), y2=-inside, octave=o)
        plant(p, "gate_o%d_out_neg" % o, Facts(gate=False), y2=-outside, octave=o)
        n_out += 2
    p.counters["epi"] = lambda run: 0 if run.coarse else n_out
    return p.done()


def degenerate_gate_scene(kind):
    """den == 0, a matrix with an infinity, a keyframe-2 x of NaN: no candidate passes the test; under bCoarse (no test) each one matches"""
    F = RECT.copy()
    if kind == "f_zero":
        F[:] = 0
    elif kind == "f_inf":
        F[2, 1] = np.inf
    p = Pair(kind, (DEFAULT, COARSE), F=F, seed=40 + len(kind))
    for j, y2 in enumerate((0.0, 1.0, -3.5)):
        plant(p, "%s_%d" % (kind, j), Facts(gate=False), y2=y2, x2=np.nan if kind == "x_nan" else 10.0 + j)
        with np.errstate(invalid="ignore"):
            assert not epipolar_constrain(10.0, 0.0, np.nan if kind == "x_nan" else 10.0 + j, y2, F, SIG2[0])
    p.counters["epi"] = lambda run: 0 if run.coarse else 3
    return p.done()


# ---------------------------------------------------------------- the epipole's disc ----------------------------------------------------------------
def disc_pair(o):
    """(d, its successor): the largest binary32 d with fl(d * d) + 0 < fl(100 * sf[o]) - inside the disc -, and the next value - outside"""
    lim = f32(f32(100) * SF[o])
    d = f32(np.sqrt(lim))
    while f32(d * d) < lim:
        d = np.nextafter(d, INF)
    while not f32(d * d) < lim:
        d = np.nextafter(d, f32(0))
    return d, np.nextafter(d, INF)


STEREO_COMBINATIONS = ((-1.0, -1.0), (5.0, -1.0), (-1.0, 5.0), (5.0, 5.0))
DISC_RUNS = (COARSE, Run(ur=False, coarse=True), Run(only_stereo=True, coarse=True))


def disc_scene():
    """the epipole at the origin: e = 0 - pt is exact.  Every probe in the four stereo combinations; the Run without mvuRight makes all mono."""
    p = Pair("disc", DISC_RUNS, ep=(0.0, 0.0), seed=3)
    n_inside = 0
    # offsets (ex, 8) from the epipole: (6, 8) stays (100 is not < 100); walking x towards the epipole, the first binary32 value whose rounded
    # fl(fl(ex * ex) + 64) falls below 100 is dropped and its neighbour outside still stays (the sums in between round back up to 100)
    inside0 = lambda x: f32(f32(f32(f32(0) - x) * f32(f32(0) - x)) + f32(64)) < f32(f32(100) * SF[0])      # noqa: E731
    x_in = f32(-6)
    while not inside0(x_in):
        x_in = np.nextafter(x_in, f32(0))
    x_on = np.nextafter(x_in, -INF)
    assert not inside0(f32(-6)) and not inside0(x_on) and inside0(x_in) and f32(-6) <= x_on < x_in < f32(-5.9999)
    for u1, u2 in STEREO_COMBINATIONS:
        tag = "%s%s" % ("s" if u1 >= 0 else "m", "s" if u2 >= 0 else "m")
        plant(p, "disc_o0_on_%s" % tag, Facts(inside=False, ur1=f32(u1), ur2=f32(u2)), x2=-6.0, y2=-8.0)          # exactly (6, 8): 100 is not < 100
        plant(p, "disc_o0_last_outside_%s" % tag, Facts(inside=False, ur1=f32(u1), ur2=f32(u2)), x2=x_on, y2=-8.0)
        plant(p, "disc_o0_in_%s" % tag, Facts(inside=True, ur1=f32(u1), ur2=f32(u2)), x2=x_in, y2=-8.0)
        n_inside += 1
        for o in range(1, 8):
            inside, outside = disc_pair(o)
            plant(p, "disc_o%d_in_%s" % (o, tag), Facts(inside=True, ur1=f32(u1), ur2=f32(u2)), x2=-inside, y2=0.0, octave=o)
            plant(p, "disc_o%d_out_%s" % (o, tag), Facts(inside=False, ur1=f32(u1), ur2=f32(u2)), x2=-outside, y2=0.0, octave=o)
            n_inside += 1
    # mvuRight >= 0 is the test: 0.0 and -0.0 are stereo, NaN and -1e-30 are not
    for j, v in enumerate((0.0, -0.0, np.nan, -1e-30)):
        plant(p, "disc_ur2_%d" % j, Facts(inside=True, ur2=f32(v)), x2=1.0, y2=1.0)
        plant(p, "disc_ur1_%d" % j, Facts(inside=True, ur1=f32(v)), x2=1.0, y2=-1.0)
        n_inside += 2
    mono_mono = (n_inside - 8) // 4 + 4                   # a quarter of the combination probes, and the four special values that are not stereo
    p.counters["disc"] = lambda run: None if run.only_stereo else (n_inside if not run.ur else mono_mono)
    return p.done()


# ---------------------------------------------------------------- distance and ties ----------------------------------------------------------------
DISTANCE_RUNS = (DEFAULT, Run(th_low=0), Run(th_low=256), Run(th_low=-1), Run(th_low=300), Run(th_low=51))


def distance_scene():
    p = Pair("distance", DISTANCE_RUNS, seed=4)
    for d in (0, 1, 50, 51, 52, 255, 256):
        plant(p, "dist_%d" % d, Facts(dist=d))
    return p.done()


def segment(p, node, n, spread=20):
    """n candidates of one node, all within th_low of each other's source: a base descriptor with `spread` bits flipped, each differently"""
    base = p.desc()
    return [p.b(node, flip(base, spread, p.rng)) for _ in range(n)]


def ties_scene():
    """equal smallest distances at list positions p < q: the LAST one wins (:1080 lets an equal distance replace the holder) - q in another
    lane, in the same lane one trip later (q = p + 16), and at 15 / 16 (the last lane of a trip, the first of the next)"""
    p = Pair("ties", (DEFAULT,), seed=5)
    n_equal = 0
    for name, a, b, n in (("other_lane", 0, 1, 20), ("same_lane_next_trip", 0, 16, 20), ("at_15_16", 15, 16, 20), ("far_apart", 3, 35, 40),
                          ("last_two", 31, 32, 33)):
        node = p.new_node()
        cands = segment(p, node, n)
        d1 = p.desc()
        twin = flip(d1, 5, p.rng)
        for pos in (a, b):
            p.k[1][cands[pos]] = p.k[1][cands[pos]][:4] + (twin,) + p.k[1][cands[pos]][5:]
        for pos in range(n):                                # the others are farther, some of them within th_low
            if pos not in (a, b):
                far = flip(d1, 30 + pos % 40, p.rng)
                p.k[1][cands[pos]] = p.k[1][cands[pos]][:4] + (far,) + p.k[1][cands[pos]][5:]
        p.probe("tie_" + name, p.a(node, d1), cands[b])
        n_equal += 1
    # the later of two equals fails the gate: the earlier one wins; and a smaller distance that fails the gate in front of a larger one that passes
    off_line = gate_pair(0)[1]
    node = p.new_node(); d1 = p.desc(); twin = flip(d1, 5, p.rng)
    first = p.b(node, twin); p.b(node, flip(d1, 40, p.rng)); p.b(node, twin, y=off_line)
    p.probe("later_equal_fails_gate", p.a(node, d1), first)
    node = p.new_node(); d1 = p.desc()
    p.b(node, flip(d1, 3, p.rng), y=off_line); second = p.b(node, flip(d1, 20, p.rng))
    p.probe("smaller_fails_gate", p.a(node, d1), second)
    # equals on both sides of a smaller one: the smaller one wins wherever it stands
    node = p.new_node(); d1 = p.desc(); twin = flip(d1, 9, p.rng)
    p.b(node, twin); mid = p.b(node, flip(d1, 8, p.rng)); p.b(node, twin)
    p.probe("smaller_between_equals", p.a(node, d1), mid)
    p.counters["equal"] = lambda run: n_equal
    p.counters["epi"] = lambda run: 2
    return p.done()


# ---------------------------------------------------------------- shapes ----------------------------------------------------------------
def segments_scene():
    """keyframe-2 segments of 1, 15, 16, 17, 32, 33 and 100 candidates; per segment a keyframe-1 feature for the winner at the first, the
    last and the positions 15 and 16 where the segment has them.  Every candidate is within th_low of every one of them."""
    p = Pair("segments", (DEFAULT,), seed=6)
    for n in (1, 15, 16, 17, 32, 33, 100):
        node = p.new_node()
        cands = segment(p, node, n, spread=12)
        for pos in sorted({0, n - 1} | {q for q in (15, 16) if q < n}):
            d1 = flip(p.k[1][cands[pos]][4], 2, p.rng)
            assert all(distance(d1, p.k[1][c][4]) <= 50 for c in cands) and sum(distance(d1, p.k[1][c][4]) <= 2 for c in cands) == 1
            p.probe("segment_%d_winner_%d" % (n, pos), p.a(node, d1), cands[pos])
    return p.done()


def one_node_scene():
    """a single node holds all of keyframe 2"""
    p = Pair("one_node", (DEFAULT,), seed=7)
    node = p.new_node()
    cands = segment(p, node, 100, spread=12)
    for pos in (0, 15, 16, 50, 99):
        p.probe("one_node_winner_%d" % pos, p.a(node, flip(p.k[1][cands[pos]][4], 1, p.rng)), cands[pos])
    return p.done()


def full_scene(n):
    """n features in either keyframe and n FeatureVector entries: M1 = n rows (one, two and three trips of the 64-row loop, a last wave with
    one to three rows) and a capacity of n that is full.  Feature i of keyframe 1 is 3 bits from feature i of keyframe 2 and far from the rest."""
    p = Pair("full_%d" % n, (DEFAULT,), seed=100 + n)
    nodes = [p.new_node() for _ in range(5)]
    for i in range(n):
        d = p.desc()
        p.a(nodes[i % 5], d); p.b(nodes[i % 5], flip(d, 3, p.rng))
    for i in sorted({0, n // 2, n - 1}):
        p.probe("full_%d_feature_%d" % (n, i), i, i)
    s = p.done()
    d12 = POPCOUNT[s["kf1"]["desc"][:, None, :] ^ s["kf2"]["desc"][None, :, :]].sum(2)
    assert (d12 + 1000 * np.eye(n, dtype=int) > 50).all()                               # no other pair is within th_low
    return s


FULL = (1, 3, 15, 16, 17, 63, 64, 65, 100, 130)


def compaction_scene():
    """1025 keypoints in keyframe 1, matches at keypoints 0, 1023 and 1024: the second trip of the output compaction"""
    p = Pair("compaction_1025", (DEFAULT,), seed=8)
    node = p.new_node()
    want = {}
    for i in range(1025):
        d = p.desc()
        if i in (0, 1023, 1024):
            p.a(node, d); want[i] = p.b(node, flip(d, 4, p.rng))
        else:
            p.a(node, d, fv=False)
    for i, m in want.items():
        p.probe("compaction_keypoint_%d" % i, i, m)
    return p.done()


# ---------------------------------------------------------------- octaves ----------------------------------------------------------------
def octaves_scene():
    """keyframe-2 octaves -1, 8 and 255 at nlevels 8: the device is handed them raw and clamps them to the tables, the walk is handed them clipped"""
    p = Pair("octaves", (DEFAULT, COARSE), ep=(0.0, 0.0), seed=9)
    raw = {}
    n_out = 0
    for o_raw, o in ((-1, 0), (8, 7), (255, 7)):
        inside, outside = gate_pair(o)
        for tag, dy, ok in (("in", inside, True), ("out", outside, False)):
            _, i2 = plant(p, "octave_%d_gate_%s" % (o_raw, tag), Facts(gate=ok), x2=500.0, y2=dy, octave=o)
            raw[i2] = o_raw
            n_out += not ok
        d_in, d_out = disc_pair(o) if o else (None, None)
        if o:
            for tag, d, ins in (("in", d_in, True), ("out", d_out, False)):
                _, i2 = plant(p, "octave_%d_disc_%s" % (o_raw, tag), Facts(inside=ins), x2=-d, y2=0.0, octave=o)
                raw[i2] = o_raw
    p.counters["epi"] = lambda run: 0 if run.coarse else n_out
    s = p.done()
    kf2 = dict(s["kf2"], kps=s["kf2"]["kps"].copy())
    for i2, o_raw in raw.items():
        kf2["kps"]["octave"][i2] = o_raw
    s["gpu"] = dict(kf2=kf2)
    return s


# ---------------------------------------------------------------- orientation ----------------------------------------------------------------
def matched(p, angle1, angle2=0.0):
    node = p.new_node()
    d = p.desc()
    i1 = p.a(node, d, angle=angle1)
    return i1, p.b(node, flip(d, 2, p.rng), angle=angle2)


def rotation_scene():
    """rot of exactly 0 (bin 0), 15 (0.5 rounds away from zero: bin 1) and 345 (bin 12), a negative difference that wraps (10 - 350 -> 20: bin 1)
    and angle1 = 0 against the smallest positive angle2 (-tiny + 360 = 360: bin 12).  Three matches each in bins 5 and 7 make the histogram
    (0: 1, 1: 2, 5: 3, 7: 3, 12: 2): bins 5, 7 and 1 stay, so the probes of bins 0 and 12 are removed and those of bin 1 are kept."""
    runs = (DEFAULT, Run(check_orientation=False))
    p = Pair("rotation", runs, seed=10)
    tiny = np.nextafter(f32(0), f32(1))
    for name, a1, a2, stays in (("rot_0", 0.0, 0.0, False), ("rot_15", 15.0, 0.0, True), ("rot_345", 345.0, 0.0, False), ("rot_wraps", 10.0, 350.0, True),
                                ("rot_tiny", 0.0, tiny, False)):
        i1, i2 = matched(p, a1, a2)
        p.probe(name, i1, (lambda run, i2=i2, stays=stays: i2 if stays or not run.check_orientation else -1))
    for a1 in (150.0, 150.0, 150.0, 210.0, 210.0, 210.0):
        i1, i2 = matched(p, a1)
        p.probe("rot_filler_%d_%d" % (int(a1), i1), i1, i2)
    p.counters["removals"] = lambda run: 3 if run.check_orientation else 0
    return p.done()


def histogram_scene(name, counts, kept):
    """counts[j] matches in bin j (rot = 30 j); kept: the bins ComputeThreeMaxima leaves"""
    runs = (DEFAULT, Run(check_orientation=False))
    p = Pair(name, runs, seed=11 + len(counts) + sum(counts))
    for j, c in enumerate(counts):
        for k in range(c):
            i1, i2 = matched(p, 30.0 * j)
            p.probe("%s_bin%d_%d" % (name, j, k), i1, (lambda run, i2=i2, stays=j in kept: i2 if stays or not run.check_orientation else -1))
    p.counters["removals"] = lambda run: sum(c for j, c in enumerate(counts) if j not in kept) if run.check_orientation else 0
    return p.done()


def nothing_scene():
    """common nodes and no match at all (every candidate holds a MapPoint): check_orientation on an empty histogram"""
    p = Pair("nothing", (DEFAULT, COARSE), seed=12)
    for j in range(3):
        node = p.new_node(); d = p.desc()
        i1 = p.a(node, d); p.b(node, d, mp=1); p.b(node, flip(d, 1, p.rng), mp=3)
        p.probe("nothing_%d" % j, i1, -1)
    p.counters["mp"] = lambda run: 6
    return p.done()


# ---------------------------------------------------------------- indices at or above the frame's count, stale counts ----------------------------------------------------------------
POLLUTION = 0xC3


def _without(kf, n):
    """the keyframe as the walk sees it: the first n rows, and the FeatureVector without the entries that name no feature"""
    keep = kf["fv"][1] < n
    return dict(kps=kf["kps"][:n], desc=kf["desc"][:n], mp=kf["mp"][:n], ur=kf["ur"][:n], fv=(kf["fv"][0][keep], kf["fv"][1][keep]))


def phantom_candidate_scene():
    """keyframe 2's FeatureVector names rows N2 and N2 + 1, which the caller's buffers hold (a stale count beside an older FeatureVector): the
    device is handed them, the walk is not.  Row N2 is the probe's twin, row N2 + 1 is the pollution byte throughout, as is another probe's
    descriptor: whatever a form compares an index >= N2 through - the caller's buffer or LDS nobody wrote - a phantom would win."""
    p = Pair("phantom_candidate", (DEFAULT, COARSE), seed=13)
    node = p.new_node()
    d = p.desc()
    polluted = np.full(32, POLLUTION, np.uint8)
    i1 = p.a(node, d); i1p = p.a(node, polluted)
    real = p.b(node, flip(d, 10, p.rng)); realp = p.b(node, flip(polluted, 10, p.rng))
    p.b(node, d); p.b(node, polluted)                     # rows N2 and N2 + 1: distance 0 from the probes
    p.probe("phantom_twin_in_the_buffer", i1, real)
    p.probe("phantom_of_pollution", i1p, realp)
    full = p.done()
    n2 = 2
    s = dict(full, kf2=_without(full["kf2"], n2))
    s["gpu"] = dict(kf2=full["kf2"], nout=(None, n2))
    return s


def phantom_key_scene():
    """keyframe 1's FeatureVector names row N1: searched, it would vote in the rotation histogram (its match is dropped only at the output).
    Real matches (2, 2, 2, 2) in bins 0 .. 3 keep bins 0, 1, 2; one phantom vote in bin 3 would keep 3, 0, 1 instead."""
    p = Pair("phantom_key", (DEFAULT,), seed=14)
    for j in range(4):
        for k in range(2):
            i1, i2 = matched(p, 30.0 * j)
            p.probe("phantom_key_bin%d_%d" % (j, k), i1, i2 if j < 3 else -1)
    n1 = len(p.k[0])
    matched(p, 90.0)                                      # row N1 of keyframe 1 and its partner, a real feature of keyframe 2
    full = p.done()
    s = dict(full, kf1=_without(full["kf1"], n1))
    s["gpu"] = dict(kf1=full["kf1"], nout=(n1, None))
    s["counters"] = dict(removals=lambda run: 2)
    return s


def stale_minus_three_scene(which):
    """a count of -3 reads as 0: d_n_out of keyframe 1 or 2 (no index names a feature) or d_n_feat (no entry): nothing matches"""
    p = Pair("minus_three_" + which, (DEFAULT, COARSE), seed=15)
    for j in range(4):
        i1, _ = matched(p, 0.0)
        p.probe("minus_three_%s_%d" % (which, j), i1, -1)
    full = p.done()
    empty = (np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    if which == "nout1":
        s = dict(full, kf1=dict(full["kf1"], fv=empty)); s["gpu"] = dict(kf1=full["kf1"], nout=(-3, None))
    elif which == "nout2":
        s = dict(full, kf2=dict(full["kf2"], fv=empty)); s["gpu"] = dict(kf2=full["kf2"], nout=(None, -3))
    elif which == "nfeat1":
        s = dict(full, kf1=dict(full["kf1"], fv=empty)); s["gpu"] = dict(kf1=full["kf1"], nfeat=(-3, None))
    else:
        s = dict(full, kf2=dict(full["kf2"], fv=empty)); s["gpu"] = dict(kf2=full["kf2"], nfeat=(None, -3))
    return s


def stale_plus_five_scene(cap):
    """counts of capacity + 5 read as the capacity: a full scene of exactly `cap` features and entries, with all four counts stale"""
    s = dict(full_scene(cap))
    s["name"] = "plus_five_%d" % cap
    s["gpu"] = dict(nout=(cap + 5, cap + 5), nfeat=(cap + 5, cap + 5))
    return s


PLUS_FIVE = (17, 100)


# ---------------------------------------------------------------- the list ----------------------------------------------------------------
def build_all():
    out = [gate_scene("gate", RECT, 1), gate_scene("gate_scaled", RECT * f32(2.0 ** -10), 2)]
    out += [degenerate_gate_scene(k) for k in ("f_zero", "f_inf", "x_nan")]
    out += [disc_scene(), distance_scene(), ties_scene(), segments_scene(), one_node_scene()]
    out += [full_scene(n) for n in FULL] + [compaction_scene(), octaves_scene(), rotation_scene()]
    out += [histogram_scene("hist_one_bin", (6,), (0,)), histogram_scene("hist_kkkk", (2, 2, 2, 2), (0, 1, 2)),
            histogram_scene("hist_20_2_1", (20, 2, 1), (0, 1)), histogram_scene("hist_20_1", (20, 1), (0,)),
            histogram_scene("hist_21_2", (21, 2), (0,)), nothing_scene()]
    out += [phantom_candidate_scene(), phantom_key_scene()] + [stale_minus_three_scene(w) for w in ("nout1", "nout2", "nfeat1", "nfeat2")]
    out += [stale_plus_five_scene(c) for c in PLUS_FIVE]
    assert len({s["name"] for s in out}) == len(out)
    return out


_all = []


def scenes():
    if not _all:
        _all.extend(build_all())
    return _all


def gpu_view(s):
    """the scene as the device is handed it"""
    g = s.get("gpu", {})
    return dict(kf1=g.get("kf1", s["kf1"]), kf2=g.get("kf2", s["kf2"]), F=s["F"], ep=s["ep"])
