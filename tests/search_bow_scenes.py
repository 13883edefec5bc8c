"""Crafted scenes for the one-camera ORBmatcher::SearchByBoW overloads (reference src/ORBmatcher.cc:269-471 and :823-963), the statement they
are judged by, and the plausible wrong forms ("mutants") of that statement that the scenes have to tell apart.

A scene is one (keyframe, frame) pair in the layout of test_search_bow.synthetic_pair, built node by node: nodes are independent, so a scene
is a list of small situations, one per vocabulary node, each reaching one branch of the reference's loop.  Every scene carries its own
nnratio and th_low; scenes with equal parameters run in one launch.  docs/history/r25_bow_edges.md lists what each scene reaches."""
import numpy as np

import extractorb_amd as X

MUTANTS = ["ratio_double", "ratio_fused", "th_swapped", "last_position", "second_is_first", "closed_ignored", "maxima_ge", "cut_le", "cut_double",
           "round_even"]


# ---- the statement ----

def _ratio_ok(b1, b2, nnratio, mutant):
    nn = np.float32(nnratio)
    if mutant == "ratio_double":            # (double)nnratio * bestDist2: exact, the product has 33 significant bits at most
        return float(b1) < float(nn) * float(b2)
    if mutant == "ratio_fused":             # fma(nnratio, bestDist2, -bestDist1) > 0: one rounding, of the exact difference
        return np.float32(float(nn) * float(b2) - float(b1)) > 0
    return bool(np.float32(b1) < nn * np.float32(b2))      # :377, :908: the product rounded to binary32, then compared


def three_maxima(cnt, mutant=None):
    """ComputeThreeMaxima (:2303-2344) over the 30 bin sizes"""
    gt = (lambda a, b: a >= b) if mutant == "maxima_ge" else (lambda a, b: a > b)
    m1 = m2 = m3 = 0; i1 = i2 = i3 = -1
    for i, s in enumerate(cnt):
        if gt(s, m1):
            m3, m2, m1, i3, i2, i1 = m2, m1, s, i2, i1, i
        elif gt(s, m2):
            m3, m2, i3, i2 = m2, s, i2, i
        elif gt(s, m3):
            m3, i3 = s, i
    # :2332 is 0.1f * (float)max1 in binary32, which rounds onto max1 / 10 where that is an integer; kept in double the product stays above it.
    # (With the double literal 0.1 the product rounds onto the integer as well: no count tells that form apart, test_search_bow_edges.py checks.)
    cut = float(np.float32(0.1)) * m1 if mutant == "cut_double" else np.float32(0.1) * np.float32(m1)
    below = (lambda a: a <= cut) if mutant == "cut_le" else (lambda a: a < cut)
    if below(m2):
        i2 = i3 = -1
    elif below(m3):
        i3 = -1
    return i1, i2, i3


def rotation_bin(angle_k, angle_f, mutant=None):
    rot = np.float32(angle_k) - np.float32(angle_f)
    if rot < 0:
        rot = np.float32(rot + np.float32(360.0))
    x = float(np.float32(rot * np.float32(1.0 / 30)))
    return int(np.rint(x) if mutant == "round_even" else np.floor(x + 0.5)) % 30


def statement(p, nnratio, th_low, check, keyframes=False, mutant=None):
    """Both overloads, per node: the frame overload returns matches[frame keypoint] = keyframe keypoint, the keyframe overload
    matches12[first keyframe's keypoint] = second keyframe's keypoint, and closes the second keyframe's keypoints whose flags2 bit 0 is clear."""
    (kn, ki), (fn, fi) = p["fv_k"], p["fv_f"]
    bits_k = np.unpackbits(p["dk"], axis=1).astype(np.int16); bits_f = np.unpackbits(p["df"], axis=1).astype(np.int16)
    flags2 = p.get("flags2") if keyframes else None
    taken = np.full(len(p["df"]), -1, np.int64)
    bins = {}
    strict = keyframes != (mutant == "th_swapped")          # :906 is "<", :375 is "<="
    for node in sorted(set(kn.tolist()) & set(fn.tolist())):
        fs = fi[fn == node]
        for k in ki[kn == node]:
            if not p["flags"][k] & 1:
                continue
            if mutant == "closed_ignored":
                free = [int(f) for f in fs]
            else:
                free = [int(f) for f in fs if taken[f] < 0 and (flags2 is None or flags2[f] & 1)]
            if not free:
                continue
            dist = np.abs(bits_f[free] - bits_k[k]).sum(1)
            b1 = int(dist.min())
            at = np.nonzero(dist == b1)[0]
            pos = int(at[-1] if mutant == "last_position" else at[0])
            b2 = int(np.sort(dist)[1]) if len(free) > 1 else (b1 if mutant == "second_is_first" else 256)
            if (b1 < th_low if strict else b1 <= th_low) and _ratio_ok(b1, b2, nnratio, mutant):
                f = free[pos]
                taken[f] = k
                bins[f] = rotation_bin(p["kps_k"]["angle"][k], p["kps_f"]["angle"][f], mutant)
    if check:
        keep = three_maxima([sum(1 for b in bins.values() if b == i) for i in range(30)], mutant)
        for f, b in bins.items():
            if b not in keep:
                taken[f] = -1
    if not keyframes:
        return int((taken >= 0).sum()), taken
    m12 = np.full(len(p["dk"]), -1, np.int64)
    for f in np.nonzero(taken >= 0)[0]:
        m12[taken[f]] = f
    return int((m12 >= 0).sum()), m12


def ratio_disagreements(nnratio):
    """the (bestDist1, bestDist2) in 0..256 on which the binary32 product of :377 and a double product decide differently"""
    nn = np.float32(nnratio)
    b1, b2 = np.meshgrid(np.arange(257), np.arange(257), indexing="ij")
    single = b1.astype(np.float32) < nn * b2.astype(np.float32)
    assert (nn * b2.astype(np.float32)).dtype == np.float32
    double = b1.astype(np.float64) < np.float64(nn) * b2.astype(np.float64)
    return [(int(a), int(b)) for a, b in zip(*np.nonzero(single != double))], single, double


# ---- building a pair node by node ----

def pattern(n, start=0):
    """a descriptor with n bits set from bit `start` on"""
    b = np.zeros(256, np.uint8)
    b[start:start + n] = 1
    assert start + n <= 256
    return np.packbits(b)


class Pair:
    def __init__(self, name, nnratio, th_low, seed=0):
        self.name, self.nnratio, self.th_low = name, nnratio, th_low
        self.rng = np.random.default_rng(seed)
        self.dk, self.df, self.ak, self.af, self.flags, self.flags2, self.nk, self.nf = [], [], [], [], [], [], [], []
        self.expect = {False: {}, True: {}}       # overload (keyframes?) -> keyframe keypoint -> frame keypoint or -1, where the scene's text says so
        self.n_nodes = 0

    def node(self, kf, fr):
        """kf, fr: lists of (pattern, angle, flag); the patterns are XORed onto one random descriptor of the node.  Node ids are scattered, so
        the FeatureVector's node order is not the order of the keypoint indices.  Returns the keypoint indices (keyframe's, frame's)."""
        nid = 3 + (self.n_nodes * 7919 + 11) % 10007 * 5
        self.n_nodes += 1
        base = self.rng.integers(0, 256, 32, dtype=np.uint8)
        ks, fs = [], []
        for pat, angle, flag in kf:
            ks.append(len(self.dk)); self.dk.append(base ^ pat); self.ak.append(angle); self.flags.append(flag); self.nk.append(nid)
        for pat, angle, flag in fr:
            fs.append(len(self.df)); self.df.append(base ^ pat); self.af.append(angle); self.flags2.append(flag); self.nf.append(nid)
        return ks, fs

    def build(self):
        def fv(node):
            node = np.array(node, np.uint32)
            order = np.lexsort((np.arange(len(node)), node))
            return node[order], order.astype(np.uint32)
        kps_k = np.zeros(len(self.dk), X.KEYPOINT_DTYPE); kps_f = np.zeros(len(self.df), X.KEYPOINT_DTYPE)
        kps_k["angle"] = np.array(self.ak, np.float32); kps_f["angle"] = np.array(self.af, np.float32)
        assert max(len(self.dk), len(self.df)) < 300, self.name      # a scene embeds in any capacity
        return dict(name=self.name, nnratio=self.nnratio, th_low=self.th_low, dk=np.array(self.dk, np.uint8).reshape(-1, 32),
                    df=np.array(self.df, np.uint8).reshape(-1, 32), fv_k=fv(self.nk), fv_f=fv(self.nf), kps_k=kps_k, kps_f=kps_f,
                    flags=np.array(self.flags, np.uint8) | 2, flags2=np.array(self.flags2, np.uint8) | 4, expect=self.expect)      # upper flag bits are noise


def _pad(n):
    return (pattern(n), 0.0, 1)


def ratio_rounding(nnratio, th_low=100):
    """One node per enumerated (b1, b2) with b1 under th_low: a keyframe feature and exactly two frame features at those distances, where the
    binary32 product rejects and a double or fused product accepts; beside it a node with (b1 - 1, b2), which every form accepts."""
    p = Pair("ratio_rounding_%g" % nnratio, nnratio, th_low, seed=int(nnratio * 100))
    pairs, single, _ = ratio_disagreements(nnratio)
    for j, (b1, b2) in enumerate((a, b) for a, b in pairs if 1 <= a < th_low):
        assert not single[b1, b2] and single[b1 - 1, b2] and b1 < b2
        for d, hit in ((b1, False), (b1 - 1, True)):
            two = [(pattern(d), 0.0, 1), (pattern(b2, 256 - b2), 0.0, 1)]
            ks, fs = p.node([(pattern(0), 0.0, 1)], two[::-1] if j & 1 else two)      # the nearer one first, or second
            want = (fs[1] if j & 1 else fs[0]) if hit else -1
            p.expect[False][ks[0]] = want; p.expect[True][ks[0]] = want
    return p.build()


def th_low_boundary(th_low=50):
    """single-candidate nodes (bestDist2 = 256) at th_low - 1, th_low, th_low + 1: th_low itself matches under :375's "<=" and not under :906's "<" """
    p = Pair("th_low_boundary", 0.7, th_low, seed=1)
    for d in (th_low - 1, th_low, th_low + 1):
        ks, fs = p.node([_pad(0)], [_pad(d)])
        p.expect[False][ks[0]] = fs[0] if d <= th_low else -1
        p.expect[True][ks[0]] = fs[0] if d < th_low else -1
    return p.build()


def single_candidate_ratio():
    """th_low = 200, nnratio = 0.7, one free candidate: 0.7f * 256 decides between 179 and 180.  A second node has two candidates of which the
    nearer is closed by an earlier keyframe feature of the node, so the single one is single only because of the closing."""
    p = Pair("single_candidate_ratio", 0.7, 200, seed=2)
    for d in (179, 180):
        p.node([_pad(0)], [_pad(d)])
        p.node([_pad(0), (pattern(2, 200), 0.0, 1)], [_pad(0), (pattern(d - 2, 0), 0.0, 1)])      # second keyframe feature: d against 256
    return p.build()


FIRST_POSITION_LENGTHS = [(1, 15, 16, 17), (32,), (33,), (100,)]      # the segment lengths of one scene (a scene stays under 300 keypoints)
FIRST_POSITION_PLACES = [(0, 16), (3, 19), (7, 8), (14, 15), (15, 16), (0, 15), (16, 31), (31, 32)]


def first_position(nnratio, lengths):
    """Frame segments of every length around the 16 lanes of a row, the smallest distance planted twice or three times: in one lane (p, p + 16),
    in neighbouring lanes, in the first and the last lane.  With nnratio = 1.5 equal distances are accepted and the smallest position must be
    chosen; with 0.7 the same nodes are rejected unless the smallest is alone, which shows bestDist2 == bestDist1."""
    p = Pair("first_position_%g_%s" % (nnratio, "_".join(map(str, lengths))), nnratio, 50, seed=3)
    for n in lengths:
        chosen = [(5, 90, 99), (1, 17, 33)] if n == 100 else [pl for pl in FIRST_POSITION_PLACES if pl[-1] < n] + [(n - 1,)]
        for places in chosen:
            fr = [(pattern(5, (7 * i) % 200) if i in places else pattern(20 + i % 7, (11 * i) % 200), 0.0, 1) for i in range(n)]
            ks, fs = p.node([_pad(0)], fr)
            want = fs[places[0]] if nnratio > 1 or len(places) == 1 else -1
            p.expect[False][ks[0]] = want; p.expect[True][ks[0]] = want
    return p.build()


def chains(nnratio):
    """K keyframe features that all have the same nearest frame feature: keyframe feature j is j bits from it and j + h[i] bits from frame feature
    i.  Each accepted one closes its match for the next; more keyframe features than frame features leave the late ones nothing free
    (bestDist1 = 256).  Some keyframe features hold no MapPoint, and in the keyframe overload some frame features are closed from the start,
    the nearest among them."""
    p = Pair("chains_%g" % nnratio, nnratio, 50, seed=4)
    geometric = [0, 2, 6, 16, 40, 100]
    for K, n_f, closed in ((2, 5, ()), (17, 20, ()), (40, 21, ()), (17, 3, ()), (17, 20, (0,)), (17, 20, (0, 2)), (40, 6, (0, 1)), (2, 2, (0, 1))):
        h = list(range(n_f)) if nnratio > 1 else (geometric + list(range(101, 120)))[:n_f]
        kf = [(pattern(j), 0.0, int(j != 5)) for j in range(1, K + 1)]
        fr = [(pattern(h[i], 128), 0.0, int(i not in closed)) for i in range(n_f)]
        p.node(kf, fr)
    return p.build()


def _angles(rot, wrap):
    """(keyframe angle, frame angle) whose difference lands at rot: directly, or as a negative difference that wraps"""
    if not wrap:
        return np.float32(rot + 2.0), np.float32(2.0)
    return np.float32(rot - 3.0), np.float32(357.0)         # rot - 360 < 0, then + 360


def histogram_counts(name, counts, far=0):
    """matches at distance 0 (always accepted), counts[bin] of them at rot = 30 * bin + 3; `far` more nodes whose only candidate is beyond th_low"""
    p = Pair(name, 0.7, 50, seed=len(name))
    j = 0
    for b, c in counts.items():
        for _ in range(c):
            ak, af = _angles(30.0 * b + 3.0, j % 3 == 1)
            p.node([(pattern(0), ak, 1)], [(pattern(0), af, 1)])
            j += 1
    for _ in range(far):
        p.node([_pad(0)], [_pad(60)])
    return p.build()


# (keyframe angle, frame angle, copies): rot * (1 / 30) is rounded with rot in [0, 360], so only bins 0 ... 12 are reachable; the values on the
# edges: 0, 15 (x = 0.5: up, to even it would be 0), 75 (2.5), 345 (11.5), the last float below 360 and 360 itself (12), met directly and as a
# negative difference that wraps (-3e-5 + 360 is the last float below 360, -1e-6 + 360 rounds to 360)
EDGE_ANGLES = [(0.0, 0.0, 2), (10.0, 10.0, 1), (123.5, 123.5, 1), (15.0, 0.0, 2), (0.0, 345.0, 1), (5.0, 350.0, 1), (75.0, 0.0, 1), (1.0, 286.0, 1),
               (345.0, 0.0, 1), (0.0, 15.0, 1), (float(np.nextafter(np.float32(360), np.float32(0))), 0.0, 1), (0.0, 3e-5, 1), (0.0, 1e-6, 1),
               (float(np.nextafter(np.float32(15), np.float32(0))), 0.0, 1), (float(np.nextafter(np.float32(15), np.float32(20))), 0.0, 1)]


def histogram_edges():
    p = Pair("histogram_edges", 0.7, 50, seed=6)
    for ak, af, copies in EDGE_ANGLES:
        for _ in range(copies):
            p.node([(pattern(0), np.float32(ak), 1)], [(pattern(0), np.float32(af), 1)])
    return p.build()


def degenerate_pairs(normal):
    """an empty keyframe FeatureVector, an empty frame FeatureVector, no common node, no MapPoint at all, no keypoints in either frame, beside
    a normal pair"""
    def variant(name, **change):
        q = dict(normal, name=name, expect={False: {}, True: {}}, nnratio=0.7, th_low=50)
        q.update(change)
        return q
    e = (np.zeros(0, np.uint32), np.zeros(0, np.uint32))
    nk, nf = len(normal["dk"]), len(normal["df"])
    none_k = dict(dk=np.zeros((0, 32), np.uint8), kps_k=np.zeros(0, X.KEYPOINT_DTYPE), fv_k=e, flags=np.zeros(0, np.uint8))
    none_f = dict(df=np.zeros((0, 32), np.uint8), kps_f=np.zeros(0, X.KEYPOINT_DTYPE), fv_f=e, flags2=np.zeros(0, np.uint8))
    return [variant("normal"), variant("empty_keyframe_fv", fv_k=e), variant("empty_frame_fv", fv_f=e),
            variant("no_common_node", fv_f=(normal["fv_f"][0] + np.uint32(1), normal["fv_f"][1])),
            variant("no_map_points", flags=np.full(nk, 2, np.uint8)), variant("second_all_closed", flags2=np.full(nf, 4, np.uint8)),
            variant("no_keyframe_keypoints", **none_k), variant("no_frame_keypoints", **none_f), variant("normal_again")]


def crafted_scenes():
    """every scene of the issue's section 2, in a fixed order"""
    from test_search_bow import synthetic_pair
    normal = dict(synthetic_pair(np.random.default_rng(77), 120, 150, 9), flags2=(np.random.default_rng(78).random(150) < 0.7).astype(np.uint8))
    s = [ratio_rounding(0.8), ratio_rounding(0.6), th_low_boundary(), single_candidate_ratio()]
    s += [first_position(nn, lengths) for nn in (1.5, 0.7) for lengths in FIRST_POSITION_LENGTHS]
    s += [chains(1.5), chains(0.7), histogram_edges(),
         histogram_counts("hist_10_1_1", {4: 10, 1: 1, 9: 1}), histogram_counts("hist_11_1_1", {4: 11, 1: 1, 9: 1}),
         histogram_counts("hist_30_3_3", {3: 30, 0: 3, 8: 3}), histogram_counts("hist_four_tens", {2: 10, 5: 10, 7: 10, 11: 10}),
         histogram_counts("hist_one_bin", {6: 5}), histogram_counts("hist_no_matches", {}, far=4)]
    return s + degenerate_pairs(normal)


def groups(scenes):
    """scenes of equal (nnratio, th_low) run in one launch"""
    g = {}
    for s in scenes:
        g.setdefault((s["nnratio"], s["th_low"]), []).append(s)
    return g


# ---- capacities (extractorb_amd/csrc/k_bow_match.hip: bowMatchLdsBytes, launchSearchBow; the entry's bound in orbx_rows.cpp) ----

def lds_bytes(capacity, staged):
    return (capacity + 15) // 16 * 16 * (4 + 4 + 4 + 4 + 1 + 2 + 2 + 1 + (64 if staged else 0)) + 64


def is_staged(capacity):
    return lds_bytes(capacity, True) <= 150 * 1024


def is_accepted(capacity):
    return capacity <= 65535 and lds_bytes(capacity, False) <= 150 * 1024


CAPACITIES = [1024, 1776, 1777, 1781, 6976]


# ---- the device ----

def run_device(ex, frames, pair_flags, pair_flags2, kf_walk, cur_walk, n_pairs, nnratio, th_low, check, cap, keyframes, poison=-7):
    """frames: [(desc, kps, (fv nodes, fv idx))] in batch order; pair_flags[p] / pair_flags2[p]: the flags of pair p's keyframe / frame.
    Returns (n_matches[n_pairs], matches[n_pairs, cap]); the outputs are pre-filled with `poison`."""
    import torch
    B = len(frames)
    desc = np.zeros((B, cap, 32), np.uint8); kps = np.zeros((B, cap), X.KEYPOINT_DTYPE)
    fn = np.zeros((B, cap), np.uint32); fi = np.zeros((B, cap), np.uint32)
    nfeat = np.zeros(B, np.int32); nout = np.zeros(B, np.int32)
    flags = np.zeros((n_pairs, cap), np.uint8); flags2 = np.zeros((n_pairs, cap), np.uint8)
    for f, (d, k, fv) in enumerate(frames):
        desc[f, :len(d)] = d; kps[f, :len(k)] = k; nout[f] = len(d)
        fn[f, :len(fv[0])] = fv[0]; fi[f, :len(fv[1])] = fv[1]; nfeat[f] = len(fv[0])
    for i in range(n_pairs):
        flags[i, :len(pair_flags[i])] = pair_flags[i]; flags2[i, :len(pair_flags2[i])] = pair_flags2[i]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8) if a.dtype.fields else np.ascontiguousarray(a)).cuda()
    d_m = torch.full((n_pairs, cap), poison, dtype=torch.int32, device="cuda"); d_nm = torch.full((n_pairs,), poison, dtype=torch.int32, device="cuda")
    head = (n_pairs, kf_walk, cur_walk, dev(fn.view(np.int32)), dev(fi.view(np.int32)), dev(nfeat), dev(flags))
    tail = (dev(kps), dev(desc), dev(nout), cap, d_m, d_nm)
    if keyframes:
        ex.search_by_bow_keyframes_device(*head, dev(flags2), *tail, nnratio=nnratio, th_low=th_low, check_orientation=check)
    else:
        ex.search_by_bow_device(*head, *tail, nnratio=nnratio, th_low=th_low, check_orientation=check)
    ex.synchronize()
    return d_nm.cpu().numpy(), d_m.cpu().numpy()


def run_pairs(ex, pairs, nnratio, th_low, check, cap, keyframes):
    """the interleaved walk: frames 2p = keyframe, 2p + 1 = frame of pair p"""
    frames = []
    for p in pairs:
        frames += [(p["dk"], p["kps_k"], p["fv_k"]), (p["df"], p["kps_f"], p["fv_f"])]
    return run_device(ex, frames, [p["flags"] for p in pairs], [p["flags2"] for p in pairs], (0, 2), (1, 2), len(pairs), nnratio, th_low, check, cap,
                      keyframes)


def oracle(p, nnratio, th_low, check, keyframes):
    import oracle_lib as O
    if keyframes:
        return O.search_by_bow_keyframes(p["fv_k"], p["fv_f"], p["flags"], p["flags2"], p["kps_k"], p["dk"], p["kps_f"], p["df"], nnratio, th_low, check)
    return O.search_by_bow(p["fv_k"], p["fv_f"], p["flags"], p["kps_k"], p["dk"], p["kps_f"], p["df"], nnratio, th_low, check)
