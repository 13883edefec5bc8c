"""Scenes for orbx_stereo_fisheye_match_device (tests/test_stereo_fisheye.py, tests/test_stereo_fisheye_gpu.py): fisheye-stereo rigs built as
tests/triangulation_two_eyes_scenes.py builds keyframes (its KannalaBrandt8 pair CAMS, its mTlr with a 10 cm baseline, points 1.5 .. 3.5 m
deep, points at 300 m for the parallax exit, at most 0.3 px of noise), seen by the two eyes of ONE rig: the left eye is the rig's frame, the
right eye mTlr's inverse of it.  Descriptors are CRAFTED to exact Hamming distances: a right row's descriptor is drawn at random (two
such rows are ~128 apart), a left row's is its right partner's with exactly d0 chosen bits flipped, and a second candidate at exactly d1 is
the left row's with d1 bits flipped.  A rig is dict(left, right, mono = (monoLeft, monoRight)), an eye dict(kps, desc); the rows in front of
mono are outside the lapping area and carry descriptors EQUAL to lapping rows of the other eye, so a matcher that did not cut them off
would choose them.

make(seed) is the crafted scene: per rig 20 left x 18 right lapping rows behind 5 / 7 mono rows (capacity 32 per eye), with accepted
pairs, rows the ratio test rejects, two left rows choosing one right row, far points, and four pairs of descriptor partners
DRAWN until the float64 statement of tests/triangulation_two_eyes_scenes.py leaves by z1, z2, the first and the second reprojection
error, clear of every threshold.  Margin condition, as there: a scene serves the float64 comparison when that statement decides every
pair the walk triangulates clear of every threshold (margin_ok).  Of seeds 1 .. 12, 12 satisfy it (true pairs by their 0.3 px noise,
drawn rows by construction); 1, 2 and 3 are used (MARGIN_SEEDS)."""
import math

import numpy as np

import extractorb_amd as X
import triangulation_two_eyes_scenes as S

f32 = np.float32
CAMS, TLR, SIGMA2 = S.CAMS, S.TLR, S.SIGMA2
R12_64, T12_64 = TLR[:, :3].astype(np.float64), TLR[:, 3].astype(np.float64)      # mRlr, mtlr as TriangulateMatches is handed them
MARGIN_SEEDS = (1, 2, 3)
CAP = 32


def flipped(rng, desc, d):
    """desc with exactly d distinct bits flipped"""
    out = desc.copy()
    for b in rng.choice(256, int(d), replace=False):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def random_desc(rng):
    return rng.integers(0, 256, 32, dtype=np.uint8)


def observe(rng, xyz, noise=0.3):
    """((u, v) in the left eye, (u, v) in the right eye) of a point given in the left eye's frame, or None if either eye misses it"""
    (Rl, tl), (Rr, tr) = S.eye_poses64(np.eye(3, 4))
    out = []
    for cam, Pc in ((CAMS[0], Rl @ xyz + tl), (CAMS[1], Rr @ xyz + tr)):
        if Pc[2] < 0.2 or math.atan2(math.hypot(Pc[0], Pc[1]), Pc[2]) > 1.2:
            return None
        u, v = S.project64(cam, Pc)
        if not (15 < u < 497 and 15 < v < 497):
            return None
        a, r = rng.uniform(0, 2 * math.pi), rng.uniform(0, noise)
        out.append((u + r * math.cos(a), v + r * math.sin(a)))
    return out


def point(rng, far=False):
    while True:
        z = 300.0 if far else rng.uniform(1.5, 3.5)
        got = observe(rng, np.array([rng.uniform(-0.6, 0.6) * z, rng.uniform(-0.6, 0.6) * z, z]))
        if got:
            return got


def statement64(left_uv, left_octave, right_uv, right_octave):
    """(accepted, margins) of the float64 statement for a left / right keypoint pair of the rig"""
    return S.triangulate64(CAMS[0], CAMS[1], (f32(left_uv[0]), f32(left_uv[1])), (f32(right_uv[0]), f32(right_uv[1])), R12_64, T12_64,
                           SIGMA2[left_octave], SIGMA2[right_octave])


def drawn_pair(rng, want):
    """(left (u, v), left octave, right (u, v), right octave) of a pair that the float64 statement rejects at `want` ('z1', 'z2', 'error1',
    'error2') clear of every threshold (and of a factor 3 of the gates).  For z1, error1 and error2 the left keypoint observes a near point
    and the right one is drawn around the image.  z2 <= 0 < z1 needs a point in front of the left eye and behind the right one, which the
    nearly parallel eyes allow only within ~1 degree of the left eye's image plane: such a point is drawn, the left keypoint is its
    projection and the right keypoint the projection of its mirror image through the right eye's centre (the ray whose backward extension
    meets it); both lie outside a 512 x 512 image, which the statement does not ask about."""
    R21 = R12_64.T
    t21 = -R21 @ T12_64
    for _ in range(20000):
        lo, ro = int(rng.integers(0, 2)), int(rng.integers(0, 2))
        if want == "z2":
            X = np.array([rng.choice((-1.0, 1.0)) * rng.uniform(0.5, 2.0), rng.uniform(-0.3, 0.3), rng.uniform(0.005, 0.02)])
            X2 = R21 @ X + t21
            if X2[2] > -2e-3:
                continue
            lu, uv = S.project64(CAMS[0], X), S.project64(CAMS[1], -X2)
        else:
            lu = point(rng)[0]
            uv = (rng.uniform(-60, 572), rng.uniform(-60, 572)) if want == "z1" else (lu[0] + rng.uniform(-90, 90), lu[1] + rng.uniform(-90, 90))
            if want == "error2":                          # the error splits about evenly between the eyes: a coarse left octave's gate lets the first pass
                lo, ro = int(rng.integers(5, 8)), 0
                uv = (lu[0] + rng.uniform(-40, 40), lu[1] + rng.uniform(-40, 40))
        ok, mg = statement64(lu, lo, uv, ro)
        if ok or mg[-1][0] != want or not S.margins_hold(mg):
            continue
        if any(thr / 3 <= val <= thr * 3 for n, val, thr in mg if n.startswith("error")):
            continue
        return lu, lo, uv, ro
    raise RuntimeError("no pair leaves by " + want)


def eye(rows):
    """rows: dicts(uv, octave, desc)"""
    n = len(rows)
    kps = np.zeros(n, X.KEYPOINT_DTYPE); desc = np.zeros((n, 32), np.uint8)
    for i, r in enumerate(rows):
        kps["x"][i], kps["y"][i] = r["uv"]
        kps["octave"][i] = r.get("octave", 0); kps["size"][i] = 31.0
        desc[i] = r["desc"]
    return dict(kps=kps, desc=desc)


def with_mono(rng, lefts, rights, mono_left, mono_right):
    """the rig of the lapping rows with mono rows in front: random keypoints whose descriptors EQUAL lapping rows of the other eye"""
    def mono_rows(n, other):
        return [dict(uv=(rng.uniform(20, 490), rng.uniform(20, 490)), octave=int(rng.integers(0, 4)), desc=other[k % len(other)]["desc"].copy())
                for k in range(n)] if other else [dict(uv=(50.0, 50.0), desc=random_desc(rng)) for _ in range(n)]
    return dict(left=eye(mono_rows(mono_left, rights) + lefts), right=eye(mono_rows(mono_right, lefts) + rights), mono=(mono_left, mono_right))


def make_rig(rng, mono_left=5, mono_right=7):
    """the crafted rig: 20 left x 18 right lapping rows.  rig["plan"] lists (kind, left row, right row) in RAW indices."""
    lefts, rights, plan = [], [], []

    def add_pair(kind, d0, far=False, left_octave=None, right_uv=None, right_octave=None):
        (lu, ru) = point(rng, far)
        lo = int(rng.integers(0, 4)) if left_octave is None else left_octave
        if right_uv is not None:
            ru = right_uv
        rd = random_desc(rng)
        rights.append(dict(uv=ru, octave=int(rng.integers(0, 4)) if right_octave is None else right_octave, desc=rd, kind=kind))
        lefts.append(dict(uv=lu, octave=lo, desc=flipped(rng, rd, d0), kind=kind, partner=rights[-1]))
        return lefts[-1], rights[-1]

    for k in range(10):                                   # true pairs: accepted
        add_pair("true", int(rng.integers(0, 26)))
    for k in range(2):                                    # far points: the parallax exit
        add_pair("far", int(rng.integers(0, 10)), far=True)
    for want in ("z1", "z2", "error1", "error2"):         # the descriptor partner is a drawn right row: the other four exits
        lu, lo, ru, ro = drawn_pair(rng, want)
        rd = random_desc(rng)
        rights.append(dict(uv=ru, octave=ro, desc=rd, kind=want))
        lefts.append(dict(uv=lu, octave=lo, desc=flipped(rng, rd, int(rng.integers(0, 10))), kind=want, partner=rights[-1]))
    for k in range(2):                                    # a second left row on the right row of true pair k: two rows choose one
        base = lefts[k]
        a, r = rng.uniform(0, 2 * math.pi), rng.uniform(0, 0.2)
        lefts.append(dict(uv=(base["uv"][0] + r * math.cos(a), base["uv"][1] + r * math.sin(a)), octave=base["octave"],
                          desc=flipped(rng, base["partner"]["desc"], int(rng.integers(0, 20))), kind="shared", partner=base["partner"]))
    lu, ru = point(rng)                                   # rejected by the ratio test: (14, 20), 140 < 140 is false; two left rows carry the descriptor
    ld = random_desc(rng)
    lefts.append(dict(uv=lu, octave=0, desc=ld, kind="ratio", partner=None))
    lefts.append(dict(uv=point(rng)[0], octave=1, desc=ld.copy(), kind="ratio", partner=None))
    rights.append(dict(uv=ru, octave=0, desc=flipped(rng, ld, 14), kind="ratio"))
    rights.append(dict(uv=(rng.uniform(20, 490), rng.uniform(20, 490)), octave=0, desc=flipped(rng, ld, 20), kind="ratio"))
    lo, ro = rng.permutation(len(lefts)), rng.permutation(len(rights))
    lefts = [lefts[i] for i in lo]; rights = [rights[i] for i in ro]
    rig = with_mono(rng, lefts, rights, mono_left, mono_right)
    where = {id(r): j + mono_right for j, r in enumerate(rights)}
    rig["plan"] = [(l["kind"], i + mono_left, where[id(l["partner"])] if l["partner"] is not None else -1) for i, l in enumerate(lefts)]
    return rig


def make(seed, rigs=3):
    rng = np.random.default_rng(seed)
    return dict(cap=CAP, tlr=TLR, cams=CAMS, sigma2=SIGMA2, rigs=[make_rig(rng) for _ in range(rigs)], seed=seed)


def margin_ok(rig, trace):
    """every pair of the walk's trace: the float64 statement decides it clear of every threshold.  Returns (holds, [(accepted64, z64, the test
    it ended at)])"""
    out, holds = [], True
    for i, j, _ok, _z, _why in trace:
        kl, kr = rig["left"]["kps"][i], rig["right"]["kps"][j]
        ok64, mg = statement64((kl["x"], kl["y"]), min(max(int(kl["octave"]), 0), 7), (kr["x"], kr["y"]), min(max(int(kr["octave"]), 0), 7))
        holds = holds and S.margins_hold(mg)
        z = [val for n, val, _ in mg if n == "z1"]
        out.append((ok64, z[0] if z else None, "parallax" if mg[-1][0] == "cos" else mg[-1][0]))
    return holds, out


# ---- small rigs for the rules ----
def edge_rig(rng, candidates, left_octave=0, right_octave=0, left_shift=(0.0, 0.0), lefts=1, mono=(2, 3)):
    """`lefts` left rows observing ONE near point (the first as drawn, the others within 0.2 px; left_shift displaces the LAST of them), and
    one right lapping row per entry of candidates = [(distance to the left rows' descriptor, is the point's right observation)], in that
    order; a right row that is not the observation sits 80 .. 150 px away from it.  All left rows carry one descriptor."""
    lu, ru = point(rng)
    ld = random_desc(rng)
    rights = []
    for d, true in candidates:
        a, r = rng.uniform(0, 2 * math.pi), rng.uniform(80, 150)
        rights.append(dict(uv=ru if true else (ru[0] + r * math.cos(a), ru[1] + r * math.sin(a)), octave=right_octave, desc=flipped(rng, ld, d)))
    rows = []
    for k in range(lefts):
        a, r = rng.uniform(0, 2 * math.pi), (rng.uniform(0, 0.2) if k else 0.0)
        uv = (lu[0] + r * math.cos(a), lu[1] + r * math.sin(a))
        if k == lefts - 1:
            uv = (uv[0] + left_shift[0], uv[1] + left_shift[1])
        rows.append(dict(uv=uv, octave=left_octave, desc=ld.copy()))
    return with_mono(rng, rows, rights, *mono)


def straddle_rig(rng, chunk, best_at, second_at, d0=5, d1=20, tie=False, mono=(3, 4)):
    """chunk + 1 right lapping rows; three left rows observe one point each, their descriptor partner (the point's right observation, at d0)
    at lapping index best_at and a second candidate at d1 (tie: at d0) at second_at; every other right row is random (~128 away).  Only the
    first left row is crafted so; the other two have partners at lapping indices 0 and chunk (the first row of each chunk)."""
    n = chunk + 1
    rights = [dict(uv=(rng.uniform(20, 490), rng.uniform(20, 490)), octave=int(rng.integers(0, 4)), desc=random_desc(rng)) for _ in range(n)]
    lefts = []
    for k, at in enumerate((best_at, 0, chunk)):
        if k and at in (best_at, second_at):
            continue
        lu, ru = point(rng)
        ld = random_desc(rng)
        rights[at] = dict(uv=ru, octave=0, desc=flipped(rng, ld, d0))
        if k == 0:
            rights[second_at] = dict(uv=rights[second_at]["uv"], octave=0, desc=flipped(rng, ld, d0 if tie else d1))
        lefts.append(dict(uv=lu, octave=0, desc=ld))
    return with_mono(rng, lefts, rights, *mono)


def pack(rigs, cap):
    """the batch of the C entry: device frames 2r, 2r + 1 = the eyes of rig r; counts and mono as orbx_extract_batch_device writes them"""
    B = 2 * len(rigs)
    kps = np.zeros((B, cap), X.KEYPOINT_DTYPE); desc = np.zeros((B, cap, 32), np.uint8)
    nout = np.zeros(B, np.int32); mono = np.zeros(B, np.int32)
    for r, rig in enumerate(rigs):
        for e, name in enumerate(("left", "right")):
            n = len(rig[name]["kps"]); f = 2 * r + e
            assert n <= cap, (n, cap)
            kps[f, :n] = rig[name]["kps"]; desc[f, :n] = rig[name]["desc"]
            nout[f] = rig["n_out"][e] if "n_out" in rig else n
            mono[f] = rig["mono"][e]
    return dict(kps=kps, desc=desc, nout=nout, mono=mono)


def make_real(seed, n=1302, rigs=4, mono=(150, 152), true_pairs=800, displaced=150):
    """rigs of n keypoints per eye: true pairs (0 .. 30 bits apart), pairs whose right keypoint is displaced by 1 .. 60 px (rejections of
    every kind, some near a threshold: byte equality only), and rows of random descriptors (~100 from their nearest: the ratio test
    rejects them), shuffled behind the mono rows"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(rigs):
        lefts, rights = [], []
        for k in range(true_pairs + displaced):
            lu, ru = point(rng, far=k % 40 == 0)
            if k >= true_pairs:
                a, r = rng.uniform(0, 2 * math.pi), rng.uniform(1, 60)
                ru = (ru[0] + r * math.cos(a), ru[1] + r * math.sin(a))
            rd = random_desc(rng)
            rights.append(dict(uv=ru, octave=int(rng.integers(0, 8)), desc=rd))
            lefts.append(dict(uv=lu, octave=int(rng.integers(0, 8)), desc=flipped(rng, rd, int(rng.integers(0, 31)))))
        for rows, m in ((lefts, mono[0]), (rights, mono[1])):
            while len(rows) < n - m:
                rows.append(dict(uv=(rng.uniform(20, 490), rng.uniform(20, 490)), octave=int(rng.integers(0, 8)), desc=random_desc(rng)))
        lefts = [lefts[i] for i in rng.permutation(len(lefts))]; rights = [rights[i] for i in rng.permutation(len(rights))]
        out.append(with_mono(rng, lefts, rights, *mono))
    return out
