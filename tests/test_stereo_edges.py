"""Frame::ComputeStereoMatches (reference src/Frame.cc:813-991) at its edges: the oracle against the independent statement of
tests/stereo_statement.py byte for byte, crafted scenes that are ASSERTED to reach every exit of the function, and liborbx's
k_stereo_rows / k_stereo_match / k_stereo_filter against the oracle on those scenes, other frame shapes, pyramids and capacities.

A scene is (the two images, the extractor's parameters, keypoint and descriptor arrays the test edits, bf, b): the entries read only the
pyramids from the handle and take the caller's arrays.  Rule for the edits: a left keypoint that reaches the window reads keeps
0 <= round(x * inv) <= w_l - 1 and 0 <= round(y * inv) <= h_l - 1 at its level, and octaves stay inside [0, nlevels) (check_rule)."""
import functools
import json
import os
import re

import numpy as np
import pytest

import helpers
import oracle_lib as O
import extractorb_amd as X
import stereo_statement as S
from test_stereo import stereo_pair

LDS_LIMIT = 160 * 1024 - 512
POISON = np.float32(-777.25)
FLIPS = (0, 40, 74, 75, 99, 100, 120)
DEFAULT = dict(nf=1200, sf=1.2, nl=8)


def filter_lds_bytes(capacity, static=None):
    """include/orbx.h: the dynamic block of k_stereo_filter plus its static one"""
    return 4 * ((capacity + 3) & ~3) + (header_static_lds() if static is None else static)


def header_static_lds():
    text = open(X.orbextractor._HEADER).read()
    return int(re.search(r"#define\s+ORBX_STEREO_FILTER_STATIC_LDS_BYTES\s+(\d+)", text).group(1))


# ---------------------------------------------------------------- scenes ----------------------------------------------------------------
def extract(left, right, nf=1200, sf=1.2, nl=8):
    oL, oR = O.Oracle(nf, sf, nl), O.Oracle(nf, sf, nl)
    _, kL, dL = oL.extract(left, (0, 0))
    _, kR, dR = oR.extract(right, (0, 0))
    return dict(left=left, right=right, nf=nf, sf=sf, nl=nl, oL=oL, oR=oR, kL=kL, dL=dL, kR=kR, dR=dR, bf=40.0, b=0.1)


def edited(s, **changes):
    out = dict(s)
    for k in ("kL", "dL", "kR", "dR"):
        out[k] = s[k].copy()
    out.update(changes)
    return out


def statement(s):
    return S.stereo_statement(s["oL"], s["oR"], s["kL"], s["dL"], s["kR"], s["dR"], s["bf"], s["b"])


def oracle(s):
    return O.stereo_match(s["oL"], s["oR"], s["kL"], s["dL"], s["kR"], s["dR"], s["bf"], s["b"])


def flipped(desc, n, rng):
    bits = np.unpackbits(desc)
    bits[rng.choice(256, n, replace=False)] ^= 1
    return np.packbits(bits)


def partners(base_res):
    """(left index, right index) of the matches of the unedited scene, each right index once"""
    seen, out = set(), []
    for i in np.flatnonzero(base_res["sad"] >= 0).tolist():
        j = int(base_res["best_r"][i])
        if j not in seen:
            seen.add(j); out.append((i, j))
    return out


def append(k, d, new_k, new_d):
    return np.concatenate([k, np.asarray(new_k, k.dtype)]), np.concatenate([d, np.asarray(new_d, np.uint8).reshape(-1, 32)])


def coordinate_rounding_to(target, level, s):
    """a binary32 coordinate whose scaled value rounds (half away from zero) to `target` at `level`"""
    x = np.float32(np.float32(target) * s["oL"].scale_factors[level])
    assert S.round_half_away(np.float32(x * s["oL"].inv_scale_factors[level])) == target
    return x


def check_rule(s):
    kL, oL = s["kL"], s["oL"]
    assert ((kL["octave"] >= 0) & (kL["octave"] < s["nl"])).all() and ((s["kR"]["octave"] >= 0) & (s["kR"]["octave"] < s["nl"])).all()
    for i in range(len(kL)):
        if kL["x"][i] < 0:
            continue                                     # leaves at maxU < 0, before any read
        l = int(kL["octave"][i]); w, h = oL.level_size(l); inv = oL.inv_scale_factors[l]
        assert 0 <= S.round_half_away(np.float32(kL["x"][i] * inv)) <= w - 1, i
        assert 0 <= S.round_half_away(np.float32(kL["y"][i] * inv)) <= h - 1, i


@functools.lru_cache(maxsize=None)
def base(seed=77, rows=480, cols=640, nf=1200, sf=1.2, nl=8, variant="textured"):
    """the extractor's output on a noisy pair of disparity 12 (the median is not 0), and the statement's walk over it"""
    left, right = stereo_pair(12, seed=seed, rows=rows, cols=cols, variant=variant, noise=3)
    s = extract(left, right, nf, sf, nl)
    s["key"] = (seed, rows, cols, nf, sf, nl, variant)
    return s


@functools.lru_cache(maxsize=None)
def base_walk(key):
    """the statement's walk over an unedited scene: where its matches are, for the edits"""
    return statement(base(*key))


def ties(s0, seed):
    """thresholds + ties + order: partners' descriptors at exact distances around 75 and 100, duplicated right keypoints (at the same place and a few
    pixels away, so WHICH holder of the best distance is taken shows in uRight), the right eye permuted"""
    rng = np.random.default_rng(seed + 1)
    s = edited(s0)
    pr = partners(base_walk(s0["key"]))
    for n, (i, j) in enumerate(pr[:len(pr) // 2]):
        s["dR"][j] = flipped(s["dL"][i], FLIPS[n % len(FLIPS)], rng)
    for n, (i, j) in enumerate(pr[len(pr) // 2:][:80]):      # partners 5 level pixels off: the SAD minimum lies at the end of the range; 4: just inside
        s["kR"]["x"][j] += np.float32((5, -5, 4, -4)[n % 4]) * s["oL"].scale_factors[int(s["kL"]["octave"][i])]
    pick = rng.choice(len(s["kR"]), min(300, len(s["kR"])), replace=False)
    dup = s["kR"][pick].copy()
    apart = np.arange(len(pick)) >= len(pick) // 3
    dup["x"][apart] += (rng.choice([-3, -2, -1, 1, 2, 3], apart.sum()) * s["oL"].scale_factors[dup["octave"][apart]]).astype(np.float32)
    s["kR"], s["dR"] = append(s["kR"], s["dR"], dup, s["dR"][pick])
    perm = rng.permutation(len(s["kR"]))
    s["kR"], s["dR"] = s["kR"][perm], s["dR"][perm]
    return s


def gates(s0, seed):
    """maxD = 12.5 cuts through the true disparity of 12; partners exactly on and one ulp outside minU and maxU; partner octaves levelL +-1, +-2"""
    s = edited(s0, bf=6.25, b=0.5)
    max_d = np.float32(np.float32(6.25) / np.float32(0.5))
    pr = partners(base_walk(s0["key"]))
    for n, (i, j) in enumerate(pr[:120]):
        uL, lvl, kind = s["kL"]["x"][i], int(s["kL"]["octave"][i]), n % 8
        min_u = np.float32(uL - max_d)
        if kind == 0: s["kR"]["x"][j] = min_u
        elif kind == 1: s["kR"]["x"][j] = np.nextafter(min_u, np.float32(-1e9))
        elif kind == 2: s["kR"]["x"][j] = uL
        elif kind == 3: s["kR"]["x"][j] = np.nextafter(uL, np.float32(1e9))
        else:
            o = lvl + (-1, 1, -2, 2)[kind - 4]
            if 0 <= o < s["nl"]:
                s["kR"]["octave"][j] = o
    return s


def borders(s0, seed):
    """right keypoints whose scaled column is w_l - 12 (inside), w_l - 11 and w_l - 1 (endu >= cols) and -1 (iniu < 0), each on the row and octave and
    with the descriptor of a left feature; left keypoints at x = -1 (maxU < 0); keypoints of every octave in the first and last four rows"""
    rng = np.random.default_rng(seed + 2)
    s = edited(s0)
    rows = s["left"].shape[0]
    pr = partners(base_walk(s0["key"]))
    newL, newLd, newR, newRd = [], [], [], []
    n = 0
    for at in (-12, -11, -1):                            # round(uR * inv) = w_l + at
        for _ in range(8):
            i = pr[n][0]; n += 1
            l = int(s["kL"]["octave"][i]); w = s["oL"].level_size(l)[0]
            kl = s["kL"][i].copy(); kl["x"] = coordinate_rounding_to(w - 1, l, s)      # far enough right that uR <= uL
            kr = kl.copy(); kr["x"] = coordinate_rounding_to(w + at, l, s)
            newL.append(kl); newLd.append(s["dL"][i]); newR.append(kr); newRd.append(s["dL"][i])
    for _ in range(8):                                   # iniu < 0: uL below maxD = 400, so minU <= uR
        while s["kL"]["x"][pr[n][0]] > 390: n += 1
        i = pr[n][0]; n += 1
        l = int(s["kL"]["octave"][i])
        kr = s["kL"][i].copy(); kr["x"] = np.float32(-0.6) * s["oL"].scale_factors[l]
        assert S.round_half_away(np.float32(kr["x"] * s["oL"].inv_scale_factors[l])) == -1
        newR.append(kr); newRd.append(s["dL"][i])
    for _ in range(8):                                   # maxU < 0
        i = pr[n][0]; n += 1
        kl = s["kL"][i].copy(); kl["x"] = -1.0
        newL.append(kl); newLd.append(s["dL"][i])
    for l in range(s["nl"]):                             # bands clamped at the first and the last row
        w, h = s["oL"].level_size(l); inv = s["oL"].inv_scale_factors[l]
        for y in (0, 1, 2, 3, rows - 4, rows - 3, rows - 2, rows - 1):
            if not 0 <= S.round_half_away(np.float32(np.float32(y) * inv)) <= h - 1:
                continue
            i = pr[n % len(pr)][0]; n += 1
            d = rng.integers(0, 256, 32, dtype=np.uint8)
            kl = s["kL"][i].copy(); kl["octave"] = l; kl["y"] = y; kl["x"] = coordinate_rounding_to(int(rng.integers(w // 3, w - 20)), l, s)
            kr = kl.copy(); kr["x"] = np.float32(kl["x"] - np.float32(12)); kr["y"] = np.float32(y + (rng.integers(0, 3) - 1) * (0 < y < rows - 1))
            newL.append(kl); newLd.append(d); newR.append(kr); newRd.append(flipped(d, int(rng.integers(0, 30)), rng))
    s["kL"], s["dL"] = append(s["kL"], s["dL"], newL, newLd)
    s["kR"], s["dR"] = append(s["kR"], s["dR"], newR, newRd)
    return s


def stripe(s0, seed):
    """no right keypoint's band touches rows 200-260: the left keypoints there meet an empty candidate list"""
    s = edited(s0)
    r = 2.0 * s["oR"].scale_factors[s["kR"]["octave"]]
    keep = (np.ceil(s["kR"]["y"] + r) < 199) | (np.floor(s["kR"]["y"] - r) > 261)
    s["kR"], s["dR"] = s["kR"][keep], s["dR"][keep]
    return s


def zero(seed, n_patches=10):
    """disparity exactly 0: identical patches in both eyes, mirror images about a centre column c, with a level-0 keypoint at (c, y) in both eyes and
    equal descriptors.  SAD(+s) = SAD(-s), the first minimum is shift 0 with SAD 0, deltaR = 0, disparity = 0 -> 0.01 and uL - 0.01 in double.  The noisy
    scene around keeps the median positive, so these matches survive the filter."""
    rng = np.random.default_rng(seed + 3)
    left, right = stereo_pair(12, seed=seed, noise=3)
    left, right = left.copy(), right.copy()
    spots = []
    for p in range(n_patches):
        y, c = 40 + 40 * p, int(rng.integers(60, 580))
        half = rng.integers(0, 256, (17, 17), dtype=np.uint8)                 # columns c .. c + 16
        patch = np.concatenate([half[:, :0:-1], half], axis=1)               # columns c - 16 .. c + 16, mirrored about c
        left[y - 8:y + 9, c - 16:c + 17] = patch; right[y - 8:y + 9, c - 16:c + 17] = patch
        spots.append((c, y))
    s = extract(left, right)
    new, newd = [], []
    for c, y in spots:
        k = s["kL"][0].copy(); k["x"] = c; k["y"] = y; k["octave"] = 0; k["angle"] = 0
        new.append(k); newd.append(rng.integers(0, 256, 32, dtype=np.uint8))
    s["kL"], s["dL"] = append(s["kL"], s["dL"], new, newd)
    s["kR"], s["dR"] = append(s["kR"], s["dR"], new, newd)
    s["n_zero"] = n_patches
    return s


def cut_to_matches(s0, m):
    """exactly m pre-filter matches (a left keypoint's walk does not depend on the other left keypoints) beside 40 unmatched ones"""
    sad = base_walk(s0["key"])["sad"]
    pick = np.sort(np.concatenate([np.flatnonzero(sad > 0)[:m], np.flatnonzero(sad < 0)[:40]]))
    return edited(s0, kL=s0["kL"][pick], dL=s0["dL"][pick])


def same_sad(s0):
    """six copies of one matched left keypoint: every match has the same SAD, the median is that value and 2.1 * median keeps them all"""
    i = int(np.flatnonzero(base_walk(s0["key"])["sad"] > 0)[5])
    pick = np.array([i] * 6 + np.flatnonzero(base_walk(s0["key"])["sad"] < 0)[:10].tolist())
    return edited(s0, kL=s0["kL"][pick], dL=s0["dL"][pick])


@functools.lru_cache(maxsize=None)
def median_zero():
    """the noise-free pair of disparity 0: every match has SAD 0, the median is 0, `0 < 0` fails and nothing is kept"""
    return extract(*stereo_pair(0))


def empty_eye(s0, which):
    s = edited(s0)
    if "L" in which: s["kL"], s["dL"] = s["kL"][:0], s["dL"][:0]
    if "R" in which: s["kR"], s["dR"] = s["kR"][:0], s["dR"][:0]
    return s


CRAFTED = ("ties", "gates", "borders", "stripe", "zero")
FILTER = ("one_match", "two_matches", "three_matches", "ten_matches", "same_sad", "median_zero")
DEGENERATE = ("empty_left", "empty_right", "both_empty", "left_full")
# (rows, cols, nfeatures, nlevels, scale): natural output plus the ties / order and borders edits
SHAPES = {"hd1080": (1080, 1920, 2000, 8, 1.2), "euroc": (480, 752, 1200, 8, 1.2), "odd": (333, 517, 700, 8, 1.2), "tall": (2100, 1400, 1500, 8, 1.2),
          "four_levels": (480, 640, 1200, 4, 1.5), "five_levels": (1024, 1280, 1200, 5, 2.0), "one_level": (480, 640, 1200, 1, 1.2)}
NATURAL = [(disp, variant, bf, b, dy, noise)
           for (dy, noise) in [(0, 0), (1, 3), (-2, 5), (2, 0)]
           for (disp, variant, bf, b) in [(12, "textured", 40.0, 0.1), (4, "noise", 40.0, 0.1), (37, "textured", 60.0, 0.5), (0, "textured", 40.0, 0.1),
                                          (25, "sparse", 40.0, 0.1)]
           if (dy, noise) == (0, 0) or variant != "sparse"]      # the parametrisation of test_stereo.py::test_gpu_stereo_match_equals_oracle


def crafted(kind, seed=77):
    if kind == "zero":
        return zero(seed)
    return dict(ties=ties, gates=gates, borders=borders, stripe=stripe)[kind](base(seed), seed)


@functools.lru_cache(maxsize=None)
def get(name):
    if name in CRAFTED: return crafted(name)
    if name in ("one_match", "two_matches", "three_matches", "ten_matches"):
        return cut_to_matches(base(), dict(one_match=1, two_matches=2, three_matches=3, ten_matches=10)[name])
    if name == "same_sad": return same_sad(base())
    if name == "median_zero": return median_zero()
    if name == "left_full":                              # run with capacity == the left count: the right eye must fit too
        s = edited(base())
        m = min(len(s["kL"]), len(s["kR"]))
        return edited(s, kR=s["kR"][:m], dR=s["dR"][:m])
    if name in DEGENERATE: return empty_eye(base(), dict(empty_left="L", empty_right="R", both_empty="LR")[name])
    if name == "natural": return edited(base())
    if name == "natural_sparse": return extract(*stereo_pair(25, variant="sparse"))      # far fewer corners than nfeatures: another left count
    if name == "natural_1000": return extract(*stereo_pair(9, seed=5, noise=2), nf=1000)
    if name == "big": return shape_scene("big", "natural")
    kind, shape = name.split("@")
    return shape_scene(shape, kind)


def shape_scene(shape, kind):
    rows, cols, nf, nl, sf = (1080, 1920, 25000, 8, 1.2) if shape == "big" else SHAPES[shape]
    s0 = base(31, rows, cols, nf, sf, nl, "noise" if shape == "big" else "textured")
    return edited(s0) if kind == "natural" else dict(ties=ties, borders=borders)[kind](s0, 31)


SHAPE_SCENES = tuple("%s@%s" % (k, sh) for sh in SHAPES for k in ("natural", "ties", "borders"))
ALL_SCENES = CRAFTED + FILTER + DEGENERATE + ("natural", "natural_sparse", "natural_1000") + SHAPE_SCENES + ("big",)


@functools.lru_cache(maxsize=None)
def walked(name):
    """(scene, statement, oracle) of a named scene"""
    s = get(name)
    return s, statement(s), oracle(s)


def natural_case(case):
    disp, variant, bf, b, dy, noise = case
    s = extract(*stereo_pair(disp, variant=variant, dy=dy, noise=noise))
    s["bf"], s["b"] = bf, b
    return s


def assert_oracle_equals_statement(s, res, orc, what):
    u, d, kept = orc
    c = S.counts(res)
    print("%s: %d left, %d right, %s, shared %d (apart %d), clamped %d, median %d" % (what, len(s["kL"]), len(s["kR"]), {k: v for k, v in c.items() if v},
                                                                                    res["shared"].sum(), res["shared_apart"].sum(), res["clamped"].sum(), res["median"]))
    assert kept == res["kept"], what
    assert u.tobytes() == res["u_right"].tobytes(), "%s: uRight differs at %s" % (what, np.flatnonzero(u != res["u_right"])[:10])
    assert d.tobytes() == res["depth"].tobytes(), what
    assert c["DELTA"] == 0, what                         # unreachable (stereo_statement.py)
    return c


# ---------------------------------------------------------------- CPU ----------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_SCENES)
def test_oracle_equals_the_statement_on_every_scene_of_the_gpu_tests(name):
    s, res, orc = walked(name)
    check_rule(s)
    assert_oracle_equals_statement(s, res, orc, name)


@pytest.mark.parametrize("case", NATURAL, ids=lambda c: "-".join(str(v) for v in c))
def test_oracle_equals_the_statement_on_the_committed_natural_cases(case):
    s = natural_case(case)
    res = statement(s)
    assert_oracle_equals_statement(s, res, oracle(s), str(case))
    assert (res["sad"] >= 0).sum() > 100                 # pre-filter matches


def test_crafted_scenes_reach_every_exit():
    """the condition of the GPU tests below: computed from the statement's exit codes on exactly the scenes they run"""
    best = {}
    for name in CRAFTED + FILTER + DEGENERATE:
        c = S.counts(walked(name)[1])
        print(name, {k: v for k, v in c.items() if v})
        for k, v in c.items():
            best[k] = max(best.get(k, 0), v if name in CRAFTED else 0)      # the degenerate scenes do not count: an empty right eye "reaches" NO_ROW
    print(best)
    for k in S.EXITS:
        if k not in ("DELTA", "OFF_IMAGE"):
            assert best[k] >= 5, (k, best)
    assert best["DELTA"] == 0
    s, res, _ = walked("ties")
    assert res["shared"].sum() >= 50
    # chosen here, not by the issue: a tie shows in the output only where its holders sit at different columns; 20 such features make an index-order
    # mistake visible well beyond one accidental agreement
    assert res["shared_apart"].sum() >= 20
    s, res, _ = walked("zero")
    took = res["clamped"] & (res["exit"] == S.KEPT)
    assert took.sum() >= 5 and res["median"] > 0
    i = np.flatnonzero(took)
    assert (res["u_right"][i] == (s["kL"]["x"][i].astype(np.float64) - 0.01).astype(np.float32)).all()
    assert (res["depth"][i] == np.float32(s["bf"]) / np.float32(0.01)).all()


def test_double_step_differs_from_binary32_only_below_a_column_no_match_can_have():
    """uL - 0.01 in double and uL - 0.01f in binary32 round to different floats only for uL < 0.0725 (0.01 - 0.01f = 2.2e-10, and the result's ulp falls
    below that only next to 0.01).  Such a uL scales to column 0 of its level; a best window centred on column 0 sees the BORDER_REFLECT_101 frame, which
    mirrors both eyes about that column, so SAD(+s) = SAD(-s), deltaR = 0, bestuR = 0 and the disparity is uL > 0: the branch is not taken (and uL = 0
    gives -0.01f both ways).  So no scene can tell the two apart through mvuRight; the statement and the kernel keep the double as the reference has it."""
    rng = np.random.default_rng(3)
    u = np.concatenate([rng.uniform(0, 4096, 1 << 20), 10 ** rng.uniform(-4, 3.6, 1 << 20)]).astype(np.float32)
    differ = (u.astype(np.float64) - 0.01).astype(np.float32) != u - np.float32(0.01)
    assert differ.any() and u[differ].max() < 0.0725 and (np.float32(0) - np.float32(0.01)) == np.float32(0.0 - 0.01)
    for sf in (1.2, 1.5, 2.0):
        inv = X.compute_tables(1000, sf, 8)["inv_scale_factors"]
        assert all(S.round_half_away(np.float32(np.float32(0.0725) * v)) == 0 for v in inv)


def test_filter_scenes_have_the_match_counts_they_are_named_for():
    for name, m in (("one_match", 1), ("two_matches", 2), ("three_matches", 3), ("ten_matches", 10)):
        res = walked(name)[1]
        assert (res["sad"] >= 0).sum() == m
    res = walked("same_sad")[1]
    assert (res["sad"] >= 0).sum() == 6 and len(set(res["sad"][res["sad"] >= 0].tolist())) == 1 and res["kept"] == 6
    res = walked("median_zero")[1]
    assert (res["sad"] >= 0).sum() > 100 and res["median"] == 0 and res["kept"] == 0
    for name in DEGENERATE[:3]:
        assert walked(name)[1]["kept"] == 0 and walked(name)[2][2] == 0


def test_stereo_match_last_pairs_have_different_left_counts_and_matches():
    """the condition of test_gpu_stereo_match_last_on_two_pairs_of_different_counts, checked where no GPU is needed"""
    a, b = walked("natural"), walked("natural_sparse")
    assert len(a[0]["kL"]) != len(b[0]["kL"]) and len(a[0]["kR"]) != len(b[0]["kR"])
    assert a[1]["kept"] > 100 and b[1]["kept"] > 100 and a[1]["kept"] != b[1]["kept"]


def test_shapes_scan_more_than_one_row_per_thread_and_every_pyramid():
    assert SHAPES["hd1080"][0] > 1024 and SHAPES["tall"][0] > 2048      # per = ceil(rows / 1024) is 2 and 3
    for name in SHAPE_SCENES + ("big",):
        assert (walked(name)[1]["sad"] >= 0).sum() > 100, name


def test_lds_bound_follows_the_kernel_table_and_the_header_documents_it():
    table = json.load(open(os.path.join(os.path.dirname(X.orbextractor.__file__), "csrc", "kernel_table.json")))
    assert header_static_lds() >= table["k_stereo_filter"]["lds_static_bytes"]
    largest = max(c for c in range(1, 65536) if filter_lds_bytes(c) <= LDS_LIMIT)
    assert largest == 40568 and filter_lds_bytes(largest + 1) > LDS_LIMIT and LDS_LIMIT == helpers.entry_lds_budget()
    text = open(X.orbextractor._HEADER).read()
    pos = text.index("int orbx_stereo_match_device(")
    doc = text[text.rindex("/*", 0, pos):pos]
    assert "ORBX_ERR_UNSUPPORTED" in doc and "4 * ((capacity + 3) & ~3) + ORBX_STEREO_FILTER_STATIC_LDS_BYTES > 160 * 1024 - 512" in doc and "40568" in doc


# ---------------------------------------------------------------- GPU ----------------------------------------------------------------
def make_extractor(s, n_pairs, **kw):
    rows, cols = s["left"].shape
    return X.ORBextractor(s["nf"], s["sf"], s["nl"], max_width=cols, max_height=rows, max_batch=2 * n_pairs, **kw)


def upload(ex, scenes):
    """both eyes of every scene through extract_batch_device: the handle builds the pyramids (its own keypoints go to scratch buffers)"""
    import torch
    P = len(scenes); rows, cols = scenes[0]["left"].shape
    cap = ex.capacity
    d_img = torch.from_numpy(np.stack([img for s in scenes for img in (s["left"], s["right"])])).cuda()
    d_k = torch.zeros((2 * P, cap, 7), dtype=torch.float32, device="cuda"); d_d = torch.zeros((2 * P, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(2 * P, dtype=torch.int32, device="cuda"); d_m = torch.zeros(2 * P, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ex.extract_batch_device(d_img, 2 * P, rows, cols, d_k, d_d, d_n, d_m, cap, lapping=(0, 0))
    ex.synchronize()
    return d_k, d_d, d_n


def match(ex, scenes, cap):
    """one orbx_stereo_match_device call on the scenes' own arrays, outputs poisoned first; returns host (uRight, depth, n_matched)"""
    import torch
    P = len(scenes)
    kps = np.zeros((2 * P, cap), X.KEYPOINT_DTYPE); desc = np.zeros((2 * P, cap, 32), np.uint8); n = np.zeros(2 * P, np.int32)
    for p, s in enumerate(scenes):
        for f, (k, d) in ((2 * p, (s["kL"], s["dL"])), (2 * p + 1, (s["kR"], s["dR"]))):
            assert len(k) <= cap
            kps[f, :len(k)] = k; desc[f, :len(k)] = d; n[f] = len(k)
    d_k = torch.from_numpy(kps.view(np.uint8).reshape(2 * P, cap, 28)).cuda(); d_d = torch.from_numpy(desc).cuda(); d_n = torch.from_numpy(n).cuda()
    d_u = torch.full((P, cap), float(POISON), dtype=torch.float32, device="cuda"); d_z = torch.full((P, cap), float(POISON), dtype=torch.float32, device="cuda")
    d_nm = torch.full((P,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ex.stereo_match_device(P, d_k, d_d, d_n, cap, scenes[0]["bf"], scenes[0]["b"], d_u, d_z, d_nm)
    ex.synchronize()
    return d_u.cpu().numpy(), d_z.cpu().numpy(), d_nm.cpu().numpy()


def assert_equals_oracle(s, u, z, nm, what, orc=None):
    u_o, d_o, kept = orc if orc is not None else oracle(s)
    n = len(s["kL"])
    print("%s: %d left, %d right, %d kept" % (what, n, len(s["kR"]), kept))
    assert int(nm) == kept, what
    assert u[:n].tobytes() == u_o.tobytes(), "%s: uRight differs at %s" % (what, np.flatnonzero(u[:n] != u_o)[:10])
    assert z[:n].tobytes() == d_o.tobytes(), what
    assert (u[n:] == POISON).all() and (z[n:] == POISON).all(), what      # the kernels return for iL >= N


def run_scenes(names, cap=None, per_pair_params=False):
    """the scenes of `names` (one frame shape and pyramid) in as many calls as they have (bf, b) values"""
    scenes = [get(n) for n in names]
    ex = make_extractor(scenes[0], len(scenes))
    upload(ex, scenes)
    cap = cap or max(max(len(s["kL"]), len(s["kR"])) for s in scenes)
    out = {}
    for key in sorted({(s["bf"], s["b"]) for s in scenes}):
        u, z, nm = match(ex, [dict(s, bf=key[0], b=key[1]) for s in scenes], cap)
        for p, (name, s) in enumerate(zip(names, scenes)):
            if (s["bf"], s["b"]) == key:
                assert_equals_oracle(s, u[p], z[p], nm[p], "%s (capacity %d)" % (name, cap))
                out[name] = (u[p], z[p], nm[p])
    return ex, out


@pytest.mark.gpu
@pytest.mark.parametrize("name", CRAFTED + FILTER + DEGENERATE)
def test_gpu_crafted_scene_equals_oracle(name):
    s = get(name)
    run_scenes([name], cap=max(len(s["kL"]), len(s["kR"]), 1) + 37)


@pytest.mark.gpu
def test_gpu_many_pairs_in_one_call_twice():
    """11 pairs with different counts in ONE call, run twice: the atomicAdd fill order of the row lists must not show"""
    names = ["ties", "natural", "empty_left", "borders", "stripe", "zero", "one_match", "empty_right", "same_sad", "both_empty", "ten_matches"]
    scenes = [get(n) for n in names]
    assert len({(len(s["kL"]), len(s["kR"])) for s in scenes}) >= 8 and all((s["bf"], s["b"]) == (40.0, 0.1) for s in scenes)
    ex = make_extractor(scenes[0], len(scenes))
    upload(ex, scenes)
    cap = max(max(len(s["kL"]), len(s["kR"])) for s in scenes) + 3
    first = match(ex, scenes, cap)
    again = match(ex, scenes, cap)
    for a, b in zip(first, again):
        assert a.tobytes() == b.tobytes()
    for p, (name, s) in enumerate(zip(names, scenes)):
        assert_equals_oracle(s, first[0][p], first[1][p], first[2][p], "pair %d %s" % (p, name))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_gpu_other_shapes_and_pyramids(shape):
    run_scenes(["%s@%s" % (k, shape) for k in ("natural", "ties", "borders")])


@pytest.mark.gpu
def test_gpu_caller_capacities():
    s = get("left_full")
    ex, _ = run_scenes(["left_full"], cap=len(s["kL"]))              # capacity == the left count
    assert ex.capacity > len(s["kL"])
    ex, _ = run_scenes(["natural", "ties"], cap=4000)
    assert ex.capacity < 4000


@pytest.mark.gpu
def test_gpu_capacity_above_16384_filter_lds_above_64k():
    s = get("big")
    ex = make_extractor(s, 1)
    cap = ex.capacity
    assert cap > 16384 and 64 * 1024 < filter_lds_bytes(cap) <= LDS_LIMIT
    upload(ex, [s])
    u, z, nm = match(ex, [s], cap)
    assert_equals_oracle(s, u[0], z[0], nm[0], "25 000-feature extractor, capacity %d" % cap)
    assert len(s["kL"]) > 5000


@pytest.mark.gpu
def test_gpu_one_handle_across_sizes():
    """480 x 640, then 1080p, then 480 x 640 again on one handle: the stereo scratch regrows in between and rowCap follows the larger capacity"""
    small, large = extract(*stereo_pair(9, seed=5, noise=2), nf=2000), get("natural@hd1080")
    ex = X.ORBextractor(2000, max_width=1920, max_height=1080, max_batch=2)
    for s in (small, large, small):
        cap = max(len(s["kL"]), len(s["kR"])) + (50 if s is small else 150)
        upload(ex, [s])
        u, z, nm = match(ex, [s], cap)
        assert_equals_oracle(s, u[0], z[0], nm[0], "%d rows, capacity %d" % (s["left"].shape[0], cap))


@pytest.mark.gpu
def test_gpu_stereo_match_last_on_two_pairs_of_different_counts():
    a, b = get("natural"), get("natural_sparse")
    assert len(a["kL"]) != len(b["kL"])
    ex = X.ORBextractor(1200, max_batch=4)
    res = ex.extract_batch(np.stack([a["left"], a["right"], b["left"], b["right"]]), lapping=(0, 0))
    u, d, nm = ex.stereo_match_last(2, 40.0, 0.1)
    for p, s in enumerate((a, b)):
        assert res[2 * p][1].tobytes() == s["kL"].tobytes() and res[2 * p + 1][1].tobytes() == s["kR"].tobytes()
        u_o, d_o, kept = oracle(s)
        n = len(s["kL"])
        assert nm[p] == kept and u[p, :n].tobytes() == u_o.tobytes() and d[p, :n].tobytes() == d_o.tobytes()
        assert (u[p, n:] == 0).all()                       # the wrapper's zeros: only n entries are copied out


@pytest.mark.gpu
def test_gpu_capacity_at_the_lds_bound_runs_and_the_next_is_refused_before_any_launch():
    import torch
    cap = max(c for c in range(1, 65536) if filter_lds_bytes(c) <= LDS_LIMIT)
    assert cap == 40568
    s = get("natural_1000")
    assert 300 < len(s["kL"]) <= cap
    ex = make_extractor(s, 1)
    upload(ex, [s])
    ex.profile(True)
    u, z, nm = match(ex, [s], cap)                                     # the largest accepted capacity runs
    assert_equals_oracle(s, u[0], z[0], nm[0], "capacity %d" % cap)
    launches = sum(v[1] for v in ex.profile_read().values())
    assert launches >= 1
    with pytest.raises(X.OrbxError) as e:                              # the first refused one
        match(ex, [s], cap + 1)
    assert e.value.code == -8
    ex.synchronize()
    assert sum(v[1] for v in ex.profile_read().values()) == launches   # nothing was launched
    torch.cuda.synchronize()


def check_gpu_on_seed(seed):
    """the body tools/fuzz_matchers.py runs with seeds outside the committed one: the crafted scenes of one seed, one call per (bf, b)"""
    scenes = [crafted(k, seed) for k in CRAFTED]
    ex = make_extractor(scenes[0], len(scenes))
    upload(ex, scenes)
    cap = max(max(len(s["kL"]), len(s["kR"])) for s in scenes) + int(seed % 5)
    for key in sorted({(s["bf"], s["b"]) for s in scenes}):
        u, z, nm = match(ex, [dict(s, bf=key[0], b=key[1]) for s in scenes], cap)
        for p, s in enumerate(scenes):
            if (s["bf"], s["b"]) == key:
                assert_equals_oracle(s, u[p], z[p], nm[p], "seed %d %s" % (seed, CRAFTED[p]))
