"""The description kernels' prologue (k_describe_body.hpp): the level table taken by value, the wave's level found from the levels' first slots,
the frame's rows of the per-level counts read in batches of eight scalar dwords with the prefix in scalar arithmetic, the selection entry
requested with a clamped slot before the wave knows whether it is active.  Every case byte for byte against the oracle: n, the mono index,
28-byte keypoints, 32-byte descriptors, per-level keypoints.

The kernels sum the counts in two forms, chosen by the launch's size: the scalar form (batches of eight dwords) in launches of more than 2048
workgroups, the lane form (lane l reads level l, a DPP scan) in smaller ones.  The small shapes of this file would only ever take the lane
form, so every case runs under both, pinned with the test aid "describe_sums" (0: scalar, 1: lanes).

Shapes: the smallest frame orbx_create accepts for a depth at scale 1.2 (4 : 3, columns a multiple of 4; asserted in
tests/test_describe_levels.py): 84 x 63 for one level, 100 x 75 for two, 120 x 90 for three, 296 x 222 for eight, 356 x 267 for nine and
1264 x 948 for sixteen.  At 200 features the eight-level frame's levels start at slots 0 48 88 122 152 178 200 220: the boundaries 122, 178
and 220 lie inside a workgroup's eight slots.
The crafted frame: five single pixels 21 above a flat ground (corners of level 0 only at thresholds 20 / 20) and two smooth blobs (sigma 7:
too flat for FAST below level 3), one of them 40 px from the left edge (outside the FAST rectangle from level 6 on): the oracle keeps
5 0 0 2 2 3 0 0 keypoints - empty levels in the middle and at the end -, four of the twelve outside the lapping window (0, 150)."""
import numpy as np
import pytest

import oracle_lib as O
import extractorb_amd as X
from extractorb_amd import synth
from helpers import assert_same_result

pytestmark = pytest.mark.gpu

SMALLEST = {1: (63, 84), 2: (75, 100), 3: (90, 120), 8: (222, 296), 9: (267, 356), 16: (948, 1264)}
NF = 200
FORMS = {"plain": dict(ORBX_PATCH_BLUR="0"), "pb": dict(ORBX_PATCH_BLUR="1", ORBX_BLUR_SPLIT="0")}
FORMS.update({"split%d" % k: dict(ORBX_PATCH_BLUR="1", ORBX_BLUR_SPLIT=str(k)) for k in range(1, 8)})
_oracle_cache = {}


def oracle(img, nlevels, lap=(0, 1000), nf=NF, ini=20, mn=7):
    """((mono, keypoints, descriptors), per-level keypoints) of the oracle, computed once per case of this module"""
    key = (img.tobytes(), nlevels, tuple(lap), nf, ini, mn)
    if key not in _oracle_cache:
        o = O.Oracle(nf, 1.2, nlevels, ini, mn)
        want = o.extract(img, lap)
        _oracle_cache[key] = (want, [o.level_keypoints(l).copy() for l in range(nlevels)])
    return _oracle_cache[key]


def crafted(rows=222, cols=296):
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64)
    img = np.full((rows, cols), 100.0)
    for py, px in ((60, 120), (100, 200), (150, 90), (170, 230), (61, 180)):
        img[py, px] += 21
    for by, bx in ((110, 40), (40, 150)):
        img += 110 * np.exp(-((yy - by) ** 2 + (xx - bx) ** 2) / (2 * 7.0 ** 2))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


@pytest.fixture(params=[0, 1], ids=["scalar_sums", "lane_sums"])
def aids(request):
    X.debug_set_option("poison", 0xA5)
    X.debug_set_option("lds_pollute", 0xC3)
    X.debug_set_option("describe_sums", request.param)
    yield request.param
    X.debug_reset_options()


def make(form, monkeypatch, nlevels, shape, max_batch=1, nf=NF, ini=20, mn=7):
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    ex = X.ORBextractor(nf, 1.2, nlevels, ini, mn, max_width=shape[1], max_height=shape[0], max_batch=max_batch)
    assert "describe_sums:" in ex.policy(), ex.policy()
    return ex


def check_form(ex, form, nlevels):
    want = {"plain": None, "pb": 3}.get(form, 5 if form.startswith("split") and int(form[5:]) < nlevels else 3)
    if want is None:
        assert ex.last_forms()[2] not in (3, 5), ex.last_forms()
    else:
        assert ex.last_forms()[2] == want, (form, ex.last_forms())


def check_frame(got, img, nlevels, lap, what, **kw):
    want, levels = oracle(img, nlevels, lap, **kw)
    assert_same_result(got[:3], want, what)
    assert [len(a) for a in got[3]] == [len(a) for a in levels], what
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got[3], levels)), "%s: per-level keypoints" % what
    return want, levels


@pytest.mark.parametrize("form", ["plain", "pb"])
@pytest.mark.parametrize("nlevels", [1, 2, 8, 9, 16])
def test_level_counts(nlevels, form, aids, monkeypatch):
    """one level, two, eight (one batch of counts, full), nine (the second batch begins) and sixteen (kMaxLevels: both batches full)"""
    rows, cols = SMALLEST[nlevels]
    img = synth.frames("textured", 5, 1, rows, cols)[0]
    lap = (40, cols // 2)
    ex = make(form, monkeypatch, nlevels, (rows, cols))
    got = ex(img, None, lap)
    check_form(ex, form, nlevels)
    want, levels = check_frame((got[0], got[1], got[2], got[3]), img, nlevels, lap, "%d levels, %s" % (nlevels, form))
    assert all(len(a) for a in levels) and 0 < want[0] < len(want[1])      # every level holds keypoints, on both sides of the lapping window


@pytest.mark.parametrize("form", ["plain", "pb", "split3", "split4"])
def test_empty_levels(form, aids, monkeypatch):
    """a flat frame (every level empty, n = 0) and the crafted frame (5 0 0 2 2 3 0 0) in one batch; the split at 3 and at 4 has an empty launch side"""
    rows, cols = SMALLEST[8]
    frames = np.stack([np.full((rows, cols), 100, np.uint8), crafted(rows, cols)])
    lap = (0, 150)
    want, levels = oracle(frames[1], 8, lap, ini=20, mn=20)
    assert [len(a) for a in levels] == [5, 0, 0, 2, 2, 3, 0, 0] and want[0] == 4 and len(want[1]) == 12
    ex = make(form, monkeypatch, 8, (rows, cols), max_batch=2, ini=20, mn=20)
    for rep in range(2):
        out = ex.extract_batch(frames, lap)
        check_form(ex, form, 8)
        assert out[0][0] == 0 and len(out[0][1]) == 0 and out[0][2].shape == (0, 32) and all(len(a) == 0 for a in out[0][3]), "flat frame, call %d" % rep
        check_frame(out[1], frames[1], 8, lap, "crafted frame, %s, call %d" % (form, rep), ini=20, mn=20)


@pytest.mark.parametrize("sums", [0, 1])
@pytest.mark.parametrize("poison", [0xA5, 0xFF, 0x00])
@pytest.mark.parametrize("nlevels", [3, 9])
def test_last_frame_of_a_full_batch(nlevels, poison, sums, monkeypatch):
    """max_batch == the batch: the count batches of the last frame reach past the last row of the arrays (three levels: five and eight entries past,
    nine levels: seven), into whatever the allocation holds there - three poisons (0xFF: every entry -1), each run twice"""
    X.debug_set_option("poison", poison)
    X.debug_set_option("describe_sums", sums)
    try:
        rows, cols = SMALLEST[nlevels]
        B = 3
        frames = np.concatenate([synth.frames("textured", 7, 2, rows, cols), synth.frames("noise", 8, 1, rows, cols)])
        lap = (30, 70)
        ex = make("split1", monkeypatch, nlevels, (rows, cols), max_batch=B)
        assert "poison:%d" % poison in ex.policy(), ex.policy()
        for rep in range(2):
            out = ex.extract_batch(frames, lap)
            for f in range(B):
                check_frame(out[f], frames[f], nlevels, lap, "%d levels, poison %#x, call %d, frame %d" % (nlevels, poison, rep, f))
    finally:
        X.debug_reset_options()


@pytest.mark.parametrize("B", [1, 20])
def test_the_policys_own_choice_of_the_sums(B):
    """640 x 480 x 1000 under the default policy, no aid: one frame per call (a few waves: the lane form) and twenty (more than eight workgroups
    per CU in the description launch: the scalar form)"""
    frames = np.concatenate([synth.frames("textured", 40, (B + 1) // 2, 480, 640), synth.frames("noise", 41, B // 2 + 1, 480, 640)])[:B]
    ex = X.ORBextractor(1000, max_batch=B)
    out = ex.extract_batch(frames)
    for f in sorted({0, B // 2, B - 1}):
        check_frame(out[f], frames[f], 8, (0, 1000), "frame %d of %d" % (f, B), nf=1000)
    one = X.ORBextractor(1000)
    for f in range(B):      # every frame against the one-frame call of the same library
        mono, k, d, _ = one(frames[f])
        assert_same_result(out[f][:3], (mono, k, d), "frame %d of %d against its own call" % (f, B))


@pytest.mark.parametrize("split", [1, 2, 3, 4, 5, 6, 7])
def test_both_kernels_and_the_straddling_workgroup(split, aids, monkeypatch):
    """the blur split at every level of the eight-level frame: the slot ranges of the two launches meet at 48, 88, 122, 152, 178, 200 or 220 - inside
    the workgroup of slots [120, 128), [176, 184) or [216, 224) for the splits at 3, 5 and 7, whose waves then run in two launches"""
    rows, cols = SMALLEST[8]
    n, desc, geom = X.describe_levels(rows, cols, NF, 1.2, 8, 2)
    assert desc[0, :8].tolist() == [0, 48, 88, 122, 152, 178, 200, 220]
    frames = np.stack([synth.frames("textured", 5, 1, rows, cols)[0], synth.frames("sparse", 5, 1, rows, cols)[0]])
    lap = [(0, 1000), (60, 200)]
    ex = make("split%d" % split, monkeypatch, 8, (rows, cols), max_batch=2)
    out = ex.extract_batch(frames, lap)
    check_form(ex, "split%d" % split, 8)
    for f in range(2):
        check_frame(out[f], frames[f], 8, lap[f], "split %d frame %d" % (split, f))


@pytest.mark.parametrize("form", ["plain", "pb", "split3"])
def test_placement_and_capacity(form, aids, monkeypatch):
    """lapping windows (0, 0) (every key in front), one with keys on both sides and one that holds every key; then a capacity below the kept total:
    every index below it holds the oracle's entry, nothing is written behind it"""
    import torch
    rows, cols = SMALLEST[8]
    frames = np.stack([synth.frames("textured", 5, 1, rows, cols)[0]] * 3)
    lap = [(0, 0), (100, 200), (0, 1000)]
    ex = make(form, monkeypatch, 8, (rows, cols), max_batch=3)
    out = ex.extract_batch(frames, lap)
    wants = [check_frame(out[f], frames[f], 8, lap[f], "%s lapping %s" % (form, lap[f])) for f in range(3)]
    n = len(wants[0][0][1])
    assert wants[0][0][0] == n and 0 < wants[1][0][0] < n and wants[2][0][0] == 0, [w[0][0] for w in wants]
    tight, guard = n - 37, 16
    assert tight > 0
    ex.set_stream(torch.cuda.current_stream().cuda_stream)
    d_img = torch.from_numpy(frames).cuda()
    d_k = torch.full((3 * tight + guard, 28), 0x7F, dtype=torch.uint8, device="cuda"); d_d = torch.full((3 * tight + guard, 32), 0x7F, dtype=torch.uint8, device="cuda")
    d_lk = torch.full((3 * tight + guard, 28), 0x7F, dtype=torch.uint8, device="cuda"); d_lc = torch.zeros((3, 8), dtype=torch.int32, device="cuda")
    d_n = torch.zeros(3, dtype=torch.int32, device="cuda"); d_m = torch.zeros(3, dtype=torch.int32, device="cuda")
    ex.extract_batch_device(d_img, 3, rows, cols, d_k, d_d, d_n, d_m, tight, lapping=lap, d_level_kps=d_lk, d_level_counts=d_lc)
    ex.synchronize()
    k, d, lk = d_k.cpu().numpy(), d_d.cpu().numpy(), d_lk.cpu().numpy()
    assert d_n.cpu().tolist() == [n] * 3 and d_m.cpu().tolist() == [w[0][0] for w in wants]
    assert d_lc.cpu().tolist() == [[len(a) for a in w[1]] for w in wants]
    for f in range(3):
        at = slice(f * tight, (f + 1) * tight)
        assert k[at].tobytes() == wants[f][0][1][:tight].tobytes() and np.array_equal(d[at], wants[f][0][2][:tight]), "%s frame %d at capacity %d" % (form, f, tight)
        assert lk[at].tobytes() == np.concatenate(wants[f][1])[:tight].tobytes()
    for a in (k, d, lk):
        assert (a[3 * tight:] == 0x7F).all(), "%s: written past the arrays" % form
