"""The description kernels (k_describe.hip: the weight words copied from the static tables into LDS, the selection entry requested across the
workgroup barrier) in every description form - blur per keypoint on all levels, blurred levels for all, the blur split at level 1 and at
level 2 - on shapes small enough to hold every edge of the slot walk, with poisoned allocations and polluted LDS.  Everything byte for byte
against the oracle: n, the mono index, 28-byte keypoints, 32-byte descriptors, per-level keypoints and counts.

The small shape is 160 x 120, 3 levels, 60 features: per-level quotas 24 / 20 / 16, selection capacities 28 / 24 / 20, so the levels' first slots
are 0 / 28 / 52 of 72 per frame: the workgroup of slots [24, 32) holds the boundary 28, the one of [48, 56) the boundary 52 (waves of one
workgroup in two levels, and in two launches where the blur is split there).
Frames of the batch (oracle, lapping area (40, 90); checked on the CPU before the list was relied on, and asserted below):
  * textured: 25 / 22 / 17 keypoints = 64 in all (odd counts: a lone active half at the end of levels 0 and 2; over the tight capacity of 40),
  * sparse:    0 /  1 /  1 (an all-zero level, lone halves, fewer keypoints than the quota),
  * natural:  13 /  2 /  2 = 17 (an odd level, few keypoints)."""
import numpy as np
import pytest

import oracle_lib as O
import extractorb_amd as X
from extractorb_amd import synth
from helpers import assert_same_result

pytestmark = pytest.mark.gpu

NF, NLEVELS, SF, ROWS, COLS, LAP, TIGHT = 60, 3, 1.2, 120, 160, (40, 90), 40
FORMS = {"pb": dict(ORBX_PATCH_BLUR="1", ORBX_BLUR_SPLIT="0"), "plain": dict(ORBX_PATCH_BLUR="0"),
         "split1": dict(ORBX_PATCH_BLUR="1", ORBX_BLUR_SPLIT="1"), "split2": dict(ORBX_PATCH_BLUR="1", ORBX_BLUR_SPLIT="2")}
BLUR_FORM = {"pb": 3, "plain": None, "split1": 5, "split2": 5}


@pytest.fixture(scope="module")
def small():
    """the three frames and what the oracle makes of each: (mono, keypoints, descriptors), per-level keypoints"""
    frames = np.stack([synth.frames("textured", 5, 1, ROWS, COLS)[0], synth.frames("sparse", 5, 1, ROWS, COLS)[0], synth.frames("natural", 5, 3, ROWS, COLS)[2]])
    want, levels = [], []
    for f in range(3):
        o = O.Oracle(NF, SF, NLEVELS, 20, 7)
        want.append(o.extract(frames[f], LAP))
        levels.append([o.level_keypoints(l).copy() for l in range(NLEVELS)])
    assert [[len(a) for a in lv] for lv in levels] == [[25, 22, 17], [0, 1, 1], [13, 2, 2]]
    assert len(want[0][1]) == 64 > TIGHT and X.compute_tables(NF, SF, NLEVELS)["features_per_level"].tolist() == [24, 20, 16]
    assert 0 < want[0][0] < 64      # lapping and non-lapping keys: both ends of the final array are filled
    return frames, want, levels


@pytest.fixture
def aids():
    X.debug_set_option("poison", 0xA5)
    X.debug_set_option("lds_pollute", 0xC3)
    yield
    X.debug_reset_options()


def make(form, monkeypatch, **kw):
    for k, v in FORMS[form].items():
        monkeypatch.setenv(k, v)
    return X.ORBextractor(kw.pop("nf", NF), SF, kw.pop("nlevels", NLEVELS), 20, 7, **kw)


def check_form(ex, form):
    if BLUR_FORM[form] is not None:
        assert ex.last_forms()[2] == BLUR_FORM[form], ex.last_forms()
    else:
        assert ex.last_forms()[2] not in (3, 5), ex.last_forms()


@pytest.mark.parametrize("form", sorted(FORMS))
def test_small_batch_tight_capacity_and_back_only(form, small, aids, monkeypatch):
    import torch
    frames, want, levels = small
    ex = make(form, monkeypatch, max_width=COLS, max_height=ROWS, max_batch=3)
    assert "lds_pollute:195" in ex.policy() and "poison:165" in ex.policy(), ex.policy()
    # the batch: level boundaries inside a workgroup's slots, lone halves, an empty level
    out = ex.extract_batch(frames, LAP)
    check_form(ex, form)
    for f in range(3):
        assert_same_result(out[f][:3], want[f], "%s frame %d" % (form, f))
        assert [len(a) for a in out[f][3]] == [len(a) for a in levels[f]]
        assert all(a.tobytes() == b.tobytes() for a, b in zip(out[f][3], levels[f])), "%s frame %d: per-level keypoints" % (form, f)
    # a capacity below frame 0's total (64): every index below it holds the oracle's entry, nothing is written behind a frame's rows
    guard = 16
    ex.set_stream(torch.cuda.current_stream().cuda_stream)
    d_img = torch.from_numpy(frames).cuda()
    d_k = torch.full((3 * TIGHT + guard, 28), 0x7F, dtype=torch.uint8, device="cuda"); d_d = torch.full((3 * TIGHT + guard, 32), 0x7F, dtype=torch.uint8, device="cuda")
    d_lk = torch.full((3 * TIGHT + guard, 28), 0x7F, dtype=torch.uint8, device="cuda"); d_lc = torch.zeros((3, NLEVELS), dtype=torch.int32, device="cuda")
    d_n = torch.zeros(3, dtype=torch.int32, device="cuda"); d_m = torch.zeros(3, dtype=torch.int32, device="cuda")
    ex.extract_batch_device(d_img, 3, ROWS, COLS, d_k, d_d, d_n, d_m, TIGHT, lapping=LAP, d_level_kps=d_lk, d_level_counts=d_lc)
    ex.synchronize()
    k, d, lk = d_k.cpu().numpy(), d_d.cpu().numpy(), d_lk.cpu().numpy()
    assert d_n.cpu().tolist() == [len(w[1]) for w in want] and d_m.cpu().tolist() == [w[0] for w in want]
    assert d_lc.cpu().tolist() == [[len(a) for a in lv] for lv in levels]
    for f in range(3):
        n = min(len(want[f][1]), TIGHT)
        rows = slice(f * TIGHT, f * TIGHT + n)
        assert k[rows].tobytes() == want[f][1][:n].tobytes() and np.array_equal(d[rows], want[f][2][:n]), "%s frame %d at capacity %d" % (form, f, TIGHT)
        assert lk[rows].tobytes() == np.concatenate(levels[f])[:n].tobytes()
        for a in (k, d, lk):
            assert (a[f * TIGHT + n:(f + 1) * TIGHT] == 0x7F).all(), "%s frame %d: written past the frame's count" % (form, f)
    for a in (k, d, lk):
        assert (a[3 * TIGHT:] == 0x7F).all(), "%s: written past the arrays" % form
    # a back-only pass (FAST, quad-tree and description on the pyramid the front call left)
    one = X.ORBextractor(NF, SF, NLEVELS, 20, 7, max_width=COLS, max_height=ROWS)
    mono, kk, dd, lvl = one(frames[0], None, LAP)
    assert_same_result((mono, kk, dd), want[0], "%s one frame" % form)
    again = one.ComputeKeyPointsOctTree()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, levels[0])), "%s: back-only pass" % form


def test_the_benchmarks_form_two_frames(aids, monkeypatch):
    """2 x 640 x 480 x 1000, eight levels, the blur split at level 3 (the form of bench.py's default workload)"""
    frames = np.stack([synth.frames("noise", 0, 1, 480, 640)[0], synth.frames("textured", 1, 1, 480, 640)[0]])
    monkeypatch.setenv("ORBX_PATCH_BLUR", "1")
    monkeypatch.setenv("ORBX_BLUR_SPLIT", "3")
    ex = X.ORBextractor(1000, max_batch=2)
    out = ex.extract_batch(frames)
    assert ex.last_forms()[2] == 5 and X.load_library().orbx_debug_last_split_level(ex._h) == 3
    for f in range(2):
        o = O.Oracle(1000, 1.2, 8, 20, 7)
        want = o.extract(frames[f], (0, 1000))
        assert_same_result(out[f][:3], want, "frame %d" % f)
        assert all(a.tobytes() == o.level_keypoints(l).tobytes() for l, a in enumerate(out[f][3])), "frame %d: per-level keypoints" % f
