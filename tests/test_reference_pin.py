"""The one known answer the reference itself holds for this path.

/root/reference/img_folder/Screenshot.png is a capture of the author's IDE after running the demo main
(src/orb_extractor/main_orb_extractor.cpp:34-53: nFeatures = 1500, scale 1.2, 8 levels, FAST 20/7; ComputePyramid +
ComputeKeyPointsOctTree; the sum of the per-level vector sizes is printed).

ASSUMPTION, stated because the file has moved on since the capture: TODAY's main_orb_extractor.cpp:43 constructs `ORBextractor(5 * nFeatures,
...)` = 7500 features and reads another picture (../pic/robot/866_im.jpg, :16).  With 7500 features the oracle gives 1547 on the screenshot's
frame, not 1420 (test_todays_demo_constructor_gives_1547 below); with the 1500 of the yaml block it gives exactly 1420 AND its 1420 positions sit
on the 1420 circles the screenshot's image window shows (test_oracle_keypoints_sit_where_the_reference_drew_them).  So the screenshot is taken to
come from an EARLIER build of the demo that passed nFeatures itself; count and picture together are what supports that reading.

Its console pane reads

    The ../pic/TUM/dataset-room4_512_16/ma...     (image path, cut off by the pane)
    ORB_SLAM3 has total 1420 keypoints

The frame is pic/TUM/dataset-room4_512_16/mav0/cam0/data/1520531124150444163.png (16-bit PNG; imread(IMREAD_GRAYSCALE) keeps the high
byte), committed as tests/golden/tum_room4_gray.png (the 16-bit original as tests/golden/tum_room4_16bit.png).  1420 is a number produced by the REAL reference on REAL OpenCV: it is the only
reference-held pin of the oracle.  What it pins and what it does not is measured below, one restated semantic at a time
(`enum Mutation` in oracle/orb_oracle.cpp; table in DESIGN.md §2, printed by tools/pin_sensitivity.py)."""
import numpy as np
import pytest

import oracle_lib as O
from helpers import load_case, load_gray

REFERENCE_TOTAL = 1420           # img_folder/Screenshot.png
REFERENCE_PARAMS = (1500, 1.2, 8, 20, 7)    # main_orb_extractor.cpp:34-38

# mutation id -> (name, does the reference's 1420 move?)  Kept in step with `enum Mutation`.
MUTATIONS = {
    1: ("resize: no +2 rounding term in the vertical pass", True),
    2: ("pyramid: every level resized from level 0 instead of level l-1", True),
    3: ("resize: right-clamped column keeps its fractional weight", False),
    4: ("level size: truncation instead of cvRound", True),
    5: ("FAST: arc pixels >= threshold instead of >", True),
    6: ("NMS: >= instead of strict >", True),
    7: ("NMS over the whole level instead of per cell ROI", True),
    8: ("no minThFAST retry for empty cells", True),
    9: ("column skip at maxBorderX-3 instead of -6", False),
    10: ("quad-tree stops at size > N instead of >= N", True),
    11: ("sorted phase entered at size+3*nToExpand >= N instead of > N", False),
    12: ("sort ties: oldest node first instead of newest", False),
    13: ("DivideNode: floor instead of ceil of the half extent", False),
    14: ("cell width W = 35 instead of 30", True),
}


def total_with(mutation, image):
    o = O.Oracle(*REFERENCE_PARAMS)
    assert o.set_mutation(mutation) == 16
    o.extract(image, (0, 1000))
    return [len(o.level_keypoints(l)) for l in range(8)]


def test_oracle_reproduces_the_reference_screenshot_count():
    counts = total_with(0, load_gray("tum_room4_gray.png"))
    assert sum(counts) == REFERENCE_TOTAL, counts
    # levels 0-4 stop at their quota exactly (326, 271, 226, 189, 157: the `size >= N` exits of :674 / :735), levels 5-7 keep every
    # FAST candidate (127, 63, 61 < quota): the sum tests both regimes
    o = O.Oracle(*REFERENCE_PARAMS)
    assert counts[:5] == o.features_per_level[:5].tolist() and all(c < q for c, q in zip(counts[5:], o.features_per_level[5:]))


def test_todays_demo_constructor_gives_1547():
    """main_orb_extractor.cpp:43 as it stands today: ORBextractor(5 * nFeatures = 7500, ...).  On the screenshot's frame every FAST candidate
    survives the quad-tree on every level: 1547 keypoints - NOT the screenshot's 1420, which is why the pin assumes the earlier 1500-feature build."""
    o = O.Oracle(7500, 1.2, 8, 20, 7)
    o.extract(load_gray("tum_room4_gray.png"), (0, 1000))
    counts = [len(o.level_keypoints(l)) for l in range(8)]
    assert sum(counts) == 1547 and all(c < q for c, q in zip(counts, o.features_per_level)), counts


def test_golden_file_of_the_pinned_frame_sums_to_the_reference_count():
    c = load_case("tum_room4_1500")
    assert int(c["level_counts"].sum()) == REFERENCE_TOTAL == len(c["keypoints"])


@pytest.mark.parametrize("mutation", sorted(MUTATIONS))
def test_what_the_count_pins(mutation):
    """Each semantic marked True is one the reference count decides between the restated form and the alternative (the mutated
    oracle no longer returns 1420); each marked False is NOT pinned by it on this frame and stays on the independent pins."""
    name, moves = MUTATIONS[mutation]
    got = sum(total_with(mutation, load_gray("tum_room4_gray.png")))
    assert (got != REFERENCE_TOTAL) == moves, "%s: %d" % (name, got)


def test_decode_of_the_16_bit_frame_is_only_weakly_pinned():
    """imread(IMREAD_GRAYSCALE) of a 16-bit PNG strips to the high byte.  A scaled conversion (v*255/65535, rounded) changes three
    levels' counts (125, 62, 64 instead of 127, 63, 61) whose sum happens to be the same 251: a sum is a weak hash and the file says so."""
    a = load_gray("tum_room4_16bit.png").astype(np.uint32)      # the 16-bit original of the pinned frame, committed unchanged
    assert a.max() > 255
    assert np.array_equal((a >> 8).astype(np.uint8), load_gray("tum_room4_gray.png"))
    scaled = ((a * 255 + 32767) // 65535).astype(np.uint8)
    counts = total_with(0, scaled)
    assert counts[5:] == [125, 62, 64] and sum(counts) == REFERENCE_TOTAL


# ---- the same screenshot also shows WHERE the reference put its keypoints ------------------------------------------------------------------
# Its "ORB_SLAM3 extract keypoints" window is imshow(drawKeypoints(image, all levels' keypoints scaled to level 0)) at native size: a 512 x 512
# client area at (577, 315) of the capture, committed as tests/golden/screenshot_room4_window.png.  Every pixel no circle touches still
# holds the frame's gray value (R = G = B = pixel), every keypoint is an anti-aliased circle of radius 3 around its (sub-pixel) position.
def _window():
    win = np.array(__import__("PIL.Image", fromlist=["Image"]).open(__import__("os").path.join(__import__("helpers").GOLDEN, "screenshot_room4_window.png"))).astype(np.int32)
    gray = load_gray("tum_room4_gray.png").astype(np.int32)
    untouched = (win[:, :, 0] == gray) & (win[:, :, 1] == gray) & (win[:, :, 2] == gray)
    return win, gray, untouched


def drawn_vs_positions(x, y):
    """(drawn pixels farther than 5 px from every given position, positions without a drawn ring).  The circle the demo draws at (0, 0) — its
    output vector starts with default-constructed keypoints (main_orb_extractor.cpp:54-60) — is left out."""
    from scipy.spatial import cKDTree
    _, _, untouched = _window()
    my, mx = np.nonzero(~untouched)
    keep = ~((mx <= 6) & (my <= 6))
    drawn = np.stack([mx[keep], my[keep]], 1).astype(float)
    pts = np.stack([x, y], 1).astype(float)
    dist, _ = cKDTree(pts).query(drawn)
    tree = cKDTree(drawn)
    ringless = 0
    for p in pts:
        near = drawn[tree.query_ball_point(p, 4.6)]
        ringless += int((np.hypot(near[:, 0] - p[0], near[:, 1] - p[1]) >= 1.9).sum() < 12)
    return int((dist > 5.0).sum()), ringless


def test_the_screenshot_shows_this_frame_decoded_to_its_high_byte():
    """0.910 of the window's pixels equal tests/golden/tum_room4_gray.png EXACTLY (the rest lie under circles).  The other room4 frame gives
    0.24 and a scaled 16 -> 8 bit conversion of the right frame 0.60 (measured in the build container against the 16-bit original): the picture
    pins which frame it was and that imread(IMREAD_GRAYSCALE) kept the high byte — the one input-side semantic the keypoint total left open."""
    _, _, untouched = _window()
    assert 0.90 < untouched.mean() < 0.93


def test_oracle_keypoints_sit_where_the_reference_drew_them():
    """All 1420 positions: every circle pixel of the reference's picture lies within 5 px of an oracle keypoint (7 stray pixels of 23 400, at
    the rim of two dense clusters) and every oracle keypoint has its ring.  Positions, unlike the total, also respond to the half-extent
    rounding of DivideNode and to the order in which equal-sized nodes split (the oracle's DECLARED tie rule — newest first — fits the
    reference's picture, oldest first does not)."""
    o = O.Oracle(*REFERENCE_PARAMS)
    _, k, _ = o.extract(load_gray("tum_room4_gray.png"), (0, 1000))
    stray, ringless = drawn_vs_positions(k["x"], k["y"])
    assert stray <= 10 and ringless == 0, (stray, ringless)
    for mutation, name in ((12, "sort ties oldest first"), (13, "DivideNode floor")):
        om = O.Oracle(*REFERENCE_PARAMS)
        om.set_mutation(mutation)
        _, km, _ = om.extract(load_gray("tum_room4_gray.png"), (0, 1000))
        assert len(km) == REFERENCE_TOTAL                                  # the total does not see these two ...
        stray_m, _ = drawn_vs_positions(km["x"], km["y"])
        assert stray_m >= 3 * max(stray, 1), (name, stray_m)                # ... the positions do
    # a semantic the total already decides moves the positions far more
    om = O.Oracle(*REFERENCE_PARAMS)
    om.set_mutation(1)
    _, km, _ = om.extract(load_gray("tum_room4_gray.png"), (0, 1000))
    assert drawn_vs_positions(km["x"], km["y"])[0] > 300


@pytest.mark.gpu
def test_hip_path_reproduces_the_reference_screenshot_count():
    """The HIP path on the reference's frame with the reference's parameters: 1420 keypoints, and bit for bit the oracle's."""
    import extractorb_amd as X
    img = load_gray("tum_room4_gray.png")
    ex = X.ORBextractor(*REFERENCE_PARAMS, max_width=512, max_height=512)
    mono, k, d, lvl = ex(img, None, (0, 1000))
    assert sum(len(x) for x in lvl) == REFERENCE_TOTAL == len(k)
    o = O.Oracle(*REFERENCE_PARAMS)
    wmono, wk, wd = o.extract(img, (0, 1000))
    assert mono == wmono and k.tobytes() == wk.tobytes() and np.array_equal(d, wd)
    stray, ringless = drawn_vs_positions(k["x"], k["y"])          # ... and they sit where the reference's picture has its circles
    assert stray <= 10 and ringless == 0
    for l in range(8):
        assert lvl[l].tobytes() == o.level_keypoints(l).tobytes()
        assert ex.debug_candidates(l).tobytes() == o.candidates(l).tobytes()
    # the demo's second call shape: ORBextractor(5 * nFeatures) (main_orb_extractor.cpp:43 today): every candidate survives
    ex5 = X.ORBextractor(7500, 1.2, 8, 20, 7, max_width=512, max_height=512)
    _, k5, _, lvl5 = ex5(img, None, (0, 1000))
    o5 = O.Oracle(7500, 1.2, 8, 20, 7)
    _, wk5, _ = o5.extract(img, (0, 1000))
    assert len(k5) == 1547 and k5.tobytes() == wk5.tobytes()
