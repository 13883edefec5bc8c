"""Every *_device entry of extractorb_amd/csrc/orbx_rows.cpp refuses what include/orbx.h says it refuses, with the documented code, and before
anything is launched: one handle, every pointer a real zero-filled device tensor, one bad argument per call.  The table is written from the
header and from the checks the entries have always made; it does not ask the library what it would answer, so the same file passes against
an earlier build of the library (ORBX_LIBRARY).

What is left to other files: a refused call whose refusal needs an extraction first (orbx_stereo_match_device checks the handle's last batch
before its capacity: tests/test_stereo_edges.py), and every accepted call (the parity tests of each entry)."""
import ctypes as C

import numpy as np
import pytest

import extractorb_amd as X
from test_bow import make_vocab

BAD, UNSUPPORTED = -2, -8      # ORBX_ERR_BAD_ARGUMENT, ORBX_ERR_UNSUPPORTED (include/orbx.h)
N, CAP, MP_CAP, Q_CAP, LEVELS = 1, 8, 8, 8, 8
LDS = 160 * 1024 - 512         # "160 KB per CU" of the header's bounds: 163 328 bytes
BOUNDS = np.array([0, 640, 0, 480], np.float32)
HOST = dict(cam=np.array([500, 500, 320, 240, 0, 0, 0, 0, 0], np.float32), cam_kb8=np.array([190, 190, 254, 256, 0, 0, 0, 0], np.float32),
            cam_right=np.array([190, 190, 254, 256, 0, 0, 0, 0], np.float32), bounds4=BOUNDS,
            trl12=np.eye(3, 4, dtype=np.float32).ravel().copy(), tlr12=np.eye(3, 4, dtype=np.float32).ravel().copy())
FRAMES = 4                     # frames the per-frame buffers hold: two rigs of two eyes
GRID = 64 * 48 + 1
DEVICE_BYTES = dict(           # the size of every device buffer at the shapes above
    d_kps=FRAMES * CAP * 28, d_kps_un=FRAMES * CAP * 28, d_desc=FRAMES * CAP * 32, d_n_out=FRAMES * 4, d_u_right=FRAMES * CAP * 4, d_depth=FRAMES * CAP * 4,
    d_n_matched=FRAMES * 4, d_depth_map=FRAMES * 480 * 640 * 4, d_depth_out=FRAMES * CAP * 4, d_src=FRAMES * 480 * 640 * 4, d_gray=FRAMES * 480 * 640,
    d_grid_off=FRAMES * GRID * 4, d_grid_idx=FRAMES * CAP * 4, d_n_inside=FRAMES * 4, d_prev_matched=FRAMES * CAP * 8, d_matches=FRAMES * 2 * CAP * 4,
    d_n_matches=FRAMES * 4, d_mp_flags=FRAMES * max(CAP, MP_CAP), d_mp_flags2=FRAMES * CAP, d_world=FRAMES * CAP * 12, d_poses=FRAMES * 48,
    d_queries=FRAMES * 2 * max(CAP, MP_CAP) * 2 * 32, d_query_desc=FRAMES * 2 * max(CAP, MP_CAP) * 2 * 32, d_n_queries=FRAMES * 4, d_occupied=FRAMES * 2 * CAP,
    d_left_to_right=FRAMES * CAP * 4, d_right_to_left=FRAMES * CAP * 4, d_xyz=4 * 12, d_uv=4 * 8, d_word_ids=FRAMES * CAP * 4, d_word_weights=FRAMES * CAP * 8,
    d_n_words=FRAMES * 4, d_feat_nodes=FRAMES * CAP * 4, d_feat_idx=FRAMES * CAP * 4, d_n_feat=FRAMES * 4, d_f12=N * 36, d_epipole=N * 8, d_pairs=N * CAP * 8,
    d_mp_world=N * MP_CAP * 12, d_mp_normal=N * MP_CAP * 12, d_mp_dist=N * MP_CAP * 12, d_mp_desc=N * MP_CAP * 32, d_mp_angle=N * MP_CAP * 4, d_n_mp=N * 4,
    d_mp_prev_depth=N * MP_CAP * 4, d_best_idx=N * MP_CAP * 4, d_best_dist=N * MP_CAP * 4, d_exit=N * MP_CAP * 2, d_n_fused=N * 4, d_match_idx=N * MP_CAP * 4,
    d_match_dist=N * MP_CAP * 4, d_query_src=N * MP_CAP * 4, d_n_wanted=N * 4, d_track=N * MP_CAP * 2 * 28, d_n_in_view=N * 4)


def D(name):
    return (name, "device")


def H(name):
    return (name, "host")


WALK_A = [("a_first", 0), ("a_step", 1)]
WALK_B = [("b_first", 0), ("b_step", 1)]
BOW = [("n", N)] + WALK_A + WALK_B + [D("d_feat_nodes"), D("d_feat_idx"), D("d_n_feat"), D("d_mp_flags")]
BOW_TAIL = [D("d_kps"), D("d_desc"), D("d_n_out"), ("capacity", CAP), ("nn_ratio", 0.7), ("th_low", 50), ("check_orientation", 1), D("d_matches"), D("d_n_matches")]
MAP_POINTS = [("n", N)] + WALK_A + WALK_B + [D("d_mp_world"), D("d_mp_normal"), D("d_mp_dist"), D("d_mp_desc")]

# entry -> its parameters after the handle, in the header's order: (name, value), D(name) for a device buffer, H(name) for a host array
ENTRIES = {
    "orbx_stereo_match_device": [("n", N), D("d_kps"), D("d_desc"), D("d_n_out"), ("capacity", CAP), ("bf", 40.0), ("b", 0.1), D("d_u_right"), D("d_depth"),
                                 D("d_n_matched")],
    "orbx_stereo_from_rgbd_device": [("n", N), D("d_kps"), D("d_kps_un"), D("d_n_out"), ("capacity", CAP), D("d_depth_map"), ("depth_is_u16", 0), ("rows", 480),
                                     ("cols", 640), ("stride", 640 * 4), ("frame_stride", 480 * 640 * 4), ("factor", 1.0), ("mbf", 40.0), D("d_u_right"),
                                     D("d_depth_out")],
    "orbx_gray_from_color_device": [("n", N), D("d_src"), ("rows", 480), ("cols", 640), ("channels", 3), ("red_first", 1), ("src_stride", 640 * 3),
                                    ("src_frame_stride", 480 * 640 * 3), D("d_gray"), ("gray_stride", 640), ("gray_frame_stride", 480 * 640)],
    "orbx_frame_finish_device": [("n", N), D("d_kps"), D("d_n_out"), ("capacity", CAP), H("cam"), H("bounds4"), D("d_kps_un"), D("d_grid_off"), D("d_grid_idx"),
                                 D("d_n_inside")],
    "orbx_frame_finish_two_eyes_device": [("n", N), D("d_kps"), D("d_n_out"), ("capacity", CAP), H("cam"), H("bounds4"), D("d_kps_un"), D("d_grid_off"),
                                          D("d_grid_idx"), D("d_n_inside")],
    "orbx_search_for_initialization_device": [("n", N)] + WALK_A + WALK_B + [D("d_kps_un"), D("d_desc"), D("d_n_out"), ("capacity", CAP), D("d_grid_off"),
                                                                             D("d_grid_idx"), H("bounds4"), D("d_prev_matched"), ("window", 100), ("nn_ratio", 0.9),
                                                                             ("check_orientation", 1), D("d_matches"), D("d_n_matches")],
    "orbx_project_last_frame_device": [("n", N)] + WALK_A + WALK_B + [D("d_kps"), D("d_kps_un"), D("d_n_out"), ("capacity", CAP), D("d_mp_flags"), D("d_world"),
                                                                      D("d_poses"), H("cam"), H("bounds4"), ("mbf", 40.0), ("mb", 0.1), ("th", 7.0), ("mono", 0),
                                                                      D("d_queries")],
    "orbx_search_by_projection_device": [("n", N)] + WALK_A + [D("d_queries"), D("d_query_desc")] + WALK_B + [
        D("d_n_queries"), ("query_capacity", Q_CAP), D("d_kps_un"), D("d_desc"), D("d_n_out"), ("capacity", CAP), D("d_grid_off"), D("d_grid_idx"), H("bounds4"),
        D("d_u_right"), D("d_occupied"), ("ratio_mode", 0), ("nn_ratio", 0.9), ("max_distance", 100), ("check_orientation", 1), D("d_matches"), D("d_n_matches")],
    "orbx_search_by_projection_two_eyes_device": [("n", N)] + WALK_A + [D("d_queries"), D("d_query_desc")] + WALK_B + [
        D("d_n_queries"), ("query_capacity", Q_CAP), D("d_kps"), D("d_desc"), D("d_n_out"), ("capacity", CAP), D("d_grid_off"), D("d_grid_idx"), H("bounds4"),
        D("d_left_to_right"), D("d_right_to_left"), D("d_occupied"), ("nn_ratio", 0.8), ("max_distance", 100), D("d_matches"), D("d_n_matches")],
    "orbx_kb8_project_device": [("n", 4), D("d_xyz"), H("cam_kb8"), D("d_uv")],
    "orbx_project_last_frame_two_eyes_device": [("n", N)] + WALK_A + WALK_B + [D("d_kps"), D("d_n_out"), ("capacity", CAP), D("d_mp_flags"), D("d_world"),
                                                                               D("d_poses"), H("trl12"), H("cam_kb8"), H("bounds4"), ("mb", 0.1), ("th", 7.0),
                                                                               ("mono", 0), D("d_queries")],
    "orbx_search_last_frame_two_eyes_device": [("n", N)] + WALK_A + [D("d_queries"), D("d_query_desc"), D("d_kps"), D("d_desc"), D("d_n_out"), ("capacity", CAP),
                                                                     D("d_grid_off"), D("d_grid_idx"), H("bounds4"), D("d_occupied"), ("max_distance", 100),
                                                                     ("check_orientation", 1), D("d_matches"), D("d_n_matches")],
    "orbx_compute_bow_device": [("vocabulary", "vocabulary"), ("n", N), D("d_desc"), D("d_n_out"), ("capacity", CAP), ("levels_up", 4), D("d_word_ids"),
                                D("d_word_weights"), D("d_n_words"), D("d_feat_nodes"), D("d_feat_idx"), D("d_n_feat")],
    "orbx_search_by_bow_device": BOW + BOW_TAIL,
    "orbx_search_by_bow_keyframes_device": BOW + [D("d_mp_flags2")] + BOW_TAIL,
    "orbx_search_by_bow_two_eyes_device": BOW + BOW_TAIL,
    "orbx_search_for_triangulation_device": BOW + [D("d_mp_flags2"), D("d_kps_un"), D("d_u_right"), D("d_desc"), D("d_n_out"), ("capacity", CAP), D("d_f12"),
                                                   D("d_epipole"), ("only_stereo", 0), ("coarse", 0), ("th_low", 50), ("check_orientation", 1), D("d_matches"),
                                                   D("d_pairs"), D("d_n_matches")],
    "orbx_fuse_device": MAP_POINTS + [D("d_n_mp"), ("mp_capacity", MP_CAP), D("d_mp_flags"), D("d_poses"), D("d_kps_un"), D("d_u_right"), D("d_desc"), D("d_n_out"),
                                      ("capacity", CAP), D("d_grid_off"), D("d_grid_idx"), H("bounds4"), H("cam"), ("nlevels", LEVELS), ("mbf", 40.0), ("th", 3.0),
                                      ("th_low", 50), ("reproj_check", 1), D("d_best_idx"), D("d_best_dist"), D("d_exit"), D("d_n_fused")],
    "orbx_search_by_projection_sim3_device": MAP_POINTS + [D("d_n_mp"), ("mp_capacity", MP_CAP), D("d_mp_flags"), D("d_poses"), D("d_kps_un"), D("d_desc"),
                                                           D("d_n_out"), ("capacity", CAP), D("d_grid_off"), D("d_grid_idx"), H("bounds4"), H("cam"),
                                                           ("nlevels", LEVELS), ("projection", 0), ("th", 3.0), ("th_low", 50), ("ratio_hamming", 1.0),
                                                           D("d_occupied"), D("d_matches"), D("d_match_idx"), D("d_match_dist"), D("d_exit"), D("d_n_matches")],
    "orbx_frustum_requests_device": MAP_POINTS + [D("d_mp_angle"), D("d_n_mp"), ("mp_capacity", MP_CAP), D("d_mp_flags"), D("d_poses"), H("cam"), H("bounds4"),
                                                  ("nlevels", LEVELS), ("mode", 0), ("mbf", 40.0), ("view_cos_limit", 0.5), ("th", 1.0), ("far_points", 0),
                                                  ("th_far_points", 0.0), D("d_queries"), D("d_query_desc"), D("d_query_src"), D("d_n_queries"), D("d_track"),
                                                  D("d_n_in_view")],
    "orbx_frustum_requests_two_eyes_device": MAP_POINTS + [D("d_n_mp"), ("mp_capacity", MP_CAP), D("d_mp_flags"), D("d_mp_prev_depth"), D("d_poses"), H("trl12"),
                                                           H("tlr12"), H("cam_kb8"), H("cam_right"), H("bounds4"), ("nlevels", LEVELS), ("view_cos_limit", 0.5),
                                                           ("th", 1.0), ("far_points", 0), ("th_far_points", 0.0), ("query_capacity", Q_CAP), D("d_queries"),
                                                           D("d_query_desc"), D("d_query_src"), D("d_n_queries"), D("d_n_wanted"), D("d_track"), D("d_n_in_view")],
}


def first_refused(lds_bytes):
    """the smallest capacity whose tables, by the header's formula, no longer fit"""
    return next(c for c in range(1, 70000) if lds_bytes(c) > LDS)


def up(c, m):
    return (c + m - 1) // m * m


# the LDS bounds as include/orbx.h states them (the one-camera projection and BoW searches: as their kernels' tables are laid out)
PAST_LDS = {
    "orbx_search_by_projection_device": first_refused(lambda c: 62 * up(c, 4) + 5 * Q_CAP + (30 + 4) * 4 + (64 * 48 + 2) * 2 + 64),
    "orbx_search_by_projection_two_eyes_device": first_refused(lambda c: 100 * up(c, 4) + 8 * Q_CAP + 12392),
    "orbx_search_last_frame_two_eyes_device": first_refused(lambda c: 96 * up(c, 4) + 12 * c + 12496),
    "orbx_search_by_bow_two_eyes_device": first_refused(lambda c: 40 * up(c, 16) + 64),
    "orbx_search_for_triangulation_device": first_refused(lambda c: 28 * up(c, 16) + 64),
    "orbx_search_by_projection_sim3_device": first_refused(lambda c: 4 * (c + MP_CAP) + 64),
    "orbx_search_by_bow_device": next(c for c in range(1, 70000) if 22 * up(c, 16) + 64 > 150 * 1024),      # this entry's bound is 150 KB
}
PAST_LDS["orbx_search_by_bow_keyframes_device"] = PAST_LDS["orbx_search_by_bow_device"]

NEEDS = "first_null last_null capacity_0 n_0"      # what every entry refuses
# entry -> (first required pointer, last required pointer, the rejection classes it has beyond NEEDS)
RULES = {
    "orbx_stereo_match_device": ("d_kps", "d_n_matched", ""),
    "orbx_stereo_from_rgbd_device": ("d_kps", "d_depth_out", "n_65536"),
    "orbx_gray_from_color_device": ("d_src", "d_gray", "n_65536 no_capacity"),
    "orbx_frame_finish_device": ("d_kps", "d_n_inside", "empty_bounds capacity_32768"),
    "orbx_frame_finish_two_eyes_device": ("d_kps", "d_n_inside", "empty_bounds capacity_32768"),
    "orbx_search_for_initialization_device": ("d_kps_un", "d_n_matches", "negative_first walk_below_zero negative_step empty_bounds capacity_32768"),
    "orbx_project_last_frame_device": ("d_kps", "d_queries", "n_65536 negative_first walk_below_zero negative_step empty_bounds"),
    "orbx_search_by_projection_device": ("d_queries", "d_n_matches", "negative_first walk_below_zero negative_step empty_bounds capacity_32768 past_lds"),
    "orbx_search_by_projection_two_eyes_device": ("d_queries", "d_n_matches",
                                                  "negative_first walk_below_zero negative_step empty_bounds capacity_32768_unsupported past_lds"),
    "orbx_kb8_project_device": ("d_xyz", "d_uv", "no_capacity"),
    "orbx_project_last_frame_two_eyes_device": ("d_kps", "d_queries", "n_65536 negative_first walk_below_zero negative_step empty_bounds"),
    "orbx_search_last_frame_two_eyes_device": ("d_queries", "d_n_matches", "negative_first walk_below_zero negative_step empty_bounds past_lds"),
    "orbx_compute_bow_device": ("vocabulary", "d_n_feat", "n_65536 capacity_16385"),
    "orbx_search_by_bow_device": ("d_feat_nodes", "d_n_matches", "negative_first walk_below_zero past_lds"),
    "orbx_search_by_bow_keyframes_device": ("d_feat_nodes", "d_n_matches", "negative_first walk_below_zero past_lds second_flags_null"),
    "orbx_search_by_bow_two_eyes_device": ("d_feat_nodes", "d_n_matches", "negative_first walk_below_zero past_lds"),
    "orbx_search_for_triangulation_device": ("d_feat_nodes", "d_n_matches", "negative_first walk_below_zero past_lds"),
    "orbx_fuse_device": ("d_mp_world", "d_n_fused", "n_65536 negative_first walk_below_zero empty_bounds other_nlevels mp_capacity_0"),
    "orbx_search_by_projection_sim3_device": ("d_mp_world", "d_n_matches",
                                              "n_65536 negative_first walk_below_zero empty_bounds other_nlevels mp_capacity_0 past_lds"),
    "orbx_frustum_requests_device": ("d_mp_world", "d_n_in_view", "negative_first walk_below_zero other_nlevels no_capacity mp_capacity_0"),
    "orbx_frustum_requests_two_eyes_device": ("d_mp_world", "d_n_in_view", "n_65536 negative_first walk_below_zero other_nlevels no_capacity mp_capacity_0"),
}
EMPTY_BOUNDS = np.array([0, 0, 0, 480], np.float32)


def cases_of(entry):
    """[(label, {parameter: value}, expected code)]: one bad argument each"""
    first, last, extra = RULES[entry]
    classes = (NEEDS + " " + extra).split()
    if "no_capacity" in classes:
        classes = [c for c in classes if c not in ("no_capacity", "capacity_0")]
    w = "b" if ("b_first", 0) in ENTRIES[entry] else "a"      # the entry's last (first, step) pair
    table = {
        "first_null": ({first: None}, BAD), "last_null": ({last: None}, BAD), "capacity_0": (dict(capacity=0), BAD), "mp_capacity_0": (dict(mp_capacity=0), BAD),
        "n_0": (dict(n=0), BAD), "n_65536": (dict(n=65536), BAD), "negative_first": (dict(a_first=-1), BAD),
        "walk_below_zero": ({w + "_first": 0, w + "_step": -1, "n": 2}, BAD),      # pair 1 would read frame -1: both walk rules refuse it
        "negative_step": (dict(a_first=5, a_step=-1), BAD),                        # no index is negative: refused where the entry tests the step itself
        "empty_bounds": (dict(bounds4=EMPTY_BOUNDS), BAD), "other_nlevels": (dict(nlevels=LEVELS + 1), BAD),
        "capacity_32768": (dict(capacity=32768), UNSUPPORTED), "capacity_32768_unsupported": (dict(capacity=32768), UNSUPPORTED),
        "capacity_16385": (dict(capacity=16385), UNSUPPORTED), "past_lds": (dict(capacity=PAST_LDS.get(entry, 0)), UNSUPPORTED),
        "second_flags_null": (dict(d_mp_flags2=None), BAD),
    }
    return [(c,) + table[c] for c in classes]


def test_the_table_names_every_device_entry_of_the_rows_file():
    import os
    import re
    src = open(os.path.join(os.path.dirname(X.orbextractor.__file__), "csrc", "orbx_rows.cpp")).read()
    assert set(re.findall(r"^int (orbx_\w+_device)\(", src, flags=re.M)) == set(ENTRIES) == set(RULES)
    # the documented figures the formulas above must reproduce (include/orbx.h)
    assert PAST_LDS["orbx_search_by_bow_two_eyes_device"] == 4081 and PAST_LDS["orbx_search_for_triangulation_device"] == 5825
    assert PAST_LDS["orbx_search_last_frame_two_eyes_device"] == 1397 and PAST_LDS["orbx_search_by_projection_device"] <= 32767
    for entry in ENTRIES:
        names = [name for name, _ in ENTRIES[entry]]
        for label, change, _ in cases_of(entry):
            assert set(change) <= set(names), (entry, label)
        assert len(getattr(X.load_library(), entry).argtypes) == 1 + len(names), entry


@pytest.mark.gpu
def test_every_rejection_class_of_every_entry():
    import torch
    L = X.load_library()
    ex = X.ORBextractor()                                   # default sizes: 1000 features, 8 levels, 640 x 480, one frame
    assert ex.nlevels == LEVELS
    voc = X.Vocabulary(arrays=make_vocab(np.random.default_rng(3), k=3, L=2))
    dev = dict((name, torch.zeros(nbytes, dtype=torch.uint8, device="cuda")) for name, nbytes in DEVICE_BYTES.items())
    torch.cuda.synchronize()
    seen, wrong = 0, []
    for entry, params in ENTRIES.items():
        fn = getattr(L, entry)
        for label, change, want in cases_of(entry):
            args, keep = [ex._h], []
            for name, value in params:
                if name in change:
                    value = change[name]
                    if isinstance(value, np.ndarray):
                        keep.append(value); value = value.ctypes.data_as(C.c_void_p)
                elif value == "device":
                    value = C.c_void_p(dev[name].data_ptr())
                elif value == "host":
                    value = HOST[name].ctypes.data_as(C.c_void_p)
                elif value == "vocabulary":
                    value = voc._v
                args.append(value)
            got = fn(*args)
            seen += 1
            if got != want:
                wrong.append((entry, label, got, want, (L.orbx_last_error(ex._h) or b"").decode()))
    assert not wrong, wrong
    assert seen >= 150
    ex.synchronize()                                        # nothing was launched, and nothing that was refused left the stream in error
    assert all(int(t.count_nonzero()) == 0 for t in dev.values())
