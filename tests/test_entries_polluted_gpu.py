"""Every device entry under polluted LDS.  The aid "lds_pollute" (include/orbx.h, orbx_debug_set_option) launches k_lds_pollute in front of
every kernel a handle enqueues, so LDS that a kernel reads without having written it holds a byte pattern instead of what the previous
launch - most often the same kernel on the same scene - left there.  One row per entry: its name, the kernels one accepted call launches,
and a body.  The body is an existing GPU check of that entry against its walk or oracle, on its smallest committed scene, called as a
function; it is run under the patterns 0xC3 (neither -1 nor a NaN in any width) and 0xFF (-1 / NaN).  Around every call of the entry the
row reads orbx_debug_lds_pollutions: it rises by the row's kernel count, so the second and later kernels of an entry are polluted too, and
the handle's policy string names the aid.  The CPU test compares the rows with the header: an entry added without a row fails."""
import numpy as np
import pytest

import extractorb_amd as X

# the extraction path is polluted through its own launch sequence and tested by tests/test_gpu_fuzz.py, test_describe_forms_gpu.py,
# test_fast_cell_edges.py and others; it has no row here
EXTRACTION = ("orbx_extract_batch_device",)
PATTERNS = (0xC3, 0xFF)


def _gpu_first():
    import torch
    torch.zeros(1).cuda()                               # torch asks for the GPU first


def _extractor(nlevels=8):
    _gpu_first()
    return X.ORBextractor(1000, 1.2, nlevels)


# ---- bodies (the test modules are imported inside: several load the library while they are imported, which torch has to precede) ----
def _stereo(tmp):
    import test_stereo_edges as T
    T.check_gpu_on_seed(77)                             # the crafted scenes at their committed seed


def _frame_finish(tmp):
    import test_frame_finish as T
    T.test_gpu_frame_finish_equals_oracle(T.PINHOLE)


def _frame_finish_two_eyes(tmp):
    import test_frame_finish as T
    T.test_gpu_two_eyes_grid_equals_oracle(T.PINHOLE)


def _search_init(tmp):
    import test_search_init_edges as T
    T.check_gpu_on_seed(T.SEED)


def _project_last(tmp):
    import test_search_projection as T
    T.test_gpu_frame_to_frame_pipeline_equals_oracle(True, 0.0, 15.0)


def _search_projection(tmp):
    import test_search_projection as T
    T.test_gpu_search_equals_oracle_on_random_scenes(1, False, False, True, 100)


def _search_projection_two_eyes(tmp):
    import test_search_projection_two_eyes as T
    T.test_gpu_crafted_chains(0)


def _kb8_project(tmp):
    import test_last_frame_two_eyes as T
    T.test_gpu_kb8_project_equals_the_host_compiled_header(T.build_kb8_host(tmp))


def _project_last_two_eyes(tmp):
    import test_last_frame_two_eyes as T
    T.test_gpu_front_half_equals_the_walk("crafted")


def _search_last_two_eyes(tmp):
    import test_last_frame_two_eyes as T
    T.test_gpu_crafted_scenes("closure_chain")


def _compute_bow(tmp):
    import test_bow as T
    T.test_gpu_bow_with_very_small_capacities(40, [33, 40])


def _search_bow(tmp):
    import test_search_bow as T
    T.test_gpu_search_by_bow_equals_oracle(T.CASES[3])              # 300 keyframe features, 500 frame features, 3 nodes


def _search_bow_keyframes(tmp):
    import test_search_bow as T
    T.test_gpu_keyframe_search_by_bow_equals_oracle(T.CASES[3])


def _search_bow_two_eyes(tmp):
    """the committed batch test runs thirteen searches under every parameter set: here its smallest search alone, under its own parameters"""
    import test_search_bow_two_eyes as T
    case = T.CASES[3]                                   # 200 + 180 keyframe features, 300 + 280 frame features, 3 nodes
    s = T.make(case)
    nn, th, chk = T.params(case)
    m, nm = T.run_searches(X.ORBextractor(1200), [s], T.CAP_1200, nn, th, chk)
    assert T.assert_equals_walk(s, m[0], nm[0], nn, th, chk, "polluted")["n"] > 0


def _search_triangulation(tmp):
    """check_gpu_on_seed's body on scenes of 300 features in 20 nodes instead of 1200 in 100, at the capacity that holds them"""
    import test_search_triangulation as T
    searches = [T.scene(k, 11, 300, 20) for k in T.STANDARD]
    cap = 304
    dv = T.pack([k for s in searches for k in (s["kf1"], s["kf2"])], cap)
    m, pr, nm = T.run(X.ORBextractor(1200), dv, searches, (0, 2), (1, 2), cap)
    assert sum(T.assert_equals_walk(s, m[i], pr[i], nm[i], "polluted scene %d" % i)["n"] for i, s in enumerate(searches)) > 30


def _fuse(tmp):
    import test_fuse_gpu as T
    T.check_gpu_on_seed(21, reproj_check=False, th=5.0)


def _fuse_two_eyes(tmp):
    import test_fuse_two_eyes_gpu as T
    T.check_gpu_on_seed(21, th=4.0)


def _sim3_search(tmp):
    import test_sim3_projection_gpu as T
    T.test_gpu_every_case_in_both_projection_forms("gates_15")


def _frustum(tmp):
    import frustum_walk as W
    import test_frustum_requests_gpu as T
    T.test_gpu_crafted_points_in_both_modes(W.LOCAL_MAP)


def _frustum_two_eyes(tmp):
    import test_frustum_requests_two_eyes_gpu as T
    T.test_gpu_crafted_points_of_both_rigs("narrow")


def _search_triangulation_two_eyes(tmp):
    import test_search_triangulation_two_eyes_gpu as T
    T.test_gpu_crafted_scene_equals_the_walk()


def _kb8_unproject(tmp):
    import test_kb8_unproject_math as M
    import test_search_triangulation_two_eyes_gpu as T
    T.test_gpu_unproject_equals_the_host_compiled_header(M.build_kb8_unproject_host(tmp))


def _kb8_triangulate(tmp):
    import test_kb8_unproject_math as M
    import test_search_triangulation_two_eyes_gpu as T
    T.test_gpu_triangulate_equals_the_host_compiled_header(M.build_kb8_unproject_host(tmp))


def _stereo_fisheye(tmp):
    import test_stereo_fisheye_gpu as T
    T.test_gpu_crafted_scene_equals_the_walk_twice()


def _new_map_points(tmp):
    import test_new_map_points_gpu as T
    T.test_gpu_crafted_scene_equals_the_walk(False)


def _new_map_points_two_eyes(tmp):
    import test_new_map_points_gpu as T
    T.test_gpu_crafted_scene_equals_the_walk(True)


def _update_map_points(tmp):
    import test_map_point_update_gpu as T
    T.test_gpu_crafted_points(False)


def _update_map_points_two_eyes(tmp):
    import test_map_point_update_gpu as T
    T.test_gpu_crafted_points(True)


def _two_view(tmp):
    import test_two_view_gpu as T
    T.test_gpu_scene_equals_the_walk(_extractor(), "n65_it1")


def _sim3_solve(tmp):
    import sim3_solver_scenes as SC
    import test_sim3_solver_gpu as T
    T.test_gpu_scene_equals_the_walk(_extractor(SC.NLEVELS), "n16_it20")


def _optimize_pose(tmp):
    import pose_optimization_scenes as SC
    import test_pose_optimization_gpu as T
    T.test_gpu_scene_equals_the_walk(_extractor(SC.NLEVELS), "mono_n65")


def _detect_candidates(tmp):
    import test_place_recognition_gpu as T
    ex = _extractor()
    voc = X.Vocabulary(arrays=T.make_vocab(np.random.default_rng(3), k=3, L=2))      # the module's vocabulary (L1_NORM)
    T.test_gpu_scene_equals_the_walk(ex, voc, "nbest_db65_q3")


def _covisibility(tmp):
    import test_covisibility_gpu as T
    T.test_gpu_scene_equals_the_walk(_extractor(), "update_th_14_15_16")


def _keyframe_redundancy(tmp):
    import test_covisibility_gpu as T
    T.test_gpu_scene_equals_the_walk(_extractor(), "redundancy_observations_3_and_4")


def _stereo_from_rgbd(tmp):
    import test_rgbd as T
    T.test_gpu_rgbd_equals_oracle_after_extraction_and_undistortion(np.uint16, 1.0, 6)


def _gray(tmp):
    import test_gray as T
    T.test_gpu_gray_equals_oracle_and_feeds_the_extractor(3, True, 37, 5)


# (entry without its orbx_ prefix = the ORBextractor method, kernels an accepted call launches, body)
ROWS = [
    ("stereo_match_device", 3, _stereo),                                # k_stereo_rows, k_stereo_match, k_stereo_filter
    ("frame_finish_device", 1, _frame_finish),
    ("frame_finish_two_eyes_device", 1, _frame_finish_two_eyes),
    ("search_for_initialization_device", 1, _search_init),
    ("project_last_frame_device", 1, _project_last),
    ("search_by_projection_device", 1, _search_projection),
    ("search_by_projection_two_eyes_device", 1, _search_projection_two_eyes),
    ("kb8_project_device", 1, _kb8_project),
    ("project_last_frame_two_eyes_device", 1, _project_last_two_eyes),
    ("search_last_frame_two_eyes_device", 1, _search_last_two_eyes),
    ("compute_bow_device", 2, _compute_bow),                            # k_bow_words, k_bow_reduce
    ("search_by_bow_device", 1, _search_bow),
    ("search_by_bow_keyframes_device", 1, _search_bow_keyframes),
    ("search_by_bow_two_eyes_device", 1, _search_bow_two_eyes),
    ("search_for_triangulation_device", 1, _search_triangulation),
    ("fuse_device", 1, _fuse),
    ("fuse_two_eyes_device", 1, _fuse_two_eyes),
    ("search_by_projection_sim3_device", 2, _sim3_search),              # k_sim3_window, k_sim3_settle
    ("frustum_requests_device", 1, _frustum),
    ("frustum_requests_two_eyes_device", 2, _frustum_two_eyes),         # k_frustum_two_eyes_check, k_frustum_two_eyes_place
    ("search_for_triangulation_two_eyes_device", 1, _search_triangulation_two_eyes),
    ("kb8_unproject_device", 1, _kb8_unproject),
    ("kb8_triangulate_device", 1, _kb8_triangulate),
    ("stereo_fisheye_match_device", 2, _stereo_fisheye),                # k_stereo_fisheye_init, k_stereo_fisheye
    ("create_new_map_points_device", 2, _new_map_points),               # k_new_map_points_init, k_new_map_points
    ("create_new_map_points_two_eyes_device", 2, _new_map_points_two_eyes),
    ("update_map_points_device", 1, _update_map_points),
    ("update_map_points_two_eyes_device", 1, _update_map_points_two_eyes),
    ("reconstruct_two_views_device", 3, _two_view),                     # k_two_view_prepare, one k_two_view_hypotheses form, k_two_view_decide
    ("sim3_solve_device", 3, _sim3_solve),                              # k_sim3_prepare, k_sim3_hypotheses, k_sim3_decide
    ("optimize_pose_device", 1, _optimize_pose),
    ("detect_candidates_device", 2, _detect_candidates),                # k_place_pairs (the database is not empty), k_place_query
    ("covisibility_device", 2, _covisibility),                          # k_covis_rank, k_covis_vote
    ("keyframe_redundancy_device", 1, _keyframe_redundancy),
    ("stereo_from_rgbd_device", 1, _stereo_from_rgbd),
    ("gray_from_color_device", 1, _gray),
]


def test_every_device_entry_has_a_row():
    entries = [s for s in X.header_symbols() if s.startswith("orbx_") and s.endswith("_device")]
    assert set(EXTRACTION) <= set(entries)
    names = [r[0] for r in ROWS]
    assert len(set(names)) == len(names)
    assert sorted("orbx_" + n for n in names) == sorted(s for s in entries if s not in EXTRACTION)
    assert all(callable(getattr(X.ORBextractor, n, None)) for n in names)
    assert all(isinstance(k, int) and k >= 1 for _, k, _ in ROWS)
    assert sum(k > 1 for _, k, _ in ROWS) >= 9                          # the entries of several kernels are among them


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", PATTERNS, ids=["0x%02X" % p for p in PATTERNS])
@pytest.mark.parametrize("name,kernels,body", ROWS, ids=[r[0] for r in ROWS])
def test_gpu_entry_under_polluted_lds(name, kernels, body, pattern, monkeypatch, tmp_path):
    _gpu_first()
    X.debug_set_option("lds_pollute", pattern)          # before any handle is made; tests/conftest.py resets the aids after the test
    entry = getattr(X.ORBextractor, name)
    rises = []

    def counted(self, *args, **kw):
        assert "lds_pollute:%d" % pattern in self.policy(), self.policy()
        before = self.lds_pollutions()
        out = entry(self, *args, **kw)                  # (a refused call raises here: it launches nothing and is not counted)
        rises.append(self.lds_pollutions() - before)
        return out

    monkeypatch.setattr(X.ORBextractor, name, counted)
    body(tmp_path)                                      # the body's own exact comparison
    assert rises and all(r == kernels for r in rises), (name, kernels, rises)
