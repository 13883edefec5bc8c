"""orbx_reconstruct_two_views_device on the GPU: the scenes of tests/two_view_scenes.py through the C ABI against the binary32 walk
(tests/two_view_walk.py), byte for byte - result rows, p3d, flags, the pruned match tables and counts, poison beyond n - and one chain
from a real orbx_search_for_initialization_device output at 320x240, with prune = 1 feeding a second call."""
import numpy as np
import pytest

import extractorb_amd as X
import two_view_scenes as SC
import two_view_walk as TW

f32 = np.float32


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda()


def gpu_run(ex, s, outputs=None):
    """one call on the scene's arrays; returns the outputs as host arrays shaped like SC.expected's"""
    import torch
    o = outputs or SC.poisoned_outputs(s)
    d = dict((k, _dev(v)) for k, v in o.items())
    kps, n_out, rnd = _dev(s["kps"]), _dev(s["n_out"]), _dev(s["rand"])
    torch.cuda.synchronize()                            # torch's copies have landed before the handle's stream runs
    ex.reconstruct_two_views_device(s["pairs"], s["frames1"], s["frames2"], kps, n_out, s["cap"], d["matches"], d["n_matches"], X.camera(*s["cam"]),
                                    rnd, d["result"], d["p3d"], d["tri"], s["sigma"], s["iterations"], s["min_parallax"], s["min_triangulated"],
                                    s["rh_threshold"], s["prune"])
    ex.synchronize()
    out = dict((k, v.cpu().numpy()) for k, v in d.items())
    out["result"] = out["result"].view(SC.RESULT_DTYPE).reshape(-1)
    return out


@pytest.fixture(scope="module")
def ex():
    import torch
    torch.zeros(1).cuda()                               # torch asks for the GPU first
    return X.ORBextractor(1000, 1.2, 8)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SC.CASES))
def test_gpu_scene_equals_the_walk(ex, name):
    s = SC.case(name)
    walked, want = SC.case_expected(name)
    got = gpu_run(ex, s)
    assert SC.differences(got, want) == [], [(TW.STATUS[a] if 0 <= a < 13 else a, TW.STATUS[b]) for a, b in zip(got["result"]["status"], want["result"]["status"])]
    n1 = int(s["n_out"][s["frames1"][0]])
    assert (got["tri"][:, n1:] == SC.POISON_B).all() and (got["p3d"][:, n1:] == SC.POISON_F).all()      # nothing beyond n of frame 1


@pytest.mark.gpu
def test_gpu_without_prune_the_table_is_not_written(ex):
    s = dict(SC.case("general_n96_it200"), prune=0)
    want = SC.expected(s, SC.case_expected("general_n96_it200")[0])
    got = gpu_run(ex, s)
    assert SC.differences(got, want) == [] and np.array_equal(got["matches"], s["matches"]) and got["result"]["status"][0] == TW.ACCEPTED_F


@pytest.mark.gpu
def test_gpu_a_smaller_call_after_a_larger_one_reuses_the_workspace(ex):
    for name in ("n300", "n8_sets_are_permutations", "one_against_many"):
        assert SC.differences(gpu_run(ex, SC.case(name)), SC.case_expected(name)[1]) == [], name


@pytest.mark.gpu
def test_gpu_both_hypothesis_kernels_equal_the_walk(ex):
    """the one-lane kernel (shape 0) beside the default, the rows over the lanes (shape 1, which every other test here runs)"""
    try:
        ex.two_view_shape(0)
        for name in ("plane_n64_it65", "general_n96_it200", "n300", "n8_sets_are_permutations", "nan_parallax_all_far"):
            assert SC.differences(gpu_run(ex, SC.case(name)), SC.case_expected(name)[1]) == [], name
    finally:
        ex.two_view_shape(1)
    assert SC.differences(gpu_run(ex, SC.case("plane_n64_it65")), SC.case_expected("plane_n64_it65")[1]) == []


@pytest.mark.gpu
def test_gpu_chained_with_the_initialisation_search():
    """extraction -> frame_finish -> SearchForInitialization -> here, all on the device at 320x240, on two layered scenes with real parallax
    (two_view_scenes.parallax_pair); the match table goes in as the search wrote it.  The first call is accepted and, with prune = 1,
    lowers d_n_matches; the second call reads the pruned table: its N is the first call's count.  Both calls against the walk on the
    tables copied back."""
    import torch
    from test_search_init import PINHOLE
    frames = np.stack([f for seed in (401, 402) for f in SC.parallax_pair(seed, shifts=(1, 40))])
    B, rows, cols, P, iters = 4, 240, 320, 2, 48
    e = X.ORBextractor(1000, max_batch=B, max_width=cols, max_height=rows)
    cap = e.capacity
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    d_k = torch.zeros((B, cap, 7), dtype=torch.float32, device="cuda"); d_d = torch.zeros((B, cap, 32), dtype=torch.uint8, device="cuda")
    d_n = torch.zeros(B, dtype=torch.int32, device="cuda"); d_m = torch.zeros(B, dtype=torch.int32, device="cuda")
    e.extract_batch_device(torch.from_numpy(frames).cuda(), B, rows, cols, d_k, d_d, d_n, d_m, cap)
    c = X.camera(**PINHOLE)
    bounds = X.compute_image_bounds(c, cols, rows)
    d_un = torch.zeros_like(d_k); d_off = torch.zeros((B, 64 * 48 + 1), dtype=torch.int32, device="cuda")
    d_idx = torch.zeros((B, cap), dtype=torch.int32, device="cuda"); d_in = torch.zeros(B, dtype=torch.int32, device="cuda")
    e.frame_finish_device(B, d_k, d_n, cap, c, bounds, d_un, d_off, d_idx, d_in)
    d_prev = d_un[torch.tensor([0, 2], device="cuda")][:, :, :2].contiguous()
    d_m12 = torch.full((P, cap), -7, dtype=torch.int32, device="cuda"); d_nm = torch.zeros(P, dtype=torch.int32, device="cuda")
    e.search_for_initialization_device(P, (0, 2), (1, 2), d_un, d_d, d_n, cap, d_off, d_idx, bounds, d_prev, d_m12, d_nm, 100, 0.9, True)
    rnd = np.random.default_rng(9).integers(0, 2 ** 31, (2, P, iters, 8)).astype(np.int32)
    d_res = torch.zeros((P, SC.RESULT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    d_p3d = torch.full((P, cap, 3), SC.POISON_F, dtype=torch.float32, device="cuda"); d_tri = torch.full((P, cap), SC.POISON_B, dtype=torch.uint8, device="cuda")
    kps = d_un.cpu().numpy().view(np.uint8).reshape(B, cap, 28).copy().view(SC.KP).reshape(B, cap)
    cam4 = (PINHOLE["fx"], PINHOLE["fy"], PINHOLE["cx"], PINHOLE["cy"])
    searched = d_nm.cpu().numpy().copy()
    assert searched.min() >= 50
    counts = []
    for call in range(2):
        torch.cuda.synchronize()
        before = dict(matches=d_m12.cpu().numpy().copy(), n_matches=d_nm.cpu().numpy().copy())
        d_p3d.fill_(SC.POISON_F); d_tri.fill_(SC.POISON_B)
        e.reconstruct_two_views_device(P, (0, 2), (1, 2), d_un, d_n, cap, d_m12, d_nm, c, torch.from_numpy(rnd[call]).cuda(), d_res, d_p3d, d_tri,
                                       iterations=iters, min_parallax=0.5, min_triangulated=20, rh_threshold=0.45, prune=True)
        torch.cuda.synchronize()
        s = dict(kps=kps, n_out=d_n.cpu().numpy(), matches=before["matches"], n_matches=before["n_matches"], rand=rnd[call], cam=cam4, frames1=(0, 2),
                 frames2=(1, 2), pairs=P, cap=cap, sigma=1.0, iterations=iters, min_parallax=0.5, min_triangulated=20, rh_threshold=0.45, prune=1)
        want = SC.expected(s)
        got = dict(result=d_res.cpu().numpy().view(SC.RESULT_DTYPE).reshape(-1), p3d=d_p3d.cpu().numpy(), tri=d_tri.cpu().numpy(),
                   matches=d_m12.cpu().numpy(), n_matches=d_nm.cpu().numpy())
        assert SC.differences(got, want) == [], (call, got["result"]["status"], want["result"]["status"])
        assert (got["result"]["status"] <= TW.ACCEPTED_F).all(), (call, got["result"]["status"])
        assert (got["result"]["n_matches"] == before["n_matches"]).all()                   # N of this call = the count the table came with
        assert (got["n_matches"] == (got["matches"] >= 0).sum(axis=1)).all() and (got["n_matches"] == (got["tri"] == 1).sum(axis=1)).all()
        counts.append(got["n_matches"].copy())
    assert (counts[0] < searched).all(), (searched, counts)      # the first call pruned matches of both pairs ...
    assert (counts[1] == counts[0]).all()                        # ... and what it left triangulates again: the second call prunes nothing
