"""orbx_search_by_projection_sim3_device against the sequential walk (tests/sim3_projection_walk.py) on the cases of
tests/test_sim3_projection.py: d_matches, d_match_idx, d_match_dist, d_exit and d_n_matches exactly, all entries of every pair written (the
outputs are poisoned first), in both projection forms.  tests/test_sim3_projection.py (d) runs the kernels' own source, compiled for the host,
against the same walks on the same cases."""
import numpy as np
import pytest

import extractorb_amd as X
import sim3_projection_walk as S
import test_sim3_projection as P

POISON = -559038737
POISON8 = 0xA5
_uploads = {}


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda()


def upload(name, cap=None, mp_cap=None):
    key = (name, cap, mp_cap)
    if key not in _uploads:
        a = P.pack(P.get(name), cap, mp_cap)
        _uploads[key] = (a, dict((k, _dev(v)) for k, v in a.items() if isinstance(v, np.ndarray)))
    return _uploads[key]


def run(ex, name, projection, cap=None, mp_cap=None, n_mp=None, use_occupied=True, exits=True, **over):
    import torch
    c = P.get(name)
    a, dv = upload(name, cap, mp_cap)
    n_pairs = len(c["pairs"])
    d_nmp = None if n_mp is None else _dev(np.asarray(n_mp, np.int32))
    d_m = torch.full((n_pairs, a["cap"]), POISON, dtype=torch.int32, device="cuda")
    d_mi = torch.full((n_pairs, a["mp_cap"]), POISON, dtype=torch.int32, device="cuda"); d_md = d_mi.clone()
    d_ex = torch.full((n_pairs, a["mp_cap"]), POISON8, dtype=torch.uint8, device="cuda") if exits else None
    d_nm = torch.full((n_pairs,), POISON, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()                            # torch's copies and fills have landed before the handle's stream runs
    s = c["scene"]
    ex.search_by_projection_sim3_device(n_pairs, c["kf"], c["mp"], dv["world"], dv["normal"], dv["dist"], dv["mdesc"], d_nmp, a["mp_cap"], dv["flags"],
                                        dv["poses"], dv["kps"], dv["desc"], dv["nout"], a["cap"], dv["off"], dv["idx"], s["bounds"], X.camera(*s["cam"]),
                                        dv["occupied"] if a["any_occupied"] and use_occupied else None, d_m, d_mi, d_md, d_ex, d_nm,
                                        projection=projection, **dict(c["opt"], **over))
    ex.synchronize()
    return d_m.cpu().numpy(), d_mi.cpu().numpy(), d_md.cpu().numpy(), None if d_ex is None else d_ex.cpu().numpy(), d_nm.cpu().numpy()


def assert_equals_walk(name, projection, got, n_mp=None, use_occupied=True):
    m, mi, md, ex, nm = got
    c = P.get(name)
    for p, q in enumerate(c["pairs"]):
        want = P.walk(name, p, projection, n_mp=None if n_mp is None else int(n_mp[q["lst"]]), use_occupied=use_occupied)
        n = len(want["matches"]); k = len(want["exit"])
        what = "%s pair %d projection %d" % (name, p, projection)
        print("%s: %d matches (walk %d), exits %s" % (what, int(nm[p]), want["n_matches"], np.bincount(want["exit"], minlength=8).tolist()))
        assert np.array_equal(m[p, :n], want["matches"]) and (m[p, n:] == -1).all(), what
        assert np.array_equal(mi[p, :k], want["match_idx"]) and np.array_equal(md[p, :k], want["match_dist"]), what
        assert ex is None or np.array_equal(ex[p, :k], want["exit"]), what
        assert int(nm[p]) == want["n_matches"], what
        # past the list: written all the same, as flag exits
        assert (mi[p, k:] == -1).all() and (md[p, k:] == 256).all() and (ex is None or (ex[p, k:] == S.EXIT_FLAG).all()), what


def extractor(setting=(1.2, 8), nfeatures=1000):
    return X.ORBextractor(nfeatures, setting[0], setting[1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in P.CASES if n != "real"])
def test_gpu_every_case_in_both_projection_forms(name):
    """mp_capacity is the list length of the case: 600, the edge scene's and the crafted ones' are no multiples of the block"""
    ex = extractor(P.get(name)["scene"]["setting"])
    for projection in (0, 1):
        got = run(ex, name, projection)
        assert_equals_walk(name, projection, got)
        again = run(ex, name, projection)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))


@pytest.mark.gpu
def test_gpu_real_sizes_two_pairs_into_one_keyframe():
    """capacity 1302, 4000 MapPoints x 2 pairs with different poses, kf_step = 0: more than one block per pair, requests strided over the
    settling workgroup several times"""
    ex = extractor(nfeatures=1200)
    assert ex.capacity == 1302
    for projection in (0, 1):
        got = run(ex, "real", projection, cap=1302)
        assert_equals_walk("real", projection, got)
        assert got[4].sum() > 600
    rounds, rescans, ticks, zero = ex.debug_sim3_search_stats()
    print("real: rounds %d, re-scans %d, %d ticks" % (rounds, rescans, ticks))
    assert 2 <= rounds <= 4001 and ticks > 0 and zero == 0


@pytest.mark.gpu
def test_gpu_the_cascade_needs_a_round_per_request_and_the_reversed_chain_does_not():
    ex = extractor()
    assert_equals_walk("cascade", 0, run(ex, "cascade", 0))
    rounds = ex.debug_sim3_search_stats()[0]
    print("cascade: %d rounds" % rounds)
    assert rounds >= 40
    assert_equals_walk("reversed", 0, run(ex, "reversed", 0))
    rounds = ex.debug_sim3_search_stats()[0]
    print("reversed: %d rounds" % rounds)
    assert 2 <= rounds <= 3


@pytest.mark.gpu
def test_gpu_a_used_up_key_list_scans_its_window_again():
    ex = extractor()
    assert_equals_walk("overflow", 1, run(ex, "overflow", 1))
    assert ex.debug_sim3_search_stats()[1] > 0
    assert_equals_walk("cascade", 0, run(ex, "cascade", 0))          # the count is the last launch's
    assert ex.debug_sim3_search_stats()[1] == 0


@pytest.mark.gpu
def test_gpu_occupied_null_no_exit_array_and_ragged_lists():
    """d_occupied NULL on a case that has occupied keypoints (all free), d_exit NULL, d_n_mp below mp_capacity 700 (above the list's 600,
    the flags beyond set): entries past the list are FLAG, -1, 256; a count above mp_capacity or below 0 is clamped"""
    ex = extractor()
    name = "contended_occupied"
    assert_equals_walk(name, 0, run(ex, name, 0, use_occupied=False), use_occupied=False)
    assert_equals_walk(name, 0, run(ex, name, 0, exits=False))
    assert_equals_walk(name, 1, run(ex, name, 1, mp_cap=700, n_mp=[600]), n_mp=[600])
    assert_equals_walk(name, 0, run(ex, name, 0, mp_cap=700, n_mp=[333]), n_mp=[333])
    assert_equals_walk(name, 0, run(ex, name, 0, mp_cap=700, n_mp=[0]), n_mp=[0])
    got = run(ex, name, 0, n_mp=[9999])
    assert_equals_walk(name, 0, got)
    assert_equals_walk(name, 0, run(ex, name, 0, n_mp=[-4]), n_mp=[0])


@pytest.mark.gpu
def test_gpu_argument_errors_and_the_lds_bound_are_rejected_before_any_launch():
    import torch
    ex = extractor()
    z = torch.zeros(8192, dtype=torch.int32, device="cuda")
    outs = [torch.full((64,), POISON, dtype=torch.int32, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    ex.profile(True)
    good = dict(n_pairs=1, kf=(0, 0), mp=(0, 0), d_mp_world=z, d_mp_normal=z, d_mp_dist=z, d_mp_desc=z, d_n_mp=None, mp_capacity=16, d_mp_flags=z,
                d_poses=z, d_kps_un=z, d_desc=z, d_n=z, capacity=16, d_grid_off=z, d_grid_idx=z, bounds=P.T.BOUNDS, cam=X.camera(*P.T.CAM),
                d_occupied=None, d_matches=outs[0], d_match_idx=outs[1], d_match_dist=outs[2], d_exit=None, d_n_matches=outs[3])
    bad = [dict(n_pairs=0), dict(n_pairs=65536), dict(kf=(-1, 1)), dict(mp=(-1, 0)), dict(n_pairs=3, kf=(1, -1)), dict(capacity=0), dict(mp_capacity=0),
           dict(th_low=-1), dict(nlevels=7), dict(projection=2), dict(projection=-1), dict(bounds=np.array([0, 0, 0, 480], np.float32)), dict(bounds=None),
           dict(cam=None)]
    bad += [dict([(k, None)]) for k in ("d_mp_world", "d_mp_normal", "d_mp_dist", "d_mp_desc", "d_mp_flags", "d_poses", "d_kps_un", "d_desc", "d_n",
                                       "d_grid_off", "d_grid_idx", "d_matches", "d_match_idx", "d_match_dist", "d_n_matches")]
    for change in bad:
        with pytest.raises(X.OrbxError) as e:
            ex.search_by_projection_sim3_device(**dict(good, **change))
        assert e.value.code == -2, change
    # the LDS bound: 4 * (capacity + mp_capacity) + 64 <= 163 328; refused before the pointers are looked at
    for change in (dict(capacity=2720, mp_capacity=38097), dict(capacity=65537, mp_capacity=16), dict(capacity=16, mp_capacity=40801)):
        with pytest.raises(X.OrbxError) as e:
            ex.search_by_projection_sim3_device(**dict(good, **change))
        assert e.value.code == -8, change      # ORBX_ERR_UNSUPPORTED
    ex.synchronize()
    assert all((o == POISON).all() for o in outs)
    assert sum(v[1] for v in ex.profile_read().values()) == 0      # nothing was launched
    ex.search_by_projection_sim3_device(**good)                    # the unchanged call is accepted: n_out = 0, an empty grid, flags 0
    ex.synchronize()
    assert (outs[0][:16] == -1).all() and (outs[1][:16] == -1).all() and (outs[2][:16] == 256).all() and int(outs[3][0]) == 0
    assert all((o[16:] == POISON).all() for o in outs[:3])


@pytest.mark.gpu
def test_gpu_the_largest_admitted_shape_runs():
    """capacity 2720 with mp_capacity 16384 (76 480 bytes of LDS): an empty keyframe, every request leaves by its flag"""
    import torch
    ex = extractor()
    cap, m = 2720, 16384
    z = torch.zeros(max(cap * 8, m * 8), dtype=torch.int32, device="cuda")
    d_m = torch.full((cap,), POISON, dtype=torch.int32, device="cuda")
    d_mi = torch.full((m,), POISON, dtype=torch.int32, device="cuda"); d_md = d_mi.clone()
    d_ex = torch.full((m,), POISON8, dtype=torch.uint8, device="cuda"); d_nm = torch.full((1,), POISON, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ex.search_by_projection_sim3_device(1, (0, 0), (0, 0), z, z, z, z, None, m, z, z, z, z, z, cap, z, z, P.T.BOUNDS, X.camera(*P.T.CAM), None, d_m, d_mi,
                                        d_md, d_ex, d_nm)
    ex.synchronize()
    assert (d_m == -1).all() and (d_mi == -1).all() and (d_md == 256).all() and (d_ex == 0).all() and int(d_nm[0]) == 0
    assert ex.debug_sim3_search_stats()[0] == 1
