"""orbx_stereo_fisheye_match_device on the GPU, every output pre-filled with a poison value: byte-equal to the sequential walk
(tests/stereo_fisheye_walk.py) on the crafted scene and the rule rigs (b) .. (g) of tests/test_stereo_fisheye.py at capacity 32 per eye,
rig_step 1, 0 and -1, a second identical call giving identical results (the atomicMax is deterministic); at the capacity whose right lapping
rows straddle the LDS chunk by one; at the real size (1302 keypoints per eye, 4 rigs, 11 workgroups per rig) against the kernel's own source
compiled for the host, which the CPU suite proves against the walk: all five arrays and both counters; the entry's rejections before any
launch; the other eye's rows of each array still holding the poison (assert_equals_walk); the debug counter against d_n_desc_matches."""
import numpy as np
import pytest

import extractorb_amd as X
import stereo_fisheye_scenes as SC
import test_stereo_fisheye as T

f32 = np.float32
POISON = T.POISON


def _dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.uint8) if a.dtype.fields else a).cuda()


def extractor():
    return X.ORBextractor(1000, 1.2, 8)


def run(ex, rigs, cap, first=0, step=1, n_rigs=None, tlr=SC.TLR, desc_matches=True):
    """the dict of test_stereo_fisheye.host_run, from the device"""
    import torch
    d = dict((k, _dev(v)) for k, v in SC.pack(rigs, cap).items())
    n_rigs = len(rigs) if n_rigs is None else n_rigs
    o = dict((k, _dev(v)) for k, v in T.outputs(2 * len(rigs), n_rigs, cap).items())
    torch.cuda.synchronize()                            # torch's copies have landed before the handle's stream runs
    ex.stereo_fisheye_count(True)
    ex.stereo_fisheye_match_device(n_rigs, (first, step), d["kps"], d["desc"], d["nout"], d["mono"], cap, tlr, X.camera_kb8(*SC.CAMS[0]),
                                   X.camera_kb8(*SC.CAMS[1]), o["l2r"], o["r2l"], o["depth"], o["x3d"], o["n"], o["nd"] if desc_matches else None)
    ex.synchronize()
    out = dict((k, v.cpu().numpy()) for k, v in o.items())
    out["calls"] = ex.stereo_fisheye_stats()
    return out


def same(a, b):
    return all(T.same_floats(a[k], b[k]) if a[k].dtype == f32 else np.array_equal(a[k], b[k]) for k in ("l2r", "r2l", "depth", "x3d", "n", "nd")) \
        and a["calls"] == b["calls"]


@pytest.mark.gpu
def test_gpu_crafted_scene_equals_the_walk_twice():
    ex = extractor()
    s = T.scene(T.CRAFTED_SEED)
    got = run(ex, s["rigs"], s["cap"])
    T.assert_equals_walk(got, s["rigs"], what="step 1")
    assert same(got, run(ex, s["rigs"], s["cap"]))                                   # every accepted left row took its atomicMax again: the same maximum
    assert got["calls"] == int(got["nd"].sum()) == 3 * 18                            # the debug counter is d_n_desc_matches summed
    T.assert_equals_walk(run(ex, s["rigs"], s["cap"], first=1, step=0, n_rigs=3), s["rigs"], first=1, step=0, n_rigs=3, what="step 0")
    T.assert_equals_walk(run(ex, s["rigs"], s["cap"], first=2, step=-1, n_rigs=2), s["rigs"], first=2, step=-1, n_rigs=2, what="step -1")
    o = run(ex, s["rigs"], s["cap"], desc_matches=False)
    assert (o["nd"] == POISON).all()
    T.assert_equals_walk(o, s["rigs"], what="no desc counter")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tie", "ratio", "shared", "octave", "nan"])
def test_gpu_rules_equal_the_walk(name):
    ex = extractor()
    if name == "nan":
        s = T.scene(T.CRAFTED_SEED)
        nan = SC.TLR.copy(); nan[1, 3] = np.nan
        got = run(ex, s["rigs"], s["cap"], tlr=nan)
        T.assert_equals_walk(got, s["rigs"], tlr=nan, what=name)
        assert (got["n"] == 0).all() and (got["nd"] == 18).all()
        return
    T.check_rules(name)
    rigs = T.rigs_of(name)
    got = run(ex, rigs, 32)
    T.assert_equals_walk(got, rigs, what=name)
    assert same(got, run(ex, rigs, 32))


@pytest.fixture(scope="module")
def sf_host(tmp_path_factory):
    return T.build_host(tmp_path_factory.mktemp("sfgpu"))


@pytest.mark.gpu
def test_gpu_chunk_boundary(sf_host):
    """kSfChunk + 1 right lapping rows: the best and the second candidate on either side of the boundary"""
    ex = extractor()
    chunk = sf_host.stereo_fisheye_chunk()
    T.check_rules("straddle", chunk)
    rigs = T.rigs_of("straddle", chunk)
    T.assert_equals_walk(run(ex, rigs, chunk + 8), rigs, what="straddle")


@pytest.mark.gpu
def test_gpu_real_size_equals_the_host_compiled_kernel(sf_host):
    """1302 keypoints per eye, 4 rigs: 1152 x 1150 lapping rows, 9 tiles and 9 chunks, the last of both partial"""
    ex = extractor()
    rigs = SC.make_real(31)
    cap = 1302
    assert all(len(r["left"]["kps"]) == cap and len(r["right"]["kps"]) == cap for r in rigs)
    got = run(ex, rigs, cap)
    want = T.host_run(sf_host, rigs, cap)
    print("matches %s of %s rows past the ratio test" % (got["n"].tolist(), got["nd"].tolist()))
    assert same(got, want)
    assert got["n"].min() > 600 and (got["nd"] - got["n"]).min() > 50 and got["calls"] == int(got["nd"].sum())
    back = got["r2l"][1::2]
    assert (back[:, :152] == -1).all() and (got["l2r"][0::2, :150] == -1).all()      # mono rows match nothing
    assert (got["l2r"][1::2] == POISON).all() and (got["r2l"][0::2] == POISON).all() and (got["depth"][1::2] == -7.0).all() and (got["x3d"][1::2] == -7.0).all()


@pytest.mark.gpu
def test_gpu_rejections():
    """ORBX_ERR_BAD_ARGUMENT (-2) before any launch: the outputs keep their poison"""
    ex = extractor()
    s = T.scene(T.CRAFTED_SEED)
    cap = s["cap"]
    d = dict((k, _dev(v)) for k, v in SC.pack(s["rigs"], cap).items())
    o = dict((k, _dev(v)) for k, v in T.outputs(6, 3, cap).items())
    import torch
    torch.cuda.synchronize()
    good = dict(n_rigs=3, rigs=(0, 1), d_kps=d["kps"], d_desc=d["desc"], d_n=d["nout"], d_mono=d["mono"], capacity=cap, tlr=SC.TLR,
                cam_left=X.camera_kb8(*SC.CAMS[0]), cam_right=X.camera_kb8(*SC.CAMS[1]), d_left_to_right=o["l2r"], d_right_to_left=o["r2l"],
                d_depth=o["depth"], d_x3d=o["x3d"], d_n_matches=o["n"], d_n_desc_matches=o["nd"])
    bad = [{k: None} for k in ("d_kps", "d_desc", "d_n", "d_mono", "tlr", "cam_left", "cam_right", "d_left_to_right", "d_right_to_left", "d_depth",
                               "d_x3d", "d_n_matches")]
    bad += [dict(n_rigs=0), dict(n_rigs=-1), dict(capacity=0), dict(rigs=(-1, 1)), dict(rigs=(1, -1)), dict(rigs=(0, -1)), dict(nlevels=7), dict(nlevels=9)]
    for change in bad:
        with pytest.raises(X.OrbxError) as e:
            ex.stereo_fisheye_match_device(**dict(good, **change))
        assert e.value.code == -2, (change, e.value.code)
    ex.synchronize()
    for k, v in o.items():
        a = v.cpu().numpy()
        assert (a == (-7.0 if a.dtype == f32 else POISON)).all(), k                   # nothing was launched
    assert X.load_library().orbx_stereo_fisheye_match_device(None, *([0] * 18)) == -2
    assert X.load_library().orbx_debug_stereo_fisheye_stats(None) == -2
