"""orbx_reconstruct_two_views_device refuses bad arguments with ORBX_ERR_BAD_ARGUMENT before any launch: the outputs' poison is intact
afterwards, and so is the match table."""
import numpy as np
import pytest

import extractorb_amd as X
import two_view_scenes as SC
from test_two_view_gpu import _dev

BAD = {
    "n_pairs_0": dict(n_pairs=0), "capacity_0": dict(capacity=0), "negative_first": dict(frames1=(-1, 1)), "negative_step": dict(frames2=(1, -1)),
    "iterations_0": dict(iterations=0), "iterations_above_the_cap": dict(iterations=4097), "sigma_0": dict(sigma=0.0), "sigma_negative": dict(sigma=-1.0),
    "sigma_nan": dict(sigma=float("nan")), "threshold_0": dict(rh_threshold=0.0), "threshold_1": dict(rh_threshold=1.0),
    "threshold_nan": dict(rh_threshold=float("nan")), "null_kps": dict(null="kps"), "null_n_out": dict(null="n_out"), "null_matches": dict(null="matches"),
    "null_n_matches": dict(null="n_matches"), "null_rand": dict(null="rand"), "null_result": dict(null="result"), "null_p3d": dict(null="p3d"),
    "null_triangulated": dict(null="tri"),
}


@pytest.mark.gpu
def test_gpu_rejections_return_before_a_launch():
    import torch
    torch.zeros(1).cuda()
    ex = X.ORBextractor(1000, 1.2, 8)
    s = SC.case("plane_n96")
    o = SC.poisoned_outputs(s)
    d = dict((k, _dev(v)) for k, v in o.items())
    d.update(kps=_dev(s["kps"]), n_out=_dev(s["n_out"]), rand=_dev(s["rand"]))
    torch.cuda.synchronize()
    for name, bad in BAD.items():
        a = dict(n_pairs=1, frames1=s["frames1"], frames2=s["frames2"], capacity=s["cap"], iterations=s["iterations"], sigma=1.0, rh_threshold=0.4)
        a.update((k, v) for k, v in bad.items() if k != "null")
        p = dict((k, None if bad.get("null") == k else v) for k, v in d.items())
        with pytest.raises(X.OrbxError) as err:
            ex.reconstruct_two_views_device(a["n_pairs"], a["frames1"], a["frames2"], p["kps"], p["n_out"], a["capacity"], p["matches"], p["n_matches"],
                                            X.camera(*s["cam"]), p["rand"], p["result"], p["p3d"], p["tri"], a["sigma"], a["iterations"], 1.0, 50,
                                            a["rh_threshold"], True)
        assert -2 in err.value.args or "null pointer" in str(err.value), (name, err.value.args)      # ORBX_ERR_BAD_ARGUMENT
        ex.synchronize()
        for k, v in o.items():
            assert d[k].cpu().numpy().tobytes() == np.ascontiguousarray(v).tobytes(), (name, k)
    # a null cam, through the C entry itself
    dp = lambda t: t.data_ptr()
    rc = ex._L.orbx_reconstruct_two_views_device(ex._h, 1, 0, 2, 1, 2, dp(d["kps"]), dp(d["n_out"]), s["cap"], dp(d["matches"]), dp(d["n_matches"]), None, 1.0,
                                                 s["iterations"], 1.0, 50, 0.4, dp(d["rand"]), 1, dp(d["result"]), dp(d["p3d"]), dp(d["tri"]))
    assert rc == -2                                          # ORBX_ERR_BAD_ARGUMENT
    ex.synchronize()
    for k, v in o.items():
        assert d[k].cpu().numpy().tobytes() == np.ascontiguousarray(v).tobytes(), ("null_cam", k)
    # and the same call with the camera is accepted: the table above refused for its one bad argument only
    ex.reconstruct_two_views_device(1, s["frames1"], s["frames2"], d["kps"], d["n_out"], s["cap"], d["matches"], d["n_matches"], X.camera(*s["cam"]),
                                    d["rand"], d["result"], d["p3d"], d["tri"], 1.0, s["iterations"], 1.0, 50, 0.4, True)
    ex.synchronize()
    assert d["result"].cpu().numpy().view(SC.RESULT_DTYPE)[0]["status"] == 0
