#!/usr/bin/env python3
"""Times orbx_create_new_map_points_device and orbx_create_new_map_points_two_eyes_device (the triangulation loop of
LocalMapping::CreateNewMapPoints, reference src/LocalMapping.cc:481-707) at the real size - 2024 keypoints one-camera, 1302 per eye; the
scenes of tests/test_new_map_points_gpu.py, one keyframe against 4 neighbours, the match lists taken from the searches and repeated - for
1, 16 and 256 pairs per call, with events around many calls; the medians over the rounds are reported.  Beside it:
  * the kernel's source compiled for the host, one thread (tests/cpp/new_map_points_host_check.cpp): what a caller pays today, without the
    copies of the match lists;
  * for the two-eye form, orbx_kb8_triangulate_device over as many keypoint pairs: both are dominated by nullVector4 and two KannalaBrandt8
    projections.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/new_map_points_rate.py --calls 20 --rounds 3` for the per-kernel table.
torch is asked for the GPU BEFORE the library is loaded: a process whose first HIP call is the library's leaves torch without a device.
Prints one JSON line.  usage: new_map_points_rate.py [--rounds 7] [--calls 50] [--pairs 1,16,256]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--pairs", default="1,16,256")
    a = ap.parse_args()
    shapes = [int(v) for v in a.pairs.split(",")]
    P = max(shapes)
    import torch
    assert torch.cuda.is_available(), "no GPU"
    torch.zeros(1, device="cuda")                       # torch's runtime first
    import extractorb_amd as X
    import new_map_points_scenes as SC
    import test_new_map_points as TN
    import test_new_map_points_gpu as G
    import triangulation_two_eyes_scenes as S2

    def span(fn, calls):
        fn(); torch.cuda.synchronize()
        t = []
        for _ in range(a.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record(); torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1) * 1000.0 / calls)
        return float(np.median(t))

    def tiled(scene, lists):
        """keyframe 0 and its 4 neighbours repeated until P pairs: batch frame 1 + p is neighbour p % 4"""
        kfs = [scene["kfs"][0]] + [scene["kfs"][1 + p % 4] for p in range(P)]
        return dict(scene, kfs=kfs, pairs=[lists[p % 4] for p in range(P)], kinds=[[]] * P, kf1=(0, 0), kf2=(1, 1))

    def host_us(host, scene, lists):
        four = dict(scene, pairs=lists, kinds=[[]] * 4, kf1=(0, 0), kf2=(1, 1))
        TN.host_run(host, four)
        t0 = time.perf_counter()
        for _ in range(3):
            TN.host_run(host, four)
        return (time.perf_counter() - t0) / 3 / 4 * 1e6

    out = dict(rounds=a.rounds, calls=a.calls)
    host = TN.build_host(tempfile.mkdtemp())
    for form in ("one_camera", "two_eyes"):
        if form == "one_camera":
            ex = X.ORBextractor(2000)
            searches, kfs = G.real_size_one_camera()
            scene, first = G.one_camera_chain(ex, searches, kfs, 2024)
        else:
            ex = G.extractor()
            s = S2.make(21, cap=1302, n_points=1500, rigs=5, nan_rig=-1, skew=0.02, nodes=300, dup=40, decoys=8)
            frames = [(0, b) for b in (1, 2, 3, 4)]
            d, d_p, d_n = G.two_eyes_search(ex, s, frames, (1, 1))
            ex.synchronize()
            n = d_n.cpu().numpy(); pr = d_p.cpu().numpy()
            scene = G.as_new_points_scene(s, frames, [[tuple(r) for r in pr[p, :n[p]].tolist()] for p in range(4)])
        lists = scene["pairs"]
        big = tiled(scene, lists)
        dv = G.upload(big)
        o = G.device_outputs(P, dv["L"])
        ex.set_stream(torch.cuda.current_stream().cuda_stream)
        res = dict(capacity=dv["cap"], matches_per_pair=[len(l) for l in lists], host_one_thread_per_pair_us=host_us(host, scene, lists))
        for r in shapes:
            calls = max(5, a.calls // max(1, r // 16))
            t = span(lambda: G.call(ex, big, dv, o, n_pairs=r), calls)
            res["pairs_%d" % r] = dict(call_us=t, per_pair_us=t / r, matches=sum(len(lists[p % 4]) for p in range(r)))
            if form == "two_eyes":
                m = res["pairs_%d" % r]["matches"]
                uv = torch.from_numpy(np.random.default_rng(0).uniform(60, 450, (m, 2)).astype(np.float32)).cuda()
                z = torch.zeros(m, device="cuda"); x = torch.zeros((m, 3), device="cuda")
                res["pairs_%d" % r]["kb8_triangulate_us"] = span(
                    lambda: ex.kb8_triangulate_device(m, uv, uv, S2.CAMS[0], S2.CAMS[1], S2.TLR[:, :3], S2.TLR[:, 3], 1.0, 1.0, z, x), calls)
        res["new_points_first_pairs"] = o["n_new"].cpu().numpy()[:4].tolist()
        out[form] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
